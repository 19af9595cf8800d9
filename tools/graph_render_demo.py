"""The graph render end to end on S-cloud (GPU): build the lighting graph of an n^3 S-cloud
GridMedium lit by its distant light, render 1280x720 with GraphIntegrator at 1 and 16 spp,
write the 16-spp EXR and a JSON with the render's times (avr_stats ms_medium = k_graph_render,
ms_total), the vertex count and the neighbour-count histogram of the 1-spp pass. Beside them,
for context, a VolPathIntegrator render of the same scene and spp at maxdepth = bounces + 1.

usage: python tools/graph_render_demo.py [--n 256] [--out DIR] [--steps 64] [--iterations 8]
                                         [--radius-modifier 20] [--bounces 10]
                                         [--interface-sphere CX,CY,CZ,R]
                                         [--uniform SPACING [--uniform-reduce first|mean] [--voxel-view]]

--interface-sphere bounds the cloud by a sphere (world space): graph, graph render and the
VolPathIntegrator render beside them then all take the sphere as the medium's boundary
(primitive="interface").

--uniform SPACING also converts the lit graph to a uniform graph of that spacing (a number, or
a multiple of the vertex radius written as 1r, 2r, ...) and times its render (view 0,
light_scale 1: the graph's light already carries Inv4Pi) against the free-graph render in
the same process: 16 spp, the two alternately, three timed runs each after one warm-up each,
median and spread of ms_medium and ms_total, and the share of the 1-spp pass's scatters that
find a vertex, for both kinds. --voxel-view also times --graph-debug's voxel view once and
writes its EXR.

--graph-file PATH renders a graph file instead (free or uniform, e.g. tools/graph_maker.py
--voxels' PREFIX_voxels.txt, made for the same --n): one 16-spp render, its EXR and times.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(ctx, fn):
    """Run fn() once to warm up (allocations, the index upload), then once timed."""
    fn()
    ctx.sync()
    ctx.reset_stats()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    s = ctx.stats()
    return {"ms_camera": s["ms_camera"], "ms_medium": s["ms_medium"], "ms_film": s["ms_film"],
            "ms_total": s["ms_total"], "ms_wall": wall}


def parser():
    from graph_maker import interface_sphere
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, default=256)
    p.add_argument("--out", default="graph_render_demo")
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--iterations", type=int, default=8)
    p.add_argument("--max-depth", type=int, default=100)
    p.add_argument("--radius-modifier", type=float, default=20.0)
    p.add_argument("--bounces", type=int, default=10)
    p.add_argument("--width", type=int, default=1280)
    p.add_argument("--height", type=int, default=720)
    p.add_argument("--interface-sphere", type=interface_sphere, metavar="CX,CY,CZ,R",
                   help="bound the medium by this sphere (world space) and use it as the graph tools' primitive")
    p.add_argument("--uniform", metavar="SPACING", help="also render the uniform graph of this spacing (number, or Nr = N vertex radii)")
    p.add_argument("--uniform-reduce", choices=("first", "mean"), default="first")
    p.add_argument("--voxel-view", action="store_true", help="with --uniform: also render the voxel view")
    p.add_argument("--graph-file", metavar="PATH",
                   help="render this graph file (made by tools/graph_maker.py for the same --n) instead of building a graph")
    return p


def uniform_spacing(text, radius):
    """--uniform's value: a number, or a multiple of the vertex radius ("1r", "2.5r")."""
    if text.endswith("r"):
        return float(np.float32(float(text[:-1] or 1) * float(radius)))
    return float(text)


def compare_uniform(a, integ, g, light_scalar, out):
    """The uniform render beside the free render on the same lit graph (see the module text)."""
    free = integ.index
    spacing = uniform_spacing(a.uniform, g.radius)
    t0 = time.perf_counter()
    ug = g.to_uniform(spacing, light_scalar, reduce=a.uniform_reduce)
    res = {"spacing": spacing, "reduce": a.uniform_reduce, "vertices": int(ug.num_vertices),
           "s_convert": time.perf_counter() - t0, "light_scale": 1.0}
    integ.light_scale = 1.0
    kinds = {"free": free, "uniform": ug.table}
    found = {}
    for name, index in kinds.items():          # the warm-up: uploads, allocations; and the found share
        integ.index = index
        integ.render(0, 1)
        c = integ.last_pass(1)["count"]
        found[name] = float(np.mean(c[c >= 0] > 0))
        integ.render(0, 16)
    res["scatters_finding_a_vertex_1spp"] = found
    runs = {"free": [], "uniform": []}
    for _ in range(3):
        for name, index in kinds.items():
            integ.index = index
            integ.ctx.sync()
            integ.ctx.reset_stats()
            integ.render(0, 16)
            integ.ctx.sync()
            st = integ.ctx.stats()
            runs[name].append({"ms_medium": st["ms_medium"], "ms_total": st["ms_total"]})
    for name, rr in runs.items():
        res[name + "_16spp"] = {k: {"median": float(np.median([r[k] for r in rr])),
                                    "min": float(min(r[k] for r in rr)), "max": float(max(r[k] for r in rr)),
                                    "runs": [float(r[k]) for r in rr]} for k in ("ms_medium", "ms_total")}
    rgb, w = integ.film_sums()
    res["image_mean"] = float(integ.write_image(os.path.join(a.out, "graph_render_uniform_16spp.exr"), rgb, w, spp=16).mean())
    if a.voxel_view:
        integ.voxel_view = True
        integ.render(0, 16)
        integ.ctx.sync()
        integ.ctx.reset_stats()
        integ.render(0, 16)
        integ.ctx.sync()
        st = integ.ctx.stats()
        res["voxel_view_16spp"] = {"ms_medium": st["ms_medium"], "ms_total": st["ms_total"]}
        rgb, w = integ.film_sums()
        integ.write_image(os.path.join(a.out, "graph_voxel_view_16spp.exr"), rgb, w, spp=16)
        integ.voxel_view = False
    integ.index = free
    out["uniform"] = res
    print("uniform vs free, 16 spp: k_graph_render_uniform %.3f ms (%.3f..%.3f), k_graph_render %.3f ms (%.3f..%.3f); "
          "scatters finding a vertex: uniform %.3f, free %.3f" % (
              res["uniform_16spp"]["ms_medium"]["median"], res["uniform_16spp"]["ms_medium"]["min"],
              res["uniform_16spp"]["ms_medium"]["max"], res["free_16spp"]["ms_medium"]["median"],
              res["free_16spp"]["ms_medium"]["min"], res["free_16spp"]["ms_medium"]["max"], found["uniform"], found["free"]))


def render_file(a, scene, primitive):
    """--graph-file: render a graph file made for this scene (tools/graph_maker.py's PREFIX_d*.txt,
    PREFIX_d*_uniform.txt or PREFIX_voxels.txt) at 16 spp; its light carries Inv4Pi, so a
    uniform graph takes light_scale 1."""
    from acceleratedvolrenderer_amd import GraphIntegrator
    integ = GraphIntegrator.from_file(scene, a.graph_file, spp=16, seed=0, primitive=primitive, light_scale=1.0)
    out = {"scene": f"S-cloud GridMedium {a.n}^3, distant light, {a.width}x{a.height}, zsobol + gaussian",
           "primitive": primitive, "graph_file": a.graph_file, "vertices": int(integ.index.num_vertices)}
    integ.render(0, 1)
    c = integ.last_pass(1)["count"]
    out["scatters_finding_a_vertex_1spp"] = float(np.mean(c[c >= 0] > 0)) if np.any(c >= 0) else 0.0
    out["graph_render_16spp"] = timed(integ.ctx, lambda: integ.render(0, 16))
    rgb, w = integ.film_sums()
    out["graph_image_mean"] = float(integ.write_image(os.path.join(a.out, "graph_file_16spp.exr"), rgb, w, spp=16).mean())
    integ.close()
    with open(os.path.join(a.out, "graph_file_render.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def main(argv=None):
    a = parser().parse_args(argv)
    primitive = "interface" if a.interface_sphere else "box"
    import torch
    from acceleratedvolrenderer_amd import GraphIntegrator, VolPathIntegrator, capi, graph, scenes
    from acceleratedvolrenderer_amd.scene import Scene
    os.makedirs(a.out, exist_ok=True)
    density = torch.empty((a.n, a.n, a.n), dtype=torch.float32, device="cuda:0")
    gen = capi.Context(0)
    gen.generate_cloud(density.data_ptr(), a.n, 0, a.n ** 3)
    gen.sync()
    gen.close()
    cloud = scenes.s_cloud(density, width=a.width, height=a.height, sampler="zsobol", spp=16, filter="gaussian")
    scene = Scene(cloud.camera, cloud.film, cloud.medium, cloud.lights[:1], sampler=cloud.sampler,   # the distant light
                  interface_sphere=a.interface_sphere)

    if a.graph_file:
        render_file(a, scene, primitive)
        return
    integ = GraphIntegrator(scene, None, spp=16, seed=0, primitive=primitive)
    cfg = graph.Config(
        graph.GraphBuilderConfig(radius_modifier=a.radius_modifier, max_depth=a.max_depth, dimension_steps=a.steps,
                                 iterations_per_step=a.iterations,
                                 render_search_range={"active": True, "neighboursToUse": 4}),
        graph.LightingCalculatorConfig(light_iterations=16, points_on_radius_light=2, bounces=[a.bounces]))
    md = graph.MediumData(scene, primitive)
    in_dir = (-np.asarray(scene.light_w[0], np.float32)).astype(np.float32)   # the way the light travels
    smp = graph.GraphSampling.for_config(cfg, sampler=0, seed=0)
    t0 = time.perf_counter()
    builder = graph.FreeGraphBuilder(integ.ctx, md, in_dir, smp, cfg.graph_builder)
    g = builder.build_graph()
    t1 = time.perf_counter()
    lc = graph.LightingCalculator(integ.ctx, g, md, in_dir, smp, cfg.lighting_calculator)
    done = lc.compute_final_light()
    t2 = time.perf_counter()
    integ.index = g.index(lc.light_scalar)
    t3 = time.perf_counter()

    out = {"scene": f"S-cloud GridMedium {a.n}^3, distant light, {a.width}x{a.height}, zsobol + gaussian",
           "primitive": primitive,
           "interface_sphere": [*a.interface_sphere[0], a.interface_sphere[1]] if a.interface_sphere else None,
           "graph": {"vertices": int(g.num_vertices), "edges": int(len(g.edge_from)), "vertex_radius": float(g.radius),
                     "dimension_steps": a.steps, "iterations_per_step": a.iterations, "max_depth": a.max_depth,
                     "bounces": a.bounces, "bounces_completed": int(done), "search_range_neighbours": 4,
                     "s_build": t1 - t0, "s_light": t2 - t1, "s_index": t3 - t2}}
    out["graph_render_1spp"] = timed(integ.ctx, lambda: integ.render(0, 1))
    npix = a.width * a.height
    counts = integ.last_pass(1)["count"]
    hist = np.bincount(counts[counts >= 0])
    out["neighbours_1spp"] = {"no_scatter": int(np.sum(counts < 0)), "scattered": int(np.sum(counts >= 0)),
                              "histogram": [int(v) for v in hist], "mean": float(counts[counts >= 0].mean()),
                              "max": int(counts.max())}
    out["graph_render_16spp"] = timed(integ.ctx, lambda: integ.render(0, 16))
    rgb, w = integ.film_sums()
    img = integ.write_image(os.path.join(a.out, "graph_render_16spp.exr"), rgb, w, spp=16)
    out["graph_image_mean"] = float(img.mean())
    if a.uniform:
        compare_uniform(a, integ, g, lc.light_scalar, out)
    integ.close()

    vp = VolPathIntegrator(scene, maxdepth=a.bounces + 1, spp=16, seed=0)
    out["volpath_1spp"] = timed(vp.ctx, lambda: vp.render(0, 1))
    out["volpath_16spp"] = timed(vp.ctx, lambda: vp.render(0, 16))
    out["volpath_maxdepth"] = a.bounces + 1
    out["volpath_image_mean"] = float(vp.get_image().mean())
    vp.close()
    out["Msamples_per_s_16spp"] = {"graph": npix * 16 / out["graph_render_16spp"]["ms_total"] / 1e3,
                                   "volpath": npix * 16 / out["volpath_16spp"]["ms_total"] / 1e3}
    with open(os.path.join(a.out, "graph_render_demo.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
