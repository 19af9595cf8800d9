"""The analyzer integrator (graph/analysis/integration_analyzer.cpp of the reference) for this
project's scenes (GPU): how well does a lighting graph serve the camera? Per --maxdepth value
the camera paths of every pixel are followed for that many real scatters (IntegrationAnalyzer,
k_graph_analyze); at each it is asked whether a graph vertex lies within the vertex radius
(node) and whether any lies within its own render search range (search), and how far those are.
Prints the reference's line

    [ x, y ], nodeScatters / totalScatters (ratio) | searchScatters / totalScatters (ratio), mean range

per --pixels entry and depth, then the same over the frame, and writes PREFIX_analysis.json and,
per depth, the maps PREFIX_d{depth}_node_ratio.exr, _search_ratio.exr and _mean_range.exr.

usage: python tools/graph_analyze.py [--scene s-cloud] [--n 64] [--graph FILE] --out PREFIX
                                     [--maxdepth 1,2,4] [--spp 16] [--pixels 640,360 ...]
                                     [--width 1280] [--height 720] [--sampler zsobol] [--filter gaussian]
                                     [--seed 0] [--time] [--compare-render] [--interface-sphere CX,CY,CZ,R]

--graph FILE is a graph file in the reference's format (tools/graph_maker.py writes them, in
this project's render space); without one the graph is built here with graph_maker's default
config. --time analyses each depth twice and reports the second run's kernel times;
--compare-render also times GraphIntegrator's render of the same samples. --interface-sphere
bounds the medium by a sphere (world space), which is then the primitive of the graph made here
and of the analysis (primitive="interface").
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

SCENES = ("s-cloud", "s-uniform")


def make_scene(name, n, width, height, sampler, spp, filt, sphere=None):
    """The preset at the given film, sampler and filter, with its distant light alone and,
    when given, the interface sphere ((cx, cy, cz), r) in world space."""
    import torch
    from acceleratedvolrenderer_amd import BoxFilter, GaussianFilter, IndependentSampler, RGBFilm, ZSobolSampler, capi, scenes
    from acceleratedvolrenderer_amd.scene import Scene
    if name == "s-cloud":
        density = torch.empty((n, n, n), dtype=torch.float32, device="cuda:0")
        gen = capi.Context(0)
        gen.generate_cloud(density.data_ptr(), n, 0, n ** 3)
        gen.sync()
        gen.close()
        base = scenes.s_cloud(density, width=width, height=height, sampler=sampler, spp=spp, filter=filt)
        return Scene(base.camera, base.film, base.medium, base.lights[:1], sampler=base.sampler, interface_sphere=sphere)
    base = scenes.s_uniform(n=n, width=width, height=height, variant="scatter")
    film = RGBFilm(width, height, filter=GaussianFilter() if filt == "gaussian" else BoxFilter())
    smp = ZSobolSampler(spp) if sampler == "zsobol" else IndependentSampler(spp)
    return Scene(base.camera, film, base.medium, base.lights[:1], sampler=smp, interface_sphere=sphere)


def build_index(ctx, scene, seed, primitive="box"):
    """graph_maker's default graph of the scene, lit: (index, description)."""
    from acceleratedvolrenderer_amd import graph
    from graph_maker import DEFAULT_CONFIG
    cfg = graph.Config.from_json(DEFAULT_CONFIG)
    md = graph.MediumData(scene, primitive)
    in_dir = (-np.asarray(scene.light_w[0], np.float32)).astype(np.float32)   # the way the light travels
    smp = graph.GraphSampling.for_config(cfg, sampler=0, seed=seed)
    g = graph.FreeGraphBuilder(ctx, md, in_dir, smp, cfg.graph_builder, search_ranges="device").build_graph()
    lc = graph.LightingCalculator(ctx, g, md, in_dir, smp, cfg.lighting_calculator)
    lc.compute_final_light()
    info = {"source": "built here (graph_maker's default config)", "config": DEFAULT_CONFIG, "primitive": primitive,
            "vertices": int(g.num_vertices), "vertex_radius": float(g.radius),
            "search_range_avg": float(np.mean(g.search_range, dtype=np.float64))}
    return g.index(lc.light_scalar), info


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
    p.add_argument("--scene", choices=SCENES, default="s-cloud", help="scene preset")
    p.add_argument("--n", type=int, default=64, help="the preset's grid resolution (n^3)")
    p.add_argument("--graph", help="graph file (the reference's format); default: build one here")
    p.add_argument("--out", required=True, help="output prefix: PREFIX_analysis.json, PREFIX_d{depth}_*.exr")
    p.add_argument("--maxdepth", default="1", help="comma-separated scatter depths, e.g. 1,2,4")
    p.add_argument("--spp", type=int, default=16)
    p.add_argument("--pixels", nargs="*", default=[], help="pixels x,y to print the reference's line for")
    p.add_argument("--width", type=int, default=1280)
    p.add_argument("--height", type=int, default=720)
    p.add_argument("--sampler", choices=("independent", "zsobol"), default="zsobol")
    p.add_argument("--filter", choices=("box", "gaussian"), default="gaussian")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--time", action="store_true", help="report the kernel times of a second, warm run per depth")
    p.add_argument("--compare-render", action="store_true", help="also time GraphIntegrator's render at the same spp")
    p.add_argument("--interface-sphere", type=interface_sphere, metavar="CX,CY,CZ,R",
                   help="bound the medium by this sphere (world space) and use it as the graph tools' primitive")
    return p


def main(argv=None):
    p = parser()
    a = p.parse_args(argv)
    primitive = "interface" if a.interface_sphere else "box"
    depths = [int(v) for v in a.maxdepth.split(",") if v != ""]
    pixels = [tuple(int(v) for v in s.split(",")) for s in a.pixels]
    for x, y in pixels:
        if not (0 <= x < a.width and 0 <= y < a.height):
            p.error(f"pixel {x},{y} outside the {a.width}x{a.height} film")
    from acceleratedvolrenderer_amd import GraphIntegrator, IntegrationAnalyzer, graph, imageio
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    scene = make_scene(a.scene, a.n, a.width, a.height, a.sampler, a.spp, a.filter, a.interface_sphere)
    an = IntegrationAnalyzer(scene, None, maxdepth=depths[0] if depths else 1, spp=a.spp, seed=a.seed,
                             primitive=primitive)
    if a.graph:
        an.index = graph.load_index(a.graph)
        info = {"source": a.graph, "vertices": int(an.index.num_vertices), "vertex_radius": float(an.index.radius)}
    else:
        an.index, info = build_index(an.ctx, scene, a.seed, primitive)
        an.ctx.set_graph_geometry(primitive)
    out = {"scene": f"{a.scene} {a.n}^3, {a.width}x{a.height}, {a.sampler} + {a.filter}, {a.spp} spp", "graph": info,
           "primitive": primitive,
           "interface_sphere": [*a.interface_sphere[0], a.interface_sphere[1]] if a.interface_sphere else None,
           "depths": []}
    for depth in depths:
        an.maxdepth = depth
        entry = {"maxdepth": depth}
        if a.time:
            entry["analyze_ms"] = timed(an.ctx, lambda: an.analyze())
            res = an.result()
        else:
            res = an.analyze()
        for x, y in pixels:
            print(res.format_line(x, y))
        print(res.format_summary())
        print()
        entry["frame"] = res.summary()
        entry["pixels"] = [dict(x=x, y=y, **res.pixel(x, y)) for x, y in pixels]
        entry["maps"] = []
        for name, img in zip(("node_ratio", "search_ratio", "mean_range"), res.ratio_maps()):
            path = f"{a.out}_d{depth}_{name}.exr"
            imageio.write_exr(path, img[:, :, None], channels=("Y",), half=False, samples_per_pixel=a.spp)
            entry["maps"].append(path)
        out["depths"].append(entry)
    npix = a.width * a.height
    if a.time:
        for e in out["depths"]:
            e["Msamples_per_s"] = npix * a.spp / e["analyze_ms"]["ms_total"] / 1e3
    if a.compare_render:
        integ = GraphIntegrator(scene, an.index, spp=a.spp, seed=a.seed, primitive=primitive)
        out["graph_render_ms"] = timed(integ.ctx, lambda: integ.render(0, a.spp))
        out["graph_render_Msamples_per_s"] = npix * a.spp / out["graph_render_ms"]["ms_total"] / 1e3
        integ.close()
    an.close()
    with open(f"{a.out}_analysis.json", "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
