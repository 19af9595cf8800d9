"""graph_maker (cmd/graph_maker.cpp of the reference) for this project's scenes (GPU): build the
free lighting graph of a scene preset lit by its distant light, compute the search ranges on
the device, take the light vector and the transport matrix once, and per entry of the
config's `bounces` run ComputeFinalLight and write PREFIX_d{depth}.txt in the reference's
graph file format (depth = bounces completed + 1), which GraphIntegrator.from_file and the
fork's `pbrt --graph` read. PREFIX_stats.json holds the graph's sizes and the seconds per stage.

usage: python tools/graph_maker.py [--scene s-cloud] [--n 64] [--config CONFIG.json] --out PREFIX
                                   [--precision 9] [--search-ranges device] [--sampler 0] [--seed 0]
                                   [--interface-sphere CX,CY,CZ,R] [--merge host]
                                   [--uniform SPACING [--uniform-reduce first|mean]]
                                   [--voxels SPACING | --wanted-vertices N] [--equator-step 10]
                                   [--capture-steps 100] [--fill-start ID|all] [--node-radius R]
                                   [--voxels-host]

--interface-sphere bounds the medium by a sphere (world space): the scene gets it as its
interface and the graph is made with the sphere as the primitive (primitive="interface").

--uniform SPACING also converts each lit graph to a uniform graph of that spacing
(FreeGraph.to_uniform; --uniform-reduce: the light of a voxel with several vertices is its first
vertex's, as in the reference, or their mean) and writes PREFIX_d{depth}_uniform.txt, which
GraphIntegrator.from_file renders with the uniform branch; such a graph's light already carries
Inv4Pi, so it takes light_scale=1.

--voxels SPACING (or --wanted-vertices N, the reference's bisection for a spacing) makes the
uniform graph straight from the medium instead, with no walks and no merge (graph.VoxelBoundary):
ray bundles from a sphere of points --equator-step degrees apart, (2 --capture-steps + 1)^2 rays
each, capture the medium's boundary; the points go onto the lattice and are thinned to a single
layer; a flood from it (--fill-start: a boundary vertex id, the lowest by default, or all) fills
the inside. The filled points are lit by the light vector alone (the config's
lightingCalculator values; the node radius is FreeGraphBuilder's default or --node-radius) and
written to PREFIX_voxels.txt, which graph.load_uniform reads and tools/graph_render_demo.py
renders; the light already carries Inv4Pi, so it takes light_scale=1.

CONFIG.json is the reference's graph config (graphBuilder / lightingCalculator, util.h:750-812);
without one the defaults below are used.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_CONFIG = {
    "graphBuilder": {"radiusModifier": 20.0, "maxDepth": 100, "dimensionSteps": 64, "iterationsPerStep": 8,
                     "renderSearchRange": {"active": True, "neighboursToUse": 4}},
    "lightingCalculator": {"lightIterations": 16, "pointsOnRadiusLight": 2, "bounces": [10]},
}
SCENES = ("s-cloud", "s-uniform")


def interface_sphere(text):
    """argparse type of --interface-sphere CX,CY,CZ,R: ((cx, cy, cz), r), world space."""
    from acceleratedvolrenderer_amd.graph import parse_interface_sphere
    try:
        return parse_interface_sphere(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def make_scene(name, n, sphere=None):
    """The preset with its distant light alone (the graph tools take exactly one); `sphere`:
    its interface sphere ((cx, cy, cz), r) in world space."""
    import torch
    from acceleratedvolrenderer_amd import capi, scenes
    from acceleratedvolrenderer_amd.scene import Scene
    if name == "s-cloud":
        density = torch.empty((n, n, n), dtype=torch.float32, device="cuda:0")
        gen = capi.Context(0)
        gen.generate_cloud(density.data_ptr(), n, 0, n ** 3)
        gen.sync()
        gen.close()
        base = scenes.s_cloud(density)
    else:
        base = scenes.s_uniform(n=n, variant="scatter")
    return Scene(base.camera, base.film, base.medium, base.lights[:1], sampler=base.sampler, interface_sphere=sphere)


def parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scene", choices=SCENES, default="s-cloud", help="scene preset")
    p.add_argument("--n", type=int, default=64, help="the preset's grid resolution (n^3)")
    p.add_argument("--config", help="graph config JSON (the reference's format)")
    p.add_argument("--out", required=True, help="output prefix: PREFIX_d{depth}.txt, PREFIX_stats.json")
    p.add_argument("--precision", type=int, default=9, help="significant digits of the floats written")
    p.add_argument("--search-ranges", choices=("device", "host", "scipy"), default="device")
    p.add_argument("--merge", choices=("host", "device"), default="host",
                   help="the vertex merge: in walk order on the host, or in rounds on the device (the same graph)")
    p.add_argument("--sampler", type=int, choices=(0, 1), default=0, help="0 independent, 1 zsobol")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--interface-sphere", type=interface_sphere, metavar="CX,CY,CZ,R",
                   help="bound the medium by this sphere (world space) and use it as the graph tools' primitive")
    p.add_argument("--uniform", type=float, metavar="SPACING",
                   help="also write PREFIX_d{depth}_uniform.txt, the uniform graph of this spacing")
    p.add_argument("--uniform-reduce", choices=("first", "mean"), default="first",
                   help="the light of a voxel that holds several vertices")
    p.add_argument("--voxels", type=float, metavar="SPACING",
                   help="write PREFIX_voxels.txt instead: the voxel boundary of the medium at this spacing, filled and lit")
    p.add_argument("--wanted-vertices", type=int, metavar="N",
                   help="as --voxels, with the spacing found by the reference's bisection for N boundary vertices")
    p.add_argument("--equator-step", type=float, default=10, metavar="DEG", help="degrees between capture sphere points")
    p.add_argument("--capture-steps", type=int, default=100, metavar="N", help="(2 N + 1)^2 rays per capture bundle")
    p.add_argument("--fill-start", metavar="ID|all", help="the boundary vertex the fill starts from (default: the lowest)")
    p.add_argument("--node-radius", type=float, help="the light vector's vertex radius (default: FreeGraphBuilder's)")
    p.add_argument("--voxels-host", action="store_true",
                   help="with --voxels: also run the conversion and the floods on the host, compare and time them")
    return p


def fill_start(text):
    """--fill-start: None (the lowest vertex), "all" or a vertex id."""
    if text is None or text == "all":
        return text
    try:
        return int(text)
    except ValueError:
        raise ValueError(f"--fill-start {text!r}: a boundary vertex id or 'all'")


def make_voxels(a, ctx, md, in_dir, smp, cfg, seconds):
    """The --voxels / --wanted-vertices run: capture, single layer, fill, light, write."""
    from acceleratedvolrenderer_amd import graph
    if a.voxels is not None and a.wanted_vertices is not None:
        raise SystemExit("--voxels and --wanted-vertices exclude each other")
    vb = graph.VoxelBoundary(ctx, md, num_steps=a.capture_steps)
    points = vb.capture_points(a.equator_step)
    boundary = vb.capture_boundary(spacing=a.voxels, wanted_vertices=a.wanted_vertices, points=points)
    filled = vb.fill_inside(boundary, start=fill_start(a.fill_start))
    seconds.update(vb.seconds)
    radius = a.node_radius if a.node_radius is not None else float(
        graph.same_spot_radius(md) * np.float32(cfg.graph_builder.radius_modifier))
    lc = cfg.lighting_calculator
    t0 = time.perf_counter()
    light = ctx.graph_light(smp.struct(), filled.points, in_dir, radius, lc.points_on_radius_light, lc.light_iterations,
                            md.max_dist_to_center)
    seconds["light_vector"] = time.perf_counter() - t0
    lit = graph.UniformGraph(graph.capi.GraphUniform(filled.coors, light, filled.spacing))
    t0 = time.perf_counter()
    name = f"{a.out}_voxels.txt"
    lit.save(name, precision=a.precision)
    seconds["write"] = time.perf_counter() - t0
    stats = {
        "spacing": float(boundary.spacing), "rays": int(vb.last_rays), "captured_points": int(len(points)),
        "vertices": {"captured": int(boundary.num_captured), "single_layer": int(boundary.num_vertices),
                     "filled": int(filled.num_vertices)},
        "visited_cells": int(boundary.visited), "cells": int(boundary.voxels.cells),
        "levels": {"single_layer": int(boundary.levels), "fill": int(filled.levels)},
        "capture_rays_per_second": vb.last_rays / max(seconds["capture"], 1e-12),
        "node_radius": radius, "light_average": float(np.mean(light, dtype=np.float64)), "file": name,
        "seconds": seconds,
    }
    print(f"voxels: {stats['vertices']['captured']} captured, {stats['vertices']['single_layer']} single layer, "
          f"{stats['vertices']['filled']} filled; {stats['visited_cells']} cells visited")
    for stage in ("capture", "to_uniform", "single_layer", "fill", "light_vector", "write"):
        print(f"  {stage}: {seconds[stage]:.4f} s")
    if a.voxels_host:
        # the same conversion and floods on the host, for the clock and as a check
        host = graph.VoxelBoundary(None, md, num_steps=a.capture_steps, device=False)
        t0 = time.perf_counter()
        full_d = graph.capi.GraphUniform.from_points_device(ctx, points, boundary.spacing)
        one_device = time.perf_counter() - t0
        t0 = time.perf_counter()
        full_h = graph.capi.GraphUniform.from_points(points, np.zeros(len(points), np.float32), boundary.spacing)
        one_host = time.perf_counter() - t0
        hb = host.to_single_layer(graph.UniformGraph(full_h))
        hf = host.fill_inside(hb, start=fill_start(a.fill_start))
        same = bool(np.array_equal(full_d.coors, full_h.coors) and np.array_equal(full_d.vertex_of, full_h.vertex_of) and
                    np.array_equal(hb.voxels.state(), boundary.voxels.state()) and np.array_equal(hf.coors, filled.coors))
        stats["host"] = {"same_result": same, "levels": {"single_layer": int(hb.levels), "fill": int(hf.levels)},
                         "seconds": {"from_points": one_host, "from_points_device": one_device,
                                     "single_layer": host.seconds["single_layer"], "fill": host.seconds["fill"]}}
        print(f"  host: from_points {one_host:.4f} s (device {one_device:.4f} s), single_layer "
              f"{host.seconds['single_layer']:.4f} s, fill {host.seconds['fill']:.4f} s; same result: {same}")
    return stats


def main(argv=None):
    a = parser().parse_args(argv)
    primitive = "interface" if a.interface_sphere else "box"
    from acceleratedvolrenderer_amd import capi, graph
    if a.config:
        with open(a.config) as fh:
            cfg = graph.Config.from_json(fh.read())
    else:
        cfg = graph.Config.from_json(DEFAULT_CONFIG)
    out_dir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(out_dir, exist_ok=True)
    seconds = {}
    t0 = time.perf_counter()
    scene = make_scene(a.scene, a.n, a.interface_sphere)
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    md = graph.MediumData(scene, primitive)
    in_dir = (-np.asarray(scene.light_w[0], np.float32)).astype(np.float32)   # the way the light travels
    smp = graph.GraphSampling.for_config(cfg, sampler=a.sampler, seed=a.seed)
    seconds["scene"] = time.perf_counter() - t0

    if a.voxels is not None or a.wanted_vertices is not None:
        stats = make_voxels(a, ctx, md, in_dir, smp, cfg, seconds)
        ctx.close()
        stats["scene"], stats["primitive"] = f"{a.scene} {a.n}^3", primitive
        with open(f"{a.out}_voxels_stats.json", "w") as fh:
            json.dump(stats, fh, indent=4)
            fh.write("\n")
        return 0

    # BuildGraph without the ranges, then ComputeSearchRanges on its own clock
    active = bool(cfg.graph_builder.render_search_range.get("active"))
    k = int(cfg.graph_builder.render_search_range.get("neighboursToUse", 0))
    t0 = time.perf_counter()
    builder = graph.FreeGraphBuilder(ctx, md, in_dir, smp, cfg.graph_builder, search_ranges=a.search_ranges,
                                     merge=a.merge)
    g = builder.build_graph(search_ranges=False)
    seconds["build_graph"] = time.perf_counter() - t0
    seconds["merge"] = builder.merge_seconds   # within build_graph: the walks into vertices, every cycle
    t0 = time.perf_counter()
    builder.compute_search_ranges(g)
    seconds["search_ranges"] = time.perf_counter() - t0

    lc = graph.LightingCalculator(ctx, g, md, in_dir, smp, cfg.lighting_calculator)
    t0 = time.perf_counter()
    light = lc.get_light_vector()
    seconds["light_vector"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    transport = lc.get_transport_matrix()
    seconds["transport_matrix"] = time.perf_counter() - t0

    files = []
    seconds["final_light"], seconds["write"] = [], []
    bounces_list = cfg.lighting_calculator.bounces
    for i, bounces in enumerate(bounces_list):
        depth = bounces + 1
        print(f"-----------\nDepth {depth} ({bounces} bounces)")
        t0 = time.perf_counter()
        depth_computed = lc.compute_final_light(i, light=light, transport=transport) + 1
        seconds["final_light"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        name = f"{a.out}_d{depth_computed}.txt"
        g.save(name, lc.light_scalar, precision=a.precision)
        seconds["write"].append(time.perf_counter() - t0)
        files.append({"file": name, "bounces": int(bounces), "depth": int(depth_computed),
                      "light_average": float(np.mean(lc.light_scalar, dtype=np.float64))})
        if a.uniform is not None:
            t0 = time.perf_counter()
            ug = g.to_uniform(a.uniform, lc.light_scalar, reduce=a.uniform_reduce)
            uname = f"{a.out}_d{depth_computed}_uniform.txt"
            ug.save(uname, precision=a.precision)
            seconds.setdefault("uniform", []).append(time.perf_counter() - t0)
            files[-1]["uniform"] = {"file": uname, "spacing": float(ug.spacing), "reduce": a.uniform_reduce,
                                    "vertices": int(ug.num_vertices)}
        if depth != depth_computed:
            print(f"Numerical limits reached with depth {depth_computed}, depth {depth} not possible")
            break
    ctx.close()

    stats = {
        "scene": f"{a.scene} {a.n}^3",
        "primitive": primitive,
        "interface_sphere": [*a.interface_sphere[0], a.interface_sphere[1]] if a.interface_sphere else None,
        "amounts": {"vertices": int(g.num_vertices), "edges": int(len(g.edge_from))},
        "in_node_path_length": {"avg": float(g.in_node_path_length), "count": int(g.in_node_path_count)},
        "render_search_range": {"avg": float(np.mean(g.search_range, dtype=np.float64)) if active else None,
                                "neighbours": k if active else 0, "computed_on": a.search_ranges if active else None},
        "sizes": {"node_radius": float(g.radius), "scene_radius": float(md.max_dist_to_center)},
        "reinforce_cycles": int(builder.reinforce_cycles),
        "merge": {"on": a.merge, "rounds": int(builder.merge_rounds) if a.merge == "device" else None},
        "files": files,
        "seconds": seconds,
    }
    with open(f"{a.out}_stats.json", "w") as fh:
        json.dump(stats, fh, indent=4)
        fh.write("\n")
    print("=== Graph stats ===")
    print(json.dumps(stats, indent=2))
    print("===================")
    return 0


if __name__ == "__main__":
    sys.exit(main())
