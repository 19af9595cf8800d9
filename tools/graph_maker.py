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

--interface-sphere bounds the medium by a sphere (world space): the scene gets it as its
interface and the graph is made with the sphere as the primitive (primitive="interface").

--uniform SPACING also converts each lit graph to a uniform graph of that spacing
(FreeGraph.to_uniform; --uniform-reduce: the light of a voxel with several vertices is its first
vertex's, as in the reference, or their mean) and writes PREFIX_d{depth}_uniform.txt, which
GraphIntegrator.from_file renders with the uniform branch; such a graph's light already carries
Inv4Pi, so it takes light_scale=1.

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
    return p


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
