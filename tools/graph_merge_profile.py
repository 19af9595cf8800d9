"""First measurement of the vertex merge in its two forms (GPU): take the walks of
tools/graph_render_demo.py's scene (S-cloud GridMedium, distant light) once, then per radius
modifier time the host builder (avr_graph_add_walks, wall, one thread) and the device path
(avr_graph_add_walks_device, wall, and its avr_graph_merge_stats split: host sort and upload,
device rounds with the id scan, host replay) on the same walks, each into a fresh graph, and
check that the two graphs are the same. The comparison is against the host builder, never
against the new code itself. Writes the JSON that profiles/graph_merge.json keeps.

usage: python tools/graph_merge_profile.py [--n 256] [--steps 256] [--iterations 8] [--max-depth 100]
                                           [--radius-modifiers 2,20] [--repeats 3] [--out graph_merge.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def summary(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "all": list(values)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=256)
    p.add_argument("--steps", type=int, default=256)
    p.add_argument("--iterations", type=int, default=8)
    p.add_argument("--max-depth", type=int, default=100)
    p.add_argument("--radius-modifiers", default="2,20")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default="graph_merge.json")
    a = p.parse_args()
    from acceleratedvolrenderer_amd import capi, graph
    from graph_maker import make_scene
    scene = make_scene("s-cloud", a.n)
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    md = graph.MediumData(scene)
    in_dir = (-np.asarray(scene.light_w[0], np.float32)).astype(np.float32)
    cfg = graph.Config(graph.GraphBuilderConfig(max_depth=a.max_depth, dimension_steps=a.steps,
                                                iterations_per_step=a.iterations), graph.LightingCalculatorConfig())
    smp = graph.GraphSampling.for_config(cfg, sampler=0, seed=0)
    b = graph.FreeGraphBuilder(ctx, md, in_dir, smp, cfg.graph_builder)
    o, d, t, idx = b.start_rays()
    pts, counts = ctx.graph_walks(smp.struct(), o, d, t, idx, a.iterations, 0, a.max_depth)
    n_points = int(counts.sum())
    print(f"{len(counts)} walks, {n_points} scatter points", flush=True)
    # the first device merge of a process also loads the kernels: keep it off the clock
    capi.Graph(1.0).add_walks_device(ctx, pts[:64], counts[:64], a.max_depth)

    runs = []
    for modifier in [float(m) for m in a.radius_modifiers.split(",")]:
        radius = float(np.float32(graph.same_spot_radius(md) * np.float32(modifier)))
        host_s, dev_s, splits = [], [], []
        gh = gd = None
        for _ in range(a.repeats):
            gh = capi.Graph(radius)
            t0 = time.perf_counter()
            gh.add_walks(pts, counts, a.max_depth)
            host_s.append(time.perf_counter() - t0)
            gd = capi.Graph(radius)
            t0 = time.perf_counter()
            s = gd.add_walks_device(ctx, pts, counts, a.max_depth)
            dev_s.append(time.perf_counter() - t0)
            splits.append(s)
        vh, sh = gh.vertices()
        vd, sd = gd.vertices()
        same = bool(np.array_equal(vh.view(np.uint32), vd.view(np.uint32)) and np.array_equal(sh, sd)
                    and all(np.array_equal(x, y) for x, y in zip(gh.edges(), gd.edges())))
        run = {
            "radius_modifier": modifier, "vertex_radius": radius, "points": n_points, "vertices": int(len(sh)),
            "edges": int(gh.size()[1]), "rounds": [s["rounds"] for s in splits],
            "host_add_walks_s": summary(host_s),
            "device_add_walks_s": summary(dev_s),
            "device_ms_sort": summary([s["ms_sort"] for s in splits]),
            "device_ms_rounds": summary([s["ms_rounds"] for s in splits]),
            "device_ms_replay": summary([s["ms_replay"] for s in splits]),
            "device_graph_equals_host": same,
        }
        print(json.dumps(run), flush=True)
        runs.append(run)
    ctx.close()
    out = {
        "scene": f"S-cloud GridMedium {a.n}^3, distant light",
        "walks": {"dimension_steps": a.steps, "iterations_per_step": a.iterations, "max_depth": a.max_depth,
                  "walks": int(len(counts)), "points": n_points},
        "repeats": a.repeats,
        "note": "wall-clock per call into a fresh graph; host: avr_graph_add_walks, one thread, same process; "
                "device: avr_graph_add_walks_device = host sort and upload (ms_sort), device rounds with the id scan "
                "and its download (ms_rounds), host replay (ms_replay)",
        "library": os.environ.get("AVR_LIB", "in-tree"),
        "runs": runs,
    }
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
