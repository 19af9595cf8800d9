"""First measurement of ComputeSearchRanges in its three forms (GPU): build one larger graph of
tools/graph_render_demo.py's scene (S-cloud GridMedium, distant light), then time
graph.compute_search_ranges (the float64 k-d tree, wall), the host routine
(avr_graph_index_search_ranges, wall, one thread) and the device call (wall, and its two
kernels by HIP events: avr_stats ms_medium = k_graph_knn, ms_film = k_graph_range_average).
Writes the JSON that profiles/graph_knn.json keeps.

usage: python tools/graph_knn_profile.py [--n 256] [--steps 256] [--iterations 8] [--radius-modifier 2]
                                         [--k 4] [--out graph_knn.json]
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


def best_of(fn, repeats):
    times, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=256)
    p.add_argument("--steps", type=int, default=256)
    p.add_argument("--iterations", type=int, default=8)
    p.add_argument("--max-depth", type=int, default=100)
    p.add_argument("--radius-modifier", type=float, default=2.0)
    p.add_argument("--k", type=int, default=4)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default="graph_knn.json")
    a = p.parse_args()
    from acceleratedvolrenderer_amd import capi, graph
    from graph_maker import make_scene
    scene = make_scene("s-cloud", a.n)
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    cfg = graph.Config(
        graph.GraphBuilderConfig(radius_modifier=a.radius_modifier, max_depth=a.max_depth, dimension_steps=a.steps,
                                 iterations_per_step=a.iterations),
        graph.LightingCalculatorConfig())
    md = graph.MediumData(scene)
    in_dir = (-np.asarray(scene.light_w[0], np.float32)).astype(np.float32)
    smp = graph.GraphSampling.for_config(cfg, sampler=0, seed=0)
    t0 = time.perf_counter()
    g = graph.FreeGraphBuilder(ctx, md, in_dir, smp, cfg.graph_builder).build_graph()
    s_build = time.perf_counter() - t0
    print(f"{g.num_vertices} vertices, radius {float(g.radius):.6g}, built in {s_build:.1f} s", flush=True)

    legacy, t_scipy = best_of(lambda: graph.compute_search_ranges(g.points, a.k), a.repeats)
    print(f"scipy {min(t_scipy):.3f} s", flush=True)
    t0 = time.perf_counter()
    idx = capi.GraphIndex(g.points, np.zeros(g.num_vertices, np.float32), None, radius=g.radius)
    s_index = time.perf_counter() - t0
    host, t_host = best_of(lambda: idx.search_ranges(a.k), a.repeats)
    print(f"host {min(t_host):.3f} s", flush=True)
    ctx.graph_search_ranges(idx, a.k)            # the index upload and first launch
    kernels = []
    dev = None
    t_dev = []
    for _ in range(a.repeats):
        ctx.sync()
        ctx.reset_stats()
        t0 = time.perf_counter()
        dev = ctx.graph_search_ranges(idx, a.k)
        t_dev.append(time.perf_counter() - t0)
        s = ctx.stats()
        kernels.append({"ms_k_graph_knn": s["ms_medium"], "ms_k_graph_range_average": s["ms_film"]})
    whole, t_whole = best_of(lambda: graph.compute_search_ranges_device(ctx, g.points, g.radius, a.k), a.repeats)
    ctx.close()
    rel = np.abs(host.astype(np.float64) - legacy) / legacy
    out = {
        "scene": f"S-cloud GridMedium {a.n}^3, distant light",
        "graph": {"vertices": int(g.num_vertices), "vertex_radius": float(g.radius), "dimension_steps": a.steps,
                  "iterations_per_step": a.iterations, "max_depth": a.max_depth, "radius_modifier": a.radius_modifier,
                  "s_build": s_build},
        "k": a.k,
        "repeats": a.repeats,
        "scipy_compute_search_ranges_s": {"min": min(t_scipy), "all": t_scipy},
        "host_index_build_s": s_index,
        "host_search_ranges_s": {"min": min(t_host), "all": t_host},
        "device_call_s": {"min": min(t_dev), "all": t_dev,
                          "note": "avr_graph_search_ranges with the index already uploaded: scratch allocation, two kernels, copy back"},
        "device_kernels_ms": kernels,
        "device_with_index_build_s": {"min": min(t_whole), "all": t_whole,
                                      "note": "graph.compute_search_ranges_device: host index build, upload, the call"},
        "device_equals_host_bitwise": bool(np.array_equal(dev.view(np.uint32), host.view(np.uint32))
                                           and np.array_equal(whole.view(np.uint32), host.view(np.uint32))),
        "host_vs_scipy_max_rel": float(rel.max()),
        "search_range_mean": float(host.mean(dtype=np.float64)),
    }
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
