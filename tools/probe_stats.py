"""k_paths walk / gather probes on the bench workload (variant build with -DAVR_PROBE_STATS):
how full the DDA walk's trips are, how many zero-majorant cells the walk crosses, and how many
distinct 64-B / 128-B lines the lanes of one collision round gather from (N1: the coalescing an
in-wave sort of the lookups could exploit). Results are unchanged by the probes.

--service: the service-round build (-DAVR_PROBE_STATS -DAVR_PROBE_SERVICE, variants/probe_service),
whose slots 4, 5 and 7 count service rounds, lanes served (event lanes + refilled lanes) and refill
runs instead of the distinct lines and the cut walks; --schedules lists threshold:batch pairs
(set_refill_min : set_refill_batch, 0 = default), each measured in turn in the same process.

usage: python tools/probe_stats.py --build [--service]      (needs no GPU: build first)
       python tools/probe_stats.py [--medium grid|nanovdb] [--steps 3] [--dda 0]
       python tools/probe_stats.py --service [--schedules 0:0,32:1] [--steps 3] [--dda 0]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(ROOT, "variants", "probe", "libavr_hip.so")
NAMES = ["walk_trips", "walking_lanes", "collision_rounds", "collision_lanes", "distinct_128B_lines",
         "distinct_64B_lines", "zero_majorant_steps", "walks_cut_with_walkers"]
VARIANT_SERVICE = os.path.join(ROOT, "variants", "probe_service", "libavr_hip.so")
NAMES_SERVICE = NAMES[:4] + ["service_rounds", "lanes_served", NAMES[6], "refill_runs"]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--build", action="store_true")
    p.add_argument("--res", type=int, default=1024)
    p.add_argument("--medium", default="grid", choices=["grid", "nanovdb"])
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--dda", type=int, default=0)
    p.add_argument("--pixelsamples", type=int, default=16384)
    p.add_argument("--service", action="store_true")
    p.add_argument("--schedules", default="0:0")
    p.add_argument("--variant", default=None, help="variants/<name> to load instead (e.g. a -DAVR_COUPLED_DEFAULT build)")
    a = p.parse_args()
    sys.path.insert(0, ROOT)
    if a.build:
        from acceleratedvolrenderer_amd import build as b
        if a.service:
            print(b.build(variant="probe_service", defines=["-DAVR_PROBE_STATS", "-DAVR_PROBE_SERVICE"]))
        else:
            print(b.build(variant="probe", defines=["-DAVR_PROBE_STATS"]))
        return
    os.environ["AVR_LIB"] = VARIANT_SERVICE if a.service else VARIANT
    if a.variant:
        os.environ["AVR_LIB"] = os.path.join(ROOT, "variants", a.variant, "libavr_hip.so")
    import torch
    from acceleratedvolrenderer_amd import VolPathIntegrator, scenes, capi
    n = a.res
    density = torch.empty((n, n, n), dtype=torch.float32, device="cuda:0")
    gen = capi.Context(0)
    slab = n * n * 64
    for first in range(0, n ** 3, slab):
        gen.generate_cloud(density.data_ptr() + 4 * first, n, first, min(slab, n ** 3 - first))
    gen.sync()
    gen.close()
    if a.medium == "nanovdb":
        scene = scenes.s_cloud_vdb(scenes.vdb_grid(density), sampler="zsobol", spp=a.pixelsamples, filter="gaussian")
        del density
    else:
        scene = scenes.s_cloud(density, sampler="zsobol", spp=a.pixelsamples, filter="gaussian")
    S = 64
    integ = VolPathIntegrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=S, device=0)
    if a.dda:
        integ.ctx.set_dda_budget(a.dda)
    lib = capi.load()
    lib.avr_debug_sections.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
    out = (ctypes.c_ulonglong * 8)()
    integ.ctx.render(0, S, 0, scenes.CLOUD_MAXDEPTH)
    integ.ctx.sync()
    npix = scene.film.width * scene.film.height
    names = NAMES_SERVICE if a.service else NAMES
    base = 1
    for sched in (a.schedules.split(",") if a.service else [None]):
        if sched is not None:
            r, b = (int(x) for x in sched.split(":"))
            integ.ctx.set_refill_min(r)
            integ.ctx.set_refill_batch(b)
        integ.ctx.render(S * base, S * (base + 1), 0, scenes.CLOUD_MAXDEPTH)   # warm this schedule
        integ.ctx.sync()
        lib.avr_debug_sections(integ.ctx.h, out)
        integ.ctx.reset_stats()
        t0 = time.perf_counter()
        for k in range(base + 1, base + 1 + a.steps):
            integ.ctx.render(S * k, S * (k + 1), 0, scenes.CLOUD_MAXDEPTH)
        integ.ctx.sync()
        dt = time.perf_counter() - t0
        base += a.steps + 1
        lib.avr_debug_sections(integ.ctx.h, out)
        c = {names[i]: int(out[i]) for i in range(8)}
        st = integ.stats()
        n = npix * S * a.steps
        iters = max(1, st.get("loop_iterations") or 1)
        d = {"medium": a.medium, "dda": a.dda, "counters": c,
             "loop_iterations": st.get("loop_iterations"), "dda_lane_steps": st.get("medium_dda_steps"),
             "samples": n, "step_ms_with_probes": round(dt * 1e3 / a.steps, 3),
             "walk_lanes_per_trip": round(c["walking_lanes"] / max(1, c["walk_trips"]), 3),
             "trips_per_iteration": round(c["walk_trips"] / iters, 3),
             "zero_majorant_step_frac": round(c["zero_majorant_steps"] / max(1, st.get("medium_dda_steps") or 1), 4),
             "collision_lanes_per_round": round(c["collision_lanes"] / max(1, c["collision_rounds"]), 3)}
        if a.service:
            d.update({"schedule": sched,
                      "iterations_per_sample": round(iters / n, 5),
                      "busy_lanes_per_iteration": round((st.get("active_lane_iterations") or 0) / iters, 3),
                      "kpaths_ms_with_probes": round(st["ms_medium"] / a.steps, 3),
                      "rounds_per_sample": round(c["service_rounds"] / n, 5),
                      "lanes_per_round": round(c["lanes_served"] / max(1, c["service_rounds"]), 3),
                      "refill_runs_per_sample": round(c["refill_runs"] / n, 5)})
        else:
            d.update({"lines128_per_lookup": round(c["distinct_128B_lines"] / max(1, c["collision_lanes"]), 4),
                      "lines64_per_lookup": round(c["distinct_64B_lines"] / max(1, c["collision_lanes"]), 4)})
        print(json.dumps(d), flush=True)
    integ.close()


if __name__ == "__main__":
    main()
