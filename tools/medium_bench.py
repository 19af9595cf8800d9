"""Persistent vs wavefront throughput on inputs beyond the default bench (GPU): an
RGBGridMedium of random sigmoid coefficients (n^3), or the S-cloud grid (n^3, CloudMedium
density) lit by an ImageInfiniteLight sky plus the distant sun, or ("cloud") by S-cloud's own
distant light or, with --point-light X,Y,Z, a PointLight at that world position in its place;
S-cloud camera, zsobol + gaussian.

usage: python tools/medium_bench.py [--scene rgb|image|cloud] [--n 128] [--steps 4] [--kernel persistent|wavefront]
                                    [--point-light X,Y,Z] [--lightsampler bvh|uniform|power]

--lightsampler power puts a scene without image or local lights on k_paths' general instantiation
too, which a point light always runs: the pair to compare.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=128)
    p.add_argument("--steps", type=int, default=4)
    p.add_argument("--kernel", default="persistent")
    p.add_argument("--emissive", action="store_true")
    p.add_argument("--scene", default="rgb", choices=["rgb", "image", "cloud"])
    p.add_argument("--point-light", default=None, metavar="X,Y,Z",
                   help="scene cloud: a PointLight at this world position in place of the distant light")
    p.add_argument("--point-scale", type=float, default=10.0)
    p.add_argument("--lightsampler", default="bvh", choices=["bvh", "uniform", "power"])
    a = p.parse_args()
    if a.point_light is not None:
        a.scene = "cloud"
    import torch
    from acceleratedvolrenderer_amd import VolPathIntegrator, scenes, RGBGridMedium
    from acceleratedvolrenderer_amd.scene import Scene
    rng = np.random.default_rng(0)
    shape = (a.n, a.n, a.n)

    def coeffs(hi):
        c = np.empty(shape + (4,), np.float32)
        c[..., 0] = rng.uniform(-2e-5, 2e-5, shape)
        c[..., 1] = rng.uniform(-0.02, 0.02, shape)
        c[..., 2] = rng.uniform(-5, 5, shape)
        c[..., 3] = rng.uniform(0.0, hi, shape)
        return c
    base = scenes.s_cloud(np.zeros((1, 1, 1), np.float32), sampler="zsobol", spp=256, filter="gaussian")
    if a.scene in ("image", "cloud"):
        from acceleratedvolrenderer_amd import capi
        density = torch.empty((a.n, a.n, a.n), dtype=torch.float32, device="cuda:0")
        gen = capi.Context(0)
        gen.generate_cloud(density.data_ptr(), a.n, 0, a.n ** 3)
        gen.sync()
        gen.close()
    if a.scene == "cloud":
        from acceleratedvolrenderer_amd import PointLight
        cloud = scenes.s_cloud(density, sampler="zsobol", spp=256, filter="gaussian")
        lights = list(cloud.lights)
        if a.point_light is not None:
            pos = tuple(float(v) for v in a.point_light.split(","))
            lights[0] = PointLight(from_=pos, scale=a.point_scale)
        scene = Scene(cloud.camera, cloud.film, cloud.medium, lights, sampler=cloud.sampler)
    elif a.scene == "image":
        from acceleratedvolrenderer_amd import ImageInfiniteLight, RGBToSpectrumTable
        table = RGBToSpectrumTable.load(os.path.join(ROOT, "oracle", "_ref", "srgb_table.npz"))
        res = 256
        y, x = np.mgrid[0:res, 0:res] / res
        sky = np.stack([0.35 + 0.2 * y, 0.5 + 0.2 * y, 0.9 - 0.1 * x], 2).astype(np.float32)
        sky[40:48, 180:188] = [40, 36, 30]
        cloud = scenes.s_cloud(density, sampler="zsobol", spp=256, filter="gaussian")
        lights = [cloud.lights[0], ImageInfiniteLight(image=sky, rgb_table=table, scale=0.3)]
        scene = Scene(cloud.camera, cloud.film, cloud.medium, lights, sampler=cloud.sampler)
    else:
        kw = dict(sigma_a_coeffs=coeffs(0.3), sigma_s_coeffs=coeffs(4.0), g=0.877)
        if a.emissive:
            kw.update(Le_coeffs=coeffs(1.0), Lescale=0.5)
        med = RGBGridMedium(**kw)
        scene = Scene(base.camera, base.film, med, base.lights, sampler=base.sampler)
    integ = VolPathIntegrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=16, device=0, kernel=a.kernel,
                              lightsampler=a.lightsampler)
    integ.ctx.render(0, 16, 0, scenes.CLOUD_MAXDEPTH)
    integ.ctx.sync()
    t0 = time.perf_counter()
    for k in range(1, 1 + a.steps):
        integ.ctx.render(16 * k, 16 * (k + 1), 0, scenes.CLOUD_MAXDEPTH)
    integ.ctx.sync()
    dt = time.perf_counter() - t0
    name = {"image": f"S-cloud-{a.n} grid + ImageInfiniteLight", "rgb": f"RGBGridMedium {a.n}^3",
            "cloud": f"S-cloud-{a.n} grid, " + ("distant light" if a.point_light is None else f"PointLight at {a.point_light}")
            }[a.scene]
    print(json.dumps({"scene": name, "kernel": a.kernel, "emissive": a.emissive, "lightsampler": a.lightsampler,
                      "k_paths": integ.ctx.last_kernel() if a.kernel == "persistent" else None,
                      "Msamples_per_s": round(1280 * 720 * 16 * a.steps / dt / 1e6, 2)}))
    integ.close()


if __name__ == "__main__":
    main()
