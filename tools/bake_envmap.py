"""Bake a scene's sky into an environment map: render it from a point with the equal-area
SphericalCamera at res x res, write the EXR, and print the world_from_light (ImageInfiniteLight's
render_from_light up to the scene's translation) under which the image, loaded as an
ImageInfiniteLight, is seen from that point as the camera saw it.

The spherical camera's film is the equal-area octahedral square ImageInfiniteLight takes: pixel
(x, y) of both stands for uv = ((x + 0.5) / res, (y + 0.5) / res). The camera sends uv along
world_from_camera * swap_yz(EqualAreaSquareToSphere(uv)) (cameras.cpp:610-630); the light looks
its image up at EqualAreaSphereToSquare(light_from_world * w). So world_from_light is the camera's
rotation times the y/z swap, which undoes the camera's.

    python tools/bake_envmap.py --variant scatter --pos 0.5 0.5 -0.2 --look 0.5 0.5 0.5 --res 256 \\
        --spp 64 --out sky.exr"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWAP_YZ = np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])


def bake_camera(pos, look, up=(0.0, 1.0, 0.0)):
    from acceleratedvolrenderer_amd.scene import SphericalCamera
    return SphericalCamera(mapping="equalarea", pos=pos, look=look, up=up)


def world_from_light(camera):
    """The world_from_light of the baked image: the camera's rotation times the y/z swap (a sky
    has no position: the translation is dropped)."""
    m = np.array(camera.world_from_camera(), np.float64)
    m[:3, 3] = 0.0
    return m @ SWAP_YZ


def bake(scene, camera, res, spp, maxdepth, device=0):
    """The res x res image (float32, RGB) of `scene`'s medium and lights from `camera`."""
    from acceleratedvolrenderer_amd import VolPathIntegrator
    from acceleratedvolrenderer_amd.scene import RGBFilm, Scene
    sc = Scene(camera, RGBFilm(res, res), scene.medium, scene.lights, sampler=type(scene.sampler)(pixelsamples=spp),
               interface_sphere=scene.interface_sphere)
    integ = VolPathIntegrator(sc, device=device, spp=spp, maxdepth=maxdepth)
    try:
        integ.render()
        return np.asarray(integ.image(), np.float32).reshape(res, res, 3)
    finally:
        integ.close()


def main(argv=None):
    from acceleratedvolrenderer_amd import imageio, scenes
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", default="scatter", help="scenes.s_uniform variant")
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--pos", type=float, nargs=3, default=(0.5, 0.5, -0.2))
    ap.add_argument("--look", type=float, nargs=3, default=(0.5, 0.5, 0.5))
    ap.add_argument("--up", type=float, nargs=3, default=(0.0, 1.0, 0.0))
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--maxdepth", type=int, default=50)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="envmap.exr")
    a = ap.parse_args(argv)
    cam = bake_camera(a.pos, a.look, a.up)
    img = bake(scenes.s_uniform(n=a.grid, width=a.res, height=a.res, variant=a.variant), cam, a.res, a.spp, a.maxdepth,
               a.device)
    imageio.write_exr(a.out, img, half=False)
    print(f"wrote {a.out} ({a.res} x {a.res}, {a.spp} spp)")
    print("world_from_light (row-major; ImageInfiniteLight(filename=..., world_from_light=...)):")
    for row in world_from_light(cam):
        print("  " + " ".join(f"{v:.9g}" for v in row))


if __name__ == "__main__":
    main()
