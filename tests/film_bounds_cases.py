"""What the film pixel-bounds tests share (no device): the bounds, the scenes over
tests/camera_cases.py's grid and camera, and the index arithmetic of "crop = slice".

A film has a full resolution (W, H) and pixel bounds [x0, x1) x [y0, y1) inside it (pbrt's
Film::fullResolution and pixelBounds, film.cpp:97-172). Samplers, pixel filter and camera take the
absolute pixel and the full resolution, so a cropped render gives the bounds' pixels, sample for
sample, what the render of the whole film gives them; storage and readbacks are bounds-sized,
row-major within the bounds. Bounds are written (x0, y0, x1, y1) here, as film.pixel_bounds; the
"pixelbounds" parameter of a film is pbrt's x0 x1 y0 y1."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_cases as cc   # noqa: E402

W, H, SPP, MAXDEPTH = cc.W, cc.H, cc.SPP, cc.MAXDEPTH
CAMERA = "persp-roll"

# name -> (x0, y0, x1, y1)
BOUNDS = {
    "interior-14x7": (3, 2, 17, 9),      # odd interior rectangle, 98 pixels
    "far-corner": (19, 11, 20, 12),
    "first-column": (0, 0, 1, 12),
    "5x3": (10, 4, 15, 7),
    "whole": (0, 0, 20, 12),             # the whole film, set explicitly
}
# name -> (kind, radius, sigma)
FILTERS = {"box": ("box", (0.5, 0.5), 0.0), "gauss": ("gaussian", (1.5, 1.5), 0.5)}
SAMPLERS = ("independent", "zsobol")
KERNELS = ("persistent", "wavefront")
# the sample ranges rendered: two quad-aligned calls (ZSobol quads in the camera stage) and one
# that is not
QUAD_RANGES = ((0, 4), (4, 8))
ODD_RANGES = ((1, 4),)

# the far crop of a non-square film
FAR_W, FAR_H = 600, 40
FAR_BOUNDS = (590, 33, 597, 38)

# cropwindow -> bounds: (resolution, fraction, ceil(float32(res) * float32(c))). In the first four
# the float64 product lies just above the integer and would give one more; the last is exact.
CROP_EDGES = [(1280, 0.1, 128), (20, 0.15, 3), (20, 0.85, 17), (1000, 0.3, 300), (12, 0.25, 3)]


def as_param(bounds):
    """film.pixel_bounds order (x0, y0, x1, y1) -> the "pixelbounds" parameter's x0 x1 y0 y1."""
    x0, y0, x1, y1 = bounds
    return (x0, x1, y0, y1)


def npix(bounds):
    return (bounds[2] - bounds[0]) * (bounds[3] - bounds[1])


def pixel_ids(bounds, width):
    """Row-major ids, in the whole film, of the bounds' pixels in the bounds' own row-major order."""
    x0, y0, x1, y1 = bounds
    y, x = np.mgrid[y0:y1, x0:x1]
    return (y * width + x).ravel()


def slice_records(arrays, bounds, width, height, ns):
    """Per-sample arrays of a whole-film pass (element s * W * H + pixel) cut to the bounds'
    layout (element s * npix + pixel within the bounds)."""
    ids = pixel_ids(bounds, width)
    idx = (np.arange(ns)[:, None] * (width * height) + ids[None, :]).ravel()
    return tuple(np.asarray(a)[idx] for a in arrays)


def slice_sums(rgb, w, bounds, width, height):
    """Whole-film fp64 sums cut to the bounds."""
    ids = pixel_ids(bounds, width)
    return np.asarray(rgb).reshape(width * height, 3)[ids].reshape(-1), np.asarray(w).reshape(-1)[ids]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_filter(name):
    from acceleratedvolrenderer_amd.scene import BoxFilter, GaussianFilter
    kind, radius, sigma = FILTERS[name]
    return BoxFilter(radius) if kind == "box" else GaussianFilter(radius, sigma)


def scene_for(bounds=None, filt="box", sampler="independent", spp=SPP, width=W, height=H, film=None, camera=CAMERA,
              medium=None, lights=None):
    """tests/camera_cases.py's scene (the 6^3 random-density grid in the unit box under `camera`)
    with a width x height film whose pixel bounds are `bounds` (None: the whole film). `film`
    replaces the film object; `medium` and `lights` the grid and its lights."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import IndependentSampler, RGBFilm, Scene, ZSobolSampler
    base = scenes.s_uniform(n=cc.GRID_N, width=width, height=height, variant="scatter", density=cc.density())
    if film is None:
        film = RGBFilm(width, height, filter=make_filter(filt),
                       pixelbounds=None if bounds is None else as_param(bounds))
    smp = IndependentSampler(pixelsamples=spp) if sampler == "independent" else ZSobolSampler(pixelsamples=spp)
    return Scene(cc.make_camera(camera), film, base.medium if medium is None else medium,
                 base.lights if lights is None else lights, sampler=smp,
                 interface_sphere=cc.CAMERAS[camera][1].get("sphere"))


def covered_once(tiles, bounds):
    """How often the tiles cover each pixel of the bounds: an (h, w) count map; raises when a
    tile leaves the bounds."""
    x0, y0, x1, y1 = bounds
    n = np.zeros((y1 - y0, x1 - x0), np.int64)
    for tx0, ty0, tx1, ty1 in tiles:
        if not (x0 <= tx0 < tx1 <= x1 and y0 <= ty0 < ty1 <= y1):
            raise ValueError(f"tile {(tx0, ty0, tx1, ty1)} leaves the bounds {bounds}")
        n[ty0 - y0:ty1 - y0, tx0 - x0:tx1 - x0] += 1
    return n
