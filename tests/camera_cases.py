"""General cameras and non-default pixel filters, shared by tests/test_camera_cases_reference.py
(CPU: scene.py's matrices and the oracle's ray code against the reference's own transforms, the
oracle's filter sampling against the reference's, the conditions on the inputs) and
tests/test_gpu_camera.py (the camera stage of the device against the oracle) — TEST INFRASTRUCTURE,
no device.

Every other GPU test looks through an orthographic camera along +z or a perspective camera with
up = +y, outside the medium, looking towards +z, and samples the film through BoxFilter (0.5, 0.5)
or GaussianFilter (1.5, 1.5, sigma 0.5). Here:

  CAMERAS  ten poses over one medium (the unit box at the origin, a 6^3 random-density scattering
           grid, the lights of scenes.s_uniform): roll, every direction component negative, a
           mirrored camera_from_world, a camera inside the medium and inside an interface sphere,
           a wide fov, an off-centre screen window, an explicit frame aspect ratio, a portrait film
           (the frame < 1 branch of the screen window), an oblique and a backward orthographic
           camera. Film 20 x 12 (portrait: 12 x 20).
  FILTERS  Gaussian tables that are not square, that do not fit the camera stage's LDS staging
           (the global-memory branch of the filter sample), the largest and the smallest accepted
           size, a table with all-zero rows, and box filters with radii other than 0.5.
  PAIRS    every camera with the box filter of radius 0.5, every filter on "persp-roll", and
           "gauss-64" and "box-wide" on "ortho-back": not the full product."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H, SPP, MAXDEPTH = 20, 12, 8, 6
GRID_N = 6

# name -> (kind, camera keywords); "mirror": camera_from_world = diag(-1, 1, 1, 1) @ look_at(...)
CAMERAS = {
    "persp-roll": ("perspective", dict(fov=40.0, pos=(1.7, 1.6, 1.9), look=(0.45, 0.5, 0.55), up=(0.3, 1.0, -0.2))),
    "persp-mirrored": ("perspective", dict(fov=40.0, pos=(1.7, 1.6, 1.9), look=(0.45, 0.5, 0.55), up=(0.3, 1.0, -0.2),
                                           mirror=True)),
    "persp-inside": ("perspective", dict(fov=100.0, pos=(0.4, 0.55, 0.3), look=(0.9, 0.2, 1.0), up=(0.0, 1.0, 0.0))),
    "persp-inside-sphere": ("perspective", dict(fov=100.0, pos=(0.4, 0.55, 0.3), look=(0.9, 0.2, 1.0),
                                                up=(0.0, 1.0, 0.0), sphere=((0.5, 0.5, 0.5), 0.6))),
    "persp-wide": ("perspective", dict(fov=130.0, pos=(0.5, 0.5, -0.2), look=(0.5, 0.5, 0.5), up=(0.0, 1.0, 0.0))),
    # the window (-0.1, 0.9, -0.7, -0.05) sees the box in exactly 80 % of the pixel centres, the
    # edge of the range (the box's front face spans +-0.72 of the screen); moved further off the
    # axis by (0.2, -0.1) and a little smaller it is 64 %
    "persp-shifted": ("perspective", dict(fov=60.0, pos=(0.5, 0.5, -1.2), look=(0.5, 0.5, 0.5), up=(0.0, 1.0, 0.0),
                                          screenwindow=(0.1, 1.0, -0.8, -0.1))),
    "persp-frame": ("perspective", dict(fov=50.0, pos=(0.5, 0.5, -1.2), look=(0.5, 0.5, 0.5), up=(0.0, 1.0, 0.0),
                                        frameaspectratio=0.8)),
    "portrait": ("perspective", dict(fov=40.0, pos=(0.5, 0.5, -1.6), look=(0.5, 0.5, 0.5), up=(0.0, 1.0, 0.0),
                                     film=(12, 20))),
    "ortho-oblique": ("orthographic", dict(pos=(1.8, 1.5, -0.6), look=(0.5, 0.5, 0.5), up=(0.2, 1.0, 0.1),
                                           screenwindow=(-0.9, 0.9, -0.6, 0.6))),
    "ortho-back": ("orthographic", dict(pos=(0.5, 0.5, 2.0), look=(0.5, 0.5, 1.0), up=(0.0, 1.0, 0.0),
                                        screenwindow=(-0.7, 0.7, -0.6, 0.6))),
}
# the share of pixel-centre rays that cross the box: (low, high), both inclusive
HIT_SHARE = {name: (0.20, 0.80) for name in CAMERAS}
HIT_SHARE["persp-inside"] = HIT_SHARE["persp-inside-sphere"] = (1.0, 1.0)

# name -> (kind, (rx, ry), sigma)
FILTERS = {
    "box": ("box", (0.5, 0.5), 0.0),
    "gauss-64": ("gaussian", (2.0, 2.0), 0.5),
    "gauss-tall": ("gaussian", (0.75, 2.5), 0.4),
    "gauss-flat": ("gaussian", (2.5, 0.75), 0.4),
    "gauss-just-over": ("gaussian", (1.5, 1.6), 0.5),
    "gauss-max": ("gaussian", (4.0, 4.0), 1.0),
    "gauss-tiny": ("gaussian", (0.5, 0.5), 0.5),
    "gauss-needle": ("gaussian", (1.5, 1.5), 0.05),
    "box-wide": ("box", (1.0, 0.25), 0.0),
    "box-2": ("box", (2.0, 2.0), 0.0),
}
# what the issue states of the tables: (nx, ny, floats behind f, staged in LDS)
FILTER_TABLES = {
    "gauss-64": (64, 64, 10483, False),
    "gauss-tall": (24, 80, 6695, False),
    "gauss-flat": (80, 24, 4721, True),
    "gauss-just-over": (48, 51, 6728, False),
    "gauss-max": (128, 128, None, False),
    "gauss-tiny": (16, 16, None, True),
    "gauss-needle": (48, 48, 6335, True),
}

PAIRS = ([(c, "box") for c in CAMERAS] + [("persp-roll", f) for f in FILTERS if f != "box"]
         + [("ortho-back", "gauss-64"), ("ortho-back", "box-wide")])
SAMPLERS = ("independent", "zsobol")
# the cases of the CPU sensitivity measurement
SENSITIVITY = ("persp-roll", "ortho-back", "persp-inside")


def pair_id(pair):
    return f"{pair[0]}+{pair[1]}"


# ---------------------------------------------------------------------------
# scenes

_density = None


def density():
    global _density
    if _density is None:
        _density = np.ascontiguousarray(
            0.2 + np.random.default_rng(2).random((GRID_N, GRID_N, GRID_N)), np.float32)
        _density.setflags(write=False)
    return _density


def film_size(camera):
    return CAMERAS[camera][1].get("film", (W, H))


def make_camera(camera, up=None):
    """The camera of a case; `up` replaces its up vector (a wrong formula of the CPU test)."""
    from acceleratedvolrenderer_amd import transform as xf
    from acceleratedvolrenderer_amd.scene import OrthographicCamera, PerspectiveCamera
    kind, kw = CAMERAS[camera]
    up = kw["up"] if up is None else up
    args = dict(screenwindow=kw.get("screenwindow"), frameaspectratio=kw.get("frameaspectratio"))
    if kw.get("mirror"):
        args["camera_from_world"] = np.diag([-1.0, 1.0, 1.0, 1.0]) @ xf.look_at(kw["pos"], kw["look"], up)
    else:
        args.update(pos=kw["pos"], look=kw["look"], up=up)
    if kind == "orthographic":
        return OrthographicCamera(**args)
    return PerspectiveCamera(fov=kw["fov"], **args)


def make_filter(name):
    from acceleratedvolrenderer_amd.scene import BoxFilter, GaussianFilter
    kind, radius, sigma = FILTERS[name]
    return BoxFilter(radius) if kind == "box" else GaussianFilter(radius, sigma)


def scene_for(camera, filt="box", sampler="independent", spp=SPP, cam=None):
    """The scene of a (camera, filter, sampler); `cam` replaces the camera object (the wrong
    formulas of the CPU test)."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import IndependentSampler, RGBFilm, Scene, ZSobolSampler
    base = scenes.s_uniform(n=GRID_N, width=W, height=H, variant="scatter", density=density())
    w, h = film_size(camera)
    smp = IndependentSampler(pixelsamples=spp) if sampler == "independent" else ZSobolSampler(pixelsamples=spp)
    return Scene(make_camera(camera) if cam is None else cam, RGBFilm(w, h, filter=make_filter(filt)), base.medium,
                 base.lights, sampler=smp, interface_sphere=CAMERAS[camera][1].get("sphere"))


# ---------------------------------------------------------------------------
# float64 geometry of the pixel-centre rays

def pixel_centre_rays(scene):
    """Render-space (o, d) of the rays through the pixel centres, row-major, float64."""
    f = scene.film
    y, x = np.mgrid[0:f.height, 0:f.width]
    pr = np.stack([x.ravel() + 0.5, y.ravel() + 0.5, np.zeros(x.size), np.ones(x.size)], 1)
    pc = pr @ np.asarray(scene.camera_from_raster, np.float64).T
    pc = pc[:, :3] / pc[:, 3:4]
    if int(scene.camera.type_id) == 0:
        o_c, d_c = pc, np.tile([0.0, 0.0, 1.0], (len(pc), 1))
    else:
        o_c, d_c = np.zeros_like(pc), pc / np.linalg.norm(pc, axis=1, keepdims=True)
    m = np.asarray(scene.render_from_camera, np.float64)
    return o_c @ m[:3, :3].T + m[:3, 3], d_c @ m[:3, :3].T


def hit_mask(scene):
    """Which pixel-centre rays cross the medium's box (t >= 0): a float64 slab test in medium space."""
    o, d = pixel_centre_rays(scene)
    mfr = np.asarray(scene.medium_from_render, np.float64)
    om, dm = o @ mfr[:3, :3].T + mfr[:3, 3], d @ mfr[:3, :3].T
    b = np.asarray(scene.medium.bounds, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (b[:3] - om) / dm, (b[3:] - om) / dm
    lo = np.nanmax(np.minimum(t0, t1), axis=1)
    hi = np.nanmin(np.maximum(t0, t1), axis=1)
    return np.maximum(lo, 0.0) < hi


# ---------------------------------------------------------------------------
# filter tables

def filter_table_size(name):
    """(nx, ny) of a Gaussian filter's FilterSampler tables: int(32 r) per axis."""
    _, (rx, ry), _ = FILTERS[name]
    return int(32 * np.float32(rx)), int(32 * np.float32(ry))


def filter_guide_k():
    """smp::kFilterGuideK as csrc/avr_sampling.h states it."""
    text = open(os.path.join(ROOT, "acceleratedvolrenderer_amd", "csrc", "avr_sampling.h")).read()
    return int(re.search(r"kFilterGuideK\s*=\s*(\d+)", text).group(1))


def filter_lds_limit():
    """kFiltLds as csrc/avr_kernels.hip states it: the floats of the staging buffer."""
    text = open(os.path.join(ROOT, "acceleratedvolrenderer_amd", "csrc", "avr_kernels.hip")).read()
    return int(re.search(r"constexpr\s+int\s+kFiltLds\s*=\s*(\d+)\s*;", text).group(1))


def filter_blob_floats(nx, ny, k=None):
    """smp::filter_blob_floats restated (tests/test_camera_cases_reference.py compares it with the
    header): tables | guide bytes padded to a float | cell weights."""
    k = filter_guide_k() if k is None else k
    tables = nx * ny + ny * (nx + 1) + ny + (ny + 1) + 1
    return tables + ((ny + 1) * (k + 1) + 3) // 4 + nx * ny


def filter_staged(name):
    """Whether stage_filter copies the filter's tables into LDS: the blob behind f fits kFiltLds
    floats. A box filter has no tables (None)."""
    if FILTERS[name][0] == "box":
        return None
    nx, ny = filter_table_size(name)
    return filter_blob_floats(nx, ny) - nx * ny <= filter_lds_limit()


def filter_branch(name):
    return {None: "no tables (box)", True: "tables in LDS", False: "tables in global memory"}[filter_staged(name)]


def gaussian_table(name):
    """The function table f (ny, nx) of avr_set_filter restated in float32 numpy, FastExp from the
    oracle: max(0, G(px) - G(rx)) max(0, G(py) - G(ry)) at the cell centres."""
    from oracle import binding
    _, (rx, ry), sigma = FILTERS[name]
    nx, ny = filter_table_size(name)
    f32 = np.float32
    L = binding.lib()

    def gauss(x):      # Gaussian(x, 0, sigma), util/math.h: 1 / sqrt(2 pi sigma^2) FastExp(-x^2 / (2 sigma^2))
        x, s = f32(x), f32(sigma)
        norm = f32(1) / f32(np.sqrt(f32(f32(2) * f32(np.pi)) * s * s))
        return f32(norm * f32(L.oracle_fastexp(float(f32(-(x * x)) / f32(f32(2) * s * s)))))

    def axis(n, r):
        r = f32(r)
        out = np.zeros(n, np.float32)
        for i in range(n):
            t = f32(f32(i + 0.5) / f32(n))
            p = f32(f32(f32(1) - t) * -r + t * r)
            out[i] = max(f32(0), f32(gauss(p) - gauss(r)))
        return out

    return np.outer(axis(ny, ry), axis(nx, rx)).astype(np.float32)


# ---------------------------------------------------------------------------
# the oracle's camera stage, per sample

def oracle_rays(run, width, height, first, ns):
    """OracleRun.camera_ray over sample indices [first, first + ns) in the last-pass layout (record
    s * npix + pix): o, d (n, 3), u (n), filter weight (n)."""
    npix = width * height
    o, d = np.zeros((ns * npix, 3), np.float32), np.zeros((ns * npix, 3), np.float32)
    u, w = np.zeros(ns * npix, np.float32), np.zeros(ns * npix, np.float32)
    for s in range(ns):
        for pix in range(npix):
            g = s * npix + pix
            o[g], d[g], u[g], _, w[g] = run.camera_ray(pix % width, pix // width, first + s)
    return o, d, u, w


def same_bits(a, b):
    """Per record: every float32 of a and b bit-identical."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    return (a.view(np.uint32) == b.view(np.uint32)).reshape(len(a), -1).all(axis=1)


# ---------------------------------------------------------------------------
# the reference's camera rays (tests/golden/camera_ray_vectors.json)

def harness_camera_lines():
    """The camera cases as oracle/ref/ref_harness --camera-rays reads them, one per line: name,
    type (0 orthographic, 1 perspective), fov, pos, look, up (3 each), mirror, has_window and the
    window (4), frame aspect ratio (0: the film's), film width and height."""
    lines = []
    for name, (kind, kw) in CAMERAS.items():
        w, h = film_size(name)
        sw = kw.get("screenwindow")
        vals = ([1 if kind == "perspective" else 0, kw.get("fov", 0.0)] + list(kw["pos"]) + list(kw["look"])
                + list(kw["up"]) + [1 if kw.get("mirror") else 0, 1 if sw else 0] + list(sw or (0, 0, 0, 0))
                + [kw.get("frameaspectratio") or 0.0, w, h])
        lines.append(name + " " + " ".join(repr(float(v)) for v in vals))
    return "\n".join(lines) + "\n"
