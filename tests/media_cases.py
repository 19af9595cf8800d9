"""Media behind a transform and a box that is not the unit cube, shared by
tests/test_media_cases_reference.py (CPU: the oracle against float64 numpy) and
tests/test_gpu_media_mapping.py (the device against the oracle) — TEST INFRASTRUCTURE, no device.

Four boxes:
  affine           world_from_medium = R_y(25) R_x(-40) diag(0.8, 1.3, 0.6), translation
                   (0.45, 0.1, 0.35); box (-0.3, 0.1, 0.2)-(0.4, 1.2, 0.5): three different
                   extents, none a power of two, behind a rotation and a non-uniform scale
  scaled           diag(0.8, 1.3, 0.6) and the same translation, no rotation: axis-parallel rays
                   keep exact zeros in medium space; the same box
  unit-off-origin  identity; p0 = 0.1, p1 = 1.1 on every axis: the float extent is exactly 1.0f, so
                   the unit-box shortcut runs with bmin != 0
  one-axis-off     unit-off-origin with p1.x one float up: extent 1 on two axes only, so the
                   general Bounds3::Offset must run
One 7 x 9 x 12 grid (nx, ny, nz) for all of them, 0.2 + random + 2 x: the gradient along grid x
alone makes an axis mix-up change every line integral. Majorant grid (5, 8, 3).

The orthographic camera of every scene looks down +z at the world bounding box of the medium's
box, through a window MARGIN times that box: 40-90 % of the pixel-centre rays cross the medium
(test_media_cases_reference.py checks it in float64)."""
import numpy as np

W, H, SPP, MAXDEPTH = 24, 20, 8, 6
NPIX = W * H
SHAPE = (12, 9, 7)            # (nz, ny, nx)
MAJORANT_RES = (5, 8, 3)
CASES = ("affine", "scaled", "unit-off-origin", "one-axis-off")
MARGIN = 1.12

# the media rendered over "affine"; the other boxes take the first two
GRID_KINDS = ("gray", "chromatic", "emissive", "temperature")
AFFINE_KINDS = GRID_KINDS + ("rgbgrid", "rgbgrid_emissive", "homogeneous", "cloud", "nanovdb", "gray_sphere")
REPLAY = [("affine", k) for k in AFFINE_KINDS] + [(c, k) for c in CASES[1:] for k in ("gray", "chromatic")]

# the interface sphere of "gray_sphere", world space. The rotated box's world centre is
# (0.325, 0.882, -0.013) with half extents 0.28, 0.715 and 0.09 along its own axes: its long axis
# leaves the sphere at both ends, the short ones lie inside
SPHERE = ((0.35, 0.8, 0.0), 0.45)


def _rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.eye(4)
    i, j = {"x": (1, 2), "y": (2, 0)}[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def transform(case):
    """world_from_medium (4 x 4, float64)."""
    m = np.eye(4)
    if case in ("affine", "scaled"):
        m = np.diag([0.8, 1.3, 0.6, 1.0])
        if case == "affine":
            m = _rot("y", 25.0) @ _rot("x", -40.0) @ m
        m[:3, 3] = (0.45, 0.1, 0.35)
    return m


def box(case):
    """(p0, p1) float32."""
    if case in ("affine", "scaled"):
        return np.array((-0.3, 0.1, 0.2), np.float32), np.array((0.4, 1.2, 0.5), np.float32)
    p0, p1 = np.full(3, 0.1, np.float32), np.full(3, 1.1, np.float32)
    if case == "one-axis-off":
        p1[0] = np.nextafter(np.float32(1.1), np.float32(2))
    return p0, p1


def unit_box_predicate(p0, p1):
    """DevMedium::unit_box as the host evaluates it: every float32 extent exactly 1."""
    p0, p1 = np.asarray(p0, np.float32), np.asarray(p1, np.float32)
    return bool(np.all((p1 - p0).astype(np.float32) == np.float32(1)))


_density = None


def density():
    """0.2 + random + 2 x over the (12, 9, 7) grid; computed once."""
    global _density
    if _density is None:
        nz, ny, nx = SHAPE
        x = np.linspace(0.0, 1.0, nx, dtype=np.float32)
        d = np.float32(0.2) + np.random.default_rng(41).random(SHAPE, dtype=np.float32) + np.float32(2) * x
        _density = np.ascontiguousarray(d, np.float32)
        _density.setflags(write=False)
    return _density


def _coords():
    nz, ny, nx = SHAPE
    return np.meshgrid(np.linspace(0, 1, nz, dtype=np.float32), np.linspace(0, 1, ny, dtype=np.float32),
                       np.linspace(0, 1, nx, dtype=np.float32), indexing="ij")


def _rgb_coeffs(rng, scale_hi):
    """Random RGBSigmoidPolynomial coefficients per voxel; the scale carries the x gradient."""
    z, y, x = _coords()
    c = np.empty(SHAPE + (4,), np.float32)
    c[..., 0] = rng.uniform(-2e-5, 2e-5, SHAPE)
    c[..., 1] = rng.uniform(-0.02, 0.02, SHAPE)
    c[..., 2] = rng.uniform(-5, 5, SHAPE)
    c[..., 3] = rng.uniform(0.2, scale_hi, SHAPE) * (0.3 + 1.4 * x)
    return c


def vdb_index_to_world():
    """The rotated index_to_world of tests/test_gpu_parity.py::_vdb_scene (n = 20)."""
    n = 20
    c, s = np.cos(np.radians(25)), np.sin(np.radians(25))
    m = np.eye(4)
    m[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([0.8 / n, 1.0 / n, 0.7 / n])
    m[:3, 3] = [0.25, 0.0, 0.15]
    return m


def _vdb_density():
    rng = np.random.default_rng(12)
    n = 20
    d = np.zeros((n, n, n), np.float32)
    d[3:17, 2:18, 4:16] = (0.2 + rng.random((14, 16, 12))).astype(np.float32)
    d[8:16, 8:16, 0:8] = 0.8
    return d


def medium(case, kind, g=None, absorber=False, density_override=None):
    """The medium `kind` in the box of `case`. g overrides the kind's own g; absorber: sigma_a of that value
    (True: 1), sigma_s 0, over the GridMedium; density_override: another grid of SHAPE."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import (CloudMedium, GridMedium, HomogeneousMedium, NanoVDBMedium,
                                                  RGBGridMedium)
    p0, p1 = box(case)
    geo = dict(p0=p0, p1=p1, world_from_medium=transform(case))
    dens = density() if density_override is None else np.ascontiguousarray(density_override, np.float32)
    ramp = np.linspace(0.0, 1.0, 471, dtype=np.float32)
    z, y, x = _coords()

    def gg(default):
        return default if g is None else g

    if absorber:
        return GridMedium(dens, sigma_a=float(absorber), sigma_s=0.0, g=0.0, majorant_res=MAJORANT_RES, **geo)
    if kind in ("gray", "gray_sphere"):
        return GridMedium(dens, sigma_a=0.5, sigma_s=4.0, g=gg(0.3), majorant_res=MAJORANT_RES, **geo)
    if kind == "chromatic":
        return GridMedium(dens, sigma_a=(0.2 + ramp).astype(np.float32), sigma_s=(4.5 - 3.0 * ramp).astype(np.float32),
                          g=gg(-0.2), majorant_res=MAJORANT_RES, **geo)
    if kind == "emissive":
        les = (2.0 * x * (1.0 - y) + 0.25 * z).astype(np.float32)
        return GridMedium(dens, sigma_a=0.6, sigma_s=3.0, g=gg(-0.2), Le=(0.5 + ramp * ramp).astype(np.float32),
                          Lescale=les, majorant_res=MAJORANT_RES, **geo)
    if kind == "temperature":
        temp = (50 + 4000 * x * (1 - y) + 300 * z).astype(np.float32)       # includes cells below 100 K
        return GridMedium(dens, sigma_a=(0.5 + ramp).astype(np.float32), sigma_s=1.5, g=gg(0.2), temperature=temp,
                          temperaturescale=1.1, temperatureoffset=20.0, majorant_res=MAJORANT_RES, **geo)
    if kind in ("rgbgrid", "rgbgrid_emissive"):
        rng = np.random.default_rng(43)
        kw = dict(sigma_a_coeffs=_rgb_coeffs(rng, 0.8), sigma_s_coeffs=_rgb_coeffs(rng, 4.0))
        if kind == "rgbgrid_emissive":
            kw.update(Le_coeffs=_rgb_coeffs(rng, 2.0), Lescale=0.7)
        return RGBGridMedium(g=gg(0.25), scale=1.3, **kw, **geo)
    if kind == "homogeneous":
        return HomogeneousMedium(sigma_a=0.5, sigma_s=4.0, g=gg(0.3), **geo)
    if kind == "cloud":
        return CloudMedium(sigma_a=0.1, sigma_s=6.0, g=gg(0.6), **geo)
    if kind == "nanovdb":
        grid = scenes.vdb_grid(_vdb_density(), index_to_world=vdb_index_to_world())
        return NanoVDBMedium(grid, world_from_medium=transform(case), sigma_a=0.5, sigma_s=2.0, g=gg(0.3))
    raise ValueError(kind)


def camera_for(med, margin=MARGIN):
    """An orthographic camera down +z, one unit before the world bounding box of the medium's box,
    through a window `margin` times that box."""
    from acceleratedvolrenderer_amd.scene import OrthographicCamera
    b = np.asarray(med.bounds, np.float64)
    c = np.array([[x, y, z, 1.0] for x in (b[0], b[3]) for y in (b[1], b[4]) for z in (b[2], b[5])])
    w = (np.asarray(med.world_from_medium, np.float64) @ c.T).T[:, :3]
    lo, hi = w.min(axis=0), w.max(axis=0)
    mid = (lo + hi) / 2
    hx, hy = margin * (hi[0] - lo[0]) / 2, margin * (hi[1] - lo[1]) / 2
    return OrthographicCamera(pos=(mid[0], mid[1], lo[2] - 1.0), look=(mid[0], mid[1], lo[2]), up=(0.0, 1.0, 0.0),
                              screenwindow=(-hx, hx, -hy, hy))


def default_lights():
    from acceleratedvolrenderer_amd.scene import DistantLight, UniformInfiniteLight
    return [DistantLight(from_=(-1.0, 1.0, -1.0), to=(0.0, 0.0, 0.0), scale=2.0), UniformInfiniteLight(scale=0.25)]


# the axis-parallel lights: `from` of a DistantLight pointing at the origin
AXIS_LIGHTS = {"+y": (0.0, 1.0, 0.0), "-y": (0.0, -1.0, 0.0), "+x": (1.0, 0.0, 0.0), "-z": (0.0, 0.0, -1.0)}


def axis_lights(name):
    from acceleratedvolrenderer_amd.scene import DistantLight, UniformInfiniteLight
    return [DistantLight(from_=AXIS_LIGHTS[name], to=(0.0, 0.0, 0.0), scale=2.0), UniformInfiniteLight(scale=0.25)]


def scene_for(case, kind, g=None, lights=None, width=W, height=H, med=None):
    """The scene of a (case, kind): 24 x 20 box-filter film, independent sampler."""
    from acceleratedvolrenderer_amd.scene import RGBFilm, Scene
    med = medium(case, kind, g=g) if med is None else med
    sphere = SPHERE if kind == "gray_sphere" else None
    return Scene(camera_for(med), RGBFilm(width, height), med, default_lights() if lights is None else lights,
                 interface_sphere=sphere)


def identity_scene(kind, g=None, lights=None):
    """The unit box at the origin with no transform (the suite's usual mapping) over the same grid:
    the control of the g and light-axis edges."""
    from acceleratedvolrenderer_amd.scene import GridMedium, HomogeneousMedium, RGBFilm, Scene
    if kind == "homogeneous":
        med = HomogeneousMedium(sigma_a=0.5, sigma_s=4.0, g=0.3 if g is None else g)
    else:
        med = GridMedium(density(), sigma_a=0.5, sigma_s=4.0, g=0.3 if g is None else g, majorant_res=MAJORANT_RES)
    return Scene(camera_for(med), RGBFilm(W, H), med, default_lights() if lights is None else lights)


# ---------------------------------------------------------------------------
# float64 geometry

def apply(m, p):
    """Points p (n, 3) through the 4 x 4 (or 3 x 4) affine m, float64."""
    m = np.asarray(m, np.float64)
    return np.asarray(p, np.float64) @ m[:3, :3].T + m[:3, 3]


def camera_rays(scene):
    """Render-space origins and the common direction of the orthographic pixel-centre rays, float64."""
    f = scene.film
    px, py = np.meshgrid(np.arange(f.width) + 0.5, np.arange(f.height) + 0.5)
    ras = np.stack([px.ravel(), py.ravel(), np.zeros(px.size)], axis=1)
    o = apply(scene.render_from_camera, apply(scene.camera_from_raster, ras))
    d = np.asarray(scene.render_from_camera, np.float64)[:3, :3] @ np.array([0.0, 0.0, 1.0])
    return o, d


def slab_hits(scene, o, d):
    """Which rays o + t d (render space, t >= 0) cross the medium's box: a float64 slab test in
    medium space."""
    mfr = np.asarray(scene.medium_from_render, np.float64)
    om = apply(mfr, o)
    dm = np.broadcast_to(mfr[:3, :3] @ np.asarray(d, np.float64), om.shape)
    b = np.asarray(scene.medium.bounds, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (b[:3] - om) / dm
        t1 = (b[3:] - om) / dm
    lo = np.nanmax(np.minimum(t0, t1), axis=1)
    hi = np.nanmin(np.maximum(t0, t1), axis=1)
    return (np.maximum(lo, 0.0) < hi)


def interior_segments(scene, q, rng, lo=0.1, hi=0.9):
    """q segments with both ends inside the box (fractions lo..hi of it): render-space float32
    (p0, p1) and their medium-space fractions."""
    b = np.asarray(scene.medium.bounds, np.float64)
    fa, fb = rng.uniform(lo, hi, (q, 3)), rng.uniform(lo, hi, (q, 3))
    rfm = np.asarray(scene.render_from_medium, np.float64)
    p0 = apply(rfm, b[:3] + fa * (b[3:] - b[:3])).astype(np.float32)
    p1 = apply(rfm, b[:3] + fb * (b[3:] - b[:3])).astype(np.float32)
    return p0, p1


def np_trilinear64(dens, u):
    """SampledGrid::Lookup restated in float64 for unit-cube points u (n, 3): zero outside."""
    nz, ny, nx = dens.shape
    d64 = np.asarray(dens, np.float64)
    ps = np.asarray(u, np.float64) * np.array([nx, ny, nz], np.float64) - 0.5
    fl = np.floor(ps)
    t = ps - fl
    i = fl.astype(np.int64)

    def at(x, y, z):
        ok = (x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (z >= 0) & (z < nz)
        return np.where(ok, d64[np.clip(z, 0, nz - 1), np.clip(y, 0, ny - 1), np.clip(x, 0, nx - 1)], 0.0)

    x, y, z = i[:, 0], i[:, 1], i[:, 2]
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    lerp = lambda s, a, b: (1 - s) * a + s * b
    d00 = lerp(tx, at(x, y, z), at(x + 1, y, z))
    d10 = lerp(tx, at(x, y + 1, z), at(x + 1, y + 1, z))
    d01 = lerp(tx, at(x, y, z + 1), at(x + 1, y, z + 1))
    d11 = lerp(tx, at(x, y + 1, z + 1), at(x + 1, y + 1, z + 1))
    return lerp(tz, lerp(ty, d00, d10), lerp(ty, d01, d11))


def optical_depth(scene, p0, p1, sigma_t, steps=2000, wrong=None):
    """tau of Integrator::Tr's segment p0 -> p1 (render space) through a GridMedium, float64:
    sigma_t times the midpoint-rule integral of the trilinear density over the render-space length
    (1 - 1e-4) |p1 - p0| (Tr's ray stops ShadowEpsilon short). `wrong` breaks the mapping on purpose
    for the tests that show the check has teeth: "swap_xy" reads the grid with x and y swapped,
    "no_scale" maps with the rotation and translation alone, "normalised" measures the length in
    medium space as if the medium-space direction were normalised."""
    med = scene.medium
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    mfr = np.asarray(scene.medium_from_render, np.float64)
    if wrong == "no_scale":
        rfm = np.asarray(scene.render_from_medium, np.float64)
        lin = rfm[:3, :3]
        col = np.linalg.norm(lin, axis=0)
        rot = np.eye(4)
        rot[:3, :3] = lin / col
        rot[:3, 3] = rfm[:3, 3]
        mfr = np.linalg.inv(rot)
    b = np.asarray(med.bounds, np.float64)
    length = np.linalg.norm(p1 - p0, axis=1) * (1 - 1e-4)
    if wrong == "normalised":
        length = np.linalg.norm(apply(mfr, p1) - apply(mfr, p0), axis=1) * (1 - 1e-4)
    s = (np.arange(steps) + 0.5) / steps * (1 - 1e-4)
    tau = np.zeros(len(p0))
    for k in range(0, len(p0), 250):
        a, c = p0[k:k + 250], p1[k:k + 250]
        pr = a[:, None, :] + s[None, :, None] * (c - a)[:, None, :]
        u = (apply(mfr, pr.reshape(-1, 3)) - b[:3]) / (b[3:] - b[:3])
        if wrong == "swap_xy":
            u = u[:, [1, 0, 2]]
        tau[k:k + 250] = np_trilinear64(med.density, u).reshape(len(a), steps).mean(axis=1)
    return sigma_t * tau * length


def mean_bound(expect, q):
    """4 sd of the mean of q estimates in [0, 1] with expectations `expect`: the Bernoulli variance
    E (1 - E) bounds that of any such estimate, so the bound is conservative for ratio tracking."""
    return 4 * np.sqrt(np.mean(expect * (1 - expect)) / q)


# ---------------------------------------------------------------------------
# Integrator::Tr queries

def random_segments(scene, q, rng):
    """q render-space float32 segments whose ends lie in the box enlarged by 15 % on every side:
    inside to inside, outside to inside, and clean misses."""
    return interior_segments(scene, q, rng, lo=-0.15, hi=1.15)


def axis_segments(scene, q, rng):
    """q segments parallel to a RENDER axis (two components of p1 - p0 exactly zero), for a medium
    whose transform keeps the axes ("scaled"): the medium-space direction then holds exact zeros."""
    p0, p1 = random_segments(scene, q, rng)
    axis = rng.integers(0, 3, q)
    keep = np.arange(3)[None, :] == axis[:, None]
    p1 = np.where(keep, p1, p0).astype(np.float32)
    flip = rng.random(q) < 0.5                      # both signs of the direction, -0 never: 0 - 0 = +0
    return np.where(flip[:, None], p1, p0).astype(np.float32), np.where(flip[:, None], p0, p1).astype(np.float32)


def medium_coordinate32(mfr, axis, p):
    """The medium-space coordinate `axis` of render-space points p (n, 3) as xf_ray and
    xf_point_pair group it in float32: (m0 x + m1 y) + (m2 z + m3)."""
    m = np.asarray(mfr, np.float32)[axis]
    p = np.asarray(p, np.float32)
    return ((m[0] * p[:, 0] + m[1] * p[:, 1]).astype(np.float32) + (m[2] * p[:, 2] + m[3]).astype(np.float32)).astype(
        np.float32)


def on_face(scene, axis, side):
    """A render-space float32 coordinate along `axis` that the float32 transform maps EXACTLY onto
    the box's face (side 0: pMin, 1: pMax), for a transform that keeps the axes; None if the
    16 floats around the float64 solution all miss it."""
    mfr = np.asarray(scene.medium_from_render, np.float32)
    face = np.float32(scene.medium.bounds[3 * side + axis])
    x = np.float32((np.float64(face) - np.float64(mfr[axis, 3])) / np.float64(mfr[axis, axis]))
    cands = [x]
    for k in range(8):
        cands.append(np.nextafter(cands[-1], np.float32(np.inf)))
    lo = x
    for k in range(8):
        lo = np.nextafter(lo, np.float32(-np.inf))
        cands.append(lo)
    for c in cands:
        p = np.zeros((1, 3), np.float32)
        p[0, axis] = c
        # the other two coordinates multiply exact zeros of the matrix
        if medium_coordinate32(mfr, axis, p)[0] == face:
            return np.float32(c)
    return None


def face_segments(scene, rng, per_face=18):
    """Segments that start exactly on a face of the box or run inside a face plane, for a transform
    that keeps the axes. Per face found (on_face; not every face has such a float): a third that start on it and end
    inside the box, a third inside its plane (one direction component exactly zero, the origin on the slab plane: 0 *
    inf in Bounds3::IntersectP), a third inside its plane and parallel to an axis (two zeros)."""
    lin = np.asarray(scene.medium_from_render, np.float32)[:3, :3]
    assert np.count_nonzero(lin) == 3, "face_segments needs a transform that keeps the axes"
    p0s, p1s = [], []
    for axis in range(3):
        for side in (0, 1):
            c = on_face(scene, axis, side)
            if c is None:
                continue
            a, b = interior_segments(scene, per_face, rng, lo=0.05, hi=0.95)
            a[:, axis] = c
            k = per_face // 3
            b[k:, axis] = c                       # in plane
            other = (axis + 1) % 3
            b[2 * k:, other] = a[2 * k:, other]   # and parallel to the third axis
            p0s.append(a)
            p1s.append(b)
    return np.concatenate(p0s).astype(np.float32), np.concatenate(p1s).astype(np.float32)


def same_bits_or_nan(a, b):
    """Elementwise: bit-identical float32, or both NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------
# The two mean checks of Integrator::Tr, shared by the CPU test (the oracle's estimates) and the
# device test (avr_transmittance's): scene, segments, float64 expectation and bound, computed once

Q = 4000
LINE_SIGMA = 2.0
_means = {}


def absorber_scene(case, ones):
    """An absorber over the box of `case`: density exactly 1 with sigma_a 1 (Beer-Lambert), or
    the gradient grid with sigma_a LINE_SIGMA (the line integral)."""
    dens = np.ones(SHAPE, np.float32) if ones else None
    med = medium(case, "gray", absorber=True if ones else LINE_SIGMA, density_override=dens)
    return scene_for(case, "gray", med=med)


def query_lambda(q=Q):
    return np.full((q, 4), 550.0, np.float32)


def beer_lambert_case(case):
    """(scene, p0, p1, expect): density 1 away from the half-voxel shell (1 / 14 of the box along
    x, ends at 0.1 .. 0.9), expect = exp(-(1 - 1e-4) |p1 - p0|) over the render-space distance."""
    key = ("beer", case)
    if key not in _means:
        scene = absorber_scene(case, ones=True)
        p0, p1 = interior_segments(scene, Q, np.random.default_rng(51))
        dist = np.linalg.norm(p1.astype(np.float64) - p0.astype(np.float64), axis=1) * (1 - 1e-4)
        _means[key] = (scene, p0, p1, np.exp(-dist))
    return _means[key]


def line_integral_case(case, wrong=None):
    """(scene, p0, p1, expect) of the heterogeneous absorber, expect = exp(-tau) from
    optical_depth with 2000 steps. The segments run mostly along grid x, at low y: an x / y swap
    then reads thinner density, and x and z are the axes whose medium-space lengths exceed the
    render-space ones (scales 0.8 and 0.6), so a distance measured in medium space is too long."""
    key = ("line", case, wrong)
    if key not in _means:
        scene = absorber_scene(case, ones=False)
        p0, p1 = interior_segments(scene, Q, np.random.default_rng(52), lo=(0.3, 0.15, 0.1), hi=(0.95, 0.25, 0.9))
        _means[key] = (scene, p0, p1, np.exp(-optical_depth(scene, p0, p1, LINE_SIGMA, steps=2000, wrong=wrong)))
    return _means[key]


def assert_mean(tr, expect, label):
    """|mean(tr) - mean(expect)| <= mean_bound; prints the figures first."""
    tr = np.asarray(tr, np.float64)
    bound = mean_bound(expect, len(expect))
    print(f"{label}: Tr mean {tr.mean():.4f} vs {expect.mean():.4f} (bound {bound:.4f})")
    assert abs(tr.mean() - expect.mean()) <= bound


# ---------------------------------------------------------------------------
# The float32 mapping of a render-space point to grid coordinates, as sample_point groups it

def grid_coordinates32(scene, p):
    """xf_point_pair(medium_from_render, p) then Bounds3::Offset (the general branch: subtract
    pMin, divide by the extent), float32, for points p (n, 3)."""
    b = np.asarray(scene.medium.bounds, np.float32)
    pm = np.stack([medium_coordinate32(scene.medium_from_render, a, p) for a in range(3)], axis=1)
    return ((pm - b[:3]).astype(np.float32) / (b[3:] - b[:3]).astype(np.float32)).astype(np.float32)


def grid_coordinates64(scene, p):
    b = np.asarray(scene.medium.bounds, np.float64)
    return (apply(scene.medium_from_render, np.asarray(p, np.float64)) - b[:3]) / (b[3:] - b[:3])


def mapping_error_ulps(scene, p, u):
    """The largest error of float32 grid coordinates u of render-space points p against the float64
    mapping, in ulps (2^-23) of S / extent, S = sum_j |m_ij p_j| + |m_i3| + |pMin_i| the magnitude
    the sums run over (cancellation makes the result itself smaller). Each coordinate is three
    products, three sums, a subtraction and a division, every one rounded once: a faithful float32
    evaluation stays below 4."""
    p = np.asarray(p, np.float64)
    m = np.asarray(scene.medium_from_render, np.float64)
    b = np.asarray(scene.medium.bounds, np.float64)
    S = np.abs(p) @ np.abs(m[:3, :3]).T + np.abs(m[:3, 3]) + np.abs(b[:3])
    err = np.abs(np.asarray(u, np.float64) - grid_coordinates64(scene, p))
    return float((err / (S / (b[3:] - b[:3]))).max() / 2.0 ** -23)


def row_order(a):
    """The permutation that puts the rows of a float32 (n, 3) array in lexicographic order of
    their bits."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1, 3)
    return np.lexsort((b[:, 2], b[:, 1], b[:, 0]))


def sorted_rows(a):
    """The rows of a float32 (n, 3) array as uint32, in that order: a multiset to compare."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1, 3)[row_order(a)]


def trace_queries():
    """(scene, p0, p1, lam) of the lookup-trace comparison: 300 segments inside the affine box, gray
    scattering grid (sigma_t 4.5: about ten lookups per query)."""
    scene = scene_for("affine", "gray")
    rng = np.random.default_rng(81)
    p0, p1 = interior_segments(scene, 300, rng, lo=0.02, hi=0.98)
    return scene, p0, p1, (360 + 470 * rng.random((300, 4))).astype(np.float32)


# ---------------------------------------------------------------------------
# The lighting-graph tools' scene

def graph_scene():
    """The gray GridMedium (g 0.3) in the affine box with the grid's first five z layers empty, so
    that the (5, 8, 3) majorant has an empty z cell and rays that cross only empty cells exist;
    one distant light, 4 spp (the recipe of tests/test_gpu_graph_voxels.py::_scene)."""
    from acceleratedvolrenderer_amd.scene import GridMedium, IndependentSampler, RGBFilm, Scene
    d = density().copy()
    d[:5] = 0
    p0, p1 = box("affine")
    med = GridMedium(d, p0=p0, p1=p1, world_from_medium=transform("affine"), sigma_a=0.4, sigma_s=6.0, g=0.3,
                     majorant_res=MAJORANT_RES)
    return Scene(camera_for(med), RGBFilm(16, 16), med, default_lights()[:1], sampler=IndependentSampler(pixelsamples=4))
