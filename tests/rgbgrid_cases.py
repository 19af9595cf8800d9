"""RGBGridMedium inputs made of real colours, shared by tests/test_rgbgrid_cases_reference.py
(CPU: the oracle and two numpy restatements against the reference's goldens) and
tests/test_gpu_rgbgrid.py (the device against the oracle) — TEST INFRASTRUCTURE, no device.

Every other RGB grid of the suite draws random sigmoid coefficients with c2 in [-5, 5] and a
scale in [0.2, 3]. Here the voxels are RGB colours converted on the host through pbrt's sRGB
table (tests/golden/srgb_table_subset_rgbgrid.npz holds the cells the palette touches):

  PALETTE  black {0, 0, -inf, 0}; greys (c0 = c1 = 0, so MaxValue's vertex wavelength is NaN or
           inf); the primaries and secondaries (the table's x = y = 0 edge); r == g != b; a
           1e-6 colour; (50, 20, 5); the HDR emission colour (30, 25, 18); two ordinary colours
  DIRECT   two coefficient voxels no colour produces but the ABI allows: c2 = +inf with a finite
           scale (the sigmoid's isinf branch gives 1), and a finite triple whose x is 9e19..6e20
           at every wavelength, so that 1 + x^2 overflows float32 and pbrt's sigmoid gives
           .5 + x / inf = 0.5 (util/color.h:356-360)

GRIDS (nz, ny, nx): (1,1,1), (2,3,5), (7,9,8), (5,17,33) drawn from the palette with a fixed
seed; "plume" (a coloured ball inside black, HDR emission), "black" (black everywhere),
"single" (one voxel that is not black), "direct" ((2,3,5) over the palette and DIRECT; not in
the reference's goldens, which take colours only). Each grid has three roles (sigma_a, sigma_s,
Le) with their own draws.

COMBOS: which grids the medium holds and the two scales. BOXES: the unit box at the origin with
the camera at the origin too (render space = medium space = grid space, so the goldens' unit-box
points are the probe points, bit for bit) and media_cases' "affine" box (rotation, non-uniform
scale, translation, three different extents: unit_box false).

probes(): per grid the unit-box points (voxel centres, lattice corners, points exactly on each
face, the half-voxel shell, points outside the box by less and by more than a voxel, seeded
interior points) and four different wavelengths each (360 and 830 exactly, values that round to
the table's ends, the vertex -c1 / (2 c0) of the voxel under the point when it lies in range,
random otherwise).

lookup64() is the float64 reference of SampledGrid<RGB*Spectrum>::Lookup(p, convert) and
tolerance its bound on a float32 evaluation; tests/test_rgbgrid_cases_reference.py derives it."""
import os
from collections import OrderedDict

import numpy as np

import media_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_FIXTURE = os.path.join(ROOT, "tests", "golden", "srgb_table_subset_rgbgrid.npz")
VECTORS = os.path.join(ROOT, "tests", "golden", "rgbgrid_vectors.json")

PALETTE = OrderedDict([
    ("black", (0.0, 0.0, 0.0)),
    ("grey0.01", (0.01, 0.01, 0.01)), ("grey0.5", (0.5, 0.5, 0.5)), ("grey1", (1.0, 1.0, 1.0)),
    ("grey7.5", (7.5, 7.5, 7.5)),
    ("red", (1.0, 0.0, 0.0)), ("green", (0.0, 1.0, 0.0)), ("blue", (0.0, 0.0, 1.0)),
    ("cyan", (0.0, 1.0, 1.0)), ("magenta", (1.0, 0.0, 1.0)), ("yellow", (1.0, 1.0, 0.0)),
    ("neargrey", (0.5, 0.5, 0.45)),
    ("tiny", (1e-6, 2e-6, 0.5e-6)),
    ("large", (50.0, 20.0, 5.0)),
    ("hdr", (30.0, 25.0, 18.0)),
    ("leaf", (0.2, 0.6, 0.3)), ("rust", (0.8, 0.35, 0.1)),
])
NAMES = list(PALETTE)
# {c0, c1, c2, scale}; indices len(PALETTE) and len(PALETTE) + 1 of a voxel-id array
DIRECT = np.array([(0.0, 0.0, np.inf, 1.5), (1e15, -2e17, 3e19, 0.8)], np.float32)

SHAPES = OrderedDict([("g111", (1, 1, 1)), ("g235", (2, 3, 5)), ("g798", (7, 9, 8)), ("g51733", (5, 17, 33)),
                      ("plume", (10, 12, 11)), ("black", (4, 5, 6)), ("single", (5, 6, 7)), ("direct", (2, 3, 5))])
GRIDS = list(SHAPES)
GOLDEN_GRIDS = [g for g in GRIDS if g != "direct"]
ROLES = ("a", "s", "Le")
COMBOS = ("a+s", "s", "a", "a+s+Le", "scale0", "Lescale0")
BOXES = ("unit", "affine")
GOLDEN_MAX_RES = ((4, 3, 2), (7, 5, 3))     # (rx, ry, rz) of the goldens' MaxValue cells
GOLDEN_LOOKUPS = 64                          # per grid

_F = np.float32


def palette_rgb():
    """(len(PALETTE), 3) float32."""
    return np.array(list(PALETTE.values()), np.float32)


_table = None


def table():
    """pbrt's sRGB RGBToSpectrumTable restricted to the cells the palette touches."""
    global _table
    if _table is None:
        from acceleratedvolrenderer_amd.rgbspectrum import RGBToSpectrumTable
        _table = RGBToSpectrumTable.load(TABLE_FIXTURE)
    return _table


def voxel_ids(grid, role):
    """(nz, ny, nx) indices into PALETTE (and, past it, DIRECT) of a grid's role."""
    shape = SHAPES[grid]
    seed = 1000 * GRIDS.index(grid) + ROLES.index(role)
    rng = np.random.default_rng(seed)
    idx = lambda name: NAMES.index(name)
    if grid == "black":
        return np.full(shape, idx("black"), np.int64)
    if grid == "single":
        ids = np.full(shape, idx("black"), np.int64)
        ids[2, 3, 4] = idx(("rust", "leaf", "hdr")[ROLES.index(role)])
        return ids
    if grid == "plume":
        z, y, x = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij")
        ball = (x - 0.5) ** 2 + (y - 0.45) ** 2 + (z - 0.5) ** 2 < 0.33 ** 2
        inside = {"a": ["rust", "leaf", "grey0.5", "magenta"], "s": ["grey7.5", "cyan", "leaf", "grey1", "yellow"],
                  "Le": ["hdr", "hdr", "large", "black"]}[role]
        ids = np.array([idx(n) for n in inside])[rng.integers(0, len(inside), shape)]
        return np.where(ball, ids, idx("black"))
    n = len(PALETTE) + (len(DIRECT) if grid == "direct" else 0)
    ids = rng.integers(0, n, shape)
    if grid == "direct":        # both DIRECT voxels in every role, next to black and to colours
        flat = ids.reshape(-1)
        flat[rng.permutation(flat.size)[:4]] = [n - 2, n - 1, idx("black"), n - 1]
    return ids


_coeffs = {}


def coeffs(grid, role):
    """(nz, ny, nx, 4) float32 {c0, c1, c2, scale} of a grid's role; computed once, read-only."""
    key = (grid, role)
    if key not in _coeffs:
        rows = np.concatenate([table().spectrum_coeffs(palette_rgb()), DIRECT]).astype(np.float32)
        c = np.ascontiguousarray(rows[voxel_ids(grid, role)], np.float32)
        c.setflags(write=False)
        _coeffs[key] = c
    return _coeffs[key]


def rgb(grid, role="a"):
    """(nz, ny, nx, 3) float32 colours of a grid without DIRECT voxels."""
    return palette_rgb()[voxel_ids(grid, role)]


# ---------------------------------------------------------------------------
# media and scenes

def medium_kwargs(grid, combo):
    a, s, le = (coeffs(grid, r) for r in ROLES)
    if combo == "a+s":
        return dict(sigma_a_coeffs=a, sigma_s_coeffs=s, scale=1.3)
    if combo == "s":
        return dict(sigma_s_coeffs=s, scale=1.3)          # sigma_a = 1 (media.h:386)
    if combo == "a":
        return dict(sigma_a_coeffs=a, scale=0.9)          # sigma_s = 1
    if combo == "a+s+Le":
        return dict(sigma_a_coeffs=a, sigma_s_coeffs=s, Le_coeffs=le, scale=1.3, Lescale=0.7)
    if combo == "scale0":
        return dict(sigma_a_coeffs=a, sigma_s_coeffs=s, Le_coeffs=le, scale=0.0, Lescale=0.7)
    if combo == "Lescale0":
        return dict(sigma_a_coeffs=a, sigma_s_coeffs=s, Le_coeffs=le, scale=1.3, Lescale=0.0)
    raise ValueError(combo)


def medium(grid, combo, box="unit", g=0.25, **override):
    from acceleratedvolrenderer_amd.scene import RGBGridMedium
    kw = medium_kwargs(grid, combo)
    kw.update(override)
    if box == "affine":
        p0, p1 = mc.box("affine")
        kw.update(p0=p0, p1=p1, world_from_medium=mc.transform("affine"))
    return RGBGridMedium(g=g, **kw)


def probe_scene(grid, combo, box, med=None):
    """The scene the point probes run in. "unit": the camera sits at the world origin, so
    render_from_medium is the identity and a render-space point is its grid coordinate."""
    from acceleratedvolrenderer_amd.scene import OrthographicCamera, RGBFilm, Scene
    med = medium(grid, combo, box) if med is None else med
    if box == "unit":
        cam = OrthographicCamera(pos=(0.0, 0.0, 0.0), look=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0),
                                 screenwindow=(-0.5, 0.5, -0.5, 0.5))
    else:
        cam = mc.camera_for(med)
    return Scene(cam, RGBFilm(8, 8), med, mc.default_lights())


def render_scene(grid, combo, g=0.25):
    """The replay scene: the unit box under the camera and lights of
    tests/test_gpu_parity.py::test_rgbgrid_medium_replay, 24 x 20 film."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import Scene
    base = scenes.s_uniform(n=1, width=24, height=20, variant="scatter")
    return Scene(base.camera, base.film, medium(grid, combo, g=g), base.lights)


# ---------------------------------------------------------------------------
# probes

def _unit_points(grid):
    """Unit-box float32 points of a grid, in the groups of the module docstring."""
    nz, ny, nx = SHAPES[grid]
    n = np.array([nx, ny, nz])
    rng = np.random.default_rng(7000 + GRIDS.index(grid))
    big = nx * ny * nz > 1500
    groups = []
    ax = [(np.arange(k) + 0.5) / k for k in n]
    centres = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    groups.append(centres[::5] if big else centres)
    lat = np.stack(np.meshgrid(*[np.arange(k + 1) / k for k in n], indexing="ij"), -1).reshape(-1, 3)
    groups.append(lat[::7] if big else lat)
    faces = []
    for axis in range(3):
        for side in (0.0, 1.0):
            q = rng.random((8, 3))
            q[:, axis] = side
            faces.append(q)
    groups.append(np.concatenate(faces))
    shell = rng.random((64, 3))
    k = rng.integers(0, 3, 64)
    d = rng.random(64) * 0.5 / n[k]
    shell[np.arange(64), k] = np.where(rng.random(64) < 0.5, d, 1.0 - d)
    groups.append(shell)
    out = rng.random((64, 3))
    k = rng.integers(0, 3, 64)
    # a hair outside, less than half a voxel outside (the edge voxels still weigh in), less than
    # one and a half (one tap plane left), and farther (every tap outside: exactly 0)
    d = np.choose(np.arange(64) % 4, [np.full(64, 1e-6), rng.random(64) * 0.5 / n[k], (0.5 + rng.random(64)) / n[k],
                                      (1.5 + rng.random(64)) / n[k]])
    out[np.arange(64), k] = np.where(rng.random(64) < 0.5, -d, 1.0 + d)
    groups.append(out)
    groups.append(rng.random((256, 3)))
    return np.concatenate(groups).astype(np.float32)


def _wavelengths(grid, u):
    """(n, 4) float32, four different wavelengths per probe."""
    rng = np.random.default_rng(8000 + GRIDS.index(grid))
    n = len(u)
    lam = (360 + 470 * rng.random((n, 4))).astype(np.float32)
    i = np.arange(n)
    lam[i % 8 == 0, 0] = 360.0
    lam[i % 8 == 0, 1] = 830.0
    ends = np.array([[360.4, 360.5, 829.5, 829.6], [360.49, 829.51, 361.5, 828.5]], np.float32)
    lam[i % 8 == 1] = ends[(i[i % 8 == 1] // 8) % 2]
    # the vertex of the voxel under the point, per role in turn
    nz, ny, nx = SHAPES[grid]
    v = np.clip(np.floor(u.astype(np.float64) * [nx, ny, nz]).astype(np.int64), 0, [nx - 1, ny - 1, nz - 1])
    for k, role in enumerate(ROLES):
        c = coeffs(grid, role)[v[:, 2], v[:, 1], v[:, 0]]
        with np.errstate(divide="ignore", invalid="ignore"):
            vert = (-c[:, 1] / (_F(2) * c[:, 0])).astype(np.float32)
        use = (i % 8 == 2) & (vert >= 360) & (vert <= 830)
        lam[use, k] = vert[use]
    for r in np.nonzero([len(set(row)) < 4 for row in lam.tolist()])[0]:      # four different ones
        lam[r] = np.sort(lam[r]) + np.arange(4, dtype=np.float32) * _F(0.25)
        lam[r] = np.minimum(lam[r], _F(830) - np.arange(3, -1, -1, dtype=np.float32) * _F(0.25))
    return lam


_probes = {}


def probes(grid):
    """(u (n, 3) unit-box float32 points, lam (n, 4)) of a grid; computed once, read-only."""
    if grid not in _probes:
        u = _unit_points(grid)
        lam = _wavelengths(grid, u)
        u.setflags(write=False)
        lam.setflags(write=False)
        _probes[grid] = (u, lam)
    return _probes[grid]


def golden_probes(grid):
    """The GOLDEN_LOOKUPS probes of a grid that the reference evaluates: an even stride."""
    u, lam = probes(grid)
    k = np.linspace(0, len(u) - 1, GOLDEN_LOOKUPS).astype(np.int64)
    return u[k], lam[k]


def render_points(scene, u):
    """Render-space float32 points of unit-box points u: exactly u in the "unit" probe scene; behind
    a transform the float64 image of the box point, rounded (its float32 grid coordinates are
    grid_coordinates(scene, p), a few ulps from u). The points exactly on a face are then moved by
    up to 8 ulps of each render coordinate to land on grid coordinate 0 or 1 exactly where such a
    float exists."""
    b = np.asarray(scene.medium.bounds, np.float64)
    rfm = np.asarray(scene.render_from_medium, np.float64)
    u = np.asarray(u, np.float32)
    p = mc.apply(rfm, b[:3] + u.astype(np.float64) * (b[3:] - b[:3])).astype(np.float32)
    if np.array_equal(np.asarray(scene.render_from_medium, np.float32), np.eye(4, dtype=np.float32)) and \
            np.array_equal(b, [0, 0, 0, 1, 1, 1]):
        return np.ascontiguousarray(u)
    want = (u == 0) | (u == 1)
    steps = np.arange(-8, 9, dtype=np.float32)
    ulp = np.spacing(np.abs(p)).astype(np.float32)
    for r in np.nonzero(want.any(axis=1))[0]:
        axis = int(np.argmax(want[r]))
        d = np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), -1).reshape(-1, 3)
        d = d[np.argsort(np.abs(d).sum(axis=1), kind="stable")]          # the nearest candidates first
        cand = (p[r] + d * ulp[r]).astype(np.float32)
        hit = np.nonzero(mc.grid_coordinates32(scene, cand)[:, axis] == u[r, axis])[0]
        if len(hit):
            p[r] = cand[hit[0]]
    return np.ascontiguousarray(p)


def grid_coordinates(scene, p):
    """The float32 grid coordinates sample_point hands to the lookup."""
    return mc.grid_coordinates32(scene, p)


# ---------------------------------------------------------------------------
# the float64 reference and its tolerance

U = 2.0 ** -24
SQRT_FLT_MAX = float(np.sqrt(np.float64(np.finfo(np.float32).max)))


def _sigmoid64(x):
    """pbrt's sigmoid in float64 with the two float32 behaviours that are results, not errors:
    +-inf gives 1 / 0, and |x| > sqrt(FLT_MAX) gives 0.5 (1 + x^2 overflows: x / inf = 0)."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = 0.5 + x / (2 * np.sqrt(1 + x * x))
    s = np.where(np.abs(x) > SQRT_FLT_MAX, 0.5, s)
    return np.where(np.isinf(x), np.where(x > 0, 1.0, 0.0), s)


def lookup64(c4, u32, lam, illuminant=None):
    """SampledGrid<RGB*Spectrum>::Lookup(p, convert) at float32 grid coordinates u32 (n, 3) and
    wavelengths lam (n, 4): the voxel offsets and lerp weights are the lookup's own float32 ones
    (p * n - .5, floor, difference), everything after them float64 from the float32 coefficients.
    Returns (value (n, 4), M (n, 4) the largest tap scale [times the illuminant], cond (n, 4) the
    largest tap's polynomial term of tolerance())."""
    nz, ny, nx, _ = c4.shape
    c = np.asarray(c4, np.float64)
    u32 = np.asarray(u32, np.float32)
    ps = (u32 * np.array([nx, ny, nz], np.float32)).astype(np.float32) - _F(0.5)
    fl = np.floor(ps)
    t = (ps - fl).astype(np.float32).astype(np.float64)
    i = fl.astype(np.int64)
    lam64 = np.asarray(lam, np.float32).astype(np.float64)
    ill = np.ones_like(lam64)
    if illuminant is not None:
        off = np.floor(lam64 + 0.5).astype(np.int64) - 360            # lround of a positive float
        ill = np.where((off < 0) | (off >= 471), 0.0, np.asarray(illuminant, np.float64)[np.clip(off, 0, 470)])
    M = np.zeros_like(lam64)
    cond = np.zeros_like(lam64)

    def tap(dx, dy, dz):
        nonlocal M, cond
        x, y, z = i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz
        ok = (x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (z >= 0) & (z < nz)
        v = c[np.clip(z, 0, nz - 1), np.clip(y, 0, ny - 1), np.clip(x, 0, nx - 1)]
        c0, c1, c2, sc = (v[:, k, None] for k in range(4))
        with np.errstate(invalid="ignore", over="ignore"):
            xx = (c0 * lam64 + c1) * lam64 + c2
            P = np.abs(c0) * lam64 * lam64 + np.abs(c1) * lam64 + np.abs(c2)
            dxx = 2 * P * U
            near = np.maximum(np.abs(xx) - dxx, 0.0)
            slope = 0.5 / (1 + near * near) ** 1.5
            term = np.where(np.isfinite(xx), np.minimum(slope * dxx, 1.0), 0.0)
        scale = np.where(ok[:, None], sc * ill, 0.0)
        val = np.where(scale == 0, 0.0, scale * _sigmoid64(xx))
        M = np.maximum(M, scale)
        cond = np.maximum(cond, np.where(scale == 0, 0.0, term))
        return val

    lerp = lambda s, a, b: a * (1 - s[:, None]) + b * s[:, None]
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    d00 = lerp(tx, tap(0, 0, 0), tap(1, 0, 0))
    d10 = lerp(tx, tap(0, 1, 0), tap(1, 1, 0))
    d01 = lerp(tx, tap(0, 0, 1), tap(1, 0, 1))
    d11 = lerp(tx, tap(0, 1, 1), tap(1, 1, 1))
    return lerp(tz, lerp(ty, d00, d10), lerp(ty, d01, d11)), M, cond


def tolerance(M, cond, out_scale):
    """|float32 lookup - lookup64| <= out_scale * M * (cond + 16 * 2^-24); derived in
    tests/test_rgbgrid_cases_reference.py."""
    return abs(float(out_scale)) * M * (cond + 16 * U)


def reference(scene, p, lam):
    """((sigma_a, sigma_s, Le), (tol_a, tol_s, tol_Le)) float64 (n, 4) of RGBGridMedium::SamplePoint
    at render-space points p: lookup64 at the float32 grid coordinates, times the medium's scales."""
    med = scene.medium
    u32 = grid_coordinates(scene, p)
    vals, tols = [], []
    n = len(p)
    for g, sc, ill in ((med.rgb_sigma_a, med.sigma_scale, None), (med.rgb_sigma_s, med.sigma_scale, None),
                       (med.rgb_Le, med.Le_scale, med.illuminant)):
        sc = float(sc)
        if ill is not None and (g is None or not sc > 0):      # IsEmissive (media.h:374)
            vals.append(np.zeros((n, 4)))
            tols.append(np.zeros((n, 4)))
        elif g is None:                                        # a missing sigma grid is 1
            vals.append(np.full((n, 4), float(_F(sc))))
            tols.append(np.zeros((n, 4)))
        else:
            v, M, cond = lookup64(g, u32, lam, ill)
            vals.append(sc * v)
            tols.append(tolerance(M, cond, sc))
    if med.rgb_Le is None:
        vals[2], tols[2] = np.zeros((n, 4)), np.zeros((n, 4))
    return tuple(vals), tuple(tols)


def cell_majorant(scene, p, maj, res):
    """The majorant of the cell holding each render-space point ((n,) float64; NaN outside the box):
    MajorantGrid's x + rx (y + ry z) over the float32 grid coordinates. A point within 4 ulps of
    a cell boundary lies in both cells (their float32 bounds x / rx are rounded too): it gets the
    larger majorant."""
    u = grid_coordinates(scene, p).astype(np.float64)
    r = np.asarray(res, np.int64)
    maj = np.asarray(maj, np.float64)
    inside = ((u >= 0) & (u <= 1)).all(axis=1)
    eps = 4 * 2.0 ** -23
    out = np.full(len(u), -np.inf)
    for sx in (-eps, eps):
        for sy in (-eps, eps):
            for sz in (-eps, eps):
                c = np.clip(np.floor((u + [sx, sy, sz]) * r).astype(np.int64), 0, r - 1)
                out = np.maximum(out, maj[c[:, 0] + r[0] * (c[:, 1] + r[1] * c[:, 2])])
    return np.where(inside, out, np.nan)


# ---------------------------------------------------------------------------
# the reference harness's input (oracle/ref/ref_harness.cpp --rgb-grid)

def _bits(a):
    return " ".join(str(int(v)) for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def harness_lines():
    lines = []
    for grid in GOLDEN_GRIDS:
        nz, ny, nx = SHAPES[grid]
        u, lam = golden_probes(grid)
        lines.append(f"grid {grid} {nx} {ny} {nz} {_bits(rgb(grid))}")
        lines.append(f"lambda {len(lam)} {_bits(lam)}")
        lines.append(f"look {grid} {len(u)} {_bits(u)}")
        for rx, ry, rz in GOLDEN_MAX_RES:
            lines.append(f"max {grid} {rx} {ry} {rz}")
    return "\n".join(lines) + "\n"


# ---------------------------------------------------------------------------
# one (grid, combo, box): scene, probes, the canonical oracle's SamplePoint, the float64 reference

_cases = {}
_points = {}


def case(grid, combo, box):
    """{"scene", "run" (canonical OracleRun), "p", "lam", "oracle" (sigma_a, sigma_s, Le), "ref", "tol"};
    computed once."""
    key = (grid, combo, box)
    if key not in _cases:
        from oracle import binding
        scene = probe_scene(grid, combo, box)
        u, lam = probes(grid)
        if (grid, box) not in _points:          # the geometry does not depend on the combination
            _points[grid, box] = render_points(scene, u)
        p = _points[grid, box]
        run = binding.OracleRun(scene, max_depth=5, seed=0, libm="canonical")
        ref, tol = reference(scene, p, lam)
        _cases[key] = dict(scene=scene, run=run, p=p, lam=lam, oracle=run.medium_sample(p, lam), ref=ref, tol=tol)
    return _cases[key]


ALL_CASES = [(g, c, b) for g in GRIDS for c in COMBOS for b in BOXES]
