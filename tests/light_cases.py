"""The light stage under the maps, transforms, parameters and light lists it accepts, shared by
tests/test_light_cases_reference.py (CPU: the oracle and scene.py against the reference's own
functions, the conditions on the inputs) and tests/test_gpu_lights.py (the device against the
oracle) — TEST INFRASTRUCTURE, no device.

Every other image-light test uses one 32 x 32 gradient with a 3 x 3 spot, untransformed or rotated
about y, and D65 lights without illuminance. Here, over one medium (the unit box, a 6^3 random
scattering grid, the camera of scenes.s_uniform, film 20 x 12, 8 samples per pixel, maxdepth 6):

  MAPS        res 1 (what "rgb L" on an infinite light builds), a constant map (the all-zero ->
              ones fallback of the compensated distribution), two surviving pixels (whole rows of
              the marginal zero), a black lower hemisphere (Le and the map pdf both zero), negative
              pixels (clamped for Le, raw in the sampling average), an odd resolution with a
              bright block around the square's centre. Non-grey pixels come from one PALETTE of
              eight colours, so the colour table fixture stays small.
  TRANSFORMS  identity, a rotation about a skew axis, a mirrored one (determinant -1), uniform
              scales, a shear.
  DISTANT     world_from_light, illuminance and L of DistantLight and UniformInfiniteLight.
  LISTS       two image lights, eight lights, an image light past the k_paths LDS records, the
              power sampler with a zero-Phi light, with all weights zero, with one light.
  PAIRS       every map under "rot-axis", every transform on "corners-5", every list."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_PATH = os.path.join(ROOT, "tests", "golden", "srgb_table_subset_lights.npz")

W, H, SPP, MAXDEPTH = 20, 12, 8, 6
GRID_N = 6

# the only non-grey pixel values of every map (two of them with a negative channel)
PALETTE = np.array([
    [30.0, 25.0, 18.0],      # 0 bright warm
    [4.0, 9.0, 22.0],        # 1 bright blue
    [0.8, 0.3, 0.2],         # 2
    [0.2, 0.7, 0.3],         # 3
    [0.25, 0.3, 0.9],        # 4
    [0.9, 0.8, 0.2],         # 5
    [-0.3, 0.6, 0.4],        # 6 negative red
    [0.5, -0.2, 0.7],        # 7 negative green
], np.float32)


def _pattern(res, colours=(2, 3, 4, 5)):
    y, x = np.mgrid[0:res, 0:res]
    return PALETTE[np.asarray(colours)[(x + 2 * y) % len(colours)]].astype(np.float32)


def _square_z_sign(res):
    """The sign of z of EqualAreaSquareToSphere at the pixel centres: 1 - (|2u - 1| + |2v - 1|)."""
    c = (np.arange(res) + 0.5) / res
    uu, vv = np.meshgrid(2 * c - 1, 2 * c - 1)
    return 1 - (np.abs(uu) + np.abs(vv))


def _rgb_1():
    return PALETTE[2].reshape(1, 1, 3).copy()


def _const_4():
    return np.full((4, 4, 3), 0.5, np.float32)


def _corners_5():
    img = np.full((5, 5, 3), 0.05, np.float32)
    img[0, 0] = PALETTE[0]
    img[4, 4] = PALETTE[1]
    return img


def _half_black_8():
    img = _pattern(8)
    img[_square_z_sign(8) < 0] = 0
    return img


def _negative_6():
    img = _pattern(6)
    img[1, 2] = img[4, 0] = PALETTE[6]
    img[2, 5] = img[5, 3] = PALETTE[7]
    return img


def _pole_33():
    img = _pattern(33)
    img[15:17, 15:17] = PALETTE[0]      # around the square's centre (16.5, 16.5): the +z pole
    img[16, 16] = PALETTE[1]
    return img


MAPS = {"rgb-1": _rgb_1, "const-4": _const_4, "corners-5": _corners_5, "half-black-8": _half_black_8,
        "negative-6": _negative_6, "pole-33": _pole_33}


def map_image(name):
    img = np.ascontiguousarray(MAPS[name](), np.float32)
    img.setflags(write=False)
    return img


def _rot_axis():
    from acceleratedvolrenderer_amd import transform as xf
    return xf.rotate(50.0, (1.0, 2.0, 3.0))


def transform(name):
    """world_from_light (4 x 4, float64) of a named transform."""
    from acceleratedvolrenderer_amd import transform as xf
    if name == "identity":
        return np.eye(4)
    if name == "rot-axis":
        return _rot_axis()
    if name == "mirror":
        return np.diag([-1.0, 1.0, 1.0, 1.0]) @ _rot_axis()
    if name == "scale-2":
        return xf.scale(2.0, 2.0, 2.0) @ _rot_axis()
    if name == "scale-half":
        return xf.scale(0.5, 0.5, 0.5) @ _rot_axis()
    if name == "shear":
        m = np.eye(4)
        m[:3, :3] = [[1.0, 0.3, 0.0], [0.0, 1.0, 0.2], [0.1, 0.0, 1.0]]
        return m
    if name == "nonuniform":
        return xf.scale(3.0, 1.0, 0.5)
    raise KeyError(name)


TRANSFORMS = ("identity", "rot-axis", "mirror", "scale-2", "scale-half", "shear")
# transforms that do not keep lengths: the render pairs under them use g = 0 (SampleLi returns an
# unnormalised wi, and HenyeyGreenstein would be evaluated at |cos theta| > 1)
UNNORMALISED = ("scale-2", "scale-half", "shear")

# name -> ("distant" | "uniform", transform or None, keywords)
DISTANT = {
    "distant-rot": ("distant", "rot-axis", dict(scale=1.5)),
    "distant-mirror": ("distant", "mirror", dict(scale=1.0)),
    "distant-nonuniform": ("distant", "nonuniform", dict(scale=1.0)),
    "distant-illuminance": ("distant", None, dict(from_=(1.0, 1.0, -1.0), to=(0.0, 0.0, 0.0), illuminance=250.0,
                                                  scale=0.01)),
    "distant-bb3200": ("distant", None, dict(from_=(-1.0, 1.0, -1.0), to=(0.0, 0.0, 0.0), L=("blackbody", 3200.0),
                                             scale=2.0)),
    "distant-const": ("distant", None, dict(from_=(0.2, -1.0, -0.5), to=(0.0, 0.0, 0.0), L=0.7, scale=1.0)),
    "uniform-bb6500": ("uniform", None, dict(L=("blackbody", 6500.0), illuminance=40.0, scale=0.02)),
    "uniform-d65": ("uniform", None, dict(scale=0.25)),
    "uniform-const": ("uniform", None, dict(L=0.7, scale=0.2)),
    "uniform-zero": ("uniform", None, dict(scale=0.0)),
    "distant-zero": ("distant", None, dict(from_=(-1.0, 1.0, -1.0), to=(0.0, 0.0, 0.0), scale=0.0)),
    "distant-base": ("distant", None, dict(from_=(-1.0, 1.0, -1.0), to=(0.0, 0.0, 0.0), scale=2.0)),
}

# name -> (light specs, light sampler, index of the light under test). A light spec is a DISTANT
# name or ("image", map, transform, keywords).
LISTS = {
    "two-images": ([("image", "corners-5", "mirror", {}), ("image", "pole-33", "identity", {})], "bvh", 1),
    "eight": (["distant-rot", "distant-mirror", "distant-nonuniform", "uniform-bb6500", "uniform-d65",
               "distant-bb3200", "uniform-const", ("image", "half-black-8", "rot-axis", {})], "bvh", 7),
    "image-slot-5": (["distant-illuminance", "uniform-d65", "distant-const", "uniform-const", "distant-rot",
                      ("image", "negative-6", "rot-axis", dict(illuminance=3.0))], "bvh", 5),
    # the zero-Phi light comes first: in the middle its bin aliases to the image light and the other
    # two keep their ranges of u, so that removing it would leave every pick, and the film, as it was
    "power-zero-phi": (["uniform-zero", "distant-base", ("image", "half-black-8", "identity", {})], "power", 0),
    "power-all-zero": (["distant-zero", "uniform-zero", ("image", "const-4", "identity", dict(scale=0.0))], "power", 2),
    "power-one": ([("image", "half-black-8", "mirror", dict(illuminant=("blackbody", 5000.0)))], "power", 0),
}

MAP_PAIRS = [(m, "rot-axis") for m in MAPS] + [("corners-5", t) for t in TRANSFORMS if t != "rot-axis"]
PAIRS = [f"{m}+{t}" for m, t in MAP_PAIRS] + list(LISTS)
ZSOBOL_PAIRS = ("two-images", "eight", "corners-5+mirror")
# every light of "power-all-zero" is black, as the case is defined: the film is black with or
# without any of them and the all-zero -> ones alias table is the uniform pick, so neither the
# share condition nor a mutation can tell anything there (light stage)
BLACK = ("power-all-zero",)


def is_list(case):
    return case in LISTS


def split_pair(case):
    m, t = case.split("+")
    return m, t


# ---------------------------------------------------------------------------
# lights and scenes

_table = None


def table():
    """The palette's cells of the sRGB RGBToSpectrumTable (tests/golden/make_srgb_subset.py)."""
    global _table
    if _table is None:
        from acceleratedvolrenderer_amd import RGBToSpectrumTable
        _table = RGBToSpectrumTable.load(TABLE_PATH)
    return _table


def _spectrum(L):
    from acceleratedvolrenderer_amd import spectra
    if isinstance(L, tuple) and L[0] == "blackbody":
        return spectra.blackbody(L[1])
    return L


def make_light(spec, rgb_table=None, transpose=False):
    """The light of a spec; `transpose` swaps the map's axes (a wrong formula of the CPU test)."""
    from acceleratedvolrenderer_amd.scene import DistantLight, ImageInfiniteLight, UniformInfiniteLight
    if isinstance(spec, tuple):
        _, m, t, kw = spec
        kw = {k: _spectrum(v) if k == "illuminant" else v for k, v in kw.items()}
        img = np.array(map_image(m))
        if transpose:
            img = np.ascontiguousarray(img.transpose(1, 0, 2))
        return ImageInfiniteLight(image=img, rgb_table=table() if rgb_table is None else rgb_table,
                                  world_from_light=transform(t), **kw)
    kind, t, kw = DISTANT[spec]
    kw = dict(kw)
    if "L" in kw:
        kw["L"] = _spectrum(kw["L"])
    if kind == "uniform":
        return UniformInfiniteLight(**kw)
    return DistantLight(world_from_light=None if t is None else transform(t), **kw)


def case_lights(case):
    """(light specs, light sampler, index of the light under test, g) of a case."""
    if is_list(case):
        specs, sampler, under_test = LISTS[case]
        return list(specs), sampler, under_test, 0.3
    m, t = split_pair(case)
    return ["distant-base", ("image", m, t, {})], "bvh", 1, 0.0 if t in UNNORMALISED else 0.3


_density = None


def density():
    global _density
    if _density is None:
        _density = np.ascontiguousarray(
            0.2 + np.random.default_rng(2).random((GRID_N, GRID_N, GRID_N)), np.float32)
        _density.setflags(write=False)
    return _density


def scene_for(case, sampler="independent", spp=SPP, drop=None, transpose=False, rgb_table=None):
    """The scene of a case; `drop` removes one light, `transpose` transposes every map."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import GridMedium, IndependentSampler, RGBFilm, Scene, ZSobolSampler
    specs, _, _, g = case_lights(case)
    lights = [make_light(s, rgb_table=rgb_table, transpose=transpose) for i, s in enumerate(specs) if i != drop]
    base = scenes.s_uniform(n=GRID_N, width=W, height=H, variant="scatter", density=density())
    med = GridMedium(density(), sigma_a=0.5, sigma_s=2.0, g=g)
    smp = IndependentSampler(pixelsamples=spp) if sampler == "independent" else ZSobolSampler(pixelsamples=spp)
    return Scene(base.camera, RGBFilm(W, H), med, lights, sampler=smp)


def light_sampler(case):
    return case_lights(case)[1]


def image_indices(scene):
    return [i for i, l in enumerate(scene.lights) if l.type_id == 2]


def expected_kernel_is_image(scene, sampler):
    """Whether k_paths runs its image instantiation: an image light or the power sampler."""
    return bool(image_indices(scene)) or sampler == "power"


def oracle_run(case, libm="canonical", seed=0, sampler="independent", lightsampler=None, swap=False, variant=0,
               **scene_kw):
    """(scene, OracleRun) of a case. The wrong formulas of the sensitivity condition: `swap`
    exchanges renderFromLight and lightFromRender, `variant` is OracleScene.light_variant (1 the
    uncompensated distribution, 2 res off by one in the lookup), `lightsampler` replaces the
    case's own (the BVH pick's bins under a power case), transpose=True transposes the maps."""
    from oracle import binding
    scene = scene_for(case, sampler=sampler, **scene_kw)
    run = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=seed, libm=libm,
                            lightsampler=light_sampler(case) if lightsampler is None else lightsampler)
    if swap:
        for i in image_indices(scene):
            a, b = list(run.s.light_rfl[i]), list(run.s.light_lfr[i])
            run.s.light_rfl[i][:] = b
            run.s.light_lfr[i][:] = a
    run.s.light_variant = int(variant)
    return scene, run


MUTATIONS = {
    "rfl-lfr-swapped": dict(swap=True),
    "uncompensated": dict(variant=1),
    "transposed": dict(transpose=True),
    "res-off-by-one": dict(variant=2),
    "bvh-bins": dict(lightsampler="bvh"),
}


def same_bits(a, b):
    """Per record: every float32 of a and b bit-identical."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    return (a.view(np.uint32) == b.view(np.uint32)).reshape(len(a), -1).all(axis=1)


def exact_fraction(got, want):
    """The share of samples whose L, lambda, pdf and filter weight are all bit-identical."""
    ok = np.ones(len(want[0]), bool)
    for a, b in zip(got, want):
        ok &= same_bits(np.asarray(a, np.float32).reshape(len(ok), -1), np.asarray(b, np.float32).reshape(len(ok), -1))
    return float(ok.mean())


# ---------------------------------------------------------------------------
# the compensated distribution restated (numpy float32, the reference's order)

def compensated(light):
    """ImageInfiniteLight's compensated sampling function (lights.cpp:1026-1038): d - average
    (a double sum, rounded to float) clamped at zero; all zero -> ones."""
    d = np.asarray(light.distribution, np.float32)
    avg = np.float32(d.astype(np.float64).reshape(-1).cumsum()[-1] / d.size)
    c = np.maximum(d - avg, np.float32(0)).astype(np.float32)
    if not c.any():
        c[:] = 1
    return c


def _cdf(f):
    """PiecewiseConstant1D's cdf over [0, 1] (util/sampling.h:617-637): (normalised cdf, funcInt)."""
    n = len(f)
    cdf = np.zeros(n + 1, np.float32)
    for i in range(1, n + 1):
        cdf[i] = np.float32(cdf[i - 1] + np.float32(np.float32(abs(f[i - 1])) * np.float32(1)) / np.float32(n))
    func_int = cdf[n]
    if func_int == 0:
        cdf[1:] = (np.arange(1, n + 1, dtype=np.float32) / np.float32(n)).astype(np.float32)
    else:
        cdf[1:] = (cdf[1:] / func_int).astype(np.float32)
    return cdf, func_int


def distribution_cdfs(light):
    """(marginal cdf, [conditional cdf per row], row integrals) of the compensated distribution."""
    c = compensated(light)
    rows = [_cdf(r) for r in c]
    ints = np.array([fi for _, fi in rows], np.float32)
    return _cdf(ints)[0], [cd for cd, _ in rows], ints


# ---------------------------------------------------------------------------
# probe inputs: at most 1024 per avr_light_probe call ("pole-33" has 1213 (u0, u1): two calls)

ONE_MINUS_EPS = np.float32(1) - np.float32(2.0 ** -24)
SPECIAL_U = np.array([0.0, 2.0 ** -24, 0.5, ONE_MINUS_EPS], np.float32)
MAX_PROBE = 1024


def _around(values):
    """Every value of a float32 array in [0, 1) with one ulp either side, kept inside [0, 1)."""
    v = np.asarray(values, np.float32)
    out = np.concatenate([v, np.nextafter(v, np.float32(-1)), np.nextafter(v, np.float32(2))]).astype(np.float32)
    return np.unique(out[(out >= 0) & (out < 1)])


def probe_u(light):
    """(u0, u1) pairs for SampleLi: 0, 2^-24, 0.5 and 1 - 2^-24 in either component, every marginal
    CDF breakpoint (with u0 from the special values) and, per non-zero row, every conditional
    breakpoint with a u1 that selects the row, each with one ulp either side."""
    marg, cond, ints = distribution_cdfs(light)
    pairs = [(a, b) for a in SPECIAL_U for b in SPECIAL_U]
    for b in _around(marg):
        pairs += [(a, b) for a in SPECIAL_U]
    rows = [v for v in range(len(ints)) if ints[v] != 0]
    for v in rows:
        b = np.float32((np.float64(marg[v]) + np.float64(marg[v + 1])) / 2)
        pairs += [(a, b) for a in _around(cond[v])]
    return np.ascontiguousarray(np.array(pairs, np.float32).reshape(-1, 2))


def square_to_sphere(u, v):
    """EqualAreaSquareToSphere in float64 (util/math.cpp:292-318)."""
    uu, vv = 2 * u - 1, 2 * v - 1
    up, vp = abs(uu), abs(vv)
    sd = 1 - (up + vp)
    d = abs(sd)
    r = 1 - d
    phi = (1 if r == 0 else (vp - up) / r + 1) * np.pi / 4
    z = np.copysign(1 - r * r, sd)
    s = r * np.sqrt(max(0.0, 2 - r * r))
    return np.array([np.copysign(np.cos(phi), uu) * s, np.copysign(np.sin(phi), vv) * s, z])


def probe_directions(res, render_from_light, n_random=256, seed=11):
    """Render-space directions for PDF_Li and Le of a map of resolution res: the axes, the equator
    diagonals, eight with a -0.0 or denormal component, the images of the square's corners, edge points and the pixel
    corners on its edges (exact in light space under the identity), random ones."""
    s = np.sqrt(0.5)
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
            (s, s, 0), (-s, s, 0), (s, -s, 0), (-s, -s, 0)]
    den = 1e-40
    dirs += [(-0.0, 1, 0), (1, -0.0, 0), (0, 1, -0.0), (-0.0, -0.0, 1), (den, 1, 0), (1, -den, 0), (0, -1, den),
             (-den, den, -1)]
    ticks = sorted({0.0, 1.0, 0.5} | {k / res for k in range(res + 1)})
    if len(ticks) > 12:
        ticks = ticks[:: len(ticks) // 12 + 1] + [1.0]
    m = np.asarray(render_from_light, np.float64)[:3, :3]
    for t in ticks:
        for (u, v) in ((0.0, t), (1.0, t), (t, 0.0), (t, 1.0)):
            w = m @ square_to_sphere(u, v)
            dirs.append(tuple(w / np.linalg.norm(w)))
    rng = np.random.default_rng(seed)
    r = rng.normal(size=(n_random, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([np.array(dirs, np.float64), r]), np.float32)


def probe_lambdas(n, seed=12):
    """n wavelength sets: the ends of the range, a half-integer wavelength, then random."""
    rng = np.random.default_rng(seed)
    lam = (360 + 470 * rng.random((n, 4))).astype(np.float32)
    lam[0] = [360.0, 830.0, 555.5, 470.25]
    lam[1] = [830.0, 830.0, 360.0, 360.0]
    lam[2] = [555.5, 360.00003, 829.99994, 600.0]
    return np.ascontiguousarray(np.clip(lam, 360, 830), np.float32)


PICK_U = np.unique(np.concatenate([
    SPECIAL_U, _around(np.arange(0, 9, dtype=np.float32) / np.float32(8)),
    _around(np.arange(0, 4, dtype=np.float32) / np.float32(3)),
    np.random.default_rng(13).random(200).astype(np.float32)])).astype(np.float32)


# ---------------------------------------------------------------------------
# the reference's light stage (tests/golden/light_vectors.json)

ALIAS_WEIGHTS = {
    "equal": [1.0, 1.0, 1.0],
    "one-zero": [2.0, 0.0, 5.0],
    "all-zero": [0.0, 0.0, 0.0],
    "one-entry": [3.0],
    "eight-1e6": [1e-3, 1.0, 10.0, 1e3, 0.5, 2.0, 100.0, 1e-2],
}
PHOTOMETRIC = {"d65": ("d", 0.0), "blackbody-3200": ("b", 3200.0), "blackbody-6500": ("b", 6500.0), "constant-0.7": ("c", 0.7)}


def alias_draws(n):
    """The draws of the alias goldens: the special values and the bin edges k / n with one ulp either side."""
    edges = _around(np.arange(0, n + 1, dtype=np.float32) / np.float32(n))
    return np.unique(np.concatenate([SPECIAL_U, edges])).astype(np.float32)


# The golden file holds part of each light's probes (the reference pins the oracle there; the device
# is compared with the oracle at all of them): per map at most GOLDEN_U (u0, u1) for Sample / PDF,
# per (map, transform) pair GOLDEN_PAIR_U of those for SampleLi and about 80 directions.
GOLDEN_U, GOLDEN_PAIR_U, GOLDEN_RANDOM = 160, 48, 16


def golden_u(light):
    """Of probe_u's pairs: the 16 pairs of special values, every marginal breakpoint with its
    neighbours one ulp away (u0 = 0.5), and the conditional breakpoint probes of the non-zero rows,
    all of them where they fit GOLDEN_U (every map but "pole-33": 45 of its 801, spread evenly)."""
    u = probe_u(light)
    n_marg = len(_around(distribution_cdfs(light)[0]))
    marg = [16 + 4 * k + 2 for k in range(n_marg)]           # SPECIAL_U[2] = 0.5
    first = 16 + 4 * n_marg
    room = GOLDEN_U - 16 - n_marg
    cond = list(range(first, len(u))) if len(u) - first <= room else [int(i) for i in np.linspace(first, len(u) - 1, room)]
    return np.ascontiguousarray(u[list(range(16)) + marg + cond])


def golden_pair_u(light):
    """GOLDEN_PAIR_U of golden_u's pairs, spread evenly over specials, marginal and conditional ones."""
    u = golden_u(light)
    return np.ascontiguousarray(u[np.unique(np.linspace(0, len(u) - 1, min(len(u), GOLDEN_PAIR_U)).astype(int))])


def golden_directions(res, render_from_light):
    """probe_directions with its first GOLDEN_RANDOM random directions: every special direction
    (axes, diagonals, signed zeros, denormals) and every edge and corner point of the square."""
    return probe_directions(res, render_from_light, n_random=GOLDEN_RANDOM)


def map_light(name, xform="identity"):
    return make_light(("image", name, xform, {}))


def _bits(a):
    return " ".join(str(int(v)) for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def harness_light_lines():
    """The cases as oracle/ref/ref_harness --lights reads them (its header comment has the format):
    floats as uint32 bits."""
    scene = scene_for("rgb-1+rot-axis")
    cam = -np.asarray(scene.render_from_world, np.float64)[:3, 3]
    lines = ["cam " + _bits(cam), "lambda 4 " + _bits(probe_lambdas(4))]
    for name in MAPS:
        img = map_image(name)
        lines.append(f"map {name} {img.shape[0]} " + _bits(img))
        u = golden_u(map_light(name))
        lines.append(f"u {name} {len(u)} " + _bits(u))
    for t in TRANSFORMS + ("nonuniform",):
        lines.append(f"xf {t} " + _bits(transform(t)))
    for m, t in MAP_PAIRS:
        sc = scene_for(f"{m}+{t}")
        u = golden_pair_u(sc.lights[1])
        d = golden_directions(sc.lights[1].res, sc.light_rfl[1])
        lines.append(f"pair {m} {t} {len(u)} " + _bits(u) + f" {len(d)} " + _bits(d))
    for name, w in ALIAS_WEIGHTS.items():
        u = alias_draws(len(w))
        lines.append(f"alias {name} {len(w)} " + _bits(w) + f" {len(u)} " + _bits(u))
    for name, (kind, value) in PHOTOMETRIC.items():
        lines.append(f"photometric {name} {kind} {value!r}")
    for name, (kind, t, kw) in DISTANT.items():
        if kind == "distant":
            ft = list(kw.get("from_", (0.0, 0.0, 0.0))) + list(kw.get("to", (0.0, 0.0, 1.0)))
            lines.append(f"distant {name} {t or '-'} " + _bits(ft))
    return "\n".join(lines) + "\n"
