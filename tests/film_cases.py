"""The film configurations that tests/test_film_reference.py (CPU: film_ref against the oracle,
clamp shares) and tests/test_gpu_film.py (k_film against both) share — TEST INFRASTRUCTURE.

One scene for every case: 20 x 16 pixels (one full block of 256 and a ragged one of 64), a
10^3 emissive chromatic grid, maxdepth 6, seed 0. The overflow cases use the medium of
tests/test_gpu_edges.py::test_film_nan_inf_guard_with_overflowing_radiance instead."""
import numpy as np

W, H, MAXDEPTH, SEED = 20, 16, 6, 0
NPIX = W * H
NARROW = dict(lambdamin=400.0, lambdamax=700.0)

# name -> (film class name, film keywords, spp)
CASES = {
    # RGBFilm sensor scale: imagingRatio = exposureTime * ISO / 100; 250 / 3 / 100 is no power of two
    "rgb_iso320_t0.25": ("RGBFilm", dict(iso=320.0, exposure_time=0.25), 7),
    "rgb_iso250_t0.333": ("RGBFilm", dict(iso=250.0, exposure_time=1.0 / 3.0), 7),
    # RGBFilm clamp: alone, and behind the sensor scale of iso 250. The exposure time of the second
    # is the 1 / 3 s of the scale case above (ratio 0.8333: the clamp fires on 42 % of samples);
    # at 1 s the ratio 2.5 would put 0.35 below the first quartile (87 %, outside the 20-80 % cap)
    "rgb_clamp": ("RGBFilm", dict(maxcomponentvalue=0.35), 7),
    "rgb_clamp_iso250": ("RGBFilm", dict(maxcomponentvalue=0.35, iso=250.0, exposure_time=1.0 / 3.0), 7),
    # SpectralFilm clamps: 0.35 the sensor-RGB clamp only, 0.0035 the L clamp too
    "spec_clamp_rgb": ("SpectralFilm", dict(maxcomponentvalue=0.35, **NARROW), 7),
    "spec_clamp_L": ("SpectralFilm", dict(maxcomponentvalue=0.0035, **NARROW), 7),
    "spec17_clamp_L": ("SpectralFilm", dict(nbuckets=17, maxcomponentvalue=0.0035, **NARROW), 7),
}
# SpectralFilm bucket paths: 1, 16 (the last count in LDS), 17 (the first in HBM), 40; spp 3 is
# the batch tail alone, 7 one batch of 4 and a tail of 3; 1 and 17 on 400-700 nm, 16 and 40 on
# the 360-830 nm default
for _nb in (1, 16, 17, 40):
    for _spp in (3, 7):
        CASES[f"spec_nb{_nb}_spp{_spp}"] = ("SpectralFilm", dict(nbuckets=_nb, **(NARROW if _nb in (1, 17) else {})),
                                            _spp)

# the clamps a case is there to exercise: each must fire on 20 % .. 80 % of its samples
RGB_CLAMP_CASES = ("rgb_clamp", "rgb_clamp_iso250", "spec_clamp_rgb")
L_CLAMP_CASES = ("spec_clamp_L", "spec17_clamp_L")
L_CLAMP_IDLE_CASES = ("spec_clamp_rgb",)

# overflow with a finite clamp: inf * (1e30 / inf) = NaN, the finite components 0
OVERFLOW_W, OVERFLOW_H, OVERFLOW_SPP, OVERFLOW_MAXDEPTH = 24, 16, 4, 4
OVERFLOW_CASES = {
    "overflow_rgb": ("RGBFilm", dict(maxcomponentvalue=1e30)),
    "overflow_spec": ("SpectralFilm", dict(maxcomponentvalue=1e30)),
}


def make_film(kind, kw, width=W, height=H):
    from acceleratedvolrenderer_amd import scene as sc
    return getattr(sc, kind)(width, height, **kw)


def scene_for(name):
    """(scene, spp) of a CASES entry."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import Scene
    kind, kw, spp = CASES[name]
    base = scenes.s_uniform(n=10, width=W, height=H, variant="emissive_chromatic",
                            density=(0.3 + 0.7 * np.random.default_rng(8).random((10, 10, 10), dtype=np.float32)))
    return Scene(base.camera, make_film(kind, kw), base.medium, base.lights), spp


def overflow_scene_for(name):
    """(scene, spp) of an OVERFLOW_CASES entry: Lescale 1e26 .. 1e38 along x."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import GridMedium, Scene
    kind, kw = OVERFLOW_CASES[name]
    n = 8
    dens = (0.5 + np.random.default_rng(11).random((n, n, n), dtype=np.float32)).astype(np.float32)
    base = scenes.s_uniform(n=n, width=OVERFLOW_W, height=OVERFLOW_H, variant="emissive", density=dens)
    x = np.linspace(0.0, 1.0, n)
    les = np.broadcast_to((10.0 ** (26.0 + 12.0 * x)).astype(np.float32), (n, n, n)).copy()
    med = GridMedium(dens, sigma_a=0.6, sigma_s=1.5, g=-0.2, Le=(0.5 + np.linspace(0, 1, 471) ** 2).astype(np.float32),
                     Lescale=les)
    return Scene(base.camera, make_film(kind, kw, OVERFLOW_W, OVERFLOW_H), med, base.lights), OVERFLOW_SPP


def oracle_records(run, width, height, first, ns):
    """The oracle's pixel_sample records of sample indices [first, first + ns) in the last-pass
    layout (record s * npix + pix): L, lambda, pdf (n, 4) and the filter weight (n)."""
    npix = width * height
    L = np.zeros((ns * npix, 4), np.float32)
    lam, pdf = np.zeros_like(L), np.zeros_like(L)
    w = np.zeros(ns * npix, np.float32)
    for s in range(ns):
        for pix in range(npix):
            g = s * npix + pix
            L[g], lam[g], pdf[g], _, w[g] = run.pixel_sample(pix % width, pix // width, first + s, with_weight=True)
    return L, lam, pdf, w


def is_spectral(film):
    return int(getattr(film, "nbuckets", 0)) > 0


def oracle_sums(run, film, first, last):
    """OracleRun.render / render_spectral as one tuple (rgb, w[, buckets, bucket weights])."""
    return run.render_spectral(first, last, nthreads=4) if is_spectral(film) else run.render(first, last, nthreads=4)


# ---------------------------------------------------------------------------
# GetImage on awkward pixels: films whose sums are written directly (part of no render)

AWK_W, AWK_H = 19, 15
AWK_NPIX = AWK_W * AWK_H
HUGE = 3e38     # finite in float32; 2 * HUGE overflows


class ImageFilm:
    """A film for the GetImage forms alone: resolution, matrix and (SpectralFilm) buckets."""

    def __init__(self, matrix, nbuckets=0):
        self.width, self.height = AWK_W, AWK_H
        self.output_from_sensor = np.asarray(matrix, np.float32).reshape(3, 3)
        self.nbuckets = nbuckets


def awkward_sums(matrix):
    """(rgb_sum, w_sum) of a 19 x 15 film: ordinary pixels and, from pixel 0 on, the awkward ones
    (the index ranges are what test_awkward_films_hold_what_they_should checks). `matrix` is
    outputRGBFromSensorRGB; where the OUTPUT rgb is to have a shape the sensor sums go through
    its inverse."""
    rng = np.random.default_rng(19)
    rgb = rng.uniform(0.0, 40.0, (AWK_NPIX, 3))
    w = rng.integers(1, 9, AWK_NPIX).astype(np.float64)
    inv = np.linalg.inv(np.asarray(matrix, np.float64))
    big, inf = 1e5, np.inf

    def sensor(out):
        return inv @ np.asarray(out, np.float64)

    special = []
    # 0-3: weight 0 with non-zero sums (GetPixelRGB does not divide), negative sums
    special += [((3.0, 2.0, 1.0), 0.0), ((7e4, 1.0, 1.0), 0.0), ((-3.0, -2.0, -1.0), 2.0), ((-1e5, 5.0, -7e4), 1.0)]
    # 4-11: one output channel above 65504 in each position, then all three; weight 1 and 4
    for out in ((big, 10.0, 20.0), (10.0, big, 20.0), (10.0, 20.0, big), (big, 2 * big, 3 * big)):
        special.append((sensor(out), 1.0))
        special.append((4.0 * sensor(out), 4.0))
    # 12-17: inf sums; every matrix entry is non-zero, so each channel becomes +-inf or inf - inf = NaN
    special += [((inf, 1.0, 1.0), 1.0), ((1.0, inf, 1.0), 2.0), ((1.0, 1.0, inf), 1.0), ((inf, 1.0, inf), 3.0),
                ((inf, 1.0, 1.0), 0.0), ((1.0, inf, inf), 1.0)]
    # 18: a NaN weight
    special.append(((1.0, 2.0, 3.0), np.nan))
    # 19-21: finite sums whose products overflow: a NaN channel beside inf and finite ones
    special += [((HUGE, HUGE, 0.0), 1.0), ((HUGE, HUGE, HUGE), 1.0), ((0.0, HUGE, HUGE), 1.0)]
    # 22: a sum that only the rounding to float makes inf
    special.append(((1e39, 1.0, 1.0), 1.0))
    k = len(special)
    rgb[:k] = [s for s, _ in special]
    w[:k] = [x for _, x in special]
    return rgb.reshape(-1), w


# One NaN output channel beside one above 65504 and one 0, in all six placements. A NaN (or inf)
# SUM reaches every output channel through the matrix (0 * NaN = NaN), so the NaN is made in
# one row only: finite sums r = g = 3e38 and a row (2, -2, 0) give inf - inf; the row
# (0, 1e5 / 3e38, 0) gives 1e5 and (0, 0, 1) gives b = 0. The six films differ in the rows'
# order. pbrt's std::max({r, g, b}) keeps a NaN first operand and skips a later one:
NAN_ROWS = {"nan": (2.0, -2.0, 0.0), "big": (0.0, 1e5 / HUGE, 0.0), "zero": (0.0, 0.0, 1.0)}
NAN_PLACEMENTS = {    # rows' order -> RGBFilm::GetImage's half image of such a pixel
    ("nan", "big", "zero"): (np.nan, np.inf, 0.0),      # maximum NaN: the gate stays shut, 1e5 -> inf in half
    ("nan", "zero", "big"): (np.nan, 0.0, np.inf),
    ("big", "nan", "zero"): (65504.0, np.nan, 0.0),
    ("zero", "nan", "big"): (0.0, np.nan, 65504.0),     # max(max(0, NaN), 1e5) = 1e5: clamped
    ("big", "zero", "nan"): (65504.0, 0.0, np.nan),
    ("zero", "big", "nan"): (0.0, 65504.0, np.nan),
}


def nan_placement_sums():
    rng = np.random.default_rng(20)
    rgb = rng.uniform(0.0, 40.0, (AWK_NPIX, 3))
    w = np.ones(AWK_NPIX)
    rgb[0], w[0] = (HUGE, HUGE, 0.0), 1.0
    rgb[1], w[1] = (HUGE / 2, HUGE / 2, 0.0), 0.5
    rgb[2], w[2] = (HUGE, HUGE, 0.0), 0.0
    return rgb.reshape(-1), w


def awkward_films():
    """[(label, film, rgb_sum, w_sum)]: the sRGB matrix on the awkward pixels and the six
    row orders of the NaN placement."""
    from acceleratedvolrenderer_amd import spectra
    srgb = spectra.TABLES["srgb_rgb_from_xyz"].astype(np.float32)
    out = [("srgb", ImageFilm(srgb)) + awkward_sums(srgb)]
    for order in NAN_PLACEMENTS:
        out.append(("-".join(order), ImageFilm([NAN_ROWS[r] for r in order])) + nan_placement_sums())
    return out
