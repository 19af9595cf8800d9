"""The film stage's plain reference (tests/film_ref.py, written from film.h / film.cpp) against
the CPU oracle's AddSample, and the host GetImage forms against it — no GPU.

The reference's film.h cannot be built on its own (media.h needs NanoVDB), so no golden from
the reference pins the oracle's film code; two restatements written independently of each
other agreeing bit for bit stands in for it. The same film configurations then run on the
device in tests/test_gpu_film.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import film_cases as fc   # noqa: E402
import film_ref           # noqa: E402

_CACHE = {}


def _oracle(name):
    """Per case, once: (film, npix, spp, oracle records, oracle sums)."""
    if name not in _CACHE:
        from oracle import binding
        if name in fc.CASES:
            scene, spp = fc.scene_for(name)
            md = fc.MAXDEPTH
        else:
            scene, spp = fc.overflow_scene_for(name)
            md = fc.OVERFLOW_MAXDEPTH
        f = scene.film
        run = binding.OracleRun(scene, max_depth=md, seed=fc.SEED, libm="canonical")
        rec = fc.oracle_records(run, f.width, f.height, 0, spp)
        _CACHE[name] = (f, f.width * f.height, spp, rec, fc.oracle_sums(run, f, 0, spp))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(fc.CASES) + list(fc.OVERFLOW_CASES))
def test_add_samples_equals_oracle(name):
    """film_ref.add_samples over the oracle's own pixel_sample records gives the oracle's film
    sums bit for bit: rgb, weights and, for a SpectralFilm, bucket sums and bucket weights."""
    f, npix, spp, (L, lam, pdf, w), want = _oracle(name)
    assert np.array_equal(film_ref.radiance_guard(f, L, lam, pdf).view(np.uint32), L.view(np.uint32)), \
        "the oracle's records have been through the NaN / Inf guard"
    got = film_ref.add_samples(f, L, lam, pdf, w, npix)
    assert len(got) == len(want) == (4 if fc.is_spectral(f) else 2)
    for what, a, b in zip(("rgb", "w", "bucket sums", "bucket weights"), got, want):
        assert a.shape == b.shape
        assert np.array_equal(a, b, equal_nan=name in fc.OVERFLOW_CASES), (name, what)
    if fc.is_spectral(f):
        assert float(got[3].sum()) == 4.0 * npix * spp
    if name in fc.OVERFLOW_CASES:
        # inf * (maxComponentValue / inf) = NaN: the clamp turns overflowing components into NaN
        assert np.isnan(want[0]).any(), "no NaN sum: the overflow case overflows nothing"
        if fc.is_spectral(f):
            # L itself stays finite (the guard), so the L clamp keeps the buckets finite: <= 1e30 * 106.86 each
            assert film_ref.clamp_shares(f, L, lam, pdf)[1] > 0 and np.isfinite(want[2]).all()
    else:
        assert all(np.isfinite(a).all() for a in want)


@pytest.mark.parametrize("name", fc.RGB_CLAMP_CASES + fc.L_CLAMP_CASES + fc.L_CLAMP_IDLE_CASES)
def test_clamp_fires_on_a_fifth_to_four_fifths_of_samples(name):
    """A clamp case cannot pass with its clamp idle (or always on): each clamp a case is there to
    exercise fires on 20 % .. 80 % of the oracle's samples of that case. Measured: the maximum
    sensor RGB has quartiles 0.21 / 0.35 / 0.57, the maximum L component 0.0021 / 0.0035 /
    0.0062, so 0.35 and 0.0035 sit at the medians; at 0.35 the L clamp fires on no sample."""
    f, _, _, (L, lam, pdf, _), _ = _oracle(name)
    rgb_share, l_share = film_ref.clamp_shares(f, L, lam, pdf)
    print(f"{name}: sensor-RGB clamp on {rgb_share:.3f}, L clamp on {l_share:.3f} of samples")
    if name in fc.RGB_CLAMP_CASES:
        assert 0.2 <= rgb_share <= 0.8
    if name in fc.L_CLAMP_CASES:
        assert 0.2 <= l_share <= 0.8
        assert rgb_share > 0.9            # 0.0035 is far below nearly every sensor RGB maximum
    if name in fc.L_CLAMP_IDLE_CASES:
        assert l_share == 0.0


def test_unclamped_cases_never_clamp():
    """The sensor-scale and bucket-path cases have an infinite maxcomponentvalue: no clamp."""
    for name in ("rgb_iso250_t0.333", "spec_nb17_spp7"):
        f, _, _, (L, lam, pdf, _), _ = _oracle(name)
        assert film_ref.clamp_shares(f, L, lam, pdf) == (0.0, 0.0)


def test_sensor_scale_is_applied_after_the_average():
    """imagingRatio multiplies the averaged sensor response (film.h:97): for a ratio that is no
    power of two the sums differ in bits from ratio x the unit-ratio sums, so a multiplication
    moved elsewhere would show."""
    from acceleratedvolrenderer_amd.scene import RGBFilm
    f, npix, _, (L, lam, pdf, w), want = _oracle("rgb_iso250_t0.333")
    assert f.imaging_ratio == np.float32(np.float32(np.float32(1.0 / 3.0) * np.float32(250)) / np.float32(100))
    unit = film_ref.add_samples(RGBFilm(f.width, f.height), L, lam, pdf, w, npix)
    assert not np.array_equal(unit[0] * float(f.imaging_ratio), want[0])
    assert np.allclose(unit[0] * float(f.imaging_ratio), want[0], rtol=1e-6)


# ---------------------------------------------------------------------------
# GetImage on awkward pixels: the host forms against film_ref's scalar restatement.
# tests/test_gpu_film.py runs the same film through k_film_image.

def _same(a, b):
    """Bit for bit, any NaN equal to any NaN (payloads are not the contract), -0 == +0."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def test_awkward_films_hold_what_they_should():
    """The constructed films really have the pixels they are there for, seen through film_ref."""
    films = fc.awkward_films()
    _, f, rgb, w = films[0]
    raw = film_ref.get_image_rgb(f, rgb, w, fp16=False).reshape(-1, 3)
    half = film_ref.get_image_rgb(f, rgb, w, fp16=True).reshape(-1, 3)
    assert np.allclose(raw[0], f.output_from_sensor @ np.float32([3, 2, 1]), rtol=1e-6)   # weight 0: undivided
    assert (raw[1] > 65504).any() and (raw[2] != 0).all() and (raw[3] < 0).any()
    over = raw[4:12] > 65504
    assert [tuple(r) for r in over[0::2]] == [(True, False, False), (False, True, False), (False, False, True),
                                               (True, True, True)]
    assert np.array_equal(over[0::2], over[1::2])
    assert (half[4:12][over] == 65504).all() and np.isfinite(half[4:12]).all()
    assert np.isinf(raw[12:18]).any() and np.isnan(raw[12:18]).any()
    assert np.isnan(raw[18]).all()
    # (3e38, 3e38, 0): 3.24 r - 1.54 g = inf - inf, -0.97 r + 1.88 g = inf, the blue row stays finite
    assert np.isnan(raw[19, 0]) and raw[19, 1] == np.inf and np.isfinite(raw[19, 2])
    assert np.isnan(raw[20, 0]) and np.isinf(raw[21]).any() and not np.isnan(raw[21]).any()
    assert raw[22, 0] == np.inf and raw[22, 1] == -np.inf
    # pbrt's max({r, g, b}) is NaN when r is: the gate stays shut and the inf beside it survives
    assert np.isnan(half[19, 0]) and half[19, 1] == np.inf
    for (label, fi, rgb2, w2), (order, want) in zip(films[1:], fc.NAN_PLACEMENTS.items()):
        rawi = film_ref.get_image_rgb(fi, rgb2, w2, fp16=False).reshape(-1, 3)
        halfi = film_ref.get_image_rgb(fi, rgb2, w2, fp16=True).reshape(-1, 3)
        for p in range(3):
            for c, row in enumerate(order):
                assert {"nan": np.isnan(rawi[p, c]), "big": 9.9e4 < rawi[p, c] < 1.01e5, "zero": rawi[p, c] == 0}[row]
            assert np.array_equal(halfi[p], np.float32(want), equal_nan=True), (label, p, halfi[p])


def _host_get_image(f, rgb, w, fp16):
    from acceleratedvolrenderer_amd.integrator import FilmIntegrator
    integ = FilmIntegrator.__new__(FilmIntegrator)     # get_image needs the scene's film alone
    integ.scene = type("S", (), {"film": f})
    return integ.get_image(rgb, w, fp16=fp16)


def _diff(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist()


@pytest.mark.parametrize("fp16", [True, False])
def test_host_get_image_on_awkward_pixels(fp16):
    """FilmIntegrator.get_image (the host RGBFilm::GetImage) equals film_ref.get_image_rgb."""
    for label, f, rgb, w in fc.awkward_films():
        got, want = _host_get_image(f, rgb, w, fp16), film_ref.get_image_rgb(f, rgb, w, fp16=fp16)
        assert _same(got, want), (label,) + _diff(got, want)


@pytest.mark.parametrize("fp16", [True, False])
def test_host_gbuffer_image_on_awkward_pixels(fp16):
    """scene.gbuffer_image equals GBufferFilm::GetImage's form (the gated clamp of film.cpp:761-769)."""
    from acceleratedvolrenderer_amd.scene import gbuffer_image
    for label, f, rgb, w in fc.awkward_films():
        got, want = gbuffer_image(f, rgb, w, fp16), film_ref.get_image_gbuffer(f, rgb, w, fp16)
        assert _same(got, want), (label,) + _diff(got, want)


@pytest.mark.parametrize("fp16", [True, False])
def test_host_spectral_image_on_awkward_pixels(fp16):
    """scene.spectral_image equals SpectralFilm::GetImage's form: per-channel clamp without a
    gate, buckets divided where their weight is > 0 (a NaN, zero or negative weight writes 0)."""
    from acceleratedvolrenderer_amd.scene import spectral_image
    nb = 5
    rng = np.random.default_rng(21)
    bs = rng.uniform(0.0, 50.0, (fc.AWK_NPIX, nb))
    bw = rng.integers(1, 5, (fc.AWK_NPIX, nb)).astype(np.float64)
    bs[0], bw[0] = (1.0, 2e5, -3.0, np.inf, np.nan), (0.0, 2.0, 1.0, 1.0, 1.0)
    bs[1], bw[1] = (7e4, 7e4, 7e4, -np.inf, 1.0), (1.0, -1.0, np.nan, 1.0, np.inf)
    bs[2], bw[2] = (65504.0, 65505.0, 65520.0, 1e300, 1e-300), (1.0, 1.0, 1.0, 1.0, 1.0)
    for label, f, rgb, w in fc.awkward_films():
        fs = fc.ImageFilm(f.output_from_sensor, nbuckets=nb)
        got, want = spectral_image(fs, rgb, w, bs, bw, fp16), film_ref.get_image_spectral(fs, rgb, w, bs, bw, fp16)
        assert _same(got, want), (label,) + _diff(got, want)
