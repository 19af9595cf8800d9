"""The film stage on the device at the parameters no other test gives it: k_film with a finite
maxcomponentvalue (the sensor-RGB clamp and SpectralFilm's L clamp), a sensor scale other than
1, bucket counts on both sides of the LDS / HBM switch with and without the batch tail, over
several passes and in another pixel order; k_film_image and the metrics on pixels that are not
ordinary (weight 0, above 65504, inf, NaN).

Every k_film case is held against two things: the canonical CPU oracle (records and sums, bit
for bit) and tests/film_ref.py — pbrt's AddSample restated in numpy from film.h — applied to the
device's OWN per-sample records, which isolates k_film from the path kernels. The film
configurations are tests/film_cases.py's; tests/test_film_reference.py checks on the CPU that
film_ref and the oracle agree on them and that each clamp fires on 20-80 % of a case's samples.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import film_cases as fc   # noqa: E402
import film_ref           # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KERNELS = ["persistent", "wavefront"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()


_ORACLE = {}


def _oracle(name):
    """Per case, once for both kernels: (scene, spp, maxdepth, OracleRun, records, sums)."""
    if name not in _ORACLE:
        from oracle import binding
        if name in fc.CASES:
            (scene, spp), md = fc.scene_for(name), fc.MAXDEPTH
        else:
            (scene, spp), md = fc.overflow_scene_for(name), fc.OVERFLOW_MAXDEPTH
        f = scene.film
        run = binding.OracleRun(scene, max_depth=md, seed=fc.SEED, libm="canonical")
        _ORACLE[name] = (scene, spp, md, run, fc.oracle_records(run, f.width, f.height, 0, spp),
                         fc.oracle_sums(run, f, 0, spp))
    return _ORACLE[name]


def _integrator(scene, spp, md, **kw):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    return VolPathIntegrator(scene, device=0, maxdepth=md, spp=spp, seed=fc.SEED, **kw)


def _sums(integ):
    """The device film as the oracle returns it: (rgb, w[, bucket sums, bucket weights])."""
    out = integ.film_sums()
    if fc.is_spectral(integ.scene.film):
        out += integ.spectral_sums()
    return out


def _records(integ, spp):
    """The device's own records of the last pass: (first, L, lambda, pdf, weight)."""
    f = integ.scene.film
    npix = f.width * f.height
    first, ns, L, lam, pdf = integ.ctx.last_pass_samples(npix, spp)
    return first, ns, L, lam, pdf, integ.ctx.last_pass_weights(npix, spp)[:npix * ns]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


NAMES = ("rgb", "w", "bucket sums", "bucket weights")


def _assert_sums(got, want, label, equal_nan=False):
    assert len(got) == len(want)
    for what, a, b in zip(NAMES, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (label, what)
        same = (a == b) | (np.isnan(a) & np.isnan(b)) if equal_nan else a == b
        assert same.all(), (label, what, int((~same).sum()), np.argwhere(~same)[:3].tolist(), a[~same][:3], b[~same][:3])


def _check_case(name, kernel, equal_nan=False):
    """The three assertions of a k_film case; returns (device sums, device records, oracle sums)."""
    scene, spp, md, _, (Lo, lo, po, wo), want = _oracle(name)
    f = scene.film
    npix = f.width * f.height
    integ = _integrator(scene, spp, md, kernel=kernel)
    try:
        integ.render()
        got = _sums(integ)
        first, ns, L, lam, pdf, w = _records(integ, spp)
    finally:
        integ.close()
    assert (first, ns) == (0, spp)
    # 1. per-sample records bit-identical to the canonical oracle: L, wavelengths, the pdfs k_film divides by, weights
    for what, a, b in (("L", L, Lo), ("lambda", lam, lo), ("pdf", pdf, po), ("weight", w, wo)):
        exact = float(np.mean(_bits(a) == _bits(b)))
        assert exact == 1.0, (name, kernel, what, exact)
    # 2. the film sums equal the oracle's
    _assert_sums(got, want, (name, kernel, "oracle"), equal_nan)
    # 3. ... and pbrt's AddSample restated, over the device's own records
    Lg = film_ref.radiance_guard(f, L, lam, pdf)
    _assert_sums(got, film_ref.add_samples(f, Lg, lam, pdf, w, npix), (name, kernel, "film_ref"), equal_nan)
    return got, (L, lam, pdf, w), want


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_k_film_case(name, kernel):
    """Sensor scale, RGB clamp, SpectralFilm clamps and bucket paths (tests/film_cases.py CASES)."""
    got, (L, lam, pdf, _), _ = _check_case(name, kernel)
    f = _oracle(name)[0].film
    assert all(np.isfinite(a).all() for a in got)
    if fc.is_spectral(f):
        assert float(got[3].sum()) == 4.0 * fc.NPIX * _oracle(name)[1]
        if f.nbuckets > 1:
            assert (got[3].sum(axis=0) > 0).all(), "every bucket is hit by some sample"
    # the clamps these records drive (the caps themselves are asserted on the CPU)
    rgb_share, l_share = film_ref.clamp_shares(f, L, lam, pdf)
    assert (rgb_share > 0) == (name in fc.RGB_CLAMP_CASES + fc.L_CLAMP_CASES)
    assert (l_share > 0) == (name in fc.L_CLAMP_CASES)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nb", [16, 17])
def test_k_film_accumulates_over_passes(nb, kernel):
    """SpectralFilm sums carried from pass to pass — the LDS slice reloaded from HBM at the
    start of a pass (16 buckets) and the read-modify-write in HBM (17): two calls [0, 3) and
    [3, 7), and one call split by max_paths into passes of 5 and 2 sample indices, equal the
    one-pass film and the oracle bit for bit."""
    name = f"spec_nb{nb}_spp7"
    scene, spp, md, _, _, want = _oracle(name)
    films = {}
    for how in ("one pass", "two calls", "max_paths"):
        integ = _integrator(scene, spp, md, kernel=kernel, max_paths=5 * fc.NPIX if how == "max_paths" else 0)
        try:
            if how == "two calls":
                integ.render(0, 3)
                assert integ.ctx.last_pass_samples(fc.NPIX, spp)[:2] == (0, 3)
                integ.render(3, 7, clear=False)
                assert integ.ctx.last_pass_samples(fc.NPIX, spp)[:2] == (3, 4)
            else:
                integ.render()
                assert integ.ctx.last_pass_samples(fc.NPIX, spp)[:2] == ((5, 2) if how == "max_paths" else (0, 7))
            films[how] = _sums(integ)
        finally:
            integ.close()
    for how, got in films.items():
        _assert_sums(got, want, (name, kernel, how, "oracle"))
        _assert_sums(got, films["one pass"], (name, kernel, how, "one pass"))


def test_k_film_pixel_order():
    """The pix / pix_slot split (buckets and sums indexed by pixel, records by the slot k_paths
    traced the pixel in) with the buckets in HBM: the film in the entry-cell order, in the
    reversed order and back in the default order is the default order's, and its records fed
    through film_ref give it too."""
    name = "spec_nb17_spp7"
    scene, spp, md, _, _, want = _oracle(name)
    integ = _integrator(scene, spp, md)
    try:
        integ.render()
        base = _sums(integ)
        _assert_sums(base, want, (name, "default", "oracle"))
        order = integ.entry_cell_order()
        assert sorted(order.tolist()) == list(range(fc.NPIX)) and order.tolist() != list(range(fc.NPIX))
        for label, o in (("entry cell", order), ("reversed", np.arange(fc.NPIX - 1, -1, -1, dtype=np.int32)),
                         ("default again", None)):
            integ.ctx.set_pixel_order(o)
            integ.render()
            got = _sums(integ)
            _assert_sums(got, base, (name, label, "default order"))
            _, _, L, lam, pdf, w = _records(integ, spp)
            _assert_sums(got, film_ref.add_samples(scene.film, film_ref.radiance_guard(scene.film, L, lam, pdf), lam,
                                                   pdf, w, fc.NPIX), (name, label, "film_ref"))
    finally:
        integ.close()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(fc.OVERFLOW_CASES))
def test_k_film_overflow_with_finite_clamp(name, kernel):
    """Radiance up to FLT_MAX with maxcomponentvalue = 1e30: a sensor RGB component that
    overflowed to inf becomes inf * (1e30 / inf) = NaN and the finite ones 0, as in pbrt; the L
    clamp keeps the buckets finite. NaN sums must be present, and equal the oracle's and
    film_ref's."""
    got, (L, lam, pdf, _), want = _check_case(name, kernel, equal_nan=True)
    assert np.isnan(got[0]).any() and np.array_equal(np.isnan(got[0]), np.isnan(want[0]))
    assert np.isfinite(got[1]).all()
    if len(got) == 4:
        f = _oracle(name)[0].film
        assert np.isfinite(got[2]).all() and film_ref.clamp_shares(f, L, lam, pdf)[1] > 0


@pytest.mark.parametrize("name", ["rgb_clamp", "spec17_clamp_L"])
def test_k_film_fast_mode(name):
    """k_film<.., kFast = true>: the film equals film_ref over the device's own records bit for
    bit — last_pass_samples returns the pdfs of the device function k_film<.., true> calls
    (film_lambda_pdf_fast), and everything after the pdfs is the replay mode's arithmetic."""
    scene, spp, md, _, _, _ = _oracle(name)
    f = scene.film
    integ = _integrator(scene, spp, md, mode="fast")
    try:
        integ.render()
        got = _sums(integ)
        first, ns, L, lam, pdf, w = _records(integ, spp)
    finally:
        integ.close()
    assert (first, ns) == (0, spp) and np.isfinite(L).all() and (pdf > 0).all()
    rgb_share, l_share = film_ref.clamp_shares(f, L, lam, pdf)
    print(f"fast/{name}: sensor-RGB clamp on {rgb_share:.3f}, L clamp on {l_share:.3f} of the device's samples")
    assert 0.2 <= (l_share if name in fc.L_CLAMP_CASES else rgb_share) <= 0.8
    _assert_sums(got, film_ref.add_samples(f, film_ref.radiance_guard(f, L, lam, pdf), lam, pdf, w, fc.NPIX),
                 (name, "fast", "film_ref"))


# ---------------------------------------------------------------------------
# GetImage and the metrics on films written directly

_HIP = []


def _hip():
    """The HIP runtime this process has already loaded (the C-ABI library links it)."""
    if not _HIP:
        with open("/proc/self/maps") as maps:
            paths = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
        assert paths, "no HIP runtime loaded"
        lib = ctypes.CDLL(paths[0])
        lib.hipMemcpy.restype = ctypes.c_int
        lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _HIP.append(lib)
    return _HIP[0]


def _write_film(integ, rgb_sum, w_sum):
    """Host sums into the context's film buffers: a plain hipMemcpy (host to device, 1)."""
    f = integ.scene.film
    rgb = np.ascontiguousarray(rgb_sum, np.float64).reshape(-1)
    w = np.ascontiguousarray(w_sum, np.float64).reshape(-1)
    assert rgb.size == 3 * f.width * f.height and w.size == f.width * f.height    # the buffers' sizes
    integ.ctx.sync()
    d_rgb, d_w = integ.ctx.film_device_ptrs()
    for dst, src in ((d_rgb, rgb), (d_w, w)):
        assert dst and _hip().hipMemcpy(dst, src.ctypes.data, src.nbytes, 1) == 0
    got_rgb, got_w = integ.film_sums()
    assert np.array_equal(got_rgb, rgb, equal_nan=True) and np.array_equal(got_w, w, equal_nan=True)


def _film_context(width, height):
    """A context whose film has this resolution (nothing is rendered into it)."""
    from acceleratedvolrenderer_amd import scenes
    scene = scenes.s_uniform(n=2, width=width, height=height, variant="scatter")
    return _integrator(scene, 1, 1)


def _device_image(integ, matrix, fp16):
    f = integ.scene.film
    buf = torch.full((f.width * f.height * 3,), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()      # the fill runs on torch's stream, the kernel on the context's
    integ.ctx.film_image_device(buf.data_ptr(), matrix, fp16=fp16)
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(f.height, f.width, 3)


def _same(got, want, label):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert got.shape == want.shape and not bad.any(), (label, np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(),
                                                       want[bad][:4].tolist())


@pytest.mark.parametrize("fp16", [True, False])
def test_film_image_on_awkward_pixels(fp16):
    """k_film_image, the host get_image and film_ref.get_image_rgb agree bit for bit (any NaN
    equal to any NaN) on weight 0, negative sums, channels above 65504 in every position, inf
    sums, and a NaN channel beside one above 65504 in all six placements: (0, NaN, 1e5) is where
    max(r, max(g, b)) instead of std::max({r, g, b}) left 1e5 unclamped, (NaN, 1e5, 0) where an
    ungated minimum clamps what pbrt does not."""
    integ = _film_context(fc.AWK_W, fc.AWK_H)
    try:
        for label, f, rgb, w in fc.awkward_films():
            _write_film(integ, rgb, w)
            want = film_ref.get_image_rgb(f, rgb, w, fp16=fp16)
            _same(_device_image(integ, f.output_from_sensor, fp16), want, (label, "k_film_image"))
            integ.scene.film.output_from_sensor = f.output_from_sensor
            _same(integ.get_image(fp16=fp16), want, (label, "get_image"))
    finally:
        integ.close()


def _metric_films():
    """[(label, film sums, reference image)] on 19 x 15 with the sRGB matrix, fp16 images:
    'inf': -inf film values (sums (inf, 1, 1) -> (65504, -inf, 65504) and (1, inf, 1)), clamped
           ones, and a +inf reference value in the blue channel — infinite terms are skipped;
           MRSE's blue is inf / inf = NaN;
    'nan': also sums (3e38, 3e38, 0) -> (NaN, inf, -inf) and a NaN reference value in red: the
           red channel of every metric is NaN, green and blue are not."""
    from acceleratedvolrenderer_amd import spectra
    srgb = spectra.TABLES["srgb_rgb_from_xyz"].astype(np.float32)
    f = fc.ImageFilm(srgb)
    out = []
    for label in ("inf", "nan"):
        rng = np.random.default_rng(23)
        rgb = rng.uniform(0.0, 40.0, (fc.AWK_NPIX, 3))
        w = rng.integers(1, 9, fc.AWK_NPIX).astype(np.float64)
        inv = np.linalg.inv(srgb.astype(np.float64))
        ordinary = film_ref.get_image_rgb(f, rgb.reshape(-1), w)     # before the awkward pixels go in
        rgb[3], w[3] = (np.inf, 1.0, 1.0), 1.0
        rgb[40], w[40] = (1.0, np.inf, 1.0), 2.0
        rgb[77], w[77] = inv @ (1e5, 10.0, 2e5), 1.0
        rgb[200], w[200] = (5.0, 4.0, 3.0), 0.0
        if label == "nan":
            rgb[150], w[150] = (fc.HUGE, fc.HUGE, 0.0), 1.0
        ref =(ordinary * np.float32(1.1) + np.float32(0.01)).astype(np.float32)
        ref[5, 7, 2] = np.inf
        if label == "nan":
            ref[9, 2, 0] = np.nan
        out.append((label, f, rgb.reshape(-1), w, ref))
    return out


METRICS = ("MSE", "MAE", "MRSE", "ME")


def _check_metrics(integ, img, ref, label, nan_channels):
    from acceleratedvolrenderer_amd import imgtool
    for m in METRICS:
        got = integ.ctx.film_metric(m)
        want = np.stack(imgtool.metric(img, ref, m)) if m == "ME" else imgtool.metric(img, ref, m)
        assert np.allclose(got, want, rtol=1e-6, atol=0, equal_nan=True), (label, m, got, want)
        isnan = np.isnan(np.atleast_2d(want))
        for c in range(3):
            # ME's positive part takes d > 0 only: a NaN difference lands in the absolute and negative parts
            rows = isnan[:, c] if m != "ME" else isnan[[0, 2], c]
            expect = c in nan_channels.get(m, nan_channels["*"])
            assert rows.all() == expect and rows.any() == expect, (label, m, c, want)


def test_film_metrics_with_inf_and_nan_pixels():
    """avr_film_metric against imgtool.metric where the film's image and the reference hold
    inf and NaN values: infinite terms are skipped, NaN terms are not."""
    integ = _film_context(fc.AWK_W, fc.AWK_H)
    try:
        for label, f, rgb, w, ref in _metric_films():
            _write_film(integ, rgb, w)
            integ.ctx.film_set_reference(ref, f.output_from_sensor, fp16=True)
            img = film_ref.get_image_rgb(f, rgb, w, fp16=True)
            assert np.isinf(img).any() and np.isinf(ref).any()
            assert np.isnan(img).any() == (label == "nan") and np.isnan(ref).any() == (label == "nan")
            _same(_device_image(integ, f.output_from_sensor, True), img, (label, "k_film_image"))
            _check_metrics(integ, img, ref, label,
                           {"*": {0} if label == "nan" else set(), "MRSE": {0, 2} if label == "nan" else {2}})
    finally:
        integ.close()


def test_film_image_and_metrics_700x3():
    """An ordinary film of 700 x 3 = 2100 pixels: more than one block of 256 and no multiple of
    it, in k_film_image and in k_metric's strided ranges."""
    W7, H7 = 700, 3
    integ = _film_context(W7, H7)
    try:
        f = integ.scene.film
        rng = np.random.default_rng(7003)
        rgb = rng.uniform(0.0, 60.0, (W7 * H7, 3))
        w = rng.integers(1, 17, W7 * H7).astype(np.float64)
        # the last pixel: red above 65504 in the output
        rgb[-1], w[-1] = np.linalg.inv(f.output_from_sensor.astype(np.float64)) @ (3e5, 1.0, 2.0), 1.0
        _write_film(integ, rgb, w)
        for fp16 in (True, False):
            want = film_ref.get_image_rgb(f, rgb.reshape(-1), w, fp16=fp16)
            _same(_device_image(integ, f.output_from_sensor, fp16), want, ("700x3", fp16, "k_film_image"))
            _same(integ.get_image(fp16=fp16), want, ("700x3", fp16, "get_image"))
        img = film_ref.get_image_rgb(f, rgb.reshape(-1), w, fp16=True)
        assert img[-1, -1, 0] == 65504 and np.isfinite(img).all()
        ref = (img * np.float32(0.9) + np.float32(0.02)).astype(np.float32)
        integ.ctx.film_set_reference(ref, f.output_from_sensor, fp16=True)
        _check_metrics(integ, img, ref, "700x3", {"*": set()})
    finally:
        integ.close()
