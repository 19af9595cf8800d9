"""Film pixel bounds on the device (avr_film_pixel_bounds; tests/film_bounds_cases.py has the
cases, tests/test_film_bounds.py the host side).

"Crop = slice": a film whose pixel bounds lie inside its full resolution renders only the bounds'
pixels, and every sampler, filter and camera input keeps using the absolute pixel and the full
resolution, so each per-sample record and each fp64 film sum of the cropped render is bit-identical
to the same pixel's in the render of the whole film. That is an exact property of the code under
test; the oracle, which serves any pixel of the full-resolution scene, anchors it.

  1. crop = slice for every bounds x sampler x kernel x filter: records and film sums;
  2. the records against the canonical oracle's pixel_sample;
  3. a far crop of a 600 x 40 film under ZSobol with the pixel and pass tables on and off;
  4. pass overlap: records made ahead for other bounds are never taken;
  5. SpectralFilm buckets, the device image and the metrics of a cropped film;
  6. one crop per k_paths instantiation family;
  7. the entry-cell pixel order under bounds;
  8. the graph integrators and the analyzer;
  9. render_tiles and replay_sample;
 10. argument errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_cases as cc          # noqa: E402
import film_bounds_cases as fb     # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP, MAXDEPTH = fb.W, fb.H, fb.SPP, fb.MAXDEPTH
INTERIOR = fb.BOUNDS["interior-14x7"]
SMALL = fb.BOUNDS["5x3"]
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()
    return torch


@pytest.fixture(autouse=True)
def _platform_libm_afterwards():
    """The canonical oracle runs set the process-wide libm mode: hand it back as the other
    modules expect it."""
    yield
    from oracle import binding
    binding.set_libm("platform")


def _integrator(scene, **kw):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    kw.setdefault("maxdepth", MAXDEPTH)
    kw.setdefault("spp", SPP)
    return VolPathIntegrator(scene, device=0, **kw)


def _records(integ, ns):
    """(first, ns, (L, lambda, pdf, filter weight)) of the last pass, bounds-sized."""
    npix = integ.scene.film.npix
    first, got, L, lam, pdf = integ.ctx.last_pass_samples(npix, ns)
    n = got * npix
    wts = integ.ctx.last_pass_weights(npix, ns)
    return first, got, (np.array(L[:n]), np.array(lam[:n]), np.array(pdf[:n], f32), np.array(wts[:n], f32))


def _run(integ, sequences):
    """Render each sequence of (begin, end) calls into a cleared film: {(begin, end): records of
    that call's pass}, {sequence: (rgb_sum, w_sum)}."""
    rec, sums = {}, {}
    for seq in sequences:
        integ.ctx.film_clear()
        for a, b in seq:
            integ.ctx.render(a, b, integ.seed, integ.maxdepth)
            first, ns, r = _records(integ, b - a)
            assert (first, ns) == (a, b - a)
            rec[a, b] = r
        sums[seq] = integ.film_sums()
    return rec, sums


SEQUENCES = (fb.QUAD_RANGES, fb.ODD_RANGES)
_whole = {}


def _whole_film(sampler, kernel, filt, width=W, height=H, sequences=SEQUENCES):
    """The render of the whole film, once per configuration: (records, sums) of _run."""
    key = (sampler, kernel, filt, width, height, sequences)
    if key not in _whole:
        integ = _integrator(fb.scene_for(None, filt, sampler, width=width, height=height), kernel=kernel)
        try:
            _whole[key] = _run(integ, sequences)
        finally:
            integ.close()
    return _whole[key]


def _assert_slice(got, want_whole, bounds, ns, label, width=W, height=H):
    """Per-sample arrays `got` of a cropped pass bit-identical to the whole film's at the bounds' pixels."""
    want = fb.slice_records(want_whole, bounds, width, height, ns)
    for name, a, b in zip(("L", "lambda", "pdf", "weight"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (label, name, a.shape, b.shape)
        bad = ~cc.same_bits(a.reshape(len(a), -1), b.reshape(len(b), -1))
        assert not bad.any(), (label, name, int(bad.sum()), a[bad][:3], b[bad][:3])


def _assert_sums(got, whole, bounds, label, width=W, height=H):
    rgb, w = fb.slice_sums(whole[0], whole[1], bounds, width, height)
    assert got[0].shape == rgb.shape and got[1].shape == w.shape, (label, got[0].shape, rgb.shape)
    assert fb.same_bits(got[0], rgb) and fb.same_bits(got[1], w), (label, int((got[0] != rgb).sum()))


# ---------------------------------------------------------------------------
# 1. crop = slice

@pytest.mark.parametrize("filt", list(fb.FILTERS))
@pytest.mark.parametrize("kernel", fb.KERNELS)
@pytest.mark.parametrize("sampler", fb.SAMPLERS)
@pytest.mark.parametrize("name", list(fb.BOUNDS))
def test_crop_is_the_slice_of_the_whole_render(name, sampler, kernel, filt):
    """Records of every call's pass and the film sums after the same explicit calls: (0, 4) and
    (4, 8), quad-aligned, and (1, 4), which is not."""
    bounds = fb.BOUNDS[name]
    rec_w, sums_w = _whole_film(sampler, kernel, filt)
    scene = fb.scene_for(bounds, filt, sampler)
    assert scene.film.pixel_bounds == bounds and (scene.film.width, scene.film.height) == (W, H)
    integ = _integrator(scene, kernel=kernel)
    try:
        assert integ.ctx.film_bounds() == bounds
        rec, sums = _run(integ, SEQUENCES)
        persistent = integ.stats()["loop_iterations"] > 0
    finally:
        integ.close()
    assert persistent == (kernel == "persistent")
    label = f"{name}/{sampler}/{kernel}/{filt}"
    lit = 0
    for (a, b), r in rec.items():
        assert len(r[0]) == (b - a) * fb.npix(bounds)
        _assert_slice(r, rec_w[a, b], bounds, b - a, f"{label} [{a}, {b})")
        lit += int((r[0] > 0).any(axis=1).sum())
    for seq in SEQUENCES:
        assert sums[seq][0].shape == (3 * fb.npix(bounds),)
        _assert_sums(sums[seq], sums_w[seq], bounds, f"{label} {seq}")
    if fb.npix(bounds) > 1:
        assert lit > 0, label


# ---------------------------------------------------------------------------
# 2. against the oracle

_oracle = {}


def _oracle_run(sampler, filt, width=W, height=H):
    key = (sampler, filt, width, height)
    if key not in _oracle:
        from oracle import binding
        scene = fb.scene_for(None, filt, sampler, width=width, height=height)
        _oracle[key] = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
    return _oracle[key]


def _oracle_records(run, bounds, first, ns):
    """pixel_sample's (L, lambda, pdf, weight) of the bounds' pixels, in the cropped pass's layout."""
    x0, y0, x1, y1 = bounds
    n = fb.npix(bounds)
    L, lam, pdf = (np.zeros((ns * n, 4), f32) for _ in range(3))
    wt = np.zeros(ns * n, f32)
    for s in range(ns):
        for j, (py, px) in enumerate((y, x) for y in range(y0, y1) for x in range(x0, x1)):
            L[s * n + j], lam[s * n + j], pdf[s * n + j], _, wt[s * n + j] = run.pixel_sample(px, py, first + s, with_weight=True)
    return L, lam, pdf, wt


def _exact_fraction(got, want):
    """The share of samples whose L, lambda, pdf and filter weight are all bit-identical: the
    criterion of tests/test_gpu_camera.py on this scene, which asks for all of them."""
    ok = np.ones(len(want[0]), bool)
    for a, b in zip(got, want):
        ok &= cc.same_bits(np.asarray(a, f32).reshape(len(ok), -1), np.asarray(b, f32).reshape(len(ok), -1))
    return float(ok.mean())


@pytest.mark.parametrize("filt", list(fb.FILTERS))
@pytest.mark.parametrize("sampler", fb.SAMPLERS)
@pytest.mark.parametrize("name", ["interior-14x7", "far-corner"])
def test_cropped_samples_are_the_oracles(name, sampler, filt):
    bounds = fb.BOUNDS[name]
    want = _oracle_records(_oracle_run(sampler, filt), bounds, 0, SPP)
    integ = _integrator(fb.scene_for(bounds, filt, sampler), kernel="persistent")
    try:
        integ.render()
        first, ns, got = _records(integ, SPP)
    finally:
        integ.close()
    assert (first, ns) == (0, SPP)
    frac = _exact_fraction(got, want)
    lit = float(np.mean((want[0] > 0).any(axis=1)))
    print(f"{name}/{sampler}/{filt}: bit-exact samples {frac:.5f}, lit samples {lit:.3f}")
    assert frac == 1.0


# ---------------------------------------------------------------------------
# 3. the far crop of a non-square film

def test_far_crop_of_a_non_square_film_with_and_without_tables():
    """[590, 597) x [33, 38) of a 600 x 40 film, ZSobol: the Morton codes of the bounds' pixels are
    far above their count, so a table row taken for a code, or a table filled from a local one,
    shows. Equal records with the pixel and pass tables on and with each switched off, equal to
    the slice of one whole render and to the oracle's 35 x 8 samples."""
    bounds, (fw, fh) = fb.FAR_BOUNDS, (fb.FAR_W, fb.FAR_H)
    seq = (((0, SPP),),)
    rec_w, sums_w = _whole_film("zsobol", "persistent", "gauss", fw, fh, seq)
    want = _oracle_records(_oracle_run("zsobol", "gauss", fw, fh), bounds, 0, SPP)
    got = {}
    for label, pixel_dims, pass_dims in (("tables on", None, None), ("pixel table off", 0, None),
                                         ("pass table off", None, 0), ("both off", 0, 0)):
        integ = _integrator(fb.scene_for(bounds, "gauss", "zsobol", width=fw, height=fh), kernel="persistent")
        try:
            if pixel_dims is not None:
                integ.ctx.set_sampler_table(pixel_dims)
            if pass_dims is not None:
                integ.ctx.set_sampler_pass_table(pass_dims)
            rec, sums = _run(integ, seq)
        finally:
            integ.close()
        got[label] = rec[0, SPP]
        _assert_slice(rec[0, SPP], rec_w[0, SPP], bounds, SPP, f"far crop, {label}", fw, fh)
        _assert_sums(sums[seq[0]], sums_w[seq[0]], bounds, f"far crop, {label}", fw, fh)
        assert _exact_fraction(rec[0, SPP], want) == 1.0, label
    for label, r in got.items():
        assert all(fb.same_bits(a, b) for a, b in zip(r, got["tables on"])), label
    assert len(want[0]) == 35 * 8


# ---------------------------------------------------------------------------
# 4. pass overlap

def _overlap_scene(bounds=None):
    """The gray non-emissive grid under ZSobol on which the next pass's camera stage runs beside
    k_paths (tests/test_gpu_render_interleaved.py's medium and light), 20 x 12 film."""
    from acceleratedvolrenderer_amd import GridMedium, scenes
    from acceleratedvolrenderer_amd.scene import RGBFilm, Scene, ZSobolSampler
    base = scenes.s_uniform(n=2, width=W, height=H, variant="scatter")
    dens = (0.2 + 0.8 * np.random.default_rng(5).random((12, 12, 12), dtype=f32)).astype(f32)
    film = RGBFilm(W, H, pixelbounds=None if bounds is None else fb.as_param(bounds))
    return Scene(base.camera, film, GridMedium(dens, sigma_a=0.4, sigma_s=6.0, g=0.5), base.lights[:1],
                 sampler=ZSobolSampler(pixelsamples=32))


def test_records_made_ahead_do_not_cross_a_bounds_change():
    """Bounds A: render(0, 4), render(4, 8), the second of which takes the camera records the
    first made ahead; each call ends by making the next one's. Then bounds B and render(8, 12):
    its records equal those of a context that only ever had bounds B, so nothing made for A's
    pixels was consumed. A's calls equal the slice of the whole render."""
    a_bounds, b_bounds = INTERIOR, SMALL
    md = 12
    whole = _integrator(_overlap_scene(), maxdepth=md, spp=32)
    try:
        whole.ctx.film_clear()
        whole.ctx.render(0, 4, 0, md)
        whole.ctx.render(4, 8, 0, md)
        assert whole.ctx.pass_overlap_active() == 1
        whole_rec = _records(whole, 4)[2]
        whole_sums = whole.film_sums()
    finally:
        whole.close()
    fresh = _integrator(_overlap_scene(b_bounds), maxdepth=md, spp=32)
    try:
        fresh.ctx.film_clear()
        fresh.ctx.render(8, 12, 0, md)
        fresh_rec = _records(fresh, 4)[2]
        fresh_sums = fresh.film_sums()
    finally:
        fresh.close()
    integ = _integrator(_overlap_scene(a_bounds), maxdepth=md, spp=32)
    try:
        integ.ctx.film_clear()
        integ.ctx.render(0, 4, 0, md)
        integ.ctx.render(4, 8, 0, md)
        assert integ.ctx.pass_overlap_active() == 1
        # (no readback yet: the records for [8, 12) of bounds A are made, or being made, ahead)
        integ.set_pixel_bounds(b_bounds)
        integ.ctx.render(8, 12, 0, md)
        assert integ.ctx.pass_overlap_active() == 0
        first, ns, b_rec = _records(integ, 4)
        b_sums = integ.film_sums()
        assert (first, ns) == (8, 4) and len(b_rec[0]) == 4 * fb.npix(b_bounds)
        # and A again on the same context, read back this time
        integ.set_pixel_bounds(a_bounds)
        integ.ctx.render(0, 4, 0, md)
        integ.ctx.render(4, 8, 0, md)
        a_active = integ.ctx.pass_overlap_active()
        a_rec = _records(integ, 4)[2]
        a_sums = integ.film_sums()
    finally:
        integ.close()
    assert all(fb.same_bits(x, y) for x, y in zip(b_rec, fresh_rec))
    assert fb.same_bits(b_sums[0], fresh_sums[0]) and fb.same_bits(b_sums[1], fresh_sums[1])
    assert a_active == 1
    _assert_slice(a_rec, whole_rec, a_bounds, 4, "bounds A, second call")
    _assert_sums(a_sums, whole_sums, a_bounds, "bounds A")
    assert float(a_sums[0].sum()) > 0 and float(b_sums[0].sum()) > 0


# ---------------------------------------------------------------------------
# 5. films

def _spectral_scene(bounds, order):
    from acceleratedvolrenderer_amd.scene import SpectralFilm
    film = SpectralFilm(W, H, nbuckets=6, lambdamin=400.0, lambdamax=700.0, filter=fb.make_filter("gauss"),
                        pixelbounds=None if bounds is None else fb.as_param(bounds))
    return fb.scene_for(None, sampler="zsobol", film=film)


def test_spectral_film_buckets():
    """Bucket sums and weights of the cropped SpectralFilm are the slice's rows; avr_film_spectral
    before the bounds (set_scene's order) and after them (again, on the live context)."""
    whole = _integrator(_spectral_scene(None, 0))
    try:
        rgb_w, w_w = whole.render()
        bs_w, bw_w = whole.spectral_sums()
    finally:
        whole.close()
    ids = fb.pixel_ids(INTERIOR, W)
    integ = _integrator(_spectral_scene(INTERIOR, 0))
    try:
        for again in (False, True):
            if again:     # the buckets allocated after the bounds
                f = integ.scene.film
                from acceleratedvolrenderer_amd.capi import _check
                _check(integ.ctx.lib.avr_film_spectral(integ.ctx.h, int(f.nbuckets), float(f.lambdamin), float(f.lambdamax)))
            rgb, w = integ.render()
            bs, bw = integ.spectral_sums()
            assert bs.shape == (98, 6)
            assert fb.same_bits(bs, bs_w[ids]) and fb.same_bits(bw, bw_w[ids]), again
            _assert_sums((rgb, w), (rgb_w, w_w), INTERIOR, f"spectral rgb, again={again}")
            assert integ.spectral_image().shape == (7, 14, 9)
        assert float(bs.sum()) > 0
    finally:
        integ.close()


METRICS = ("MSE", "MAE", "MRSE", "ME")


@pytest.mark.parametrize("fp16", [True, False])
def test_device_image_and_metrics_of_a_cropped_film(gpu, fp16):
    """avr_film_image_device and avr_film_metric (against a crop-shaped reference) equal the host
    computation on the slice of the whole render: the image bit for bit, the metrics within
    rtol 1e-6 of imgtool.metric, as tests/test_gpu_film.py asks of the uncropped film."""
    from acceleratedvolrenderer_amd import imgtool
    from acceleratedvolrenderer_amd.integrator import FilmIntegrator
    torch = gpu
    rec_w, sums_w = _whole_film("zsobol", "persistent", "gauss")
    host = FilmIntegrator()       # the host's GetImage over the whole film's sums
    host.scene, host.spp = fb.scene_for(None, "gauss", "zsobol"), SPP
    integ = _integrator(fb.scene_for(INTERIOR, "gauss", "zsobol"))
    try:
        want = np.ascontiguousarray(host.get_image(*sums_w[fb.QUAD_RANGES], fp16=fp16)[integ.scene.film.crop_slice()])
        assert want.shape == (7, 14, 3)
        integ.ctx.film_clear()
        for a, b in fb.QUAD_RANGES:
            integ.ctx.render(a, b, 0, MAXDEPTH)
        f = integ.scene.film
        buf = torch.full((f.npix * 3 + 8,), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        integ.ctx.film_image_device(buf.data_ptr(), f.output_from_sensor, fp16=fp16)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[f.npix * 3:] == -7.0).all()          # nothing written past the bounds' pixels
        got = out[:f.npix * 3].reshape(7, 14, 3)
        assert fb.same_bits(got, want)
        assert fb.same_bits(integ.get_image(fp16=fp16), want)
        ref = (want * f32(0.9) + f32(0.02)).astype(f32)
        with pytest.raises(ValueError, match="pixel bounds"):
            integ.ctx.film_set_reference(np.zeros((H, W, 3), f32), f.output_from_sensor, fp16=fp16)
        integ.ctx.film_set_reference(ref, f.output_from_sensor, fp16=fp16)
        for m in METRICS:
            got_m = integ.ctx.film_metric(m)
            want_m = np.stack(imgtool.metric(want, ref, m)) if m == "ME" else imgtool.metric(want, ref, m)
            assert np.allclose(got_m, want_m, rtol=1e-6, atol=0), (m, got_m, want_m)
        # a bounds change drops the reference: it has the old bounds' shape
        integ.set_pixel_bounds(SMALL)
        with pytest.raises(RuntimeError, match="no reference"):
            integ.ctx.film_metric("MSE")
    finally:
        integ.close()


# ---------------------------------------------------------------------------
# 6. one crop per k_paths instantiation family

def _family(name):
    """(scene, integrator keywords, crop bounds) of a family, the smallest scenes of
    tests/media_cases.py and tests/test_gpu_fast_matrix.py."""
    import media_cases as mc
    if name == "nanovdb":
        return mc.scene_for("affine", "nanovdb"), {}, (5, 3, 18, 14)
    if name == "rgbgrid-emissive":
        return mc.scene_for("affine", "rgbgrid_emissive"), {}, (5, 3, 18, 14)
    if name == "interface-sphere":
        return fb.scene_for(None, "box", "zsobol", camera="persp-inside-sphere"), {}, INTERIOR
    if name == "image-light":
        import test_gpu_fast_matrix as fm
        return fb.scene_for(None, "box", "independent", lights=[fm._image_light()]), {}, INTERIOR
    if name == "fast":
        return fb.scene_for(None, "gauss", "zsobol"), dict(mode="fast"), INTERIOR
    raise ValueError(name)


# k_paths<emissive, gray, sampler, medium, image light, fast>: what the family's instantiation must show
FAMILY_KERNEL = {"nanovdb": {3: "3"}, "rgbgrid-emissive": {0: "true", 3: "4"}, "interface-sphere": {3: "0"},
                 "image-light": {4: "true"}, "fast": {5: "true"}}


@pytest.mark.parametrize("name", ["nanovdb", "rgbgrid-emissive", "interface-sphere", "image-light", "fast"])
def test_crop_is_the_slice_in_every_family(name):
    """Persistent kernel, per-sample records: the whole film, then the bounds on the same context."""
    scene, kw, bounds = _family(name)
    fw, fh = scene.film.width, scene.film.height
    integ = _integrator(scene, kernel="persistent", **kw)
    try:
        integ.render()
        _, ns, whole = _records(integ, SPP)
        kernel = integ.ctx.last_kernel()
        integ.set_pixel_bounds(bounds)
        assert scene.film.pixel_bounds == bounds
        integ.render()
        first, ns_c, crop = _records(integ, SPP)
        assert integ.ctx.last_kernel() == kernel
        integ.set_pixel_bounds(None)
        assert scene.film.pixel_bounds == (0, 0, fw, fh) and integ.ctx.film_bounds() == (0, 0, fw, fh)
    finally:
        scene.film.pixel_bounds = (0, 0, fw, fh)
        integ.close()
    print(f"{name}: {kernel}")
    args = kernel[len("k_paths<"):-1].split(", ")
    assert kernel.startswith("k_paths<") and all(args[i] == v for i, v in FAMILY_KERNEL[name].items()), kernel
    assert ns == ns_c == SPP and first == 0
    _assert_slice(crop, whole, bounds, SPP, name, fw, fh)
    assert (crop[0] > 0).any()


# ---------------------------------------------------------------------------
# 7. pixel order

def test_entry_cell_order_under_bounds():
    """entry_cell_order() of a cropped film orders the bounds' pixels (numbered within the
    bounds); rendering in it changes neither the film nor the records read back in pixel order."""
    rec_w, sums_w = _whole_film("zsobol", "persistent", "gauss")
    scene = fb.scene_for(INTERIOR, "gauss", "zsobol")
    integ = _integrator(scene, kernel="persistent")
    try:
        base_rec, base_sums = _run(integ, (fb.QUAD_RANGES,))
        order = integ.entry_cell_order()
        assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(98))
        # the order of the whole film's pixels, restricted to the bounds, is the same ranking
        hit = cc.hit_mask(fb.scene_for(None, "gauss", "zsobol")).reshape(H, W)[2:9, 3:17].ravel()
        nhit = int(hit.sum())
        assert 0 < nhit < 98 and hit[order[:nhit]].all() and not hit[order[nhit:]].any()
        assert not np.array_equal(order, np.arange(98))
        integ.ctx.set_pixel_order(order)
        rec, sums = _run(integ, (fb.QUAD_RANGES,))
    finally:
        integ.close()
    for k in base_rec:
        assert all(fb.same_bits(a, b) for a, b in zip(rec[k], base_rec[k])), k
        _assert_slice(rec[k], rec_w[k], INTERIOR, k[1] - k[0], f"entry-cell order {k}")
    assert fb.same_bits(sums[fb.QUAD_RANGES][0], base_sums[fb.QUAD_RANGES][0])
    assert fb.same_bits(sums[fb.QUAD_RANGES][1], base_sums[fb.QUAD_RANGES][1])
    _assert_sums(sums[fb.QUAD_RANGES], sums_w[fb.QUAD_RANGES], INTERIOR, "entry-cell order")


# ---------------------------------------------------------------------------
# 8. graph integrators

def _graph_scene(bounds):
    """tests/test_graph_render.py's smallest graph scene (the 9 x 12 x 5 gray grid, one distant
    light, ZSobol) under a 20 x 12 film."""
    import test_graph_render as tgr
    from acceleratedvolrenderer_amd.scene import RGBFilm, Scene
    s = tgr._graph_scene((9, 12, 5), sampler=1)
    film = RGBFilm(W, H, pixelbounds=None if bounds is None else fb.as_param(bounds))
    return Scene(s.camera, film, s.medium, s.lights, sampler=s.sampler)


def _slice_rows(a, bounds, ns):
    return fb.slice_records((a,), bounds, W, H, ns)[0]


@pytest.fixture(scope="module")
def graphs(gpu):
    """The free graph test_graph_render builds for that scene, its index with a random positive
    light, and its uniform conversion."""
    import test_graph_render as tgr
    from acceleratedvolrenderer_amd import GraphIntegrator
    scene = _graph_scene(None)
    maker = GraphIntegrator(scene, None, spp=4, seed=tgr.SEED)
    try:
        _, g = tgr._build_graph(scene, maker.ctx, 1)
        light = (np.random.default_rng(21).random(g.num_vertices, dtype=f32) + f32(0.05)).astype(f32)
        yield dict(free=g.index(light), uniform=g.to_uniform(f32(2) * g.radius, light, reduce="mean"), seed=tgr.SEED)
    finally:
        maker.close()


@pytest.mark.parametrize("kind", ["free", "uniform"])
def test_graph_render_under_bounds(graphs, kind):
    from acceleratedvolrenderer_amd import GraphIntegrator
    out = {}
    for bounds in (None, INTERIOR):
        integ = GraphIntegrator(_graph_scene(bounds), graphs[kind], spp=4, seed=graphs["seed"])
        try:
            rgb, w = integ.render()
            out[bounds] = (rgb, w, integ.last_pass(), integ.get_image())
        finally:
            integ.close()
    (rgb_w, w_w, last_w, img_w), (rgb, w, last, img) = out[None], out[INTERIOR]
    _assert_sums((rgb, w), (rgb_w, w_w), INTERIOR, f"graph {kind}")
    assert img.shape == (7, 14, 3) and fb.same_bits(img, img_w[2:9, 3:17])
    assert (last["first"], last["samples"]) == (last_w["first"], last_w["samples"]) == (0, 4)
    for k in ("L", "lam", "pdf", "o", "d", "p", "count"):
        assert len(last[k]) == 4 * 98, k
        assert fb.same_bits(np.asarray(last[k]), _slice_rows(np.asarray(last_w[k]), INTERIOR, 4)), (kind, k)
    assert (last["count"] > 0).any() and float(rgb.sum()) > 0


def test_analyzer_under_bounds(graphs):
    from acceleratedvolrenderer_amd import IntegrationAnalyzer
    out = {}
    for bounds in (None, INTERIOR):
        an = IntegrationAnalyzer(_graph_scene(bounds), graphs["free"], maxdepth=2, spp=4, seed=graphs["seed"])
        try:
            res = an.analyze(detail=True)
            out[bounds] = (res, an.last_pass())
        finally:
            an.close()
    (res_w, last_w), (res, last) = out[None], out[INTERIOR]
    for k in ("total", "node", "search", "in_range", "range_sum"):
        a, b = getattr(res, k), getattr(res_w, k)
        assert a.shape == (7, 14) and fb.same_bits(a, np.ascontiguousarray(b[2:9, 3:17])), k
    for k in ("lam", "o", "d", "count", "p", "node", "in_range", "range_sum"):
        assert fb.same_bits(np.asarray(last[k]), _slice_rows(np.asarray(last_w[k]), INTERIOR, 4)), k
    assert int(res.total.sum()) > 0


# ---------------------------------------------------------------------------
# 9. assembled renders

def test_render_tiles_assembles_the_whole_render():
    """Tiles of 7 x 5 (neither divides 20 x 12) with the whole render's explicit ranges: the
    assembled sums are its sums; of a cropped film, the crop's."""
    rec_w, sums_w = _whole_film("zsobol", "persistent", "gauss")
    scene = fb.scene_for(None, "gauss", "zsobol")
    integ = _integrator(scene, kernel="persistent")
    try:
        rgb, w = integ.render_tiles(tile=(7, 5), ranges=fb.QUAD_RANGES)
        assert scene.film.pixel_bounds == (0, 0, W, H) and integ.ctx.film_bounds() == (0, 0, W, H)
        assert fb.same_bits(rgb, sums_w[fb.QUAD_RANGES][0]) and fb.same_bits(w, sums_w[fb.QUAD_RANGES][1])
        integ.set_pixel_bounds(INTERIOR)
        crop = integ.render_tiles(tile=(5, 3), ranges=fb.QUAD_RANGES)
        assert scene.film.pixel_bounds == INTERIOR
        _assert_sums(crop, sums_w[fb.QUAD_RANGES], INTERIOR, "tiles of a cropped film")
    finally:
        integ.close()
    assert float(rgb.sum()) > 0


@pytest.mark.parametrize("sampler,kernel", [("zsobol", "persistent"), ("independent", "persistent"),
                                            ("zsobol", "wavefront")])
def test_replay_sample(sampler, kernel):
    """One sample through one-pixel bounds: the whole render's record of it."""
    rec_w, _ = _whole_film(sampler, kernel, "gauss")
    integ = _integrator(fb.scene_for(None, "gauss", sampler), kernel=kernel)
    try:
        for px, py, s in ((0, 0, 0), (7, 5, 2), (19, 11, 7), (12, 6, 4)):
            a, b = (0, 4) if s < 4 else (4, 8)
            want = [np.asarray(r)[(s - a) * W * H + py * W + px] for r in rec_w[a, b]]
            got = integ.replay_sample(px, py, s)
            for name, g, wnt in zip(("L", "lambda", "pdf", "weight"), got, want):
                assert fb.same_bits(np.asarray(g, f32), np.asarray(wnt, f32)), (px, py, s, name, g, wnt)
            assert integ.ctx.film_bounds() == (0, 0, W, H)
        with pytest.raises(ValueError, match="outside"):
            integ.replay_sample(W, 0, 0)
    finally:
        integ.close()


# ---------------------------------------------------------------------------
# 10. argument errors

def test_argument_errors():
    from acceleratedvolrenderer_amd import capi
    bare = capi.Context(0)
    try:
        with pytest.raises(RuntimeError, match="need a film"):
            bare.film_pixel_bounds(0, 0, 1, 1)
    finally:
        bare.close()
    integ = _integrator(fb.scene_for(None, "box", "zsobol"))
    ctx = integ.ctx
    try:
        for b in ((-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, W + 1, H), (0, 0, W, H + 1), (W, 0, W + 3, H)):
            with pytest.raises(RuntimeError, match="reach outside"):
                ctx.film_pixel_bounds(*b)
        for b in ((5, 5, 5, 9), (5, 5, 9, 5), (9, 5, 3, 9), (0, 0, 0, 0)):
            with pytest.raises(RuntimeError, match="empty"):
                ctx.film_pixel_bounds(*b)
        assert ctx.film_bounds() == (0, 0, W, H)        # a refused call changes nothing
        ctx.set_pixel_order(np.arange(W * H, dtype=np.int32))
        ctx.film_pixel_bounds(*SMALL)
        assert ctx.film_bounds() == SMALL
        with pytest.raises(RuntimeError, match="every pixel"):      # the whole film's permutation
            ctx.set_pixel_order(np.arange(W * H, dtype=np.int32))
        ctx.set_pixel_order(np.arange(15, dtype=np.int32)[::-1])
        ctx.render(0, 4, 0, MAXDEPTH)
        rgb, w = ctx.film_read(15)
        assert (w > 0).all()
        with pytest.raises(RuntimeError, match="too small"):
            ctx.last_pass_samples(14, 4)
        # avr_film resets the bounds to the whole film
        ctx.set_scene(integ.scene)
        assert ctx.film_bounds() == (0, 0, W, H)
    finally:
        integ.close()
