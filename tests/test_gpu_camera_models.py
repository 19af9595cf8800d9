"""The camera stage of the device (k_paths_camera of the persistent organisation, k_camera of the
wavefront one and of the graph integrators) under thin-lens and spherical cameras
(tests/camera_model_cases.py; tests/test_camera_models.py holds the CPU side).

The truth of a ray is the host-compiled chain the kernels run (cameraFromRaster's point,
csrc/avr_camera.h, xf_ray) fed with the canonical oracle's per-sample pFilm of a pinhole over the
same film and the sampler's lens draw at dimensions 4 and 5: the same code on both sides, so the
compare is bit for bit. The oracle is never handed a lens or a spherical camera.

  3. rays of the persistent kernel, every case x both samplers;
  4. the sampler stream does not shift: lambda, pdf, filter weight and u of a lens case equal the
     same scene's with lensradius = 0;
  5. persistent and wavefront agree per sample, the film is film_ref's over the read-back samples,
     lensradius = 0 is the camera built without the arguments, fast mode keeps rays and weights;
  6. the ZSobol index paths of the camera stage with a lens;
  7. pixel bounds: crop = slice, replay_sample, render_tiles;
  8. pass overlap, and avr_camera_lens between two renders;
  9. the graph integrators' camera rays;
 10. a furnace through the equal-area camera."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_cases as cc          # noqa: E402
import camera_model_cases as cm    # noqa: E402
import film_bounds_cases as fb     # noqa: E402
import film_ref                    # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP, MAXDEPTH = cm.W, cm.H, cm.SPP, cm.MAXDEPTH
NPIX = W * H
CASES = [(c, s) for c in cm.CASES for s in cm.SAMPLERS]
IDS = [f"{c}-{s}" for c, s in CASES]
LENS = [(c, s) for c in cm.LENS_CASES for s in cm.SAMPLERS]
LENS_IDS = [f"{c}-{s}" for c, s in LENS]
SPHERE_MARGIN = cm.SPHERE_MARGIN


@pytest.fixture(scope="module", autouse=True)
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()
    return torch


@pytest.fixture(autouse=True)
def _platform_libm_afterwards():
    yield
    from oracle import binding
    binding.set_libm("platform")


def _integrator(scene, **kw):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    kw.setdefault("maxdepth", MAXDEPTH)
    kw.setdefault("spp", SPP)
    return VolPathIntegrator(scene, device=0, **kw)


def _records(integ, ns=SPP):
    npix = integ.scene.film.npix
    first, got, L, lam, pdf = integ.ctx.last_pass_samples(npix, ns)
    n = got * npix
    wts = integ.ctx.last_pass_weights(npix, ns)
    return first, got, (np.array(L[:n]), np.array(lam[:n]), np.array(pdf, np.float32)[:n], np.array(wts, np.float32)[:n])


def _rays(integ, got, ns=SPP):
    npix = integ.scene.film.npix
    o, d, u = integ.ctx.last_pass_rays(npix, ns)
    n = got * npix
    return np.array(o[:n]), np.array(d[:n]), np.array(u[:n])


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return cc.same_bits(a.reshape(len(b), -1), b.reshape(len(b), -1))


def _assert_bits(got, want, names, label):
    shares = [float(_same(a, b).mean()) for a, b in zip(got, want)]
    print(f"{label}: bit-identical " + ", ".join(f"{n} {s:.5f}" for n, s in zip(names, shares)))
    for n, s, a, b in zip(names, shares, got, want):
        bad = ~_same(a, b)
        assert s == 1.0, (label, n, int(bad.sum()), np.asarray(a)[bad][:3], np.asarray(b)[bad][:3])


def _render(scene, kernel="persistent", fast=False, ns=SPP, **kw):
    """One render of all samples: (film sums, records, rays or None)."""
    integ = _integrator(scene, kernel=kernel, **kw)
    try:
        if fast:
            integ.ctx.set_render_mode("fast")
        film = integ.render()
        first, got, rec = _records(integ, ns)
        assert (first, got) == (0, ns)
        rays = _rays(integ, got, ns) if kernel == "persistent" else None
        kern = integ.ctx.last_kernel() if kernel == "persistent" else ""
    finally:
        integ.close()
    return film, rec, rays, kern


_renders = {}


def _persistent(case, sampler):
    key = (case, sampler)
    if key not in _renders:
        _renders[key] = _render(cm.scene_for(case, sampler))
    return _renders[key]


# ---------------------------------------------------------------------------
# 3. rays of the persistent kernel

@pytest.mark.parametrize("case,sampler", CASES, ids=IDS)
def test_rays_persistent(case, sampler):
    """Origin, direction, u and filter weight bit-identical to the chain's.

    "lens-sphere-outside": the direction is bit-identical and the origin lies within SPHERE_MARGIN
    of the float64 first crossing of the sphere from the lens origin. The margin is 4 x the largest
    such deviation of the same pose as a pinhole, 1.66e-6 (independent; ZSobol 8.9e-7), measured once
    on the canonical oracle's interface entry (tests/test_camera_models.py measures it again), which
    the parent commit's device origins equal bit for bit (checked here again for the pinhole). Every
    ray that crosses the sphere in float64 is held to the margin and every ray that misses it keeps
    the lens origin, with no exemption: the case's pose is chosen so that no lens ray is nearer the
    tangent than the rays the margin was measured on (camera_model_cases.SPHERE_POSE)."""
    scene, o, d, u, w, pf, lens = cm.truth(case, sampler)
    assert np.isfinite(o).all() and np.isfinite(d).all()
    film, rec, (go, gd, gu), kern = _persistent(case, sampler)
    lit = float(np.mean((rec[0] > 0).any(axis=1)))
    print(f"{case}/{sampler}: {kern}, lit samples {lit:.3f}")
    label = f"{case}/{sampler}/persistent"
    if cm.CASES[case][4] is None:
        _assert_bits((go, gd, gu, rec[3]), (o, d, u, w), ("origin", "direction", "u", "weight"), label)
    else:
        _assert_bits((gd, gu, rec[3]), (d, u, w), ("direction", "u", "weight"), label)
        hit, p, rel = cm.sphere_crossing(scene, o, d)
        dev = np.abs(go.astype(np.float64) - p).max(axis=1)
        stay = np.abs(go - o).max(axis=1) == 0
        near = int(np.argmin(np.abs(rel)))
        print(f"{label}: {hit.mean():.3f} cross the sphere, origin deviation {dev[hit].max():.3g} (margin "
              f"{SPHERE_MARGIN:.3g}); nearest the tangent: discriminant / scale {rel[near]:.3g}, "
              f"{'deviation %.3g' % dev[near] if hit[near] else 'stays: %s' % bool(stay[near])}")
        assert hit.mean() > 0.2
        assert (dev[hit] <= SPHERE_MARGIN).all(), (int((dev[hit] > SPHERE_MARGIN).sum()), float(dev[hit].max()))
        assert stay[~hit].all()
        # the lens moved the origins: they are not the pinhole's
        pin = cm.pinhole_scene(case, sampler)
        from oracle import binding
        run = binding.OracleRun(pin, max_depth=MAXDEPTH, seed=0, libm="canonical")
        po, pd, _, _ = cc.oracle_rays(run, W, H, 0, SPP)
        _, _, (qo, qd, _), _ = _render(pin)
        _assert_bits((qo, qd), (po, pd), ("origin", "direction"), label + " as a pinhole against the oracle")
        assert not _same(go, qo).all()
    assert np.abs(np.linalg.norm(gd.astype(np.float64), axis=1) - 1).max() < 2e-6
    assert lit > 0.15
    if case.startswith("lens-"):
        assert (np.abs(lens - 0.5) > 0).any() and not _same(gd, cm.chain(scene, pf, np.full_like(lens, 0.5))[1]).all()


# ---------------------------------------------------------------------------
# 4. the stream does not shift

@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("case,sampler", LENS, ids=LENS_IDS)
def test_the_lens_draw_does_not_shift_the_stream(case, sampler, kernel):
    """lambda, pdf and filter weight on both kernels; u on the persistent kernel only (the wavefront
    organisation has no ray readback: there a shifted u would show in L, which
    test_persistent_and_wavefront_agree compares)."""
    lens_scene = cm.scene_for(case, sampler)
    flat = cm.scene_for(case, sampler, cam=cm.make_camera(case, lens=False))
    _, rec, rays, _ = _persistent(case, sampler) if kernel == "persistent" else _render(lens_scene, kernel)
    _, rec0, rays0, _ = _render(flat, kernel)
    _assert_bits(rec[1:], rec0[1:], ("lambda", "pdf", "weight"), f"{case}/{sampler}/{kernel} against lensradius 0")
    if kernel == "persistent":
        _assert_bits((rays[2],), (rays0[2],), ("u",), f"{case}/{sampler} against lensradius 0")
        assert not _same(rays[1], rays0[1]).all()       # ... and the lens is there


# ---------------------------------------------------------------------------
# 5. two implementations agree

@pytest.mark.parametrize("case,sampler", CASES, ids=IDS)
def test_persistent_and_wavefront_agree(case, sampler):
    scene = cm.scene_for(case, sampler)
    film_p, rec_p, _, _ = _persistent(case, sampler)
    film_w, rec_w, _, _ = _render(scene, "wavefront")
    _assert_bits(rec_w, rec_p, ("L", "lambda", "pdf", "weight"), f"{case}/{sampler} wavefront against persistent")
    f = scene.film
    for name, film, rec in (("persistent", film_p, rec_p), ("wavefront", film_w, rec_w)):
        L, lam, pdf, w = rec
        want = film_ref.add_samples(f, film_ref.radiance_guard(f, L, lam, pdf), lam, pdf, w, NPIX)
        assert np.array_equal(film[0], want[0]) and np.array_equal(film[1], want[1]), (case, sampler, name)
    assert float(film_p[0].sum()) > 0


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("case", ["lens-persp", "lens-ortho"])
def test_radius_zero_is_the_camera_without_the_arguments(case, kernel):
    from acceleratedvolrenderer_amd.scene import OrthographicCamera, PerspectiveCamera
    kind, pose, kw, _, _ = cm.CASES[case]
    pk = cc.CAMERAS[pose][1]
    args = dict(pos=pk["pos"], look=pk["look"], up=pk["up"], screenwindow=pk.get("screenwindow"))
    make = (lambda **k: OrthographicCamera(**args, **k)) if kind == "orthographic" else (
        lambda **k: PerspectiveCamera(fov=pk["fov"], **args, **k))
    for sampler in cm.SAMPLERS:
        zero = _render(cm.scene_for(case, sampler, cam=make(lensradius=0.0, focaldistance=kw["focaldistance"])), kernel)
        plain = _render(cm.scene_for(case, sampler, cam=make()), kernel)
        assert zero[0][0].tobytes() == plain[0][0].tobytes() and zero[0][1].tobytes() == plain[0][1].tobytes()
        assert zero[3] == plain[3] and float(plain[0][0].sum()) > 0


@pytest.mark.parametrize("case,sampler", CASES, ids=IDS)
def test_fast_mode_keeps_rays_and_weights(case, sampler):
    _, rec, rays, _ = _persistent(case, sampler)
    film, rec_f, rays_f, kern = _render(cm.scene_for(case, sampler), fast=True)
    assert kern.endswith(", true>")
    _assert_bits(rays_f + (rec_f[3],), rays + (rec[3],), ("origin", "direction", "u", "weight"),
                 f"{case}/{sampler}/fast against replay")
    assert np.isfinite(film[0]).all() and float(film[0].sum()) > 0


# ---------------------------------------------------------------------------
# 6. ZSobol index paths with a lens

ZS_SPP = 16


@pytest.mark.parametrize("lo,hi,per_pass", [(0, 8, 0), (5, 11, 0), (0, 8, 3)], ids=["0-8", "5-11", "0-8-by-3"])
def test_zsobol_index_paths_with_a_lens(lo, hi, per_pass):
    """tests/test_gpu_camera.py::test_zsobol_index_paths' matrix for "lens-persp" + "gauss-64":
    quad-aligned [0, 8), the unaligned [5, 11) (plain draws) and [0, 8) in passes of 3, each without
    a pass table, with one of 8 dimensions (the per-draw lookups: the lens draw's dimension 4 is
    inside it, the stage's dimension 9 not) and with one of 64 (the preloaded entries and the paired
    indices, where the lens draw's entry comes from the pass-table row). The rays are the truth's
    in all of them — every later draw stayed where it was — and the films are equal."""
    case, filt = "lens-persp", "gauss-64"
    first, ns = (lo, hi - lo) if not per_pass else (6, 2)
    scene, o, d, u, w, _, _ = cm.truth(case, "zsobol", spp=ZS_SPP, first=first, ns=ns, filt=filt)
    films = []
    for dims in (0, 8, 64):
        integ = _integrator(scene, spp=ZS_SPP, kernel="persistent", max_paths=NPIX * per_pass)
        try:
            integ.ctx.set_sampler_pass_table(dims)
            films.append(integ.render(lo, hi))
            got_first, got_ns, rec = _records(integ, hi - lo)
            assert (got_first, got_ns) == (first, ns)
            label = f"lens, zsobol [{lo}, {hi}) passes of {per_pass or hi - lo}, pass table {dims}"
            _assert_bits(_rays(integ, got_ns, hi - lo) + (rec[3],), (o, d, u, w), ("origin", "direction", "u", "weight"),
                         label)
        finally:
            integ.close()
    for f in films[1:]:
        assert np.array_equal(f[0], films[0][0]) and np.array_equal(f[1], films[0][1])
    assert float(films[0][0].sum()) > 0


WIDE_SPP = 16384


@pytest.mark.parametrize("dims", [0, 64], ids=["no-pass-table", "pass-table-64"])
def test_zsobol_64_bit_index_with_a_lens(dims):
    """The films above stay on 32-bit sample indices (20 x 12 at 16 spp: k_paths_camera<2, *, 1>).
    tests/film_bounds_cases.py's far crop of a 600 x 40 film at 16384 pixel samples has 17 base-4
    digits: the 64-bit instantiation k_paths_camera<3, false, 1>, with quads (log2 spp = 14), without
    a pass table and with the paired indices. Rays and weights of the crop's 35 pixels are the
    truth's."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import RGBFilm, Scene, ZSobolSampler
    from oracle import binding
    fw, fh, bounds = fb.FAR_W, fb.FAR_H, fb.FAR_BOUNDS
    base = scenes.s_uniform(n=cc.GRID_N, width=fw, height=fh, variant="scatter", density=cc.density())

    def scene(cam):
        return Scene(cam, RGBFilm(fw, fh, filter=cc.make_filter("gauss-64"), pixelbounds=fb.as_param(bounds)), base.medium,
                     base.lights, sampler=ZSobolSampler(pixelsamples=WIDE_SPP))

    sc = scene(cm.make_camera("lens-persp"))
    run = binding.OracleRun(scene(cm.make_camera("lens-persp", lens=False)), max_depth=MAXDEPTH, seed=0, libm="canonical")
    pf, u, w = cm.oracle_film_points(run, 0, SPP, bounds)
    draws = cm.camera_draws("zsobol", WIDE_SPP, 0, SPP, bounds=bounds, res=(fw, fh))
    assert cc.same_bits(draws[:, 8], u).all()
    o, d = cm.chain(sc, pf, draws[:, 4:6])
    integ = _integrator(sc, spp=WIDE_SPP)
    try:
        integ.ctx.set_sampler_pass_table(dims)
        film = integ.render(0, SPP)
        first, got, rec = _records(integ)
        assert (first, got) == (0, SPP)
        assert integ.ctx.last_kernel().startswith("k_paths<false, true, 3,")      # the 64-bit sampler variant
        _assert_bits(_rays(integ, got) + (rec[3],), (o, d, u, w), ("origin", "direction", "u", "weight"),
                     f"lens, 64-bit zsobol index, pass table {dims}")
    finally:
        integ.close()
    assert np.isfinite(film[0]).all()


# ---------------------------------------------------------------------------
# 7. pixel bounds

BOUNDS = (3, 2, 17, 9)      # pixelbounds = (3, 17, 2, 9)


@pytest.mark.parametrize("sampler", cm.SAMPLERS)
@pytest.mark.parametrize("case", ["sph-ea-outside", "lens-persp"])
def test_pixel_bounds_are_the_slice_of_the_full_render(case, sampler):
    """uv divides by the full resolution and the lens draw belongs to the absolute pixel: the crop
    is the slice, bit for bit; replay_sample and render_tiles agree with the full render."""
    film, rec, rays, _ = _persistent(case, sampler)
    scene = cm.scene_for(case, sampler, pixelbounds=(3, 17, 2, 9))
    assert scene.film.pixel_bounds == BOUNDS
    integ = _integrator(scene)
    try:
        crop = integ.render()
        first, got, crec = _records(integ)
        assert (first, got) == (0, SPP)
        crays = _rays(integ, got)
        _assert_bits(crec + crays, fb.slice_records(rec + rays, BOUNDS, W, H, SPP),
                     ("L", "lambda", "pdf", "weight", "origin", "direction", "u"), f"{case}/{sampler} crop against slice")
        rgb, w = fb.slice_sums(film[0], film[1], BOUNDS, W, H)
        assert fb.same_bits(crop[0], rgb) and fb.same_bits(crop[1], w)
        for px, py, s in ((3, 2, 0), (16, 8, 7), (9, 5, 3)):
            L, lam, pdf, wt = integ.replay_sample(px, py, s)
            g = s * NPIX + py * W + px
            assert (_same(L[None], rec[0][g][None]).all() and _same(lam[None], rec[1][g][None]).all()
                    and _same(pdf[None], rec[2][g][None]).all() and np.float32(wt) == rec[3][g]), (px, py, s)
        tiles = integ.render_tiles((8, 5))
        assert fb.same_bits(tiles[0], rgb) and fb.same_bits(tiles[1], w)
    finally:
        integ.close()


# ---------------------------------------------------------------------------
# 8. pass overlap

def _overlap_run(scene, overlap, lens_between=None, ranges=((0, 8), (8, 16))):
    integ = _integrator(scene, spp=ZS_SPP)
    try:
        integ.ctx.set_pass_overlap(overlap)
        integ.ctx.film_clear()
        active = []
        for i, (a, b) in enumerate(ranges):
            if i and lens_between is not None:
                integ.ctx.set_camera_lens(*lens_between)
            integ.ctx.render(a, b, 0, MAXDEPTH)
            active.append(integ.ctx.pass_overlap_active())
        return integ.film_sums(), active
    finally:
        integ.close()


def test_pass_overlap_with_a_lens():
    """A gray grid under ZSobol: the next pass's camera stage (the lens instantiation) runs ahead;
    the film equals the serial one. avr_camera_lens between two renders drops the records made ahead
    for the old lens: the film is that of a context that had the new lens for the second call."""
    scene = cm.scene_for("lens-persp", "zsobol", spp=ZS_SPP)
    on, act_on = _overlap_run(scene, True)
    off, act_off = _overlap_run(scene, False)
    assert act_on == [False, True] and act_off == [False, False]
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and float(on[0].sum()) > 0
    new = (0.12, 1.8)
    changed, act = _overlap_run(scene, True, lens_between=new)
    assert act == [False, False]
    # a fresh context: the first call under the old lens, the second under the new one, no overlap
    fresh, _ = _overlap_run(scene, False, lens_between=new)
    assert np.array_equal(changed[0], fresh[0]) and np.array_equal(changed[1], fresh[1])
    assert not np.array_equal(changed[0], on[0])
    # and the second call alone equals a context built with that lens
    from acceleratedvolrenderer_amd.scene import PerspectiveCamera
    pk = cc.CAMERAS["persp-roll"][1]
    cam = PerspectiveCamera(fov=pk["fov"], pos=pk["pos"], look=pk["look"], up=pk["up"], lensradius=new[0], focaldistance=new[1])
    built, _ = _overlap_run(cm.scene_for("lens-persp", "zsobol", spp=ZS_SPP, cam=cam), True, ranges=((8, 16),))
    first, _ = _overlap_run(scene, True, ranges=((0, 8),))
    assert np.array_equal(changed[1], first[1] + built[1])
    assert np.allclose(changed[0], first[0] + built[0], rtol=1e-12, atol=0)


def test_lens_call_errors_on_a_context():
    from acceleratedvolrenderer_amd import capi
    ctx = capi.Context(0)
    try:
        with pytest.raises(RuntimeError, match="avr error 3.*avr_camera first"):
            ctx.set_camera_lens(0.1, 1.0)
        ctx.set_scene(cm.scene_for("lens-persp"))
        for bad in ((-0.1, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (0.1, 0.0), (0.1, -2.0), (0.1, float("nan"))):
            with pytest.raises(RuntimeError, match="avr error 1"):
                ctx.set_camera_lens(*bad)
        ctx.set_camera_lens(0.0, 1.0)
        ctx.set_scene(cm.scene_for("sph-ea-inside"))
        with pytest.raises(RuntimeError, match="avr error 1.*spherical"):
            ctx.set_camera_lens(0.1, 1.0)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# 9. graph integrators

@pytest.mark.parametrize("sampler", cm.SAMPLERS)
@pytest.mark.parametrize("case", ["lens-persp", "sph-ea-inside"])
def test_graph_integrator_rays(case, sampler):
    """An index of 8 arbitrary vertices inside the box: avr_graph_last_pass's camera rays (k_camera
    without the interface entry) are the chain's."""
    from acceleratedvolrenderer_amd import GraphIntegrator, capi
    from acceleratedvolrenderer_amd.scene import DistantLight, Scene
    scene, o, d, u, w, _, _ = cm.truth(case, sampler)
    one = Scene(scene.camera, scene.film, scene.medium, [DistantLight(from_=(-1.0, 1.0, -1.0), to=(0.0, 0.0, 0.0), scale=2.0)],
                sampler=scene.sampler)
    rng = np.random.default_rng(21)
    verts = (np.asarray(one.render_from_world, np.float64)[:3, 3] + 0.1 + 0.8 * rng.random((8, 3))).astype(np.float32)
    integ = GraphIntegrator(one, capi.GraphIndex(verts, np.ones(8, np.float32), None, radius=0.3), spp=SPP, seed=0)
    try:
        rgb, _ = integ.render()
        lp = integ.last_pass()
    finally:
        integ.close()
    assert np.isfinite(rgb).all()
    _assert_bits((lp["o"], lp["d"]), (o, d), ("origin", "direction"), f"{case}/{sampler} graph against the chain")


# ---------------------------------------------------------------------------
# 10. known answer

@pytest.mark.parametrize("sampler", cm.SAMPLERS)
def test_furnace_through_the_equal_area_camera(sampler):
    """scenes.s_uniform's furnace (albedo 1, a uniform infinite light of radiance Le around it) seen
    from inside by "sph-ea-inside": every direction sees Le. The mean of the per-sample Y over Y(Le)
    lies within 4 standard errors (from the read-back samples) of 1; the pinhole "persp-inside" on
    the same context is the control and passes the same check. (Measured: with an isotropic phase
    function and one uniform light NEE and escape weights add up to 1 on every path, so every sample
    has the same ratio, 1.0000000, under both cameras and the standard error is 0.)"""
    furnace = cm.scene_for("sph-ea-inside", sampler, variant="furnace", density=False)
    f = furnace.film
    assert len(furnace.lights) == 1 and float(furnace.medium.sigma_a.max()) == 0
    integ = _integrator(furnace, maxdepth=1000)
    try:
        for name in ("sph-ea-inside", "persp-inside"):
            if name == "persp-inside":
                integ.ctx.set_camera(cm.scene_for("sph-ea-inside", sampler, variant="furnace", density=False,
                                                  cam=cc.make_camera("persp-inside")))
            integ.render()
            _, got, (L, lam, pdf, w) = _records(integ)
            assert got == SPP
            # Le at the samples' wavelengths: the light's table (DenselySampledSpectrum::Sample) times its scale
            Le = np.float32(furnace.light_scale[0]) * film_ref._sample_dense(furnace.light_L[0], lam)
            y = film_ref.sensor_rgb(f, L, lam, pdf)[:, 1].astype(np.float64)
            y_le = film_ref.sensor_rgb(f, Le, lam, pdf)[:, 1].astype(np.float64)
            r = y / y_le
            m, se = float(r.mean()), float(r.std(ddof=1) / np.sqrt(r.size))
            print(f"furnace/{sampler}/{name}: mean Y / Y(Le) {m:.7f}, standard error {se:.3g}, "
                  f"ratios {r.min():.7f} .. {r.max():.7f}")
            assert np.isfinite(r).all() and (y_le > 0).all() and abs(m - 1) <= 4 * se
    finally:
        integ.close()
