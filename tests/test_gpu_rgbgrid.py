"""RGBGridMedium on the device over real colours (tests/rgbgrid_cases.py; the CPU side, the
goldens of the reference and the derivation of the tolerance are in
tests/test_rgbgrid_cases_reference.py).

rsp_eval, rsp_max, rgb_tap, rgb_lookup, the type-4 branch of sample_point and k_majorant_rgb were
reached through whole renders of random coefficients only (c2 in [-5, 5], scale in [0.2, 3]).
Here:

  * avr_rgbgrid_probe (sample_point alone, one lane per probe) against the oracle's SamplePoint
    for every grid, combination and box: every output bit for bit, finite, within the derived
    tolerance of the float64 reference. Black voxels ({0, 0, -inf, 0}: the sigmoid's isinf branch,
    0 * 0), greys, primaries, HDR scales, c2 = +inf, 1 + x^2 = inf; border taps, faces, a box
    that is not the unit cube, missing grids, zero scales;
  * the same through avr_medium_rgbgrid_device;
  * k_majorant_rgb bit for bit at 16^3 and at (5, 7, 3) for every grid, all-black exactly 0;
  * replay in both kernel organisations: the plume (black outside, HDR emission), sigma_a only,
    and the all-black grid, where every sample is the escape radiance of its camera ray;
  * avr_transmittance: exactly 1 through black, bit for bit through the plume;
  * fast mode on the plume; the entry point's argument errors."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import film_cases as fc      # noqa: E402
import media_cases as mc     # noqa: E402
import rgbgrid_cases as rc   # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP, MAXDEPTH = 24, 20, 8, 8
NPIX = W * H
KERNELS = ("persistent", "wavefront")
OTHER_RES = (5, 7, 3)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()
    return torch


@pytest.fixture(scope="module")
def ctx(gpu):
    from acceleratedvolrenderer_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(1e-12, np.sqrt(np.mean(b ** 2))))


def _assert_probe(got, k, label):
    worst = 0.0
    for name, dev, ora, ref, tol in zip(("sigma_a", "sigma_s", "Le"), got, k["oracle"], k["ref"], k["tol"]):
        assert np.all(np.isfinite(dev)), (label, name)
        same = _bits(dev) == _bits(ora)
        bad = np.argwhere(~same)
        assert same.all(), (label, name, f"{same.mean():.5f} bit-exact", k["p"][bad[0][0]], k["lam"][bad[0][0]],
                            dev[tuple(bad[0])], ora[tuple(bad[0])])
        err = np.abs(dev.astype(np.float64) - ref)
        assert np.all(err <= tol), (label, name)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.where(err == 0, 0.0, err / tol).max()))
    return worst


# ---------------------------------------------------------------------------
# the point probe

@pytest.mark.parametrize("grid,combo,box", rc.ALL_CASES, ids=[f"{g}-{c}-{b}" for g, c, b in rc.ALL_CASES])
def test_probe_equals_oracle(ctx, grid, combo, box):
    k = rc.case(grid, combo, box)
    ctx.set_scene(k["scene"])
    got = ctx.rgbgrid_probe(k["p"], k["lam"])
    worst = _assert_probe(got, k, f"{grid}/{combo}/{box}")
    lit = float(np.mean(k["oracle"][0] > 0))
    print(f"{grid}/{combo}/{box}: {len(k['p'])} probes bit-exact, sigma_a > 0 in {lit:.3f}, largest error / bound {worst:.3f}")
    # any output may be NULL: the others are unchanged
    only = ctx.rgbgrid_probe(k["p"][:64], k["lam"][:64], outputs=("Le",))
    assert only[0] is None and only[1] is None and np.array_equal(_bits(only[2]), _bits(got[2][:64]))


@pytest.mark.parametrize("box", rc.BOXES)
def test_probe_device_resident_grids(gpu, ctx, box):
    """avr_medium_rgbgrid_device (the caller's tensors, adopted in place) gives what the host upload gives."""
    torch = gpu
    k = rc.case("g798", "a+s+Le", box)
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0").contiguous()
    t = [dev(rc.coeffs("g798", r)) for r in rc.ROLES]
    kw = rc.medium_kwargs("g798", "a+s+Le")
    kw.update(sigma_a_coeffs=t[0], sigma_s_coeffs=t[1], Le_coeffs=t[2])
    if box == "affine":
        p0, p1 = mc.box("affine")
        kw.update(p0=p0, p1=p1, world_from_medium=mc.transform("affine"))
    from acceleratedvolrenderer_amd.scene import RGBGridMedium
    med = RGBGridMedium(g=0.25, **kw)
    assert med.on_device
    ctx.set_scene(rc.probe_scene("g798", "a+s+Le", box, med=med))
    got = ctx.rgbgrid_probe(k["p"], k["lam"])
    _assert_probe(got, k, f"device-resident/{box}")
    assert got[2].max() > 0
    ctx.set_scene(k["scene"])          # release the tensors before they go
    torch.cuda.synchronize()


def test_probe_argument_errors(gpu):
    from acceleratedvolrenderer_amd import capi, scenes
    c = capi.Context(0)
    try:
        fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        p, lam = np.full((8, 3), 0.5, np.float32), np.full((8, 4), 550.0, np.float32)
        out = [np.full((8, 4), 7.0, np.float32) for _ in range(3)]
        call = lambda n, a, b, o=out: c.lib.avr_rgbgrid_probe(c.h, n, a, b, fp(o[0]), fp(o[1]), fp(o[2]))
        assert call(8, fp(p), fp(lam)) == 3                                   # no medium
        c.set_scene(scenes.s_uniform(n=4, width=4, height=4, variant="scatter"))
        assert call(8, fp(p), fp(lam)) == 3                                   # a GridMedium
        assert call(0, None, None) == 3
        with pytest.raises(RuntimeError, match="avr error 3"):
            c.rgbgrid_probe(p, lam)
        k = rc.case("g235", "a+s+Le", "unit")
        c.set_scene(k["scene"])
        assert call(-1, fp(p), fp(lam)) == 1
        assert call(8, None, fp(lam)) == 1
        assert call(8, fp(p), None) == 1
        assert call(0, None, None) == 0 and call(0, fp(p), fp(lam)) == 0       # n = 0: nothing launched
        assert all(np.all(o == 7.0) for o in out)
        assert c.lib.avr_rgbgrid_probe(c.h, 8, fp(p), fp(lam), None, None, None) == 0   # every output NULL
        assert call(8, fp(p), fp(lam)) == 0
        want = k["run"].medium_sample(p, lam)
        assert all(np.array_equal(_bits(o), _bits(w)) for o, w in zip(out, want))
    finally:
        c.close()


# ---------------------------------------------------------------------------
# the majorant

MAJORANT_CASES = [(g, "a+s") for g in rc.GRIDS] + [("g798", "s"), ("g798", "a"), ("black", "s"), ("g111", "a"),
                                                   ("plume", "scale0")]


@pytest.mark.parametrize("grid,combo", MAJORANT_CASES, ids=[f"{g}-{c}" for g, c in MAJORANT_CASES])
def test_majorant_bit_exact(ctx, grid, combo):
    """k_majorant_rgb against oracle_rgb_majorant at the constructor's 16^3 and, through
    avr_set_majorant_res (which takes an RGBGridMedium), at (5, 7, 3)."""
    from oracle import binding
    k = rc.case(grid, combo, "unit")
    ctx.set_scene(k["scene"])
    got = ctx.majorant(16 ** 3)
    assert _bits(got).tolist() == _bits(k["run"].majorant).tolist()
    assert np.all(np.isfinite(got))
    if grid == "black" and combo == "a+s" or combo == "scale0":
        assert not got.any()
    elif grid == "black":
        assert np.all(got == np.float32(1.3))              # 1.3 * (0 + 1)
    else:
        assert got.max() > 0
    med = rc.medium(grid, combo)
    med.majorant_res = OTHER_RES
    ctx.set_majorant_res(OTHER_RES)
    got = ctx.majorant(int(np.prod(OTHER_RES)))
    assert _bits(got).tolist() == _bits(binding.rgb_majorant(med)).tolist()
    ctx.set_majorant_res((16, 16, 16))
    assert _bits(ctx.majorant(16 ** 3)).tolist() == _bits(k["run"].majorant).tolist()


# ---------------------------------------------------------------------------
# replay

REPLAY = (("plume", "a+s+Le"), ("g798", "a"), ("black", "a+s+Le"))
_refs = {}


def _replay_ref(grid, combo):
    """Scene, canonical oracle run and records, the platform oracle's film and two-seed noise; once."""
    key = (grid, combo)
    if key not in _refs:
        from oracle import binding
        from acceleratedvolrenderer_amd.scene import film_rgb
        scene = rc.render_scene(grid, combo)
        run = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
        img = [film_rgb(scene.film, *binding.OracleRun(scene, max_depth=MAXDEPTH, seed=s).render(0, SPP, nthreads=8))
               for s in (0, 1)]
        _refs[key] = dict(scene=scene, run=run, records=fc.oracle_records(run, W, H, 0, SPP), img=img[0],
                          noise=_rel_rms(img[1], img[0]))
    return _refs[key]


def _records(integ):
    first, got, L, lam, pdf = integ.ctx.last_pass_samples(NPIX, SPP)
    n = got * NPIX
    wts = integ.ctx.last_pass_weights(NPIX, SPP)
    return got, (L[:n], lam[:n], np.asarray(pdf, np.float32)[:n], np.asarray(wts, np.float32)[:n])


def _exact_fraction(got, want):
    ok = np.ones(len(want[0]), bool)
    for a, b in zip(got, want):
        a = np.asarray(a, np.float32).reshape(len(ok), -1)
        b = np.asarray(b, np.float32).reshape(len(ok), -1)
        ok &= (a.view(np.uint32) == b.view(np.uint32)).all(axis=1)
    return float(ok.mean())


def _integrator(scene, **kw):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    return VolPathIntegrator(scene, device=0, maxdepth=MAXDEPTH, spp=SPP, **kw)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("grid,combo", REPLAY, ids=[f"{g}-{c}" for g, c in REPLAY])
def test_replay(grid, combo, kernel):
    """Per-sample replay against the canonical oracle: 100 % bit-identical (L, lambda, pdf, filter
    weight), film within 0.5 x the two-seed oracle noise, as test_rgbgrid_medium_replay asserts."""
    r = _replay_ref(grid, combo)
    integ = _integrator(r["scene"], kernel=kernel)
    try:
        assert _bits(integ.ctx.majorant(16 ** 3)).tolist() == _bits(r["run"].majorant).tolist()
        rgb, w = integ.render()
        assert (integ.stats()["loop_iterations"] > 0) == (kernel == "persistent")
        ns, got = _records(integ)
        assert ns == SPP
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(rgb))
        frac = _exact_fraction(got, r["records"])
        err = _rel_rms(integ.image(rgb, w), r["img"])
        print(f"{grid}/{combo}/{kernel}: bit-exact samples {frac:.5f}, film rel RMS {err:.3e} (noise {r['noise']:.3e})")
        assert frac == 1.0
        assert err <= 0.5 * r["noise"]
        if grid == "black":
            # nothing to collide with: every sample is the escape radiance of its camera ray, the sum
            # of the infinite lights' Le along it, whatever the kernel organisation
            lam = got[1]
            d = np.array([r["run"].camera_ray(pix % W, pix // W, s)[1] for s in range(SPP) for pix in range(NPIX)],
                         np.float32)
            want = sum(r["run"].light_le(i, d, lam) for i, lt in enumerate(r["scene"].lights) if lt.type_id == 1)
            assert want.min() > 0
            assert np.array_equal(_bits(got[0]), _bits(want))
        else:
            assert len(np.unique(got[0])) > NPIX               # not a constant frame
    finally:
        integ.close()


def test_replay_kernel_organisations_agree_on_black():
    films = []
    for kernel in KERNELS:
        integ = _integrator(_replay_ref("black", "a+s+Le")["scene"], kernel=kernel)
        try:
            films.append(integ.render())
        finally:
            integ.close()
    assert np.array_equal(films[0][0], films[1][0]) and np.array_equal(films[0][1], films[1][1])
    assert np.all(np.isfinite(films[0][0])) and films[0][0].min() > 0


# ---------------------------------------------------------------------------
# Integrator::Tr

def _segments(scene):
    """256 render-space segments: 32 with both ends in one black corner of the plume's box, 32 from
    one black corner to the opposite one, the rest with ends anywhere in the box enlarged by 15 %."""
    rng = np.random.default_rng(91)
    a, _ = mc.interior_segments(scene, 32, rng, lo=0.02, hi=0.12)
    _, b = mc.interior_segments(scene, 32, rng, lo=0.02, hi=0.12)
    c, _ = mc.interior_segments(scene, 32, rng, lo=0.02, hi=0.12)
    _, d = mc.interior_segments(scene, 32, rng, lo=0.88, hi=0.98)
    e, f = mc.random_segments(scene, 192, rng)
    return np.concatenate([a, c, e]).astype(np.float32), np.concatenate([b, d, f]).astype(np.float32)


def test_transmittance(ctx):
    lam = (360 + 470 * np.random.default_rng(92).random((256, 4))).astype(np.float32)
    black = _replay_ref("black", "a+s+Le")
    p0, p1 = _segments(black["scene"])
    ctx.set_scene(black["scene"])
    tr = ctx.transmittance(p0, p1, lam)
    assert np.all(tr == 1.0)
    assert np.all(black["run"].transmittance4(p0, p1, lam) == 1.0)
    plume = _replay_ref("plume", "a+s+Le")
    ctx.set_scene(plume["scene"])
    dev = ctx.transmittance(p0, p1, lam)
    ora = plume["run"].transmittance4(p0, p1, lam)
    same = (_bits(dev) == _bits(ora)).all(axis=1)
    print(f"plume Tr: bit-exact {same.mean():.5f}, mean {dev.mean():.4f}, exactly 1 in {np.mean(dev == 1):.3f}, "
          f"distinct values {len(np.unique(ora))}")
    assert np.all(np.isfinite(dev))
    assert same.all()
    assert np.all(dev[:32] == 1.0)                     # both ends and the way between them in black voxels
    assert np.any(dev[32:64] < 1.0) and len(np.unique(ora)) > 64


# ---------------------------------------------------------------------------
# fast mode

def test_fast_mode_plume():
    """avr_set_render_mode 1 on the plume: finite everywhere; against replay mode and against the
    platform oracle within tests/test_gpu_fast_matrix.py's correlated-film margin of its RGB cases
    (rel RMS <= 0.5 x the rel RMS between two oracle seeds)."""
    r = _replay_ref("plume", "a+s+Le")
    integ = _integrator(r["scene"], mode="fast")
    try:
        rgb, w = integ.render()
        assert integ.ctx.last_kernel() == "k_paths<true, false, 0, 4, false, true>"
        _, got = _records(integ)
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(rgb)) and np.all(got[0] >= 0)
        fast = integ.image(rgb, w)
        integ.ctx.set_render_mode("replay")
        rgb_r, w_r = integ.render(0, SPP)
        replay = integ.image(rgb_r, w_r)
        assert np.array_equal(w_r, w) and not np.array_equal(rgb_r, rgb)
        e_replay, e_oracle = _rel_rms(fast, replay), _rel_rms(fast, r["img"])
        print(f"plume fast: rel RMS vs replay {e_replay:.3e}, vs the platform oracle {e_oracle:.3e} (noise {r['noise']:.3e})")
        assert e_replay <= 0.5 * r["noise"]
        assert e_oracle <= 0.5 * r["noise"]
    finally:
        integ.close()
