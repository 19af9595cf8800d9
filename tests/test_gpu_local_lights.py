"""PointLight, SpotLight and pbrt's whole BVHLightSampler on the device (tests/local_light_cases.py;
tests/test_local_lights.py holds the CPU side: the host-compiled csrc/avr_local_light.h against an
independent restatement of the reference's text).

  * avr_light_probe_at, avr_light_pick_at and avr_light_bvh equal the host-compiled header bit for
    bit (wi, Ls, distance, index, pmf: 100 %; a NaN at the light itself counts as equal to a NaN);
  * the persistent and the wavefront kernels give bit-identical per-sample records for one point
    light, one spot light, a point light with a distant one and eight mixed lights, under "bvh",
    "uniform" and "power", with the independent and the ZSobol sampler (one case with a 64-bit
    sample index); k_paths runs a general instantiation;
  * SpotLight(coneangle=180, conedeltaangle=0) and PointLight give bit-identical films under
    "uniform" (under "bvh" such a spot light has cosTheta_e = 1 and with it importance 0: pbrt never
    samples it there, and neither does the device);
  * an interface sphere with one light inside and one outside: both kernels agree, all finite;
  * anchors to the oracle, per sample and bit for bit: a local light that contributes nothing leaves
    the oracle's render of the equivalent infinite-only list (sampler dimensions, pInfinite, the
    escape PMF);
  * a known answer: single scattering of a point / spot light in a homogeneous medium against a
    float64 quadrature, within 5 standard errors, replay and fast;
  * errors.

Measured (MI355X): every share above is 1.00000 (76 probes per light, 28875 picks per list, 1920
records per render); the known answer deviates by at most 1.9 standard errors, the standard error
0.30 to 0.63 % of G (replay and fast)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import film_cases as fc             # noqa: E402
import light_cases as lc            # noqa: E402
import local_light_cases as ll      # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP, MAXDEPTH = ll.W, ll.H, ll.SPP, ll.MAXDEPTH
NPIX = W * H
AVR_ERR_ARG, AVR_ERR_STATE = 1, 3


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


def _integrator(scene, lightsampler="bvh", **kw):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    kw.setdefault("maxdepth", MAXDEPTH)
    kw.setdefault("spp", SPP)
    return VolPathIntegrator(scene, device=0, lightsampler=lightsampler, **kw)


def _records(integ, npix=NPIX, first=0, ns=SPP):
    f, got, L, lam, pdf = integ.ctx.last_pass_samples(npix, ns)
    assert (f, got) == (first, ns)
    wts = integ.ctx.last_pass_weights(npix, ns)
    return L, lam, np.asarray(pdf, np.float32), np.asarray(wts, np.float32)


def _image_flag(kernel_name):
    args = kernel_name[kernel_name.index("<") + 1:kernel_name.rindex(">")].split(", ")
    assert len(args) == 6, kernel_name
    return args[4] == "true"


def _same(a, b):
    """Per row: every float32 bit-identical, a NaN equal to a NaN."""
    a = np.ascontiguousarray(a, np.float32).reshape(len(a), -1)
    b = np.ascontiguousarray(b, np.float32).reshape(len(b), -1)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all(axis=1)


# ---------------------------------------------------------------------------
# the device functions against the host-compiled header

@pytest.mark.parametrize("case", list(ll.LISTS))
def test_probes_and_picks_equal_the_header(case):
    scene = ll.scene_for(case)
    integ = _integrator(scene)
    try:
        for index, light in enumerate(scene.lights):
            if light.type_id < 3:
                continue
            p = ll.probe_points(scene, index)
            lam = lc.probe_lambdas(len(p))
            u2 = np.zeros((len(p), 2), np.float32)
            wi, ps, Ls, r = integ.ctx.light_probe_at(index, u2, p, lam)
            hwi, hLi, hr, _ = ll.hdr_sample(scene, index, p, lam)
            shares = [float(_same(a, b).mean()) for a, b in ((wi, hwi), (Ls, hLi), (r.reshape(-1, 1), hr.reshape(-1, 1)))]
            print(f"{case} light {index} (type {light.type_id}, {len(p)} probes): bit-identical wi {shares[0]:.5f}, "
                  f"Ls {shares[1]:.5f}, distance {shares[2]:.5f}")
            assert shares == [1.0, 1.0, 1.0]
            assert np.array_equal(ps, np.where((hLi != 0).any(axis=1), 1.0, 0.0).astype(np.float32))
        got = integ.ctx.light_bvh()
        want = ll.hdr_build(scene)
        for k in ("phi", "w", "qcos", "qb", "link", "leaf", "all_bounds"):
            assert np.array_equal(got[k], want[k]), (case, k)
        assert got["n_infinite"] == want["n_infinite"]
        p, u = ll.pick_inputs()
        idx, pmf = integ.ctx.light_pick_at(u, p)
        hidx, hpmf = ll.hdr_pick(scene, p, u)
        si, sp = float((idx == hidx).mean()), float(_same(pmf.reshape(-1, 1), hpmf.reshape(-1, 1)).mean())
        print(f"{case}: {len(u)} picks, index {si:.5f}, pmf {sp:.5f} bit-identical; no light {float((idx < 0).mean()):.3f}")
        assert si == 1.0 and sp == 1.0
    finally:
        integ.close()


# ---------------------------------------------------------------------------
# persistent against wavefront

def _both_kernels(scene, lightsampler, npix=NPIX, first=0, ns=SPP, **kw):
    out = {}
    for kernel in ("persistent", "wavefront"):
        integ = _integrator(scene, lightsampler, kernel=kernel, **kw)
        try:
            rgb, w = integ.render(first, first + ns)
            out[kernel] = (_records(integ, npix, first, ns), rgb, w)
            if kernel == "persistent":
                name = integ.ctx.last_kernel()
                assert _image_flag(name) and ll.is_general(scene), name
                out["name"] = name
        finally:
            integ.close()
    return out


@pytest.mark.parametrize("sampler", ["independent", "zsobol"])
@pytest.mark.parametrize("lightsampler", ll.SAMPLERS)
@pytest.mark.parametrize("case", list(ll.LISTS))
def test_persistent_equals_wavefront(case, lightsampler, sampler):
    scene = ll.scene_for(case, sampler=sampler)
    out = _both_kernels(scene, lightsampler)
    a, b = out["persistent"][0], out["wavefront"][0]
    frac = lc.exact_fraction(a, b)
    L = a[0]
    lit = float((L != 0).any(axis=1).mean())
    print(f"{case}/{lightsampler}/{sampler}: {out['name']}, bit-identical records {frac:.5f}, lit samples {lit:.3f}, "
          f"mean L {float(np.nanmean(L)):.4g}")
    assert frac == 1.0
    assert np.isfinite(L).all() and lit > 0.2


def test_persistent_equals_wavefront_with_a_wide_zsobol_index():
    """2048 x 2 pixels at pixelsamples 4096: the sample index needs 34 bits (the 64-bit ZSobol
    instantiation), three samples of it."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import RGBFilm, Scene, ZSobolSampler
    base = scenes.s_uniform(n=1, width=2048, height=2, variant="scatter")
    small = ll.scene_for("point+distant")
    scene = Scene(base.camera, RGBFilm(2048, 2), small.medium, small.lights, sampler=ZSobolSampler(4096))
    out = _both_kernels(scene, "bvh", npix=2048 * 2, first=4093, ns=3, spp=4096)
    assert out["name"].startswith("k_paths<false, true, 3,"), out["name"]
    frac = lc.exact_fraction(out["persistent"][0], out["wavefront"][0])
    print(f"64-bit ZSobol index: {out['name']}, bit-identical records {frac:.5f}")
    assert frac == 1.0


def test_a_spot_light_with_the_whole_sphere_is_a_point_light():
    from acceleratedvolrenderer_amd.scene import PointLight, SpotLight
    films = []
    for light in (PointLight(from_=(0.3, 0.7, 0.4), scale=2.0),
                  SpotLight(from_=(0.3, 0.7, 0.4), to=(0.3, 0.7, 1.4), coneangle=180.0, conedeltaangle=0.0, scale=2.0)):
        integ = _integrator(ll.scene_of([light]), "uniform")
        try:
            films.append(integ.render() + _records(integ))
        finally:
            integ.close()
    assert films[0][0].any()
    assert lc.exact_fraction(films[0][2:], films[1][2:]) == 1.0
    assert np.array_equal(films[0][0], films[1][0]) and np.array_equal(films[0][1], films[1][1])


def test_an_interface_sphere_with_a_light_inside_and_one_outside():
    scene = ll.scene_of(["p-centre", "p-outside"], interface_sphere=((0.5, 0.5, 0.5), 0.45))
    out = _both_kernels(scene, "bvh")
    a, b = out["persistent"][0], out["wavefront"][0]
    frac = lc.exact_fraction(a, b)
    print(f"interface sphere: bit-identical records {frac:.5f}, lit {float((a[0] != 0).any(axis=1).mean()):.3f}")
    assert frac == 1.0
    assert np.isfinite(a[0]).all() and a[0].any()


# ---------------------------------------------------------------------------
# anchors to the oracle

ANCHORS = {
    # name: (device lights, oracle lights, light sampler)
    "uniform: [D, point I = 0] == [D, black D]": (["distant-base", "p-zero"], ["distant-base", "distant-zero"], "uniform"),
    "bvh: [D, point I = 0] == [D]": (["distant-base", "p-zero"], ["distant-base"], "bvh"),
    "bvh: [D, spot aimed away] == [D, black D]": (["distant-base", "s-away"], ["distant-base", "distant-zero"], "bvh"),
    "bvh: [U, spot aimed away] == [U, black D]": (["uniform-d65", "s-away"], ["uniform-d65", "distant-zero"], "bvh"),
}


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("anchor", list(ANCHORS))
def test_a_light_that_contributes_nothing_leaves_the_oracles_render(anchor, kernel):
    from oracle import binding
    dev, orc, sampler = ANCHORS[anchor]
    want_scene = ll.scene_of(orc)
    run = binding.OracleRun(want_scene, max_depth=MAXDEPTH, seed=0, libm="canonical", lightsampler=sampler)
    want = fc.oracle_records(run, W, H, 0, SPP)
    integ = _integrator(ll.scene_of(dev), sampler, kernel=kernel)
    try:
        integ.render()
        got = _records(integ)
        frac = lc.exact_fraction(got, want)
        print(f"{anchor} ({kernel}): bit-identical samples {frac:.5f}, lit {float((want[0] != 0).any(axis=1).mean()):.3f}")
        assert (want[0] != 0).any()
        assert frac == 1.0
        if kernel == "persistent":
            assert _image_flag(integ.ctx.last_kernel())
    finally:
        integ.close()


# ---------------------------------------------------------------------------
# a known answer

SIG_A, SIG_S, HG_G = 0.5, 1.0, 0.3
SIG_T = SIG_A + SIG_S
CROP = (0, 0, 4, 12)            # pixels whose rays pass >= 0.3 from the light at the box centre
KA_LIGHTS = {
    # name: (samples per pixel, (coneangle, conedeltaangle) or None). Chosen so that the standard error
    # of a 4 x 4 block is below 1 % of G. A sample is 0 (absorbed or through) or p_HG T / r^2, where T is
    # ratio tracking against the homogeneous medium's own sigma_t as majorant: 1 or 0 with mean
    # e^{-sigma_t r}. The relative spread per sample of that estimator is about 2.1 for the point light
    # and 6.2 for the blocks the cone's edge crosses, so 16 pixels x spp samples give 0.6 % of G in
    # either case, which leaves room for the +-18 % by which a spread estimated from 16 batches
    # itself scatters. (Measured on the MI355X: 0.4 to 0.75 % of G.)
    "point": (8192, None),
    "spot": (65536, (40.0, 15.0)),
}


def _hg(c):
    d = 1 + HG_G * HG_G + 2 * HG_G * c
    return (1 - HG_G * HG_G) / (4 * np.pi * d * np.sqrt(d))


_quad = {}


def _quadrature(x0, x1, y0, y1, cone, nxy, ns):
    key = (x0, x1, y0, y1, cone, nxy, ns)
    if key not in _quad:
        _quad[key] = _quadrature_once(*key)
    return _quad[key]


def _quadrature_once(x0, x1, y0, y1, cone, nxy, ns):
    """The block mean of G = int sigma_s e^{-sigma_t s} p_HG(cos theta) e^{-sigma_t r} / r^2 ds (times
    the smoothstep of the cone) over world [x0, x1] x [y0, y1], rays along +z from z = 0 to 1: midpoint
    rule, float64."""
    xs = x0 + (np.arange(nxy) + 0.5) / nxy * (x1 - x0)
    ys = y0 + (np.arange(nxy) + 0.5) / nxy * (y1 - y0)
    s = (np.arange(ns) + 0.5) / ns
    X, Y, S = np.meshgrid(xs, ys, s, indexing="ij")
    v = np.stack([0.5 - X, 0.5 - Y, 0.5 - S], -1)
    r2 = (v * v).sum(-1)
    wi = v / np.sqrt(r2)[..., None]
    f = SIG_S * np.exp(-SIG_T * S) * _hg(-wi[..., 2]) * np.exp(-SIG_T * np.sqrt(r2)) / r2     # wo = (0, 0, -1)
    if cone is not None:
        ce, cs = np.cos(np.radians(cone[0])), np.cos(np.radians(cone[0] - cone[1]))
        t = np.clip((wi[..., 0] - ce) / (cs - ce), 0, 1)       # the spot light looks down -x: cos = (-wi) . (-1, 0, 0)
        f = f * t * t * (3 - 2 * t)
    return float(f.mean())


@pytest.mark.parametrize("mode", ["replay", "fast"])
@pytest.mark.parametrize("name", list(KA_LIGHTS))
def test_single_scattering_equals_the_quadrature(name, mode):
    from acceleratedvolrenderer_amd import spectra
    from acceleratedvolrenderer_amd.scene import HomogeneousMedium, PointLight, RGBFilm, SpotLight
    spp, cone = KA_LIGHTS[name]
    phot = float(spectra.spectrum_to_photometric(spectra.constant(1.0)))     # scale * I = 1
    if cone is None:
        light = PointLight(from_=(0.5, 0.5, 0.5), I=1.0, scale=phot)
    else:
        light = SpotLight(from_=(0.5, 0.5, 0.5), to=(0.0, 0.5, 0.5), I=1.0, scale=phot, coneangle=cone[0],
                          conedeltaangle=cone[1])
    assert abs(float(light.scale) * 1.0 - 1) < 1e-6
    med = HomogeneousMedium(sigma_a=SIG_A, sigma_s=SIG_S, g=HG_G)
    scene = ll.scene_of([light], medium=med, film=RGBFilm(W, H, pixelbounds=(CROP[0], CROP[2], CROP[1], CROP[3])),
                        spp=spp)
    cw, ch = CROP[2] - CROP[0], CROP[3] - CROP[1]
    npix, nb, per = cw * ch, 16, spp // 16
    integ = _integrator(scene, "bvh", maxdepth=1, spp=spp, mode=mode)
    try:
        # per batch of sample indices the mean L of every 4 x 4 block and channel
        means = np.zeros((nb, ch // 4, 4))
        for b in range(nb):
            integ.render(b * per, (b + 1) * per)
            L = _records(integ, npix, b * per, per)[0].astype(np.float64).reshape(per, ch, cw, 4)
            assert np.isfinite(L).all()
            means[b] = L.reshape(per, ch // 4, 4, cw, 4).mean(axis=(0, 2, 3))
        assert _image_flag(integ.ctx.last_kernel())
    finally:
        integ.close()
    est = means.mean(axis=0)
    se = means.std(axis=0, ddof=1) / np.sqrt(nb)
    worst = 0.0
    for k in range(ch // 4):
        y1, y0 = 1 - 4 * k / H, 1 - 4 * (k + 1) / H            # raster y runs down
        G = _quadrature(CROP[0] / W, CROP[2] / W, y0, y1, cone, 48, 1500)
        coarse = _quadrature(CROP[0] / W, CROP[2] / W, y0, y1, cone, 24, 750)
        print(f"{name}/{mode} block {k}: G {G:.6g} (half the steps: {coarse / G - 1:+.2e}), estimate "
              f"{est[k].round(6)}, standard error / G {(se[k] / G).round(5)}, deviation in standard errors "
              f"{((est[k] - G) / se[k]).round(2)}")
        assert abs(coarse / G - 1) < 2e-3
        assert (se[k] <= 0.01 * G).all()
        assert (np.abs(est[k] - G) <= 5 * se[k]).all()
        worst = max(worst, float(np.abs((est[k] - G) / se[k]).max()))
    # a lost 1 / 4 pi, sigma_s or r^2 is off by far more than 5 standard errors of 1 %
    assert worst <= 5


# ---------------------------------------------------------------------------
# errors

def test_errors():
    from acceleratedvolrenderer_amd import capi
    from acceleratedvolrenderer_amd.capi import _fp
    scene = ll.scene_for("point+distant")
    integ = _integrator(scene)
    try:
        lib, h = integ.ctx.lib, integ.ctx.h
        eye = np.eye(4, dtype=np.float32)
        # avr_light_local on a light of type 0
        assert lib.avr_light_local(h, 1, _fp(eye), _fp(eye), 1.0, -1.0) == AVR_ERR_ARG
        assert lib.avr_light_local(h, 5, _fp(eye), _fp(eye), 1.0, -1.0) == AVR_ERR_ARG
        assert lib.avr_light_sampler(h, 3) == AVR_ERR_ARG
        # the list given again without avr_light_local: no render, no probe, no pick
        types = np.ascontiguousarray(scene.light_types, np.int32)
        w, L, sc = (np.ascontiguousarray(a, np.float32) for a in (scene.light_w, scene.light_L, scene.light_scale))
        assert lib.avr_lights(h, 2, types.ctypes.data_as(capi.c_int_p), _fp(w), _fp(L), _fp(sc), float(scene.scene_radius)) == 0
        assert lib.avr_render(h, 0, 1, 0, MAXDEPTH) == AVR_ERR_STATE
        assert b"avr_light_local" in lib.avr_last_error()
        u = np.zeros(1, np.float32)
        idx, pmf = np.zeros(1, np.int32), np.zeros(1, np.float32)
        assert lib.avr_light_pick(h, 1, _fp(u), idx.ctypes.data_as(capi.c_int_p), _fp(pmf)) == AVR_ERR_STATE
        rfl, lfr = np.ascontiguousarray(scene.light_rfl[0], np.float32), np.ascontiguousarray(scene.light_lfr[0], np.float32)
        assert lib.avr_light_local(h, 0, _fp(rfl), _fp(lfr), 1.0, -1.0) == 0
        assert lib.avr_render(h, 0, 1, 0, MAXDEPTH) == 0
        # nine lights
        t9 = np.zeros(9, np.int32)
        assert lib.avr_lights(h, 9, t9.ctypes.data_as(capi.c_int_p), _fp(w), _fp(L), _fp(sc), 1.0) == AVR_ERR_ARG
    finally:
        integ.close()
    # the graph render takes exactly one distant light: its own error
    idx = capi.GraphIndex(np.array([[0.5, 0.5, 0.5]], np.float32), np.array([1.0], np.float32), None, radius=0.1)
    ctx = capi.Context(0)
    try:
        ctx.set_scene(ll.scene_for("point"))
        with pytest.raises(RuntimeError, match="avr error 3.*one distant light"):
            ctx.graph_render(idx, 0, 1, 0)
    finally:
        ctx.close()
