"""The light stage of the device under the maps, transforms, parameters and light lists of
tests/light_cases.py (tests/test_light_cases_reference.py holds the CPU side: the conditions on
the inputs and the oracle and scene.py against the reference's own functions).

Every other image-light test renders one 32 x 32 map, alone or beside one distant light, and checks
whole paths only; random paths almost never put a direction on an octahedral seam or a draw on a
CDF breakpoint. Here:

  * avr_light_probe (one small kernel over the device functions the path kernels call) for every
    light of every case at the CDF breakpoints of its compensated distribution with one ulp either
    side, 0, 2^-24, 0.5 and 1 - 2^-24, the axes, the equator diagonals, signed zeros and denormals,
    the square's edges and corners, random directions, the ends of the wavelength range: wi, both
    pdfs, Ls and Le bit-identical to the canonical oracle;
  * avr_light_pick and avr_light_sampler_table bit-identical to it for every case;
  * renders of every case in both kernel organisations: 100 % of the (L, lambda, pdf, weight)
    records bit-identical to the canonical oracle, the film within 0.5 x the two-seed noise of the
    platform oracle, the image instantiation of k_paths named for image and power cases;
  * ZSobol on three cases;
  * light lists replaced on one context (image lights dropped and given again): each render equals
    a fresh context's; an image light without its map after another's was given twice: AVR_ERR_STATE."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import film_cases as fc      # noqa: E402
import light_cases as lc     # noqa: E402

pytestmark = pytest.mark.gpu

SPP, MAXDEPTH = lc.SPP, lc.MAXDEPTH
NPIX = lc.W * lc.H
AVR_ERR_STATE = 3


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


def _integrator(scene, case, **kw):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    return VolPathIntegrator(scene, device=0, maxdepth=MAXDEPTH, spp=SPP, lightsampler=lc.light_sampler(case), **kw)


def _records(integ):
    first, got, L, lam, pdf = integ.ctx.last_pass_samples(NPIX, SPP)
    assert (first, got) == (0, SPP)
    wts = integ.ctx.last_pass_weights(NPIX, SPP)
    return L, lam, np.asarray(pdf, np.float32), np.asarray(wts, np.float32)


_canon = {}


def _canonical(case, sampler="independent"):
    """(scene, canonical OracleRun, its records), once per (case, sampler)."""
    key = (case, sampler)
    if key not in _canon:
        scene, run = lc.oracle_run(case, sampler=sampler)
        _canon[key] = (scene, run, fc.oracle_records(run, lc.W, lc.H, 0, SPP))
    return _canon[key]


_platform = {}


def _rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(1e-12, np.sqrt(np.mean(b ** 2))))


def _platform_films(case, integ):
    """The platform oracle's images at seeds 0 and 1, once per case."""
    if case not in _platform:
        imgs = []
        for seed in (0, 1):
            _, run = lc.oracle_run(case, libm="platform", seed=seed)
            imgs.append(integ.image(*run.render(0, SPP, nthreads=8)))
        _platform[case] = imgs
    return _platform[case]


def _image_flag(kernel_name):
    """The image argument of "k_paths<emissive, gray, sampler, medium, image, fast>"."""
    args = kernel_name[kernel_name.index("<") + 1:kernel_name.rindex(">")].split(", ")
    assert len(args) == 6, kernel_name
    return args[4] == "true"


# ---------------------------------------------------------------------------
# renders

@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("case", lc.PAIRS)
def test_render_replays_the_oracle(case, kernel):
    scene, run, want = _canonical(case)
    integ = _integrator(scene, case, kernel=kernel)
    try:
        rgb, w = integ.render()
        assert (integ.stats()["loop_iterations"] > 0) == (kernel == "persistent")
        got = _records(integ)
        frac = lc.exact_fraction(got, want)
        img = integ.image(rgb, w)
        ref0, ref1 = _platform_films(case, integ)
        err, noise = _rel_rms(img, ref0), _rel_rms(ref1, ref0)
        print(f"{case}/{kernel}: bit-exact samples {frac:.5f}, film rel RMS {err:.3e} (two-seed noise {noise:.3e})")
        assert np.isfinite(rgb).all()
        assert frac == 1.0
        assert err <= 0.5 * noise
        if kernel == "persistent":
            name = integ.ctx.last_kernel()
            assert _image_flag(name) == lc.expected_kernel_is_image(scene, lc.light_sampler(case)), name
    finally:
        integ.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("case", lc.ZSOBOL_PAIRS)
def test_render_replays_the_oracle_zsobol(case, kernel):
    scene, run, want = _canonical(case, "zsobol")
    integ = _integrator(scene, case, kernel=kernel)
    try:
        integ.render()
        frac = lc.exact_fraction(_records(integ), want)
        print(f"{case}/zsobol/{kernel}: bit-exact samples {frac:.5f}")
        assert frac == 1.0
    finally:
        integ.close()


def test_the_staged_instantiation_without_image_lights():
    """One distant light, BVH pick: k_paths' staged (non-image) instantiation, as before."""
    from acceleratedvolrenderer_amd import VolPathIntegrator
    scene = lc.scene_for("rgb-1+rot-axis", drop=1)
    integ = VolPathIntegrator(scene, device=0, maxdepth=MAXDEPTH, spp=SPP)
    try:
        integ.render()
        assert not _image_flag(integ.ctx.last_kernel())
    finally:
        integ.close()


# ---------------------------------------------------------------------------
# the probe

def _probe_inputs(scene, index):
    light = scene.lights[index]
    if light.type_id == 2:
        u = lc.probe_u(light)
        d = lc.probe_directions(light.res, scene.light_rfl[index])
    else:
        u = np.array([(a, b) for a in lc.SPECIAL_U for b in lc.SPECIAL_U], np.float32)
        d = lc.probe_directions(4, np.eye(4), n_random=32)
    n = max(len(u), len(d))
    u = u[np.arange(n) % len(u)]
    d = d[np.arange(n) % len(d)]
    return np.ascontiguousarray(u), np.ascontiguousarray(d), lc.probe_lambdas(n)


def _assert_same(label, names, got, want):
    shares = [float(lc.same_bits(np.asarray(a).reshape(len(b), -1), np.asarray(b).reshape(len(b), -1)).mean())
              for a, b in zip(got, want)]
    print(f"{label}: bit-identical " + ", ".join(f"{n} {s:.5f}" for n, s in zip(names, shares)))
    for n, s, a, b in zip(names, shares, got, want):
        bad = ~lc.same_bits(np.asarray(a).reshape(len(b), -1), np.asarray(b).reshape(len(b), -1))
        assert s == 1.0, (label, n, int(bad.sum()), np.flatnonzero(bad)[:4], np.asarray(a)[bad][:3], np.asarray(b)[bad][:3])


@pytest.mark.parametrize("case", lc.PAIRS)
def test_probe_equals_the_oracle(case):
    scene, run, _ = _canonical(case)
    integ = _integrator(scene, case)
    try:
        for index, light in enumerate(scene.lights):
            u, d, lam = _probe_inputs(scene, index)
            # at most MAX_PROBE per call: "pole-33" takes two
            parts = [integ.ctx.light_probe(index, u[k:k + lc.MAX_PROBE], d[k:k + lc.MAX_PROBE], lam[k:k + lc.MAX_PROBE])
                     for k in range(0, len(u), lc.MAX_PROBE)]
            wi, ps, Ls, pl, Le = (np.concatenate(a) for a in zip(*parts))
            wi_o, ps_o, Ls_o = run.light_sample(index, u, lam)
            pl_o, Le_o = run.light_pdf(index, d), run.light_le(index, d, lam)
            for a in (wi_o, ps_o, Ls_o, pl_o, Le_o):
                assert np.isfinite(a).all()
            label = f"{case} light {index} (type {light.type_id}, {len(u)} probes)"
            _assert_same(label, ("wi", "pdf", "Ls", "PDF_Li", "Le"), (wi, ps, Ls, pl, Le), (wi_o, ps_o, Ls_o, pl_o, Le_o))
            if light.type_id == 1:      # allowIncompletePDF = true: no sample, PDF_Li 0
                assert not ps.any() and not pl.any() and not wi.any() and not Ls.any()
            if light.type_id == 2:
                print(f"    samples with pdf 0: {int((ps == 0).sum())}, PDF_Li 0: {int((pl == 0).sum())}, "
                      f"Le 0: {int((~Le.any(axis=1)).sum())}")
    finally:
        integ.close()


@pytest.mark.parametrize("case", lc.PAIRS)
def test_pick_and_sampler_table_equal_the_oracle(case):
    scene, run, _ = _canonical(case)
    integ = _integrator(scene, case)
    try:
        n = len(scene.lights)
        q, p, alias = integ.ctx.light_sampler_table(n)
        q_o, p_o, alias_o = run.light_sampler_table()
        print(f"{case}: q {q.tolist()} p {p.tolist()} alias {alias.tolist()}")
        assert q.view(np.uint32).tolist() == q_o.view(np.uint32).tolist()
        assert p.view(np.uint32).tolist() == p_o.view(np.uint32).tolist()
        assert alias.tolist() == alias_o.tolist()
        # the draws: the bin edges k / n with one ulp either side, the special values, random ones
        edges = lc._around(np.arange(0, n + 1, dtype=np.float32) / np.float32(n))
        u = np.unique(np.concatenate([lc.PICK_U, edges])).astype(np.float32)
        idx, pmf = integ.ctx.light_pick(u)
        idx_o, pmf_o = run.light_pick(u)
        assert idx.tolist() == idx_o.tolist()
        assert pmf.view(np.uint32).tolist() == pmf_o.view(np.uint32).tolist()
        assert set(idx.tolist()) <= set(range(n))
    finally:
        integ.close()


# ---------------------------------------------------------------------------
# state

def _ctx_render(ctx, scene):
    ctx.set_scene(scene)
    ctx.film_clear()
    ctx.render(0, SPP, 0, MAXDEPTH)
    return ctx.film_read(NPIX)


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
def test_light_lists_replaced_on_one_context(kernel):
    """set_scene("two-images"), then one distant light (avr_lights frees both maps), then
    "two-images" again: each render equals a fresh context's."""
    two = lc.scene_for("two-images")
    one = lc.scene_for("rgb-1+rot-axis", drop=1)
    fresh = {}
    for name, scene in (("two", two), ("one", one)):
        integ = _integrator(scene, "two-images", kernel=kernel)
        try:
            fresh[name] = integ.render()
        finally:
            integ.close()
    assert not np.array_equal(fresh["two"][0], fresh["one"][0])
    integ = _integrator(two, "two-images", kernel=kernel)
    try:
        for name, scene in (("two", two), ("one", one), ("two", two)):
            rgb, w = _ctx_render(integ.ctx, scene)
            assert np.array_equal(rgb, fresh[name][0]) and np.array_equal(w, fresh[name][1]), name
    finally:
        integ.close()


def test_an_image_light_without_its_map_is_refused():
    """avr_lights with two type-2 lights, then avr_light_image twice for index 0 (its map replaced):
    light 1 has no map, and avr_render and avr_light_probe return AVR_ERR_STATE."""
    from acceleratedvolrenderer_amd.capi import _fp, c_int_p
    scene = lc.scene_for("two-images")
    integ = _integrator(scene, "two-images")
    try:
        ctx = integ.ctx
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
        types = np.ascontiguousarray(scene.light_types, np.int32)
        args = [f32(scene.light_w.reshape(-1)), f32(scene.light_L.reshape(-1)), f32(scene.light_scale)]
        assert ctx.lib.avr_lights(ctx.h, 2, types.ctypes.data_as(c_int_p), *[_fp(a) for a in args],
                                  float(scene.scene_radius)) == 0
        light = scene.lights[0]
        arrs = [f32(light.coeffs), f32(light.distribution), f32(light.illuminant), f32(scene.light_rfl[0]),
                f32(scene.light_lfr[0])]
        for _ in range(2):
            assert ctx.lib.avr_light_image(ctx.h, 0, int(light.res), *[_fp(a) for a in arrs]) == 0
        assert ctx.lib.avr_render(ctx.h, 0, SPP, 0, MAXDEPTH) == AVR_ERR_STATE
        assert b"avr_light_image" in ctx.lib.avr_last_error()
        one = np.zeros(4, np.float32)
        assert ctx.lib.avr_light_probe(ctx.h, 1, 1, _fp(one), _fp(one), _fp(one), None, None, None, None,
                                       None) == AVR_ERR_STATE
        # the second light's own map completes the list
        light = scene.lights[1]
        arrs = [f32(light.coeffs), f32(light.distribution), f32(light.illuminant), f32(scene.light_rfl[1]),
                f32(scene.light_lfr[1])]
        assert ctx.lib.avr_light_image(ctx.h, 1, int(light.res), *[_fp(a) for a in arrs]) == 0
        assert ctx.lib.avr_render(ctx.h, 0, SPP, 0, MAXDEPTH) == 0
        ctx.sync()
    finally:
        integ.close()
