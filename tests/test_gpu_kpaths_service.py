"""k_paths' service round: the light records its handlers read from LDS and the way a
wave claims sample ids from the work heads.

Neither enters a sample's arithmetic: the staged records hold the device array's values, the
light pick's two per-launch floats are the same operations evaluated once per block, and which
lane renders which sample id changes no sample. So every case renders a small scene in replay
mode and compares every sample of every pass bit for bit against the canonical CPU oracle
(last_pass_samples against oracle_pixel_sample, as tests/test_gpu_parity.py does), asks that
every sample id was started exactly once (medium_items_in == N) and that no pass found stale
work heads (stats() raises on stats[7] != 0).

Shapes: a 32^3 GridMedium under a 48 x 32 film, 8-16 sample indices in 1-3 passes. Light sets
from none to six: up to four are staged in LDS, the fifth and sixth (one distant, one infinite)
take the device array in the NEE spawn, the shadow ray's end and the escape. One emissive
chromatic, one gray emissive, one NanoVDB and one independent-sampler case run the other
instantiation families, and the power light sampler the image-light one (no staged records).
Sample counts N per pass: fewer than 8 (some XCD ranges are empty), fewer than one wave, odd
(no multiple of 8 or of a claim), and a little more than 64 per block of the persistent grid,
where most waves find every head used up at their first claim."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAXDEPTH = 100
W, H = 48, 32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()


@pytest.fixture(scope="module")
def density():
    from oracle import binding
    return binding.cloud_grid(32)


def _lights(kind):
    from acceleratedvolrenderer_amd.scene import DistantLight, UniformInfiniteLight
    key = DistantLight(from_=(0.7, 1.0, 0.6), to=(0.0, 0.0, 0.0), scale=3.0)
    sky = UniformInfiniteLight(scale=0.15)
    more = [DistantLight(from_=(-1.0, 0.4, -0.8), to=(0.0, 0.0, 0.0), scale=1.25),
            UniformInfiniteLight(scale=0.05),
            DistantLight(from_=(0.1, -1.0, 0.3), to=(0.0, 0.0, 0.0), scale=2.0),
            UniformInfiniteLight(scale=0.1)]
    return {"none": [], "distant": [key], "distant_sky": [key, sky], "four": [key, sky] + more[:2],
            "five": [key, sky] + more[:3], "six": [key, sky] + more}[kind]


def _scene(density, lights=None, sampler="zsobol", filter="gaussian", width=W, height=H):
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import Scene
    base = scenes.s_cloud(density, width=width, height=height, sampler=sampler, spp=64, filter=filter)
    if lights is None:
        return base
    return Scene(base.camera, base.film, base.medium, lights, sampler=base.sampler)


def _oracle_pass(canon, film, first, ns):
    """(L, lambda) of the pass's samples from the oracle, in the device's record order."""
    from oracle import binding
    npix = film.width * film.height
    L = np.zeros((ns * npix, 4), np.float32)
    lam = np.zeros((ns * npix, 4), np.float32)
    pdf = np.zeros(4, np.float32)
    w = np.zeros(1, np.float32)
    binding.set_libm(canon.libm)
    fn, s = binding.lib().oracle_pixel_sample, ctypes.byref(canon.s)
    fpp = ctypes.POINTER(ctypes.c_float)
    pL, pl = L.ctypes.data, lam.ctypes.data
    for k in range(ns):
        for pix in range(npix):
            g = 16 * (k * npix + pix)
            fn(s, pix % film.width, pix // film.width, first + k, ctypes.cast(pL + g, fpp), ctypes.cast(pl + g, fpp),
               binding.fp(pdf), binding.fp(w))
    return L, lam


def _check_passes(scene, passes, kernel=None, overlap=None, want_active=None, last_only=False, **kw):
    """Render the passes [(first, end), ...] one call each; every sample of every pass must equal
    the oracle's bit for bit, every sample id be started once and no pass be dropped. last_only:
    read back the last pass alone (a readback between two calls discards the records made ahead)."""
    from acceleratedvolrenderer_amd import VolPathIntegrator
    from oracle import binding
    film = scene.film
    npix = film.width * film.height
    integ = VolPathIntegrator(scene, maxdepth=MAXDEPTH, spp=64, seed=0, device=0, **kw)
    try:
        canon = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
        if overlap is not None:
            integ.ctx.set_pass_overlap(overlap)
        integ.ctx.film_clear()
        integ.ctx.reset_stats()
        exact = total = started = 0
        active = []
        for i, (first, end) in enumerate(passes):
            ns = end - first
            integ.ctx.render(first, end, 0, MAXDEPTH)
            active.append(integ.ctx.pass_overlap_active())
            if kernel is not None:    # the instantiation's name, or the (start, end) of it
                name = integ.ctx.last_kernel()
                assert name == kernel if isinstance(kernel, str) else (name.startswith(kernel[0]) and
                                                                       name.endswith(kernel[1])), name
            started += ns * npix
            if last_only and i + 1 < len(passes):
                continue
            got_first, got_ns, L, lam, _ = integ.ctx.last_pass_samples(npix, ns)
            assert (got_first, got_ns) == (first, ns)
            Lo, lo = _oracle_pass(canon, film, first, ns)
            same = np.all(L.view(np.uint32) == Lo.view(np.uint32), axis=1) & \
                np.all(lam.view(np.uint32) == lo.view(np.uint32), axis=1)
            exact += int(same.sum())
            total += ns * npix
        st = integ.ctx.stats()          # raises if a pass found its work heads stale (stats[7])
        print(f"{exact}/{total} samples bit-identical, {st['medium_items_in']} paths started")
        assert exact == total
        assert st["medium_items_in"] == started
        assert st["medium_launches"] == len(passes)
        if want_active is not None:
            assert active == want_active
        return integ.film_sums()
    finally:
        integ.close()


@pytest.mark.parametrize("kind", ["none", "distant", "distant_sky", "four", "five", "six"])
def test_light_sets_replay(density, kind):
    scene = _scene(density, _lights(kind))
    rgb, _ = _check_passes(scene, [(0, 8)], kernel="k_paths<false, true, 2, 0, false, false>")
    assert (float(rgb.sum()) > 0) == (kind != "none")


def test_six_lights_chromatic_emissive_replay():
    """The 4-wavelength emissive family (not parked) with lights on both sides of kLdsLights."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import Scene
    dens = (0.25 + np.random.default_rng(5).random((32, 32, 32), dtype=np.float32)).astype(np.float32)
    base = scenes.s_uniform(n=32, width=W, height=H, variant="emissive_chromatic", density=dens)
    scene = Scene(base.camera, base.film, base.medium, _lights("six"))
    _check_passes(scene, [(0, 8)], kernel=("k_paths<true, false, ", ", 0, false, false>"))


def test_gray_emissive_replay():
    from acceleratedvolrenderer_amd import scenes
    dens = (0.25 + np.random.default_rng(6).random((32, 32, 32), dtype=np.float32)).astype(np.float32)
    scene = scenes.s_uniform(n=32, width=W, height=H, variant="emissive", density=dens)
    _check_passes(scene, [(0, 8)], kernel=("k_paths<true, true, ", ", 0, false, false>"))


def test_nanovdb_replay(density):
    from acceleratedvolrenderer_amd import scenes
    scene = scenes.s_cloud_vdb(density, width=W, height=H, sampler="zsobol", spp=64, filter="gaussian")
    _check_passes(scene, [(0, 8)], kernel=("k_paths<false, ", ", 3, false, false>"))


def test_independent_sampler_replay(density):
    scene = _scene(density, _lights("five"), sampler="independent", filter="box")
    _check_passes(scene, [(0, 8)], kernel="k_paths<false, true, 0, 0, false, false>")


def test_power_light_sampler_six_lights_replay(density):
    """The power sampler runs k_paths' image-light instantiation, which stages no records: every
    light's record and alias bin from the device array, under the chunked claims."""
    from acceleratedvolrenderer_amd import VolPathIntegrator
    from oracle import binding
    scene = _scene(density, _lights("six"))
    npix = W * H
    integ = VolPathIntegrator(scene, maxdepth=MAXDEPTH, spp=64, seed=0, device=0, lightsampler="power")
    try:
        canon = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical", lightsampler="power")
        integ.ctx.reset_stats()
        integ.ctx.render(0, 8, 0, MAXDEPTH)
        _, ns, L, lam, _ = integ.ctx.last_pass_samples(npix, 8)
        Lo, lo = _oracle_pass(canon, scene.film, 0, 8)
        assert ns == 8
        assert np.array_equal(L.view(np.uint32), Lo.view(np.uint32))
        assert np.array_equal(lam.view(np.uint32), lo.view(np.uint32))
        assert integ.ctx.stats()["medium_items_in"] == npix * 8
    finally:
        integ.close()


@pytest.mark.parametrize("width,height,ns", [(3, 2, 1), (11, 9, 1), (47, 31, 3)], ids=["N6", "N99", "N4371"])
def test_small_and_odd_sample_counts(density, width, height, ns):
    """Three passes each: N = 6 leaves two of the eight ranges empty, N = 99 is less than any
    claim, N = 4371 is odd, so the ranges' ends fall inside claims."""
    scene = _scene(density, width=width, height=height)
    _check_passes(scene, [(0, ns), (ns, 2 * ns), (2 * ns, 3 * ns)])


def test_more_samples_than_a_round_of_the_grid(density):
    """N a little over 64 per block of the persistent grid (five blocks per CU): each head is
    used up after a few claims, and most waves find nothing at their first. (A thin copy of the
    medium: short paths keep the oracle's 80 000 samples to a second or two. An id that no lane
    took leaves its record unwritten, where the sky alone makes every sample's L nonzero, and an
    id taken twice shows in the count of paths started, whatever the paths' length.)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ns = min(63, (5 * cus * 64) // (W * H) + 1)
    scene = _scene((density * np.float32(0.05)).astype(np.float32))
    _check_passes(scene, [(0, ns)], kernel="k_paths<false, true, 2, 0, false, false>")


def test_pass_overlap_takes_the_records_made_ahead(density):
    """Two equal calls with pass overlap on: the second takes the camera records made beside the
    first (the held grid of four blocks per CU claims from the other set's heads)."""
    scene = _scene(density)
    on = _check_passes(scene, [(0, 8), (8, 16)], overlap=True, want_active=[False, True], last_only=True)
    off = _check_passes(scene, [(0, 8), (8, 16)], overlap=False, want_active=[False, False])
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
