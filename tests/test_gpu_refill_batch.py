"""k_paths' two-parameter wave schedule (DESIGN §4 "Refill and events"): the service threshold
(set_refill_min) and the refill batch (set_refill_batch).

Which lane renders which sample id, and in which service round, enters no sample. So every case
renders a small scene in replay mode under one schedule (threshold, batch) and compares every
sample of every pass bit for bit against the canonical CPU oracle (last_pass_samples against
oracle_pixel_sample, as tests/test_gpu_kpaths_service.py does), asks that every sample id was
started exactly once (medium_items_in == N), that no pass was dropped (medium_launches) and that
no pass found stale work heads (stats() raises on stats[7] != 0). A schedule that leaves a lane
state unserved would hang, not miscompute: the two termination arms (no lane busy: the tracking
loop ends and the refill runs whatever the batch) are what the small shapes below lean on.

Shapes: a 32^3 S-cloud under a 24 x 16 film, passes of 8 sample indices, ZSobol, under eager
(batch 1), batched-at-threshold, small, large (64: every lane) and unit thresholds, a batch above
the threshold (40, 64: only the no-lane-busy arm ever refills) and the default (0, 0); the
independent sampler, a NanoVDB medium and a chromatic emissive grid (the non-parked family) under
(32, 1) and (1, 1), and a gray emissive grid under those and its default (the coupled schedule).
One case asks that the batch reaches the kernel: the wave loop's iteration count tells (32, 1)
from (32, 32). Every case prints its tracking iterations and its seconds. Claim and lane boundaries with batch 1 and 64: 15 ids (less than a wave and
than any threshold), 63 / 64 / 65 (one wave's lanes), 255 / 256 / 257 (one claim) and 315 (a claim
and a part). The oracle's samples of a scene are computed once and shared by its schedules."""
import ctypes
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAXDEPTH = 100
W, H = 24, 16
GRAY = "k_paths<false, true, 2, 0, false, false>"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()


@pytest.fixture(scope="module")
def density():
    from oracle import binding
    return binding.cloud_grid(32)


@pytest.fixture(scope="module")
def oracle_cache():
    """(scene key, first, ns) -> (L, lambda) of the oracle; read-only once made."""
    return {}


def _cloud(density, sampler="zsobol", filter="gaussian", width=W, height=H):
    from acceleratedvolrenderer_amd import scenes
    return scenes.s_cloud(density, width=width, height=height, sampler=sampler, spp=64, filter=filter)


def _oracle_pass(cache, key, scene, first, ns):
    from oracle import binding
    k = (key, first, ns)
    if k not in cache:
        canon = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
        film = scene.film
        npix = film.width * film.height
        L = np.zeros((ns * npix, 4), np.float32)
        lam = np.zeros((ns * npix, 4), np.float32)
        pdf = np.zeros(4, np.float32)
        w = np.zeros(1, np.float32)
        binding.set_libm(canon.libm)
        fn, s = binding.lib().oracle_pixel_sample, ctypes.byref(canon.s)
        fpp = ctypes.POINTER(ctypes.c_float)
        pL, pl = L.ctypes.data, lam.ctypes.data
        for j in range(ns):
            for pix in range(npix):
                g = 16 * (j * npix + pix)
                fn(s, pix % film.width, pix // film.width, first + j, ctypes.cast(pL + g, fpp), ctypes.cast(pl + g, fpp),
                   binding.fp(pdf), binding.fp(w))
        L.setflags(write=False)
        lam.setflags(write=False)
        cache[k] = (L, lam)
    return cache[k]


def _check(cache, key, scene, passes, schedule, kernel=None, overlap=None, want_active=None, last_only=False):
    """Render the passes under schedule = (threshold, batch); every sample of every pass read back
    equals the oracle's bit for bit, every id is started once and no pass is dropped."""
    from acceleratedvolrenderer_amd import VolPathIntegrator
    film = scene.film
    npix = film.width * film.height
    integ = VolPathIntegrator(scene, maxdepth=MAXDEPTH, spp=64, seed=0, device=0)
    t0 = time.perf_counter()
    try:
        integ.ctx.set_refill_min(schedule[0])
        integ.ctx.set_refill_batch(schedule[1])
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
            if kernel is not None:
                name = integ.ctx.last_kernel()
                assert name == kernel if isinstance(kernel, str) else (name.startswith(kernel[0]) and
                                                                       name.endswith(kernel[1])), name
            started += ns * npix
            if last_only and i + 1 < len(passes):
                continue
            got_first, got_ns, L, lam, _ = integ.ctx.last_pass_samples(npix, ns)
            assert (got_first, got_ns) == (first, ns)
            Lo, lo = _oracle_pass(cache, key, scene, first, ns)
            same = np.all(L.view(np.uint32) == Lo.view(np.uint32), axis=1) & \
                np.all(lam.view(np.uint32) == lo.view(np.uint32), axis=1)
            exact += int(same.sum())
            total += ns * npix
        st = integ.ctx.stats()
        print(f"schedule {schedule}: {exact}/{total} samples bit-identical, {st['medium_items_in']} paths started, "
              f"{st['loop_iterations']} tracking iterations, {time.perf_counter() - t0:.2f} s")
        assert exact == total
        assert st["medium_items_in"] == started
        assert st["medium_launches"] == len(passes)
        if want_active is not None:
            assert active == want_active
        return st
    finally:
        integ.close()


@pytest.mark.parametrize("schedule", [(32, 1), (32, 32), (12, 1), (64, 1), (1, 1), (24, 8), (40, 64), (0, 0)],
                         ids=lambda s: f"{s[0]}-{s[1]}")
def test_zsobol_cloud_schedules(density, oracle_cache, schedule):
    _check(oracle_cache, "cloud", _cloud(density), [(0, 8)], schedule, kernel=GRAY)


@pytest.mark.parametrize("schedule", [(32, 1), (1, 1)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_independent_sampler(density, oracle_cache, schedule):
    scene = _cloud(density, sampler="independent", filter="box")
    _check(oracle_cache, "independent", scene, [(0, 8)], schedule, kernel="k_paths<false, true, 0, 0, false, false>")


@pytest.mark.parametrize("schedule", [(32, 1), (1, 1)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_nanovdb(density, oracle_cache, schedule):
    from acceleratedvolrenderer_amd import scenes
    scene = scenes.s_cloud_vdb(density, width=W, height=H, sampler="zsobol", spp=64, filter="gaussian")
    _check(oracle_cache, "nanovdb", scene, [(0, 8)], schedule, kernel=("k_paths<false, ", ", 3, false, false>"))


@pytest.mark.parametrize("schedule", [(32, 1), (1, 1)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_chromatic_emissive_not_parked(oracle_cache, schedule):
    from acceleratedvolrenderer_amd import scenes
    dens = (0.25 + np.random.default_rng(5).random((32, 32, 32), dtype=np.float32)).astype(np.float32)
    scene = scenes.s_uniform(n=32, width=W, height=H, variant="emissive_chromatic", density=dens)
    _check(oracle_cache, "chromatic", scene, [(0, 8)], schedule, kernel=("k_paths<true, false, ", ", 0, false, false>"))


@pytest.mark.parametrize("schedule", [(32, 1), (1, 1), (0, 0)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_gray_emissive_grid(oracle_cache, schedule):
    """The gray emissive family (k_paths<true, true, ...>): its default is the coupled schedule."""
    from acceleratedvolrenderer_amd import scenes
    dens = (0.25 + np.random.default_rng(6).random((32, 32, 32), dtype=np.float32)).astype(np.float32)
    scene = scenes.s_uniform(n=32, width=W, height=H, variant="emissive", density=dens)
    _check(oracle_cache, "gray_emissive", scene, [(0, 8)], schedule, kernel=("k_paths<true, true, ", ", 0, false, false>"))


def test_the_batch_reaches_the_kernel(density, oracle_cache):
    """No schedule changes a sample, so the cases above would pass with a setter that did nothing.
    The wave loop's own counter tells the schedules apart: at threshold 32, waves that refill at
    every round track with fuller waves than waves that hold finished lanes until 32 wait, so
    they take fewer tracking iterations for the same samples (a third fewer on the flagship
    cloud). Which wave claims which ids varies from run to run and the counts with it, so the
    gray grid's default, batch 1, is compared with the batched count too, not with (32, 1)'s."""
    scene = _cloud(density)
    it = {sch: _check(oracle_cache, "cloud", scene, [(0, 8)], sch, kernel=GRAY)["loop_iterations"]
          for sch in ((32, 1), (32, 32), (0, 0))}
    print(it)
    assert it[(32, 1)] < it[(32, 32)]
    assert it[(0, 0)] < it[(32, 32)]


# (width, height, sample indices): the ids of one pass
BOUNDARIES = {15: (5, 3, 1), 63: (9, 7, 1), 64: (8, 8, 1), 65: (13, 5, 1), 255: (17, 15, 1), 256: (16, 16, 1),
              257: (257, 1, 1), 315: (7, 9, 5)}


@pytest.mark.parametrize("batch", [1, 64])
@pytest.mark.parametrize("ids", sorted(BOUNDARIES))
def test_claim_and_lane_boundaries(density, oracle_cache, ids, batch):
    width, height, ns = BOUNDARIES[ids]
    assert width * height * ns == ids
    _check(oracle_cache, f"ids{ids}", _cloud(density, width=width, height=height), [(0, ns)], (0, batch), kernel=GRAY)


def test_two_passes_with_the_camera_records_made_ahead(density, oracle_cache):
    """The second call takes the camera records made beside the first (held grid of four blocks
    per CU, the other set's heads), under an eager refill at threshold 24."""
    _check(oracle_cache, "cloud", _cloud(density), [(0, 8), (8, 16)], (24, 1), overlap=True,
           want_active=[False, True], last_only=True)


def test_setter_arguments():
    from acceleratedvolrenderer_amd import capi
    ctx = capi.Context(0)
    try:
        for bad in (-1, 65):
            with pytest.raises(RuntimeError, match="refill batch"):
                ctx.set_refill_batch(bad)
        ctx.set_refill_batch(64)
        ctx.set_refill_batch(0)
    finally:
        ctx.close()
