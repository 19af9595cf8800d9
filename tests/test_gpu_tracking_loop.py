"""k_paths' tracking loop (DESIGN §4 "DDA walk"): the walk's trip is straight-line code whose
candidate test and RNG advance are committed by select, and the DDA-step count is summed per
walk instead of per trip. Neither may change a sample, and no schedule may change a counter.

Every case renders a small S-cloud scene (distant light + sky, maxdepth 100: medium lanes and
shadow lanes both reach collisions in every pass, which each case asserts from the two lookup
counters; that they share collision rounds follows from the wave schedule and is not asserted)
with the persistent kernel in replay mode, reads every sample
of the pass back and compares it bit for bit with the canonical CPU oracle (exact == total):
ZSobol + Gaussian and independent + box, a 32^3 cloud grid and a non-cubic 8 x 32 x 16 grid, a
47 x 31 and a 3 x 2 film, 64 sample indices, DDA budgets 1, 2 and 10 under refill thresholds 1
and 32 with batch 1. With budget 1 every walk ends on the budget, and on the 3 x 2 film (384
ids: six lanes of waves that are otherwise empty) nearly every lane of a wave computes the
trip's selects on stale state.

The density layouts (fat, linear, brick) give array_equal films and equal lookup counters; the
work counters (DDA steps, medium and shadow lookups) are properties of the samples and equal
under every budget and threshold. The oracle's samples of a scene are computed once and shared."""
import ctypes
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAXDEPTH = 100
NS = 64
SAMPLERS = {"zsobol": ("zsobol", "gaussian"), "independent": ("independent", "box")}
FILMS = {"47x31": (47, 31), "3x2": (3, 2)}
COUNTERS = ("medium_dda_steps", "medium_lookups", "shadow_lookups")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()


@pytest.fixture(scope="module")
def grids():
    """name -> density (nz, ny, nx): the 32^3 S-cloud grid and an 8 x 32 x 16 part of it."""
    from oracle import binding
    cube = binding.cloud_grid(32)
    slab = np.ascontiguousarray(cube[8:24, :, 12:20])
    assert slab.shape == (16, 32, 8) and float(slab.max()) > 0
    cube.setflags(write=False)
    slab.setflags(write=False)
    return {"32x32x32": cube, "8x32x16": slab}


@pytest.fixture(scope="module")
def oracle_cache():
    """(grid, sampler, film) -> (L, lambda) of the oracle's NS x npix samples; read-only once made."""
    return {}


def _scene(grids, grid, sampler, film):
    from acceleratedvolrenderer_amd import scenes
    smp, flt = SAMPLERS[sampler]
    w, h = FILMS[film]
    return scenes.s_cloud(grids[grid], width=w, height=h, sampler=smp, spp=NS, filter=flt)


def _oracle(cache, key, scene):
    from oracle import binding
    if key not in cache:
        canon = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
        film = scene.film
        npix = film.width * film.height
        L = np.zeros((NS * npix, 4), np.float32)
        lam = np.zeros((NS * npix, 4), np.float32)
        pdf = np.zeros(4, np.float32)
        w = np.zeros(1, np.float32)
        binding.set_libm(canon.libm)
        fn, s = binding.lib().oracle_pixel_sample, ctypes.byref(canon.s)
        fpp = ctypes.POINTER(ctypes.c_float)
        pL, pl = L.ctypes.data, lam.ctypes.data
        for j in range(NS):
            for pix in range(npix):
                g = 16 * (j * npix + pix)
                fn(s, pix % film.width, pix // film.width, j, ctypes.cast(pL + g, fpp), ctypes.cast(pl + g, fpp),
                   binding.fp(pdf), binding.fp(w))
        L.setflags(write=False)
        lam.setflags(write=False)
        cache[key] = (L, lam)
    return cache[key]


def _render(scene, budget=0, threshold=0, batch=0, layout="fat", samples=True):
    """One pass of NS sample indices: (stats, samples or None, film rgb, film weights)."""
    from acceleratedvolrenderer_amd import VolPathIntegrator
    film = scene.film
    npix = film.width * film.height
    integ = VolPathIntegrator(scene, maxdepth=MAXDEPTH, spp=NS, seed=0, device=0, grid_layout=layout)
    try:
        assert integ.ctx.grid_layout_active() == {"linear": 0, "fat": 1, "brick": 2}[layout]
        integ.ctx.set_dda_budget(budget)
        integ.ctx.set_refill_min(threshold)
        integ.ctx.set_refill_batch(batch)
        integ.ctx.film_clear()
        integ.ctx.reset_stats()
        integ.ctx.render(0, NS, 0, MAXDEPTH)
        got = None
        if samples:
            first, ns, L, lam, _ = integ.ctx.last_pass_samples(npix, NS)
            assert (first, ns) == (0, NS)
            got = (L, lam)
        st = integ.ctx.stats()
        assert st["medium_items_in"] == NS * npix and st["medium_launches"] == 1
        rgb, w = integ.ctx.film_read(npix)
        return st, got, rgb, w
    finally:
        integ.close()


@pytest.mark.parametrize("threshold", [1, 32])
@pytest.mark.parametrize("budget", [1, 2, 10])
@pytest.mark.parametrize("film", sorted(FILMS))
@pytest.mark.parametrize("grid", ["32x32x32", "8x32x16"])
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
def test_replay_is_bit_exact(grids, oracle_cache, sampler, grid, film, budget, threshold):
    scene = _scene(grids, grid, sampler, film)
    t0 = time.perf_counter()
    Lo, lo = _oracle(oracle_cache, (grid, sampler, film), scene)
    t1 = time.perf_counter()
    st, (L, lam), _, _ = _render(scene, budget=budget, threshold=threshold, batch=1)
    same = np.all(L.view(np.uint32) == Lo.view(np.uint32), axis=1) & np.all(lam.view(np.uint32) == lo.view(np.uint32), axis=1)
    exact, total = int(same.sum()), len(same)
    print(f"budget {budget}, threshold {threshold}: {exact}/{total} samples bit-identical, "
          f"{st['medium_dda_steps']} DDA steps, {st['medium_lookups']} + {st['shadow_lookups']} lookups, "
          f"oracle {t1 - t0:.2f} s, render {time.perf_counter() - t1:.2f} s")
    assert total == NS * scene.film.width * scene.film.height
    assert exact == total
    # both kinds of lane reached collisions in this pass (not: in the same round)
    assert st["medium_lookups"] > 0 and st["shadow_lookups"] > 0 and st["medium_dda_steps"] > 0


@pytest.mark.parametrize("grid", ["32x32x32", "8x32x16"])
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
def test_counters_do_not_depend_on_the_schedule(grids, sampler, grid):
    """DDA steps and lookups are counted per sample: the same under every DDA budget and refill
    threshold (the budget only cuts a walk into more trips, the threshold moves samples between
    lanes)."""
    scene = _scene(grids, grid, sampler, "47x31")
    seen = {}
    for budget, threshold in ((1, 1), (2, 32), (10, 32), (10, 1), (1, 32), (0, 0)):
        st, _, _, _ = _render(scene, budget=budget, threshold=threshold, batch=1 if threshold else 0, samples=False)
        seen[(budget, threshold)] = tuple(st[k] for k in COUNTERS)
    print(seen)
    assert all(v > 0 for v in seen[(1, 1)])
    assert len(set(seen.values())) == 1, seen


@pytest.mark.parametrize("grid", ["32x32x32", "8x32x16"])
@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
def test_layouts_render_the_same_film(grids, oracle_cache, sampler, grid):
    """grid_layout fat, linear and brick: array_equal films and samples, equal lookup counters;
    the fat one's samples are the oracle's."""
    scene = _scene(grids, grid, sampler, "47x31")
    out = {layout: _render(scene, layout=layout) for layout in ("fat", "linear", "brick")}
    Lo, lo = _oracle(oracle_cache, (grid, sampler, "47x31"), scene)
    st0, (L0, lam0), rgb0, w0 = out["fat"]
    assert np.array_equal(L0.view(np.uint32), Lo.view(np.uint32)) and np.array_equal(lam0.view(np.uint32), lo.view(np.uint32))
    for layout in ("linear", "brick"):
        st, (L, lam), rgb, w = out[layout]
        assert np.array_equal(rgb, rgb0) and np.array_equal(w, w0), layout
        assert np.array_equal(L.view(np.uint32), L0.view(np.uint32)), layout
        assert tuple(st[k] for k in COUNTERS) == tuple(st0[k] for k in COUNTERS), layout
