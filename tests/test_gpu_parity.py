"""GPU parity: the HIP path (through the C-ABI) against the CPU oracle on identical
seeded inputs. Run on an MI355X with `pytest -m gpu`.

Tolerances (stated per BASELINE.md §3 "Parity"):
  * integer / index work (majorant max, cloud generator, sample counts): bit-exact;
  * per-sample radiance: the device replays the CPU sample stream (same PCG32/Murmur
    streams, same float operation order, -ffp-contract=off) with correctly rounded
    transcendentals (log/sin/cos/atanh/cosh evaluated in f64, rounded once). The oracle's
    "canonical" libm mode implements the same convention, so replay is compared to it:
    EVERY sample bit-identical (the device and the oracle evaluate the same f64 op sequences;
    100 % observed in every round, so the tests assert equality and print the count). The oracle's default "platform" mode is pbrt as built
    here (glibc float libm, pinned by the reference goldens); the two modes agree on ~99%
    of samples (tests/test_oracle_known_answers.py), and the film test below compares the
    device to the platform mode.
  * film: relative RMS over pixels between the GPU film and the oracle film at the SAME
    seed must be <= 0.5 x the relative RMS between two oracle films at DIFFERENT seeds
    (i.e. the GPU deviates from the CPU reference by well under its own Monte Carlo
    noise), and <= 1e-6 when every sample matched.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()


def _rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(1e-12, np.sqrt(np.mean(b ** 2))))


def _oracle_noise(scene, max_depth, spp, integ, rgb_o, w_o):
    """Monte Carlo noise level: relative RMS between oracle films at seeds 0 and 1."""
    from oracle import binding
    other = binding.OracleRun(scene, max_depth=max_depth, seed=1)
    rgb1, w1 = other.render(0, spp, nthreads=8)
    return _rel_rms(integ.image(rgb1, w1), integ.image(rgb_o, w_o))


def _integrator(scene, **kw):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    return VolPathIntegrator(scene, device=0, **kw)


def _compare_samples(integ, ref, first, ns):
    """Per-sample replay: GPU L / lambda / lambda pdfs / filter weight of the last pass vs
    oracle_pixel_sample. A sample counts as exact when all four are bit-identical (the pdfs are
    the ones k_film divides by: avr_last_pass_samples evaluates them with k_film's overload)."""
    f = integ.scene.film
    npix = f.width * f.height
    _, _, L, lam, pdf = integ.ctx.last_pass_samples(npix, ns)
    wts = integ.ctx.last_pass_weights(npix, ns)
    exact = 0
    total = 0
    worst = 0.0
    for s in range(ns):
        for pix in range(npix):
            px, py = pix % f.width, pix // f.width
            Lo, lo, po, _, wo = ref.pixel_sample(px, py, first + s, with_weight=True)
            g = s * npix + pix
            total += 1
            if (np.array_equal(L[g].view(np.uint32), Lo.view(np.uint32))
                    and np.array_equal(lam[g].view(np.uint32), lo.view(np.uint32))
                    and np.array_equal(np.asarray(pdf[g], np.float32).view(np.uint32),
                                       np.asarray(po, np.float32).view(np.uint32))
                    and np.float32(wts[g]).view(np.uint32) == np.float32(wo).view(np.uint32)):
                exact += 1
            worst = max(worst, float(np.max(np.abs(lam[g] - lo))))
    return exact / total, worst


def test_majorant_grid_bit_exact():
    from acceleratedvolrenderer_amd import scenes
    from oracle import binding
    rng = np.random.default_rng(3)
    dens = rng.random((27, 33, 40), dtype=np.float32)
    scene = scenes.s_uniform(n=1, width=8, height=8, variant="scatter", density=dens)
    integ = _integrator(scene, spp=1)
    got = integ.ctx.majorant(16 * 16 * 16)
    want = binding.build_majorant(dens, (16, 16, 16))
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    integ.close()


def test_cloud_generator_bit_exact():
    from acceleratedvolrenderer_amd import capi
    from oracle import binding
    n = 40
    ctx = capi.Context(0)
    t = torch.empty(n * n * n, dtype=torch.float32, device="cuda:0")
    ctx.generate_cloud(t.data_ptr(), n, 0, n * n * n)
    ctx.sync()
    got = t.cpu().numpy().reshape(n, n, n)
    want = binding.cloud_grid(n)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    ctx.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("variant", ["scatter", "absorber", "chromatic", "emissive", "emissive_chromatic"])
def test_uniform_box_film_parity(variant, kernel):
    from acceleratedvolrenderer_amd import scenes
    from oracle import binding
    n, W, H, spp = 16, 32, 32, 8
    rng = np.random.default_rng(5)
    dens = (0.25 + rng.random((n, n, n), dtype=np.float32)).astype(np.float32)
    scene = scenes.s_uniform(n=n, width=W, height=H, variant=variant, density=dens)
    integ = _integrator(scene, maxdepth=5, spp=spp, kernel=kernel)
    rgb, w = integ.render()
    ref = binding.OracleRun(scene, max_depth=5, seed=0)
    rgb_o, w_o = ref.render(0, spp, nthreads=8)
    assert np.array_equal(w, w_o)
    err = _rel_rms(integ.image(rgb, w), integ.image(rgb_o, w_o))
    noise = _oracle_noise(scene, 5, spp, integ, rgb_o, w_o)
    canon = binding.OracleRun(scene, max_depth=5, seed=0, libm="canonical")
    frac, worst_lambda = _compare_samples(integ, canon, 0, spp)
    rgb_c, w_c = canon.render(0, spp, nthreads=8)
    err_c = _rel_rms(integ.image(rgb, w), integ.image(rgb_c, w_c))
    print(f"{variant}/{kernel}: film rel RMS {err:.3e} vs platform oracle (MC noise {noise:.3e}), {err_c:.3e} vs "
          f"canonical; bit-exact samples {frac:.5f}, max |dlambda| {worst_lambda:.2e}")
    assert worst_lambda < 1e-3
    assert frac == 1.0
    assert err <= 0.5 * noise
    if frac == 1.0:
        assert err_c <= 1e-6
    integ.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
def test_cloud_film_parity_perspective(kernel):
    from acceleratedvolrenderer_amd import scenes
    from oracle import binding
    n, W, H, spp = 32, 64, 36, 8
    dens = binding.cloud_grid(n)
    scene = scenes.s_cloud(dens, width=W, height=H)
    integ = _integrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=spp, kernel=kernel)
    rgb, w = integ.render()
    ref = binding.OracleRun(scene, max_depth=scenes.CLOUD_MAXDEPTH, seed=0)
    rgb_o, w_o = ref.render(0, spp, nthreads=8)
    err = _rel_rms(integ.image(rgb, w), integ.image(rgb_o, w_o))
    noise = _oracle_noise(scene, scenes.CLOUD_MAXDEPTH, spp, integ, rgb_o, w_o)
    canon = binding.OracleRun(scene, max_depth=scenes.CLOUD_MAXDEPTH, seed=0, libm="canonical")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    print(f"cloud/{kernel}: film rel RMS {err:.3e} vs platform oracle (MC noise {noise:.3e}), "
          f"bit-exact samples vs canonical {frac:.5f}")
    assert frac == 1.0
    assert err <= 0.5 * noise
    integ.close()


def test_persistent_and_wavefront_kernels_agree_bit_for_bit():
    """Both kernel organisations run the same device arithmetic per sample, so the
    per-sample radiance and the fp64 film sums are identical."""
    from acceleratedvolrenderer_amd import scenes
    from oracle import binding
    dens = binding.cloud_grid(24)
    scene = scenes.s_cloud(dens, width=40, height=24)
    a = _integrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=6, kernel="persistent")
    b = _integrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=6, kernel="wavefront")
    ra, wa = a.render()
    rb, wb = b.render()
    npix = 40 * 24
    La = a.ctx.last_pass_samples(npix, 6)[2]
    Lb = b.ctx.last_pass_samples(npix, 6)[2]
    assert np.array_equal(La.view(np.uint32), Lb.view(np.uint32))
    assert np.array_equal(ra, rb) and np.array_equal(wa, wb)
    a.close()
    b.close()


def test_fat_and_linear_grid_layouts_agree_bit_for_bit():
    """The fat footprint copy of the density grid changes where the 8 taps are read from,
    not their values or the lerp order: films are identical."""
    from acceleratedvolrenderer_amd import scenes
    from oracle import binding
    dens = binding.cloud_grid(20)
    scene = scenes.s_cloud(dens, width=32, height=18)
    a = _integrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=4, grid_layout="fat")
    b = _integrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=4, grid_layout="linear")
    assert a.ctx.grid_layout_active() == 1 and b.ctx.grid_layout_active() == 0
    ra, wa = a.render()
    rb, wb = b.render()
    assert np.array_equal(ra, rb) and np.array_equal(wa, wb)
    a.close()
    b.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("dims", [(20, 20, 20), (13, 9, 21), (8, 16, 7)])
def test_brick_layout_agrees_bit_for_bit(dims, kernel):
    """The bricked copy (avr_set_grid_layout 2: 8^3 apron bricks) reads the same
    8 taps in the same lerp order as the fat and the linear layouts: films and per-sample records
    are identical, for grid sizes that are and are not multiples of the brick edge."""
    from acceleratedvolrenderer_amd import scenes
    from oracle import binding
    nx, ny, nz = dims
    dens = np.ascontiguousarray(binding.cloud_grid(max(dims))[:nz, :ny, :nx])
    scene = scenes.s_cloud(dens, width=32, height=18)
    out = []
    for layout, code in (("linear", 0), ("fat", 1), ("brick", 2)):
        integ = _integrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=4, grid_layout=layout, kernel=kernel)
        assert integ.ctx.grid_layout_active() == code
        rgb, w = integ.render()
        st = integ.stats()
        out.append((rgb, w, st["medium_lookups"], st["shadow_lookups"]))
        if kernel == "persistent":
            _, ns, L, lam, _ = integ.ctx.last_pass_samples(32 * 18, 4)
            out[-1] += (L, lam)
        integ.close()
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
def test_multipass_equals_single_pass_and_deterministic(kernel):
    """Pass splitting (max_paths) and repeat runs give bit-identical fp64 film sums."""
    from acceleratedvolrenderer_amd import scenes, VolPathIntegrator
    n, W, H, spp = 16, 20, 20, 8
    rng = np.random.default_rng(9)
    dens = rng.random((n, n, n), dtype=np.float32)
    scene = scenes.s_uniform(n=n, width=W, height=H, variant="scatter", density=dens)
    a = VolPathIntegrator(scene, maxdepth=5, spp=spp, device=0, kernel=kernel)
    rgb1, w1 = a.render()
    rgb2, w2 = a.render()
    b = VolPathIntegrator(scene, maxdepth=5, spp=spp, device=0, max_paths=W * H * 3,
                          kernel=kernel)  # passes of 3 samples
    rgb3, w3 = b.render()
    assert np.array_equal(rgb1, rgb2) and np.array_equal(w1, w2)
    assert np.array_equal(rgb1, rgb3) and np.array_equal(w1, w3)
    a.close()
    b.close()


def test_absorber_beer_lambert_analytic():
    """Known answer: L = exp(-integral of sigma_a), with the half-voxel trilinear shell:
    integral of density along z through [0,1]^3 of ones = 1 - 0.25/n (containers.h:822-835)."""
    from acceleratedvolrenderer_amd import scenes
    n, W, H, spp = 8, 16, 16, 256
    scene = scenes.s_uniform(n=n, width=W, height=H, variant="absorber")
    integ = _integrator(scene, maxdepth=5, spp=spp, max_paths=W * H * 64)
    integ.render(spp - 64, spp)
    _, ns, L, _, _ = integ.ctx.last_pass_samples(W * H, 64)
    Lm = L.reshape(ns, H, W, 4)[:, 2:-2, 2:-2, 0].mean()
    want = np.exp(-(1 - 0.25 / n))
    assert abs(Lm - want) < 4 * np.sqrt(want * (1 - want) / (ns * (H - 4) * (W - 4)))
    integ.close()


def test_white_furnace():
    """Albedo-1 medium in a uniform infinite light: every path that escapes carries L = Le = 1."""
    from acceleratedvolrenderer_amd import scenes
    n, W, H, spp = 8, 16, 16, 16
    scene = scenes.s_uniform(n=n, width=W, height=H, variant="furnace")
    integ = _integrator(scene, maxdepth=1000, spp=spp)
    integ.render()
    _, ns, L, _, _ = integ.ctx.last_pass_samples(W * H, spp)
    assert np.all(L == 1.0)
    integ.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
def test_stats_accumulate_reset_and_count_every_sample_once(kernel):
    """avr_get_stats folds asynchronously recorded counters: every (pixel, sample) path is
    started exactly once, counters accumulate over renders until avr_reset_stats."""
    from acceleratedvolrenderer_amd import scenes
    n, W, H = 16, 24, 20
    dens = (0.25 + np.random.default_rng(2).random((n, n, n), dtype=np.float32)).astype(np.float32)
    scene = scenes.s_uniform(n=n, width=W, height=H, variant="scatter", density=dens)
    integ = _integrator(scene, maxdepth=5, spp=6, kernel=kernel, max_paths=W * H * 4)   # 2 passes per render
    integ.ctx.reset_stats()
    integ.ctx.render(0, 6, 0, 5)
    integ.ctx.render(6, 9, 0, 5)
    st = integ.ctx.stats()
    if kernel == "persistent":
        assert st["medium_items_in"] == W * H * 9          # paths started
    else:
        assert st["medium_items_in"] >= W * H * 9          # queue items over all launches
    assert st["medium_lookups"] > 0 and st["ms_medium"] > 0 and st["ms_total"] > 0
    assert st["medium_launches"] >= (3 if kernel == "persistent" else 4)
    integ.ctx.reset_stats()
    st = integ.ctx.stats()
    assert st["medium_items_in"] == 0 and st["ms_medium"] == 0 and st["medium_launches"] == 0
    integ.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("sampler,filt,spp", [("zsobol", "box", 8), ("zsobol", "gaussian", 16),
                                              ("independent", "gaussian", 4), ("zsobol", "box", 2)])
def test_samplers_and_filters_replay(kernel, sampler, filt, spp):
    """ZSobolSampler (pbrt's default, samplers.h:225-330) and GaussianFilter (the default
    filter, filters.h:80-118): per-sample replay of L, lambda and filter weight against the
    canonical oracle, film vs the platform oracle within MC noise."""
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import (BoxFilter, GaussianFilter, IndependentSampler, RGBFilm, Scene,
                                                  ZSobolSampler)
    from oracle import binding
    n, W, H = 16, 24, 20
    dens = (0.25 + np.random.default_rng(9).random((n, n, n), dtype=np.float32)).astype(np.float32)
    base = scenes.s_uniform(n=n, width=W, height=H, variant="scatter", density=dens)
    film = RGBFilm(W, H, filter=GaussianFilter() if filt == "gaussian" else BoxFilter())
    smp = (ZSobolSampler if sampler == "zsobol" else IndependentSampler)(pixelsamples=spp)
    scene = Scene(base.camera, film, base.medium, base.lights, sampler=smp)
    integ = _integrator(scene, maxdepth=5, spp=spp, kernel=kernel)
    rgb, w = integ.render()
    canon = binding.OracleRun(scene, max_depth=5, seed=0, libm="canonical")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    ref = binding.OracleRun(scene, max_depth=5, seed=0)
    rgb_o, w_o = ref.render(0, spp, nthreads=8)
    assert np.allclose(w, w_o, rtol=1e-6)
    err = _rel_rms(integ.image(rgb, w), integ.image(rgb_o, w_o))
    noise = _oracle_noise(scene, 5, spp, integ, rgb_o, w_o)
    print(f"{sampler}/{filt}/{kernel}: bit-exact samples {frac:.5f}, film rel RMS {err:.3e} (noise {noise:.3e})")
    assert frac == 1.0
    assert err <= 0.5 * noise
    integ.close()


def test_cloud_pbrt_defaults_zsobol_gaussian():
    """The metric scene with pbrt's default sampler and filter (the bench configuration)."""
    from acceleratedvolrenderer_amd import scenes
    from oracle import binding
    n, W, H, spp = 32, 48, 27, 16
    dens = binding.cloud_grid(n)
    scene = scenes.s_cloud(dens, width=W, height=H, sampler="zsobol", spp=spp, filter="gaussian")
    integ = _integrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=spp)
    rgb, w = integ.render()
    canon = binding.OracleRun(scene, max_depth=scenes.CLOUD_MAXDEPTH, seed=0, libm="canonical")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    rgb_c, w_c = canon.render(0, spp, nthreads=8)
    print(f"cloud zsobol+gaussian: bit-exact samples {frac:.5f}")
    assert frac == 1.0
    if frac == 1.0:
        assert np.array_equal(rgb, rgb_c) and np.array_equal(w, w_c)
    integ.close()


def test_transmittance_matches_oracle_and_beer_lambert():
    """avr_transmittance = Integrator::Tr (integrators.cpp:324-374): per query bit-exact
    against the canonical oracle on a heterogeneous chromatic medium; on a homogeneous
    interior the mean over queries matches Beer-Lambert exp(-sigma_t (1 - eps) |p1 - p0|)."""
    from acceleratedvolrenderer_amd import scenes, capi
    from oracle import binding
    rng = np.random.default_rng(4)
    n = 16
    dens = (0.25 + rng.random((n, n, n), dtype=np.float32)).astype(np.float32)
    scene = scenes.s_uniform(n=n, width=8, height=8, variant="chromatic", density=dens)
    rfm = scene.render_from_medium.astype(np.float64)

    def to_render(pm):
        h = np.concatenate([pm, np.ones((len(pm), 1))], axis=1) @ rfm.T
        return h[:, :3].astype(np.float32)

    q = 4000
    p0 = to_render(rng.random((q, 3)))
    p1 = to_render(rng.random((q, 3)))
    lam = (360 + 470 * rng.random((q, 4))).astype(np.float32)
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    dev = ctx.transmittance(p0, p1, lam)
    ora = binding.OracleRun(scene, max_depth=5, seed=0, libm="canonical").transmittance4(p0, p1, lam)
    same = np.mean(np.all(dev.view(np.uint32) == ora.view(np.uint32), axis=1))
    print(f"Tr bit-exact queries {same:.5f}")
    assert same == 1.0
    # homogeneous interior: density 1 exactly away from the zero-padded faces
    hom = scenes.s_uniform(n=n, width=8, height=8, variant="absorber")
    ctx.set_scene(hom)
    a = rng.uniform(0.1, 0.9, (q, 3))
    b = rng.uniform(0.1, 0.9, (q, 3))
    p0 = to_render(a)
    p1 = to_render(b)
    lam = np.full((q, 4), 550.0, np.float32)
    tr = ctx.transmittance(p0, p1, lam)[:, 0].astype(np.float64)
    dist = np.linalg.norm((p1 - p0).astype(np.float64), axis=1) * (1 - 1e-4)
    expect = np.exp(-1.0 * dist)           # absorber variant: sigma_a = 1, sigma_s = 0
    # ratio tracking with sigma_maj = sigma_t is 0/1 per query: compare means, binomial noise
    err = abs(tr.mean() - expect.mean())
    sd = np.sqrt(np.mean(expect * (1 - expect)) / q)
    print(f"Tr mean {tr.mean():.4f} vs Beer-Lambert {expect.mean():.4f} (sd {sd:.4f})")
    assert err <= 4 * sd
    ctx.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("kind", ["homogeneous", "homogeneous_emissive", "cloud"])
def test_homogeneous_and_cloud_media_replay(kind, kernel):
    """HomogeneousMedium (media.h:217-262) and CloudMedium (media.h:430-528): one majorant
    segment per ray (HomogeneousMajorantIterator), constant or procedural density, in both
    kernel organisations."""
    from acceleratedvolrenderer_amd import scenes, HomogeneousMedium, CloudMedium
    from acceleratedvolrenderer_amd.scene import Scene
    from oracle import binding
    W, H, spp = 24, 20, 8
    base = scenes.s_uniform(n=4, width=W, height=H, variant="scatter")
    med = {"homogeneous": HomogeneousMedium(sigma_a=0.5, sigma_s=2.0, g=0.3),
           "homogeneous_emissive": HomogeneousMedium(sigma_a=np.linspace(0.5, 1.5, 471), sigma_s=1.0, Le=1.0,
                                                     Lescale=2.0),
           "cloud": CloudMedium(sigma_a=0.1, sigma_s=3.0, g=0.6)}[kind]
    scene = Scene(base.camera, base.film, med, base.lights)
    integ = _integrator(scene, maxdepth=8, spp=spp, kernel=kernel)
    rgb, w = integ.render()
    assert (integ.stats()["loop_iterations"] > 0) == (kernel == "persistent")
    canon = binding.OracleRun(scene, max_depth=8, seed=0, libm="canonical")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    ref = binding.OracleRun(scene, max_depth=8, seed=0)
    rgb_o, w_o = ref.render(0, spp, nthreads=8)
    err = _rel_rms(integ.image(rgb, w), integ.image(rgb_o, w_o))
    noise = _oracle_noise(scene, 8, spp, integ, rgb_o, w_o)
    print(f"{kind}/{kernel}: bit-exact samples {frac:.5f}, film rel RMS {err:.3e} (noise {noise:.3e})")
    assert frac == 1.0
    assert err <= 0.5 * noise
    integ.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("chromatic", [False, True])
def test_temperature_blackbody_emission_replay(kernel, chromatic):
    """GridMedium temperature grid (media.h:299-316): Le = LeScale * normalised blackbody at
    T = (temperature - offset) * scale, emitting only above 100 K."""
    from acceleratedvolrenderer_amd import scenes, GridMedium
    from acceleratedvolrenderer_amd.scene import Scene
    from oracle import binding
    n, W, H, spp = 12, 24, 20, 8
    base = scenes.s_uniform(n=n, width=W, height=H, variant="scatter")
    z, y, x = np.meshgrid(*(np.linspace(0, 1, n, dtype=np.float32),) * 3, indexing="ij")
    temp = (50 + 4000 * x * (1 - y) + 300 * z).astype(np.float32)     # includes cells below 100 K
    dens = (0.3 + 0.7 * np.random.default_rng(3).random((n, n, n), dtype=np.float32)).astype(np.float32)
    sa = np.linspace(0.5, 1.5, 471).astype(np.float32) if chromatic else 1.0
    med = GridMedium(dens, sigma_a=sa, sigma_s=0.5, g=0.2, temperature=temp, temperaturescale=1.1,
                     temperatureoffset=20.0)
    scene = Scene(base.camera, base.film, med, base.lights)
    integ = _integrator(scene, maxdepth=6, spp=spp, kernel=kernel)
    rgb, w = integ.render()
    canon = binding.OracleRun(scene, max_depth=6, seed=0, libm="canonical")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    ref = binding.OracleRun(scene, max_depth=6, seed=0)
    rgb_o, w_o = ref.render(0, spp, nthreads=8)
    err = _rel_rms(integ.image(rgb, w), integ.image(rgb_o, w_o))
    noise = _oracle_noise(scene, 6, spp, integ, rgb_o, w_o)
    print(f"temperature/{kernel}/chromatic={chromatic}: bit-exact {frac:.5f}, film rel RMS {err:.3e} (noise {noise:.3e})")
    assert frac == 1.0
    assert err <= 0.5 * noise
    integ.close()


def _vdb_scene(case, W, H):
    from acceleratedvolrenderer_amd import scenes
    rng = np.random.default_rng(12)
    n = 20
    d = np.zeros((n, n, n), np.float32)
    d[3:17, 2:18, 4:16] = (0.2 + rng.random((14, 16, 12))).astype(np.float32)
    d[8:16, 8:16, 0:8] = 0.8                                     # block-aligned constant: a tile
    if case == "aligned":
        return scenes.s_vdb(d, W, H, variant="scatter")
    c, s = np.cos(np.radians(25)), np.sin(np.radians(25))
    m = np.eye(4)
    m[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([0.8 / n, 1.0 / n, 0.7 / n])
    m[:3, 3] = [0.25, 0.0, 0.15]
    if case == "rotated":
        return scenes.s_vdb(d, W, H, variant="scatter", index_to_world=m)
    z, y, x = np.meshgrid(*(np.linspace(0, 1, n, dtype=np.float32),) * 3, indexing="ij")
    temp = (50 + 4000 * x * (1 - y) + 300 * z).astype(np.float32)   # includes voxels below 100 K
    tg = scenes.vdb_grid(temp, index_to_world=m, index_min=(2, 0, -1))   # offset: bounds are a union
    return scenes.s_vdb(scenes.vdb_grid(d, index_to_world=m), W, H, variant="scatter", temperature=tg,
                        sigma_a=np.linspace(0.5, 1.5, 471).astype(np.float32), Lescale=1.5,
                        temperatureoffset=20.0, temperaturescale=1.1)


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("case", ["aligned", "rotated", "temperature"])
def test_nanovdb_medium_replay(case, kernel):
    """NanoVDBMedium (media.h:602-685): bounds and the 64^3 majorant (media.cpp:556-613)
    bit-exact against the oracle; per-sample replay 100 % bit-identical; film within
    noise of the platform oracle, in both kernel organisations (k_paths<.., kVdb> reads the
    majorant through L2). NanoVDB's own semantics are restated (parity unpinned,
    tests/test_vdb.py)."""
    from oracle import binding
    W, H, spp = 24, 20, 8
    scene = _vdb_scene(case, W, H)
    integ = _integrator(scene, maxdepth=8, spp=spp, kernel=kernel)
    assert integ.ctx.medium_bounds().view(np.uint32).tolist() == scene.medium.bounds.view(np.uint32).tolist()
    canon = binding.OracleRun(scene, max_depth=8, seed=0, libm="canonical")
    got = integ.ctx.majorant(64 ** 3)
    assert got.view(np.uint32).tolist() == canon.majorant.view(np.uint32).tolist()
    assert float(got.max()) > 0
    rgb, w = integ.render()
    assert (integ.stats()["loop_iterations"] > 0) == (kernel == "persistent")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    ref = binding.OracleRun(scene, max_depth=8, seed=0)
    rgb_o, w_o = ref.render(0, spp, nthreads=8)
    err = _rel_rms(integ.image(rgb, w), integ.image(rgb_o, w_o))
    noise = _oracle_noise(scene, 8, spp, integ, rgb_o, w_o)
    print(f"nanovdb/{case}/{kernel}: bit-exact samples {frac:.5f}, film rel RMS {err:.3e} (noise {noise:.3e})")
    assert frac == 1.0
    assert err <= 0.5 * noise
    integ.close()


def test_nanovdb_transmittance_matches_oracle():
    from acceleratedvolrenderer_amd import capi
    from oracle import binding
    scene = _vdb_scene("rotated", 8, 8)
    rng = np.random.default_rng(21)
    b = scene.medium.bounds
    q = 3000
    p0 = (b[:3] + rng.random((q, 3)) * (b[3:] - b[:3])).astype(np.float32)
    p1 = (b[:3] + rng.random((q, 3)) * (b[3:] - b[:3])).astype(np.float32)
    rfm = scene.render_from_medium.astype(np.float64)
    to_r = lambda pm: (np.concatenate([pm, np.ones((len(pm), 1))], axis=1) @ rfm.T)[:, :3].astype(np.float32)
    p0, p1 = to_r(p0), to_r(p1)
    lam = (360 + 470 * rng.random((q, 4))).astype(np.float32)
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    dev = ctx.transmittance(p0, p1, lam)
    ora = binding.OracleRun(scene, max_depth=5, seed=0, libm="canonical").transmittance4(p0, p1, lam)
    same = np.mean(np.all(dev.view(np.uint32) == ora.view(np.uint32), axis=1))
    print(f"nanovdb Tr bit-exact queries {same:.5f}")
    assert same == 1.0
    assert 0.05 < float(dev.mean()) < 0.95
    ctx.close()


def _rgb_coeffs(rng, shape, scale_hi=3.0):
    """Random RGBSigmoidPolynomial coefficients + scale per voxel (any coefficients are a
    valid RGBUnboundedSpectrum; the RGB->coefficient table is checked in test_rgbgrid.py).
    No colour gives these: c2 stays in [-5, 5] and the scale in [0.2, 3]. Converted colours
    (black = {0, 0, -inf, 0}, greys with c0 = c1 = 0, primaries, HDR scales) run on the device
    in test_gpu_rgbgrid.py, over the grids of rgbgrid_cases.py."""
    c = np.empty(shape + (4,), np.float32)
    c[..., 0] = rng.uniform(-2e-5, 2e-5, shape)
    c[..., 1] = rng.uniform(-0.02, 0.02, shape)
    c[..., 2] = rng.uniform(-5, 5, shape)
    c[..., 3] = rng.uniform(0.2, scale_hi, shape)
    return c


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("case", ["absorbing_scattering", "sigma_s_only", "emissive"])
def test_rgbgrid_medium_replay(case, kernel):
    """RGBGridMedium (media.h:355-427): 16^3 majorant (media.cpp:364-377) bit-exact, per-sample
    replay 100 % bit-identical against the canonical oracle, film within noise."""
    from acceleratedvolrenderer_amd import scenes, RGBGridMedium
    from acceleratedvolrenderer_amd.scene import Scene
    from oracle import binding
    W, H, spp = 24, 20, 8
    rng = np.random.default_rng(31)
    shape = (7, 9, 8)
    base = scenes.s_uniform(n=1, width=W, height=H, variant="scatter")
    kw = dict(g=0.25, scale=1.3)
    if case == "absorbing_scattering":
        med = RGBGridMedium(sigma_a_coeffs=_rgb_coeffs(rng, shape, 0.8), sigma_s_coeffs=_rgb_coeffs(rng, shape), **kw)
    elif case == "sigma_s_only":
        med = RGBGridMedium(sigma_s_coeffs=_rgb_coeffs(rng, shape), **kw)     # sigma_a = 1 (media.h:388)
    else:
        med = RGBGridMedium(sigma_a_coeffs=_rgb_coeffs(rng, shape, 0.8), sigma_s_coeffs=_rgb_coeffs(rng, shape),
                            Le_coeffs=_rgb_coeffs(rng, shape, 2.0), Lescale=0.7, **kw)
    scene = Scene(base.camera, base.film, med, base.lights)
    integ = _integrator(scene, maxdepth=8, spp=spp, kernel=kernel)
    canon = binding.OracleRun(scene, max_depth=8, seed=0, libm="canonical")
    got = integ.ctx.majorant(16 ** 3)
    assert got.view(np.uint32).tolist() == canon.majorant.view(np.uint32).tolist()
    rgb, w = integ.render()
    assert (integ.stats()["loop_iterations"] > 0) == (kernel == "persistent")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    ref = binding.OracleRun(scene, max_depth=8, seed=0)
    rgb_o, w_o = ref.render(0, spp, nthreads=8)
    err = _rel_rms(integ.image(rgb, w), integ.image(rgb_o, w_o))
    noise = _oracle_noise(scene, 8, spp, integ, rgb_o, w_o)
    print(f"rgbgrid/{case}/{kernel}: bit-exact samples {frac:.5f}, film rel RMS {err:.3e} (noise {noise:.3e})")
    assert frac == 1.0
    assert err <= 0.5 * noise
    integ.close()


def test_film_image_metric_and_mse_waves(tmp_path):
    """RGBFilm::GetImage on the device equals the host restatement bit for bit (fp16 and
    fp32); the device MSE/MAE/MRSE/ME against a reference equal imgtool's pbrt-order f64 sums
    (to f64 reduction order); the --mse-reference-image wave loop logs one line per sample
    and ends on the same film as one render; the EXR written reads back as GetImage."""
    from acceleratedvolrenderer_amd import scenes, imgtool, imageio
    n, W, H, spp = 12, 40, 28, 8
    dens = (0.3 + np.random.default_rng(8).random((n, n, n), dtype=np.float32)).astype(np.float32)
    scene = scenes.s_uniform(n=n, width=W, height=H, variant="emissive_chromatic", density=dens)
    integ = _integrator(scene, maxdepth=6, spp=spp)
    rgb, w = integ.render()
    f = scene.film
    for fp16 in (True, False):
        buf = torch.empty(W * H * 3, dtype=torch.float32, device="cuda:0")
        integ.ctx.film_image_device(buf.data_ptr(), f.output_from_sensor, fp16=fp16)
        torch.cuda.synchronize()
        dev = buf.cpu().numpy().reshape(H, W, 3)
        host = integ.get_image(rgb, w, fp16=fp16)
        assert dev.view(np.uint32).tolist() == host.view(np.uint32).tolist()
    ref = (integ.get_image(rgb, w) * np.float32(1.1) + np.float32(0.01)).astype(np.float32)
    integ.ctx.film_set_reference(ref, f.output_from_sensor, fp16=True)
    img = integ.get_image(rgb, w)
    for m in ("MSE", "MAE", "MRSE"):
        got = integ.ctx.film_metric(m)
        want = imgtool.metric(img, ref, m)
        assert np.allclose(got, want, rtol=1e-6, atol=0), (m, got, want)
    me = integ.ctx.film_metric("ME")
    assert np.allclose(me, np.stack(imgtool.metric(img, ref, "ME")), rtol=1e-6, atol=0)
    rgb2, w2, log = integ.render_waves(mse_reference=ref, mse_out=str(tmp_path / "mse.txt"))
    assert [s for s, _ in log] == list(range(1, spp + 1))
    assert np.array_equal(rgb2, rgb) and np.array_equal(w2, w)
    lines = open(tmp_path / "mse.txt").read().splitlines()
    assert len(lines) == spp and lines[-1].startswith(f"{spp}, ")
    assert abs(float(lines[-1].split(",")[1]) - float(imgtool.channel_average(imgtool.metric(img, ref, "MSE")))) \
        <= 1e-6 * abs(float(lines[-1].split(",")[1]))
    integ.write_image(str(tmp_path / "a.exr"), rgb, w, spp=spp)
    assert np.array_equal(imageio.read_rgb(str(tmp_path / "a.exr")), img)
    integ.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
def test_zsobol_pixel_table_identical(kernel):
    """The ZSobol pixel table (avr_set_sampler_table) changes nothing: films and per-sample
    records equal the per-call computation, with paths running past the table's dimensions."""
    from acceleratedvolrenderer_amd import scenes
    n, W, H, spp = 12, 33, 21, 16
    dens = (0.5 + np.random.default_rng(9).random((n, n, n), dtype=np.float32)).astype(np.float32)
    scene = scenes.s_uniform(n=n, width=W, height=H, variant="chromatic", density=dens)
    from acceleratedvolrenderer_amd import ZSobolSampler, GaussianFilter
    from acceleratedvolrenderer_amd.scene import Scene, RGBFilm
    scene = Scene(scene.camera, RGBFilm(W, H, filter=GaussianFilter()), scene.medium, scene.lights,
                  sampler=ZSobolSampler(spp))
    out = []
    for dims in (0, 24, 256):
        integ = _integrator(scene, maxdepth=20, spp=spp, kernel=kernel)
        integ.ctx.set_sampler_table(dims)
        rgb, w = integ.render()
        _, ns, L, lam, _ = integ.ctx.last_pass_samples(W * H, spp)
        st = integ.stats()
        assert (st["ms_setup"] > 0) == (dims > 0)
        out.append((rgb, w, L, lam))
        integ.close()
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("pixelsamples", [2048, 4096])
def test_zsobol_pass_table_identical(pixelsamples):
    """The per-pass ZSobol table (avr_set_sampler_pass_table: the digits a k_paths pass's sample
    indices share) changes nothing: films and per-sample records equal the renders without it,
    for aligned and unaligned index ranges, several passes per render (different low-bit counts
    plo), odd and even log2(pixelsamples) and paths running past the table's dimensions; odd
    dimension counts (11) are rounded up to even rows (the 16-B entry-pair loads)."""
    from acceleratedvolrenderer_amd import scenes, ZSobolSampler, GaussianFilter
    from acceleratedvolrenderer_amd.scene import Scene, RGBFilm
    n, W, H = 12, 33, 21
    dens = (0.5 + np.random.default_rng(19).random((n, n, n), dtype=np.float32)).astype(np.float32)
    base = scenes.s_uniform(n=n, width=W, height=H, variant="scatter", density=dens)
    scene = Scene(base.camera, RGBFilm(W, H, filter=GaussianFilter()), base.medium, base.lights,
                  sampler=ZSobolSampler(pixelsamples))
    for lo, hi, per_pass in ((64, 128, 64), (5, 71, 24), (1000, 1040, 7), (512, 544, 8), (0, 64, 16)):
        out = []
        for dims in (0, 8, 11, 64):
            integ = _integrator(scene, maxdepth=30, spp=pixelsamples, kernel="persistent", max_paths=W * H * per_pass)
            integ.ctx.set_sampler_pass_table(dims)
            rgb, w = integ.render(lo, hi)
            first, ns, L, lam, _ = integ.ctx.last_pass_samples(W * H, per_pass)
            out.append((rgb, w, L[:W * H * ns], lam[:W * H * ns]))
            integ.close()
        for o in out[1:]:
            for a, b in zip(out[0], o):
                assert np.array_equal(a, b), (lo, hi, per_pass)


@pytest.mark.parametrize("with_distant", [False, True])
@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("variant", ["chromatic", "scatter"])
def test_image_infinite_light_replay(with_distant, variant, kernel):
    """ImageInfiniteLight (lights.h:552-640): compensated-distribution NEE with MIS
    (integrators.cpp:1282-1399) and MIS-weighted escapes (1090-1107) through a rotated
    equal-area map with a bright spot; with a distant light too, the escape loop's r_l
    accumulation over lights is exercised. Replay 100 % bit-identical vs the canonical
    oracle, film within noise of the platform oracle."""
    import os
    import sys
    from acceleratedvolrenderer_amd import scenes, ImageInfiniteLight, DistantLight, RGBToSpectrumTable
    from acceleratedvolrenderer_amd.scene import Scene
    from oracle import binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the cells of pbrt's sRGB table this image touches (tests/golden/make_srgb_subset.py)
    table = RGBToSpectrumTable.load(os.path.join(root, "tests", "golden", "srgb_table_subset.npz"))
    sys.path.insert(0, os.path.join(root, "tests", "golden"))
    from make_srgb_subset import envmap_image
    img = envmap_image()
    rot = np.eye(4)
    c, s = np.cos(0.7), np.sin(0.7)
    rot[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    light = ImageInfiniteLight(image=img, rgb_table=table, world_from_light=rot, scale=2.0)
    W, H, spp = 24, 20, 8
    base = scenes.s_uniform(n=6, width=W, height=H, variant=variant,
                            density=(0.2 + np.random.default_rng(2).random((6, 6, 6), dtype=np.float32)))
    lights = ([DistantLight(from_=(1, 1, -1), to=(0, 0, 0), scale=1.5)] if with_distant else []) + [light]
    scene = Scene(base.camera, base.film, base.medium, lights)
    integ = _integrator(scene, maxdepth=6, spp=spp, kernel=kernel)
    rgb, w = integ.render()
    assert (integ.stats()["loop_iterations"] > 0) == (kernel == "persistent")
    canon = binding.OracleRun(scene, max_depth=6, seed=0, libm="canonical")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    ref = binding.OracleRun(scene, max_depth=6, seed=0)
    rgb_o, w_o = ref.render(0, spp, nthreads=8)
    err = _rel_rms(integ.image(rgb, w), integ.image(rgb_o, w_o))
    noise = _oracle_noise(scene, 6, spp, integ, rgb_o, w_o)
    print(f"image light ({variant}/{kernel}, distant={with_distant}): bit-exact {frac:.5f}, film rel RMS {err:.3e} (noise {noise:.3e})")
    assert frac == 1.0
    assert err <= 0.5 * noise
    integ.close()


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("case", ["scatter", "chromatic", "image"])
def test_power_light_sampler_replay(case, kernel):
    """lightsampler "power" (PowerLightSampler, lightsamplers.h:63-99): NEE picks a light from
    the AliasTable over Average(Phi / pdf) at SampleVisible(0.5) (util/sampling.cpp:563-645)
    and escapes weight r_l by its PMF (integrators.cpp:1090-1107). Distant + uniform infinite
    lights (gray and chromatic media) and distant + image light: replay 100 %
    bit-identical vs the canonical oracle's own alias table, and the film differs from the
    BVH sampler's (the pick PMF changed)."""
    import os
    import sys
    from acceleratedvolrenderer_amd import scenes, ImageInfiniteLight, DistantLight, RGBToSpectrumTable
    from acceleratedvolrenderer_amd.scene import Scene
    from oracle import binding
    W, H, spp = 24, 20, 8
    variant = "scatter" if case == "image" else case
    base = scenes.s_uniform(n=6, width=W, height=H, variant=variant,
                            density=(0.2 + np.random.default_rng(6).random((6, 6, 6), dtype=np.float32)))
    lights = base.lights
    if case == "image":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        table = RGBToSpectrumTable.load(os.path.join(root, "tests", "golden", "srgb_table_subset.npz"))
        sys.path.insert(0, os.path.join(root, "tests", "golden"))
        from make_srgb_subset import envmap_image
        lights = [DistantLight(from_=(1, 1, -1), to=(0, 0, 0), scale=1.5),
                  ImageInfiniteLight(image=envmap_image(), rgb_table=table, scale=2.0)]
    scene = Scene(base.camera, base.film, base.medium, lights)
    integ = _integrator(scene, maxdepth=6, spp=spp, kernel=kernel, lightsampler="power")
    rgb, w = integ.render()
    canon = binding.OracleRun(scene, max_depth=6, seed=0, libm="canonical", lightsampler="power")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    integ.close()
    bvh = _integrator(scene, maxdepth=6, spp=spp, kernel=kernel)
    rgb_b, _ = bvh.render()
    bvh.close()
    print(f"power light sampler ({case}/{kernel}): bit-exact {frac:.5f}")
    assert frac == 1.0
    assert not np.array_equal(rgb, rgb_b)


def test_flip_on_device_matches_reference():
    """avr_flip (k_flip_prep / k_flip_error) against the reference FLIP's error maps
    (tests/golden/flip_vectors.npz). The taps are summed in the reference's order and powf is
    the canonical f64 exp(y log x) rounded once (99.9 % equal to the host libm's powf), so
    ~99 % of pixels are bit-identical, |difference| <= 2e-6 on errors in [0, 1], means to 1e-6."""
    import os
    from acceleratedvolrenderer_amd import capi, imgtool
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    z = np.load(os.path.join(root, "tests", "golden", "flip_vectors.npz"))
    ctx = capi.Context(0)
    for case in ("smooth_noise", "edges_ppd20", "identical"):
        got = ctx.flip(z[case + "_test"], z[case + "_ref"], float(z[case + "_ppd"]))
        want = z[case + "_flip"]
        same = float(np.mean(got.view(np.uint32) == want.view(np.uint32)))
        print(f"flip {case}: max |d| {np.abs(got - want).max():.2e}, bit-identical pixels {same:.4f}")
        assert np.abs(got - want).max() <= 2e-6
        assert same >= 0.95
        assert abs(float(got.mean()) - float(want.mean())) <= 1e-6
    ctx.close()
    e = imgtool.diff(z["smooth_noise_test"], z["smooth_noise_ref"], "FLIP")
    assert abs(e["FLIP"] - float(z["smooth_noise_flip"].mean())) < 1e-5


@pytest.mark.parametrize("kernel", ["persistent", "wavefront"])
@pytest.mark.parametrize("film_kw", [dict(), dict(nbuckets=7, lambdamin=400.0, lambdamax=700.0)],
                         ids=["default", "narrow"])
def test_spectral_film_replay(kernel, film_kw):
    """SpectralFilm (film.h:401-530): uniform wavelengths (SampleUniform) in both kernel
    organisations, per-sample replay 100 % bit-identical against the canonical oracle,
    RGB sums and fp64 bucket sums / weights against the oracle's SpectralFilm::AddSample
    (bit-exact when every sample matched: same per-pixel sample order)."""
    from acceleratedvolrenderer_amd import scenes, SpectralFilm
    from acceleratedvolrenderer_amd.scene import Scene
    from oracle import binding
    W, H, spp = 20, 16, 8
    base = scenes.s_uniform(n=10, width=W, height=H, variant="emissive_chromatic",
                            density=(0.3 + 0.7 * np.random.default_rng(8).random((10, 10, 10), dtype=np.float32)))
    film = SpectralFilm(W, H, **film_kw)
    scene = Scene(base.camera, film, base.medium, base.lights)
    integ = _integrator(scene, maxdepth=6, spp=spp, kernel=kernel)
    rgb, w = integ.render()
    bs, bw = integ.spectral_sums()
    canon = binding.OracleRun(scene, max_depth=6, seed=0, libm="canonical")
    frac, _ = _compare_samples(integ, canon, 0, spp)
    rgb_o, w_o, bs_o, bw_o = canon.render_spectral(0, spp, nthreads=8)
    print(f"spectral/{kernel}/{film.nbuckets}: bit-exact samples {frac:.5f}")
    assert frac == 1.0
    assert np.array_equal(bw, bw_o)                     # weights: bucket choice only
    assert float(bw.sum()) == pytest.approx(4 * W * H * spp)
    if frac == 1.0:
        assert np.array_equal(bs, bs_o) and np.array_equal(rgb, rgb_o)
    else:
        assert _rel_rms(bs, bs_o) < 1e-3 and _rel_rms(rgb, rgb_o) < 1e-3
    img = integ.spectral_image()
    assert img.shape == (H, W, 3 + film.nbuckets) and np.all(np.isfinite(img))
    integ.close()
