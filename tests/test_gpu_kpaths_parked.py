"""k_paths' parked instantiations (gray GridMedium, no emission, no image light: DESIGN §4).

Their handler-only path state lives in per-lane LDS arrays, the cooperative draws' results
in the shadow-ray slots, and the majorant grid is read through a bounds-checked buffer. None
of this changes a sample's arithmetic, so every test compares all samples of a small render
bit for bit against the canonical CPU oracle (last_pass_samples against
OracleRun.pixel_sample, as tests/test_gpu_fullsize.py does on a pixel subset). The shapes are
the small ones at which the moved state can go wrong: a non-cubic grid under non-cubic
majorant grids (strides, the unclamped one-cell-ahead index at both ends, 255 cells on an
axis), the 64-bit ZSobol index, every scatter spawning a shadow ray / none spawning one under
small and large service batches, and the independent sampler's state layout."""
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
    """24 x 40 x 56 voxels (x, y, z) cut from the cloud density: empty regions included."""
    from oracle import binding
    return np.ascontiguousarray(binding.cloud_grid(56)[:, :40, :24])


def _cloud_scene(density, sampler="zsobol", filter="gaussian", lights=None, majorant_res=(16, 16, 16)):
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import Scene
    base = scenes.s_cloud(density, width=W, height=H, sampler=sampler, spp=64, filter=filter)
    base.medium.majorant_res = tuple(majorant_res)
    if lights is None:
        return base
    return Scene(base.camera, base.film, base.medium, lights, sampler=base.sampler)


def _count_exact(integ, canon, film, first, ns):
    """(bit-identical samples, samples) of the last pass against the oracle."""
    npix = film.width * film.height
    got_first, got_ns, L, lam, _ = integ.ctx.last_pass_samples(npix, ns)
    assert (got_first, got_ns) == (first, ns)
    exact = total = 0
    for s in range(ns):
        for pix in range(npix):
            Lo, lo, _, _ = canon.pixel_sample(pix % film.width, pix // film.width, first + s)
            g = s * npix + pix
            total += 1
            exact += int(np.array_equal(L[g].view(np.uint32), Lo.view(np.uint32)) and
                         np.array_equal(lam[g].view(np.uint32), lo.view(np.uint32)))
    return exact, total


@pytest.mark.parametrize("res", [(16, 16, 16), (3, 5, 7), (1, 1, 1), (255, 4, 4)], ids=lambda r: "x".join(map(str, r)))
def test_non_cubic_grid_and_majorants_replay(density, res):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    from oracle import binding
    scene = _cloud_scene(density, majorant_res=res)
    integ = VolPathIntegrator(scene, maxdepth=MAXDEPTH, spp=8, seed=0, device=0)
    try:
        canon = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
        n = res[0] * res[1] * res[2]
        assert integ.ctx.majorant(n).view(np.uint32).tolist() == canon.majorant.view(np.uint32).tolist()
        integ.render(0, 8)
        assert integ.ctx.last_kernel() == "k_paths<false, true, 2, 0, false, false>"
        exact, total = _count_exact(integ, canon, scene.film, 0, 8)
        print(f"majorant {res}: {exact}/{total} samples bit-identical")
        assert exact == total == W * H * 8
    finally:
        integ.close()


def test_wide_zsobol_index_on_a_small_film(density):
    """2048 x 2 pixels at pixelsamples 4096: Morton(pixel) takes 22 bits and log2 spp 12, so the
    sample index needs 34 bits (samplers.h:250-254) and the parked sampler state its wide form.
    Orthographic camera over the medium's z = 0 face, so every pixel's ray enters the medium."""
    from acceleratedvolrenderer_amd import VolPathIntegrator, scenes
    from acceleratedvolrenderer_amd.scene import Scene, RGBFilm, GaussianFilter, ZSobolSampler
    from oracle import binding
    base = scenes.s_uniform(n=1, width=2048, height=2, variant="scatter")
    cloud = _cloud_scene(density)
    scene = Scene(base.camera, RGBFilm(2048, 2, filter=GaussianFilter()), cloud.medium, cloud.lights,
                  sampler=ZSobolSampler(4096))
    integ = VolPathIntegrator(scene, maxdepth=MAXDEPTH, spp=4096, seed=0, device=0)
    try:
        canon = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
        integ.render(4093, 4096)
        assert integ.ctx.last_kernel() == "k_paths<false, true, 3, 0, false, false>"
        exact, total = _count_exact(integ, canon, scene.film, 4093, 3)
        print(f"64-bit ZSobol index: {exact}/{total} samples bit-identical")
        assert exact == total == 2048 * 2 * 3
    finally:
        integ.close()


@pytest.mark.parametrize("refill", [12, 40])
@pytest.mark.parametrize("lights", ["distant", "sky"])
def test_result_slots_reused_with_and_without_shadow_rays(density, lights, refill):
    """distant: every scatter spawns a shadow ray, so a lane's NEE slots are written, read back
    and then taken by the cooperative draws' results at every bounce; sky: none does, and a lane
    goes from the scatter to the phase handler directly. Two consecutive passes under a small
    and a large service batch: each bit-identical to the oracle, and their sum equal to one pass."""
    from acceleratedvolrenderer_amd import VolPathIntegrator
    from acceleratedvolrenderer_amd.scene import DistantLight, UniformInfiniteLight
    from oracle import binding
    ls = ([DistantLight(from_=(0.7, 1.0, 0.6), to=(0.0, 0.0, 0.0), scale=3.0)] if lights == "distant"
          else [UniformInfiniteLight(scale=0.5)])
    scene = _cloud_scene(density, lights=ls)
    integ = VolPathIntegrator(scene, maxdepth=MAXDEPTH, spp=8, seed=0, device=0)
    try:
        canon = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
        integ.ctx.set_refill_min(refill)
        integ.ctx.film_clear()
        exact = total = 0
        for first in (0, 4):
            integ.ctx.render(first, first + 4, 0, MAXDEPTH)
            assert integ.ctx.last_kernel() == "k_paths<false, true, 2, 0, false, false>"
            e, t = _count_exact(integ, canon, scene.film, first, 4)
            exact, total = exact + e, total + t
        two = integ.film_sums()
        integ.ctx.film_clear()
        integ.ctx.render(0, 8, 0, MAXDEPTH)
        one = integ.film_sums()
        print(f"{lights}, refill {refill}: {exact}/{total} samples bit-identical")
        assert exact == total == W * H * 8
        assert np.array_equal(two[0], one[0]) and np.array_equal(two[1], one[1])
        assert float(one[0].sum()) > 0
    finally:
        integ.close()


def test_independent_sampler_box_filter_replay(density):
    """The other parked sampler state: the independent sampler's PCG32 (state, increment)."""
    from acceleratedvolrenderer_amd import VolPathIntegrator
    from oracle import binding
    scene = _cloud_scene(density, sampler="independent", filter="box")
    integ = VolPathIntegrator(scene, maxdepth=MAXDEPTH, spp=8, seed=0, device=0)
    try:
        canon = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
        integ.render(0, 8)
        assert integ.ctx.last_kernel() == "k_paths<false, true, 0, 0, false, false>"
        exact, total = _count_exact(integ, canon, scene.film, 0, 8)
        print(f"independent + box: {exact}/{total} samples bit-identical")
        assert exact == total == W * H * 8
    finally:
        integ.close()
