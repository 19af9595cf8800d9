"""Fast render mode (avr_set_render_mode 1) over every k_paths instantiation family.

tests/test_gpu_fast.py runs the fast half of avr_create's kernel table in one family (gray
GridMedium, no emission, no image light, box interface, RGBFilm). This module runs it in the
others: one named case per (medium kind, emission, gray, sampler, image light / power sampler,
interface shape, film) family, built from the scene builders of the replay tests
(tests/test_gpu_parity.py, test_gpu_sphere.py, test_gpu_kpaths_parked.py) on their small films,
two (grid-affine, cloud-affine) behind a rotation, a non-uniform scale and a box that is not
the unit cube (tests/media_cases.py), and three of the light stage's cases (tests/light_cases.py: two
surviving map pixels under a mirrored transform, two image lights, eight lights), which keep their
full depth: the corners' variance does not defeat the correlated-film criterion (err / noise 0.204).
Each case names, by hand, the instantiation `avr_last_kernel` must report; avr_last_kernel prints
the flags and not the table slot, so every case also checks what the launched kernel computed:

  * counts: film weights and every per-sample filter weight bit-equal to the oracle's;
  * wavelengths: |lambda_fast - lambda_canonical| < 1e-3 nm per sample (the replay bound; the
    hardware log moves lambda by ~2e-5 nm); the pdf the film divides by within relative 1e-5 of
    0.0039398042 / cosh^2(0.0072 (lambda - 538)) in float64 at the device's own lambda (RGB films:
    __expf is a few ulp and the square doubles it), exactly 1 / (lmax - lmin) for the spectral film;
  * film, correlated: rel RMS against the platform oracle at seed 0 <= 0.5 x the rel RMS between
    two oracle seeds (tests/test_gpu_fast.py's criterion);
  * film, unbiased: the frame mean of a 64 x longer device render within 4 se + 1e-6 |mean| of
    the two-seed oracle mean (same source);
  * gray instantiations: >= 90 % of the samples with L_canonical > 0 within relative 1e-3 of the
    canonical oracle per component (a gray path weight cancels T_maj against its own first
    component, so only last bits of log / sin / cos and flipped decisions differ; the platform
    and canonical oracles, which differ in the same way, leave < 0.4 % outside 1e-2). Non-gray
    cases carry FastExp-vs-exp differences in their T_maj ratios: quantiles printed only.

Where the closeness premise ends. VolPathIntegrator seeds a shadow ray's RNG with the bits of
its origin and direction (SampleLd, integrators.cpp:1338), so a scatter position that differs
in its last bit draws another, equally valid transmittance estimate for the light sample. The
first scatter position comes from one hardware log and mostly keeps its bits (>= 94.8 % of the
samples stay within 1e-3 at maxdepth 1 in every gray case); behind the first phase sample
(hardware sin / cos) nearly every origin differs, and the share falls with depth to 78-92 % in
the gray cases with a dense single-segment medium, an image light or the cloud's forward peak
(measured: homogeneous 0.873, cloudmedium 0.881, image-gray 0.835, power-image 0.834,
homogeneous-image 0.784, power 0.919, grid-zsobol-parked 0.900 at their full depths; a scene
with the uniform sky alone, which spawns no shadow ray, stays 100 % bit-identical to replay at
maxdepth 8). Those cases keep their full depth for every other criterion and assert the 90 %
share on a second render at `close_depth` 1 (one NEE, one phase sample, a second free flight and
the MIS-weighted escape). grid-zsobol-wide's three samples per pixel of the forward-peaked cloud
miss the correlated film criterion from maxdepth 2 on for the same reason (err / noise 0.67 at 2,
0.75 at 100, 0.02 at 1: a few unoccluded light samples carry the frame's variance), so that case
runs at maxdepth 1, where the reference alone and the device both pass.

Two tests need no device: the table's expected strings cover every (medium, image) pair and,
within GridMedium, every (emissive, gray) pair and sampler; and every case's inputs pass the
correlated-film and closeness caps with the canonical oracle standing in for the device.

test_fast_order_not_results: the schedule (passes, refill / DDA budget, pixel order, ZSobol pass
table, camera records made ahead) changes no bit in fast mode either. Known answers (white
furnace, Beer-Lambert) and the edge shapes of tests/test_gpu_edges.py follow.

Measured on an MI355X (film error / two-seed noise; frame mean distance in se; share of samples
within 1e-3 and the 50 / 90 / 99 % quantiles of the per-sample relative difference, at the case's
full depth; the share at its close_depth, which is the one asserted; max |dlambda| in nm; max
relative pdf error):

  case                     err/noise  mean (se)  share   q50 q90 q99              share, shallow     max |dlam|  max pdf err
  grid-chromatic           0.137      +1.09      0.9030  1.9e-04 3.9e-04 8.9e-01  -                  6.1e-05     5.0e-07
  grid-emissive            0.078      +0.64      0.9534  0.0e+00 1.8e-07 3.1e-01  -                  6.1e-05     5.0e-07
  grid-emissive-chromatic  0.097      +1.35      0.9276  1.2e-04 3.0e-04 4.1e-01  -                  6.1e-05     5.0e-07
  grid-chromatic-zsobol    0.142      +0.79      0.9105  1.8e-04 3.5e-04 8.6e-01  -                  1.2e-04     6.3e-07
  grid-zsobol-parked       0.144      -2.52      0.9000  0.0e+00 8.7e-04 4.1e-01  0.9968 at depth 1  1.2e-04     6.3e-07
  grid-zsobol-wide         0.020      -          0.9984  0.0e+00 0.0e+00 2.2e-07  -                  6.1e-05     5.2e-07
  homogeneous              0.336      -1.10      0.8729  0.0e+00 4.0e-01 1.7e+00  0.9681 at depth 1  6.1e-05     5.0e-07
  homogeneous-emissive     0.047      +0.96      0.9727  6.7e-05 1.1e-04 2.0e-01  -                  6.1e-05     5.0e-07
  cloudmedium              0.240      +1.37      0.8806  0.0e+00 2.4e-02 3.6e-01  0.9577 at depth 1  6.1e-05     5.0e-07
  vdb-aligned              0.184      -2.28      0.9681  0.0e+00 0.0e+00 4.0e-01  -                  6.1e-05     5.0e-07
  vdb-rotated-temperature  0.011      +0.45      0.9877  7.1e-05 2.6e-04 7.0e-02  -                  6.1e-05     5.0e-07
  rgb                      0.110      +0.17      0.9297  1.5e-07 3.7e-07 3.6e-01  -                  6.1e-05     5.0e-07
  rgb-emissive             0.002      -0.82      0.9510  1.2e-07 5.5e-07 1.6e-02  -                  6.1e-05     5.0e-07
  image-gray               0.115      -0.57      0.8352  0.0e+00 1.0e-01 5.9e-01  0.9949 at depth 1  6.1e-05     5.0e-07
  image-distant-chromatic  0.131      +2.11      0.8686  1.3e-04 7.9e-02 7.2e-01  -                  6.1e-05     5.0e-07
  power                    0.194      -0.45      0.9186  0.0e+00 1.2e-07 6.6e-01  0.9964 at depth 1  6.1e-05     5.0e-07
  power-image              0.157      +1.05      0.8342  0.0e+00 1.2e-01 7.7e-01  0.9936 at depth 1  6.1e-05     5.0e-07
  vdb-image                0.099      -2.23      0.9466  0.0e+00 4.8e-07 3.2e-01  -                  6.1e-05     5.0e-07
  rgb-image                0.068      +0.35      0.8799  1.8e-07 2.9e-02 3.4e-01  -                  6.1e-05     5.0e-07
  homogeneous-image        0.209      -2.81      0.7838  0.0e+00 3.8e-01 1.3e+00  0.9481 at depth 1  6.1e-05     5.0e-07
  sphere                   0.057      +0.30      0.9954  0.0e+00 3.8e-05 1.7e-04  -                  6.1e-05     5.0e-07
  convex                   0.140      +0.44      0.9742  0.0e+00 0.0e+00 3.2e-01  -                  6.1e-05     5.0e-07
  spectral                 0.125      +1.03      0.9051  1.7e-04 3.2e-04 6.3e-01  -                  0.0e+00     0.0e+00
  grid-affine              0.182      -1.93      0.9509  0.0e+00 0.0e+00 5.1e-01  -                  6.1e-05     5.0e-07
  cloud-affine             0.056      -0.65      0.9935  0.0e+00 0.0e+00 3.5e-07  -                  6.1e-05     5.0e-07
  lights-corners-mirror    0.204      +0.29      0.8509  0.0e+00 2.1e-01 2.0e+00  0.9969 at depth 1  6.1e-05     4.8e-07
  lights-two-images        0.042      -0.68      0.8428  0.0e+00 1.7e-01 1.3e+00  0.9962 at depth 1  6.1e-05     4.8e-07
  lights-eight             0.150      +0.92      0.8912  0.0e+00 1.8e-02 7.8e-01  0.9971 at depth 1  6.1e-05     4.8e-07

  spectral film: bucket sums rel RMS 7.2e-02 against a two-seed noise of 6.5e-01.
  White furnace (grid, homogeneous, NanoVDB): max |L - 1| = 0 over 4096 samples each.
  Beer-Lambert: grid 0.37904 (0.37956), homogeneous 0.36873 (0.36788), NanoVDB 0.39084 (0.39161),
  4 se = 1.0e-02; sphere chords: frame sum 737.54 (738.52, sd 0.77).
  Edge shapes: err / noise <= 0.34 (single_voxel); "empty": fast L == replay L in every sample.
"""
import functools
import os
import sys
from typing import Callable, NamedTuple

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import light_cases   # noqa: E402
import media_cases   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 24, 20, 8

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()


def device(fn):
    """A device test: marked gpu, skipped without a HIP device."""
    return gpu(pytest.mark.usefixtures("_gpu")(fn))


def _rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(1e-12, np.sqrt(np.mean(b ** 2))))


# ---------------------------------------------------------------------------------- scenes
def _dens(n, seed, lo=0.25):
    return (lo + np.random.default_rng(seed).random((n, n, n), dtype=np.float32)).astype(np.float32)


def _grid(variant, n=16, seed=5, lo=0.25):
    from acceleratedvolrenderer_amd import scenes
    return scenes.s_uniform(n=n, width=W, height=H, variant=variant, density=_dens(n, seed, lo))


def _with(base, **kw):
    """The scene `base` with some of camera / film / medium / lights / sampler replaced."""
    from acceleratedvolrenderer_amd.scene import Scene
    a = dict(camera=base.camera, film=base.film, medium=base.medium, lights=base.lights, sampler=base.sampler)
    a.update(kw)
    return Scene(a["camera"], a["film"], a["medium"], a["lights"], sampler=a["sampler"])


def _zsobol_gaussian(base, pixelsamples, width=W, height=H):
    from acceleratedvolrenderer_amd.scene import GaussianFilter, RGBFilm, ZSobolSampler
    return _with(base, film=RGBFilm(width, height, filter=GaussianFilter()), sampler=ZSobolSampler(pixelsamples))


def _cloud_cut():
    """24 x 40 x 56 voxels cut from the cloud density (tests/test_gpu_kpaths_parked.py)."""
    from oracle import binding
    return np.ascontiguousarray(binding.cloud_grid(56)[:, :40, :24])


def _zsobol_wide(pixelsamples=None):
    """tests/test_gpu_kpaths_parked.py::test_wide_zsobol_index_on_a_small_film's scene."""
    from acceleratedvolrenderer_amd import scenes
    base = scenes.s_uniform(n=1, width=2048, height=2, variant="scatter")
    cloud = scenes.s_cloud(_cloud_cut(), width=48, height=32, sampler="zsobol", spp=64, filter="gaussian")
    return _zsobol_gaussian(_with(base, medium=cloud.medium, lights=cloud.lights), 4096, 2048, 2)


def _zsobol_parked(pixelsamples=None):
    from acceleratedvolrenderer_amd import scenes
    from oracle import binding
    return scenes.s_cloud(binding.cloud_grid(24), width=W, height=H, sampler="zsobol", spp=pixelsamples or 16,
                          filter="gaussian")


def _analytic(kind):
    from acceleratedvolrenderer_amd import CloudMedium, HomogeneousMedium, scenes
    base = scenes.s_uniform(n=4, width=W, height=H, variant="scatter")
    med = {"homogeneous": lambda: HomogeneousMedium(sigma_a=0.5, sigma_s=2.0, g=0.3),
           "homogeneous_emissive": lambda: HomogeneousMedium(sigma_a=np.linspace(0.5, 1.5, 471), sigma_s=1.0, Le=1.0,
                                                             Lescale=2.0),
           "cloud": lambda: CloudMedium(sigma_a=0.1, sigma_s=3.0, g=0.6)}[kind]()
    return _with(base, medium=med)


def _vdb(case):
    """tests/test_gpu_parity.py::test_nanovdb_medium_replay's scenes ("aligned", "temperature":
    the rotated transform, an offset temperature grid and a chromatic sigma_a)."""
    from acceleratedvolrenderer_amd import scenes
    rng = np.random.default_rng(12)
    n = 20
    d = np.zeros((n, n, n), np.float32)
    d[3:17, 2:18, 4:16] = (0.2 + rng.random((14, 16, 12))).astype(np.float32)
    d[8:16, 8:16, 0:8] = 0.8
    if case == "aligned":
        return scenes.s_vdb(d, W, H, variant="scatter")
    c, s = np.cos(np.radians(25)), np.sin(np.radians(25))
    m = np.eye(4)
    m[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([0.8 / n, 1.0 / n, 0.7 / n])
    m[:3, 3] = [0.25, 0.0, 0.15]
    z, y, x = np.meshgrid(*(np.linspace(0, 1, n, dtype=np.float32),) * 3, indexing="ij")
    temp = (50 + 4000 * x * (1 - y) + 300 * z).astype(np.float32)
    tg = scenes.vdb_grid(temp, index_to_world=m, index_min=(2, 0, -1))
    return scenes.s_vdb(scenes.vdb_grid(d, index_to_world=m), W, H, variant="scatter", temperature=tg,
                        sigma_a=np.linspace(0.5, 1.5, 471).astype(np.float32), Lescale=1.5,
                        temperatureoffset=20.0, temperaturescale=1.1)


def _rgb_coeffs(rng, shape, scale_hi=3.0):
    """Random RGBSigmoidPolynomial coefficients + scale per voxel (tests/test_gpu_parity.py)."""
    c = np.empty(shape + (4,), np.float32)
    c[..., 0] = rng.uniform(-2e-5, 2e-5, shape)
    c[..., 1] = rng.uniform(-0.02, 0.02, shape)
    c[..., 2] = rng.uniform(-5, 5, shape)
    c[..., 3] = rng.uniform(0.2, scale_hi, shape)
    return c


def _rgb(case):
    from acceleratedvolrenderer_amd import RGBGridMedium, scenes
    rng = np.random.default_rng(31)
    shape = (7, 9, 8)
    base = scenes.s_uniform(n=1, width=W, height=H, variant="scatter")
    kw = dict(g=0.25, scale=1.3)
    if case == "absorbing_scattering":
        med = RGBGridMedium(sigma_a_coeffs=_rgb_coeffs(rng, shape, 0.8), sigma_s_coeffs=_rgb_coeffs(rng, shape), **kw)
    else:
        med = RGBGridMedium(sigma_a_coeffs=_rgb_coeffs(rng, shape, 0.8), sigma_s_coeffs=_rgb_coeffs(rng, shape),
                            Le_coeffs=_rgb_coeffs(rng, shape, 2.0), Lescale=0.7, **kw)
    return _with(base, medium=med)


def _image_light(rotated=True):
    """tests/test_gpu_parity.py::test_image_infinite_light_replay's light: the equal-area map with
    a bright spot over the cells of pbrt's sRGB table it touches (tests/golden)."""
    from acceleratedvolrenderer_amd import ImageInfiniteLight, RGBToSpectrumTable
    golden = os.path.join(ROOT, "tests", "golden")
    table = RGBToSpectrumTable.load(os.path.join(golden, "srgb_table_subset.npz"))
    if golden not in sys.path:
        sys.path.insert(0, golden)
    from make_srgb_subset import envmap_image
    rot = np.eye(4)
    if rotated:
        c, s = np.cos(0.7), np.sin(0.7)
        rot[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    return ImageInfiniteLight(image=envmap_image(), rgb_table=table, world_from_light=rot, scale=2.0)


def _distant():
    from acceleratedvolrenderer_amd import DistantLight
    return DistantLight(from_=(1, 1, -1), to=(0, 0, 0), scale=1.5)


def _sphere():
    from acceleratedvolrenderer_amd import scenes
    return scenes.s_sphere(n=16, width=W, height=H, variant="chromatic", density=_dens(16, 9, 0.3),
                           center=(0.5, 0.45, 0.5), radius=0.4, camera="perspective")


def _convex():
    from acceleratedvolrenderer_amd import scenes
    return scenes.s_mesh_interface(n=16, width=W, height=H, variant="scatter", density=_dens(16, 9, 0.3))


def _spectral():
    from acceleratedvolrenderer_amd import SpectralFilm
    return _with(_grid("chromatic"), film=SpectralFilm(W, H, nbuckets=7, lambdamin=400.0, lambdamax=700.0))


def _affine(kind):
    """tests/media_cases.py's "affine" box: world_from_medium a rotation times a non-uniform scale,
    the general Bounds3::Offset branch."""
    return media_cases.scene_for("affine", kind)


class Case(NamedTuple):
    id: str
    make: Callable          # (pixelsamples=None) -> Scene; pixelsamples: a ZSobol sampler's, for a longer render
    maxdepth: int
    kernel: str             # avr_last_kernel(), written by hand from the scene's flags
    spp: int = SPP
    lightsampler: str = "bvh"
    first: int = 0          # the sample range is [first, first + spp)
    unbiased: bool = True   # False: the sample range is pinned, no longer render
    close_depth: int = -1   # a gray case's maxdepth for the per-sample closeness share (-1: maxdepth)


def _k(em, gray, sampler, med, image):
    b = lambda v: "true" if v else "false"
    return f"k_paths<{b(em)}, {b(gray)}, {sampler}, {med}, {b(image)}, true>"


CASES = [
    Case("grid-chromatic", lambda pixelsamples=None: _grid("chromatic"), 5, "k_paths<false, false, 0, 0, false, true>"),
    Case("grid-emissive", lambda pixelsamples=None: _grid("emissive"), 5, "k_paths<true, true, 0, 0, false, true>"),
    Case("grid-emissive-chromatic", lambda pixelsamples=None: _grid("emissive_chromatic"), 5,
         "k_paths<true, false, 0, 0, false, true>"),
    Case("grid-chromatic-zsobol", lambda pixelsamples=None: _zsobol_gaussian(_grid("chromatic"), pixelsamples or 16), 5,
         "k_paths<false, false, 2, 0, false, true>", spp=16),
    Case("grid-zsobol-parked", _zsobol_parked, 100, "k_paths<false, true, 2, 0, false, true>", spp=16, close_depth=1),
    Case("grid-zsobol-wide", _zsobol_wide, 1, "k_paths<false, true, 3, 0, false, true>", spp=3, first=4093,
         unbiased=False),
    Case("homogeneous", lambda pixelsamples=None: _analytic("homogeneous"), 8, "k_paths<false, true, 0, 1, false, true>",
         close_depth=1),
    Case("homogeneous-emissive", lambda pixelsamples=None: _analytic("homogeneous_emissive"), 8,
         "k_paths<true, false, 0, 1, false, true>"),
    Case("cloudmedium", lambda pixelsamples=None: _analytic("cloud"), 8, "k_paths<false, true, 0, 1, false, true>",
         close_depth=1),
    Case("vdb-aligned", lambda pixelsamples=None: _vdb("aligned"), 8, "k_paths<false, true, 0, 3, false, true>"),
    Case("vdb-rotated-temperature", lambda pixelsamples=None: _vdb("temperature"), 8,
         "k_paths<true, false, 0, 3, false, true>"),
    Case("rgb", lambda pixelsamples=None: _rgb("absorbing_scattering"), 8, "k_paths<false, false, 0, 4, false, true>"),
    Case("rgb-emissive", lambda pixelsamples=None: _rgb("emissive"), 8, "k_paths<true, false, 0, 4, false, true>"),
    Case("image-gray", lambda pixelsamples=None: _with(_grid("scatter", 6, 2, 0.2), lights=[_image_light()]), 6,
         "k_paths<false, true, 0, 0, true, true>", close_depth=1),
    Case("image-distant-chromatic",
         lambda pixelsamples=None: _with(_grid("chromatic", 6, 2, 0.2), lights=[_distant(), _image_light()]), 6,
         "k_paths<false, false, 0, 0, true, true>"),
    Case("power", lambda pixelsamples=None: _grid("scatter", 6, 6, 0.2), 6, "k_paths<false, true, 0, 0, true, true>",
         lightsampler="power", close_depth=1),
    Case("power-image", lambda pixelsamples=None: _with(_grid("scatter", 6, 6, 0.2), lights=[_distant(), _image_light(False)]),
         6, "k_paths<false, true, 0, 0, true, true>", lightsampler="power", close_depth=1),
    Case("vdb-image", lambda pixelsamples=None: _with(_vdb("aligned"), lights=[_image_light()]), 8,
         "k_paths<false, true, 0, 3, true, true>"),
    Case("rgb-image", lambda pixelsamples=None: _with(_rgb("absorbing_scattering"), lights=[_image_light()]), 8,
         "k_paths<false, false, 0, 4, true, true>"),
    Case("homogeneous-image", lambda pixelsamples=None: _with(_analytic("homogeneous"), lights=[_image_light()]), 8,
         "k_paths<false, true, 0, 1, true, true>", close_depth=1),
    Case("sphere", lambda pixelsamples=None: _sphere(), 8, "k_paths<false, false, 0, 0, false, true>"),
    Case("convex", lambda pixelsamples=None: _convex(), 8, "k_paths<false, true, 0, 0, false, true>"),
    Case("spectral", lambda pixelsamples=None: _spectral(), 5, "k_paths<false, false, 0, 0, false, true>"),
    # a rotation, a non-uniform scale and a box of three different extents (tests/media_cases.py)
    Case("grid-affine", lambda pixelsamples=None: _affine("gray"), 6, "k_paths<false, true, 0, 0, false, true>"),
    Case("cloud-affine", lambda pixelsamples=None: _affine("cloud"), 6, "k_paths<false, true, 0, 1, false, true>"),
    # the light stage's cases (tests/light_cases.py): two surviving pixels under a mirrored transform,
    # two image lights, eight lights with the image light in the last slot
    Case("lights-corners-mirror", lambda pixelsamples=None: light_cases.scene_for("corners-5+mirror"), 6,
         "k_paths<false, true, 0, 0, true, true>", close_depth=1),
    Case("lights-two-images", lambda pixelsamples=None: light_cases.scene_for("two-images"), 6,
         "k_paths<false, true, 0, 0, true, true>", close_depth=1),
    Case("lights-eight", lambda pixelsamples=None: light_cases.scene_for("eight"), 6,
         "k_paths<false, true, 0, 0, true, true>", close_depth=1),
]
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]

# tests/test_gpu_fast.py::test_fast_mode_statistical_parity: "uniform" and "cloud"
EXISTING = ["k_paths<false, true, 0, 0, false, true>", "k_paths<false, true, 2, 0, false, true>"]


def _flags(kernel):
    """(emissive, gray, sampler, medium, image, fast) of a "k_paths<...>" string."""
    assert kernel.startswith("k_paths<") and kernel.endswith(">"), kernel
    a = [s.strip() for s in kernel[len("k_paths<"):-1].split(",")]
    assert len(a) == 6, kernel
    t = {"true": True, "false": False}
    return t[a[0]], t[a[1]], int(a[2]), int(a[3]), t[a[4]], t[a[5]]


def test_case_table_names_every_dispatch_family():
    """The expected strings, with tests/test_gpu_fast.py's two, name every (medium, image) pair
    and, within GridMedium, every (emissive, gray) pair and each sampler: a case deleted later
    shows as a hole."""
    assert len(set(IDS)) == len(IDS)
    flags = [_flags(k) for k in [c.kernel for c in CASES] + EXISTING]
    assert all(f[5] for f in flags), "every case names a fast instantiation"
    assert all(not (f[3] == 4 and f[1]) for f in flags), "RGBGridMedium has no gray instantiation"
    assert {(f[3], f[4]) for f in flags} == {(m, i) for m in (0, 1, 3, 4) for i in (False, True)}
    grid = [f for f in flags if f[3] == 0]
    assert {(f[0], f[1]) for f in grid} == {(e, g) for e in (False, True) for g in (False, True)}
    assert {f[2] for f in grid} == {0, 2, 3}


# ------------------------------------------------------------------------------- references
def _samples(run, film, first, ns):
    """(L, lambda, pdf, filter weight) of every (sample, pixel) of [first, first + ns), in the
    order of avr_last_pass_samples (sample-major, row-major pixels)."""
    npix = film.width * film.height
    L = np.zeros((ns * npix, 4), np.float32)
    lam = np.zeros((ns * npix, 4), np.float32)
    pdf = np.zeros((ns * npix, 4), np.float32)
    wts = np.zeros(ns * npix, np.float32)
    for s in range(ns):
        for pix in range(npix):
            g = s * npix + pix
            L[g], lam[g], pdf[g], _, wts[g] = run.pixel_sample(pix % film.width, pix // film.width, first + s,
                                                               with_weight=True)
    return L, lam, pdf, wts


class Ref:
    """The oracle's answers for one scene and sample range, each computed once."""

    def __init__(self, scene, maxdepth, first, spp, lightsampler="bvh"):
        self.scene, self.maxdepth, self.first, self.spp, self.lightsampler = scene, maxdepth, first, spp, lightsampler
        self.spectral = bool(getattr(scene.film, "nbuckets", 0))

    def _run(self, seed, libm="platform"):
        from oracle import binding
        return binding.OracleRun(self.scene, max_depth=self.maxdepth, seed=seed, libm=libm, lightsampler=self.lightsampler)

    def _film(self, run):
        """{"rgb", "w"[, "bs", "bw"]} of the sample range."""
        a, b = self.first, self.first + self.spp
        if self.spectral:
            return dict(zip(("rgb", "w", "bs", "bw"), run.render_spectral(a, b, nthreads=8)))
        return dict(zip(("rgb", "w"), run.render(a, b, nthreads=8)))

    @functools.cached_property
    def seed0(self):
        return self._film(self._run(0))

    @functools.cached_property
    def seed1(self):
        return self._film(self._run(1))

    @functools.cached_property
    def canonical_film(self):
        return self._film(self._run(0, "canonical"))

    @functools.cached_property
    def canonical(self):
        return _samples(self._run(0, "canonical"), self.scene.film, self.first, self.spp)

    @functools.cached_property
    def platform(self):
        return _samples(self._run(0), self.scene.film, self.first, self.spp)

    def image(self, film):
        from acceleratedvolrenderer_amd.scene import film_rgb
        return film_rgb(self.scene.film, film["rgb"], film["w"])

    @functools.cached_property
    def noise(self):
        return _rel_rms(self.image(self.seed1), self.image(self.seed0))

    @functools.cached_property
    def mean_and_se(self):
        """The two-seed oracle frame mean and its standard error from the per-pixel seed
        difference (tests/test_gpu_fast.py: var of (o + o1) / 2 over N values = var(o - o1) / (4 N);
        a 64 x longer device render adds 1 / 64 of it)."""
        o, o1 = self.image(self.seed0), self.image(self.seed1)
        return 0.5 * (o.mean() + o1.mean()), 1.02 * float(np.std(o - o1)) / (2 * np.sqrt(o.size))


@functools.lru_cache(maxsize=None)
def _ref(case_id, shallow=False):
    """The case's reference; shallow: at its close_depth, over the same scene."""
    c = BY_ID[case_id]
    if shallow and c.close_depth >= 0:
        return Ref(_ref(case_id).scene, c.close_depth, c.first, c.spp, c.lightsampler)
    return _ref(case_id) if shallow else Ref(c.make(), c.maxdepth, c.first, c.spp, c.lightsampler)


def _assert_film_correlated(ref, film, what):
    """rel RMS against the platform oracle at seed 0 <= 0.5 x the two-seed noise; a spectral
    film's RGB part and its bucket sums. Returns err / noise of the RGB image."""
    err, noise = _rel_rms(ref.image(film), ref.image(ref.seed0)), ref.noise
    assert err <= 0.5 * noise, f"{what}: film rel RMS {err:.3e} vs 0.5 x MC noise {noise:.3e}"
    if ref.spectral:
        err_b, noise_b = _rel_rms(film["bs"], ref.seed0["bs"]), _rel_rms(ref.seed1["bs"], ref.seed0["bs"])
        print(f"{what}: bucket sums rel RMS {err_b:.3e} (MC noise {noise_b:.3e})")
        assert np.array_equal(film["bw"], ref.seed0["bw"]), f"{what}: bucket weights (bucket choice only)"
        assert err_b <= 0.5 * noise_b, f"{what}: bucket sums rel RMS {err_b:.3e} vs 0.5 x MC noise {noise_b:.3e}"
    return err / noise if noise > 0 else 0.0


def _closeness(L, L_ref):
    """Per-sample relative difference (the largest over the four components; 0 / 0 = 0, x / 0 = inf)
    over the samples with L_ref > 0: (share within 1e-3, [50, 90, 99 % quantiles], samples)."""
    L, L_ref = L.astype(np.float64), L_ref.astype(np.float64)
    lit = (L_ref > 0).any(axis=1)
    d, r = np.abs(L - L_ref)[lit], np.abs(L_ref)[lit]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(d == 0, 0.0, d / r).max(axis=1)
    if rel.size == 0:
        return 1.0, [0.0, 0.0, 0.0], 0
    return float(np.mean(rel <= 1e-3)), [float(q) for q in np.quantile(rel, [0.5, 0.9, 0.99])], int(rel.size)


def _is_gray(case):
    return _flags(case.kernel)[1]


@pytest.mark.parametrize("case_id", IDS)
def test_case_inputs_pass_their_caps_by_the_oracle_alone(case_id):
    """No device: the canonical oracle stands in for it. Its film passes the correlated
    criterion against the platform oracle, a gray case's samples the closeness share, the
    two-seed standard error is non-zero and the frame is not black — so a device failure of
    these caps is the device's, not the inputs'."""
    case, ref = BY_ID[case_id], _ref(case_id)
    assert np.array_equal(ref.canonical_film["w"], ref.seed0["w"])
    assert np.array_equal(ref.canonical[3], ref.platform[3]), "filter weights do not depend on the libm"
    ratio = _assert_film_correlated(ref, ref.canonical_film, f"{case_id} (canonical oracle)")
    share, q, n = _closeness(ref.canonical[0], ref.platform[0])
    mean, se = ref.mean_and_se
    print(f"inputs {case_id}: err/noise {ratio:.3f}, noise {ref.noise:.3e}, frame mean {mean:.5f} (se {se:.2e}); "
          f"canonical vs platform: {share:.4f} of {n} lit samples within 1e-3, quantiles {q[0]:.1e} {q[1]:.1e} {q[2]:.1e}")
    assert se > 0 and mean > 0 and n > 0
    assert float(ref.image(ref.seed0).min()) >= 0
    if _is_gray(case):
        assert share >= 0.9
        if case.close_depth >= 0:
            shallow = _ref(case_id, True)
            share, q, n = _closeness(shallow.canonical[0], shallow.platform[0])
            print(f"inputs {case_id} at maxdepth {case.close_depth}: {share:.4f} of {n} lit samples within 1e-3")
            assert share >= 0.9 and n > 0


# ----------------------------------------------------------------------------- device: matrix
def _integ(scene, maxdepth, spp, lightsampler="bvh", mode="fast", **kw):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    return VolPathIntegrator(scene, maxdepth=maxdepth, spp=spp, seed=0, device=0, mode=mode,
                             lightsampler=lightsampler, **kw)


def _device_film(integ, ref, first, spp):
    rgb, w = integ.render(first, first + spp)
    film = {"rgb": rgb, "w": w}
    if ref.spectral:
        film["bs"], film["bw"] = integ.spectral_sums()
    return film


def _pdf_error(ref, lam, pdf):
    """Spectral film: every pdf exactly 1 / (lmax - lmin) in float32 (returns 0). RGB film: the
    largest relative error against VisibleWavelengthsPDF in float64 at the device's lambda."""
    f = ref.scene.film
    if ref.spectral:
        want = np.float32(1) / (np.float32(f.lambdamax) - np.float32(f.lambdamin))
        assert np.all(pdf.view(np.uint32) == want.view(np.uint32))
        return 0.0
    want = 0.0039398042 / np.cosh(0.0072 * (lam.astype(np.float64) - 538.0)) ** 2
    return float(np.max(np.abs(pdf.astype(np.float64) - want) / want))


@device
@pytest.mark.parametrize("case_id", IDS)
def test_fast_matrix(case_id):
    case, ref = BY_ID[case_id], _ref(case_id)
    scene, first, spp = ref.scene, case.first, case.spp
    npix = scene.film.width * scene.film.height
    integ = _integ(scene, case.maxdepth, first + spp, case.lightsampler)
    try:
        film = _device_film(integ, ref, first, spp)
        # instantiation
        assert integ.ctx.last_kernel() == case.kernel
        assert integ.stats()["loop_iterations"] > 0
        got_first, ns, L, lam, pdf = integ.ctx.last_pass_samples(npix, spp)
        assert (got_first, ns) == (first, spp)
        wts = integ.ctx.last_pass_weights(npix, spp)
        # counts, exact
        assert np.array_equal(film["w"], ref.seed0["w"]), "every (pixel, sample) path traced once, same filter weights"
        L_c, lam_c, _, wts_c = ref.canonical
        assert np.array_equal(wts.view(np.uint32), wts_c.view(np.uint32))
        # wavelengths
        dlam = float(np.max(np.abs(lam.astype(np.float64) - lam_c.astype(np.float64))))
        pdf_err = _pdf_error(ref, lam, pdf)
        share, q, n = _closeness(L, L_c)
        print(f"fast matrix {case_id}: max |dlambda| {dlam:.2e} nm, max pdf error {pdf_err:.2e}; {share:.4f} of {n} lit "
              f"samples within 1e-3 of the canonical oracle, quantiles {q[0]:.1e} {q[1]:.1e} {q[2]:.1e}")
        assert dlam < 1e-3
        assert pdf_err <= 1e-5
        assert np.all(np.isfinite(L))
        # film, correlated
        ratio = _assert_film_correlated(ref, film, f"fast matrix {case_id}")
        # film, unbiased: 64 x the samples on the device (a ZSobol case on a sampler of that many)
        dist = float("nan")
        if case.unbiased:
            mean, se = ref.mean_and_se
            if scene.sampler.type_id == 1:
                big = _integ(case.make(pixelsamples=64 * spp), case.maxdepth, 64 * spp, case.lightsampler)
                try:
                    rgb_b, w_b = big.render()
                    assert big.ctx.last_kernel() == case.kernel
                finally:
                    big.close()
            else:
                rgb_b, w_b = integ.render(0, 64 * spp)
            got = float(ref.image({"rgb": rgb_b, "w": w_b}).mean())
            dist = (got - mean) / se
            print(f"fast matrix {case_id}: frame mean {got:.6f} vs oracle {mean:.6f} (se {se:.2e}: {dist:+.2f} se)")
            assert abs(got - mean) <= 4 * se + 1e-6 * abs(mean)
        # the fast pass really ran other arithmetic than replay on the same context
        integ.ctx.set_render_mode("replay")
        rgb_r, w_r = integ.render(first, first + spp)
        assert integ.ctx.last_kernel() == case.kernel.replace("true>", "false>")
        assert np.array_equal(w_r, film["w"]) and not np.array_equal(rgb_r, film["rgb"])
        # per-sample closeness: gray instantiations only (90 % is a cap, not a measurement), at the
        # case's close_depth (module docstring)
        close = share
        if _is_gray(case) and case.close_depth >= 0:
            integ.ctx.set_render_mode("fast")
            integ.ctx.film_clear()
            integ.ctx.render(first, first + spp, 0, case.close_depth)
            assert integ.ctx.last_kernel() == case.kernel
            _, _, L_s, _, _ = integ.ctx.last_pass_samples(npix, spp)
            close, q_s, n_s = _closeness(L_s, _ref(case_id, True).canonical[0])
            print(f"fast matrix {case_id} at maxdepth {case.close_depth}: {close:.4f} of {n_s} lit samples within 1e-3, "
                  f"quantiles {q_s[0]:.1e} {q_s[1]:.1e} {q_s[2]:.1e}")
            assert n_s > 0
        shallow = f"{close:.4f} at depth {case.close_depth}" if case.close_depth >= 0 else "-"
        print(f"fast matrix record | {case_id} | {ratio:.3f} | {dist:+.2f} | {share:.4f} | {q[0]:.1e} {q[1]:.1e} {q[2]:.1e} | "
              f"{shallow} | {dlam:.1e} | {pdf_err:.1e} |")
        if _is_gray(case):
            assert close >= 0.9
    finally:
        integ.close()


# ------------------------------------------------------------------ device: schedule invariants
ORDER_CASES = ["grid-chromatic-zsobol", "vdb-aligned", "image-gray", "grid-zsobol-parked"]


@device
@pytest.mark.parametrize("case_id", ORDER_CASES)
def test_fast_order_not_results(case_id):
    """Fast mode walks differently (kLite off, one decision per candidate), but its schedule is
    as result-neutral as replay's: film sums (and the last pass's samples, which the accessor
    returns in pixel order) bit-identical over repeats, pass splits, refill / DDA-budget
    schedules, a reversed pixel order, ZSobol pass-table sizes and two equal-stride calls, the
    second of which takes the camera records made ahead where the instantiation allows the
    overlap (the parked one: gray GridMedium, no emission, no image light, ZSobol)."""
    case = BY_ID[case_id]
    scene, spp, md = case.make(), case.spp, case.maxdepth
    npix = W * H
    zsobol = scene.sampler.type_id == 1
    integ = _integ(scene, md, spp, case.lightsampler)
    split = _integ(scene, md, spp, case.lightsampler, max_paths=npix * (3 if spp == 8 else 6))

    def bits(a):
        return [x.view(np.uint32) if x.dtype == np.float32 else x for x in a]

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))

    def shot(it=integ, ns=spp):
        rgb, w = it.render()
        _, got, L, lam, pdf = it.ctx.last_pass_samples(npix, spp)
        assert got == ns
        return (rgb, w), (L, lam, pdf, it.ctx.last_pass_weights(npix, spp)[:npix * ns])

    try:
        film, smp = shot()
        assert integ.ctx.last_kernel() == case.kernel and float(film[0].sum()) > 0
        film2, smp2 = shot()
        assert same(film, film2) and same(smp, smp2), "two renders of the same range"
        # three passes: the last one holds the last samples of the range
        split.ctx.reset_stats()
        tail = spp - 2 * (3 if spp == 8 else 6)
        film3, smp3 = shot(split, tail)
        assert split.ctx.stats()["medium_launches"] == 3 and split.ctx.last_kernel() == case.kernel
        assert same(film, film3), "one pass vs three"
        assert same([a[npix * (spp - tail):] for a in smp], smp3)
        for refill in (8, 32, 48):
            for dda in (4, 12):
                integ.ctx.set_refill_min(refill)
                integ.ctx.set_dda_budget(dda)
                f, s = shot()
                assert same(film, f) and same(smp, s), (refill, dda)
        integ.ctx.set_refill_min(0)
        integ.ctx.set_dda_budget(0)
        integ.ctx.set_pixel_order(np.arange(npix, dtype=np.int32)[::-1])
        f, s = shot()
        assert same(film, f) and same(smp, s), "reversed pixel order"
        integ.ctx.set_pixel_order(None)
        if zsobol:
            for dims in (0, 8, 64):
                integ.ctx.set_sampler_pass_table(dims)
                f, s = shot()
                assert same(film, f) and same(smp, s), ("pass table", dims)
            integ.ctx.set_sampler_pass_table(96)
        # two equal-stride calls, with the next pass's camera stage made ahead and without
        half = spp // 2
        for overlap in (True, False):
            integ.ctx.set_pass_overlap(overlap)
            integ.ctx.film_clear()
            integ.ctx.render(0, half, 0, md)
            integ.ctx.render(half, spp, 0, md)
            active = integ.ctx.pass_overlap_active()
            assert active == (overlap and case_id == "grid-zsobol-parked")
            assert integ.ctx.last_kernel() == case.kernel
            f = integ.film_sums()
            _, got, L, lam, pdf = integ.ctx.last_pass_samples(npix, spp)
            assert got == spp - half
            assert same(film, f), ("equal-stride calls", overlap)
            assert same([a[npix * half:] for a in smp[:3]], (L, lam, pdf))
        integ.ctx.set_pass_overlap(True)
    finally:
        integ.close()
        split.close()


# ------------------------------------------------------------------------ device: known answers
def _furnace(kind):
    from acceleratedvolrenderer_amd import HomogeneousMedium, scenes
    if kind == "grid":
        return scenes.s_uniform(n=8, width=16, height=16, variant="furnace")
    if kind == "homogeneous":
        return _with(scenes.s_uniform(n=1, width=16, height=16, variant="furnace"),
                     medium=HomogeneousMedium(sigma_a=0.0, sigma_s=4.0))
    return scenes.s_vdb(np.ones((8, 8, 8), np.float32), 16, 16, variant="furnace")


@device
@pytest.mark.parametrize("kind", ["grid", "homogeneous", "vdb"])
def test_fast_white_furnace(kind):
    """Albedo 1 in a uniform infinite light: every path that escapes carries L = Le = 1. A gray
    medium's weight is x / x, so exactly 1 is expected; the bound is 1e-5."""
    integ = _integ(_furnace(kind), 1000, 16)
    try:
        integ.render()
        assert _flags(integ.ctx.last_kernel())[1:] == (True, 0, {"grid": 0, "homogeneous": 1, "vdb": 3}[kind], False, True)
        _, ns, L, _, _ = integ.ctx.last_pass_samples(16 * 16, 16)
        worst = float(np.max(np.abs(L.astype(np.float64) - 1.0)))
        print(f"fast furnace {kind}: max |L - 1| {worst:.2e} over {L.shape[0]} samples")
        assert ns == 16 and worst <= 1e-5
    finally:
        integ.close()


def _absorber(kind):
    """(scene, expected transmittance along +z through the interior pixels)."""
    from acceleratedvolrenderer_amd import HomogeneousMedium, scenes
    n = 8
    if kind == "grid":      # the half-voxel trilinear shell: integral of the density = 1 - 0.25 / n
        return scenes.s_uniform(n=n, width=16, height=16, variant="absorber"), np.exp(-(1 - 0.25 / n))
    if kind == "homogeneous":
        return _with(scenes.s_uniform(n=1, width=16, height=16, variant="absorber"),
                     medium=HomogeneousMedium(sigma_a=1.0, sigma_s=0.0)), np.exp(-1.0)
    # NanoVDB: index i at world i / n, values at integer indices, background 0 past index n - 1:
    # ones over [0, n - 1] and a linear ramp to 0 over [n - 1, n], so the integral is 1 - 0.5 / n
    return scenes.s_vdb(np.ones((n, n, n), np.float32), 16, 16, variant="absorber"), np.exp(-(1 - 0.5 / n))


@device
@pytest.mark.parametrize("kind", ["grid", "homogeneous", "vdb"])
def test_fast_absorber_beer_lambert(kind):
    """L = exp(-integral of sigma_a) (tests/test_gpu_parity.py::test_absorber_beer_lambert_analytic):
    the mean over the interior pixels at 256 spp within 4 binomial standard errors."""
    Wf = Hf = 16
    spp = 256
    scene, want = _absorber(kind)
    integ = _integ(scene, 5, spp)
    try:
        integ.render()
        assert _flags(integ.ctx.last_kernel())[5]
        _, ns, L, _, _ = integ.ctx.last_pass_samples(Wf * Hf, spp)
        assert ns == spp
        Lm = L.reshape(ns, Hf, Wf, 4)[:, 2:-2, 2:-2, :].astype(np.float64)
        tol = 4 * np.sqrt(want * (1 - want) / Lm[..., 0].size)
        print(f"fast absorber {kind}: mean L {Lm[..., 0].mean():.6f} vs Beer-Lambert {want:.6f} (tol {tol:.2e})")
        for c in range(4):
            assert abs(Lm[..., c].mean() - want) < tol
    finally:
        integ.close()


@device
def test_fast_sphere_absorber_beer_lambert():
    """tests/test_gpu_sphere.py::test_sphere_interface_absorber_beer_lambert_on_device in fast
    mode: Beer-Lambert along the chords of the interface sphere."""
    from acceleratedvolrenderer_amd import scenes
    n, Ws, Hs, R, spp = 16, 32, 32, 0.45, 256
    integ = _integ(scenes.s_sphere(n=n, width=Ws, height=Hs, variant="absorber", radius=R), 5, spp)
    try:
        integ.render()
        assert _flags(integ.ctx.last_kernel())[5]
        _, _, L, _, _ = integ.ctx.last_pass_samples(Ws * Hs, spp)
        got = L[:, 0].reshape(spp, Hs, Ws).mean(axis=0)
        o = (np.arange(32) + 0.5) / 32
        want = np.empty((Hs, Ws))
        for py in range(Hs):
            for px in range(Ws):
                x = (px + o[None, :]) / Ws - 0.5
                y = (py + o[:, None]) / Hs - 0.5
                want[py, px] = np.exp(-2 * np.sqrt(np.maximum(0.0, R * R - x * x - y * y))).mean()
        var = np.sum(want * (1 - want)) / spp
        print(f"fast sphere absorber: frame sum {got.sum():.3f} vs Beer-Lambert {want.sum():.3f} (sd {np.sqrt(var):.3f})")
        assert abs(got.sum() - want.sum()) < 4 * np.sqrt(var)
        assert np.all(got[want == 1.0] == 1.0)   # rays missing the sphere see no medium
    finally:
        integ.close()


# --------------------------------------------------------------------------- device: edge shapes
def _edge_scene(Wf, Hf, density):
    from acceleratedvolrenderer_amd import scenes
    return scenes.s_uniform(n=density.shape[0], width=Wf, height=Hf, variant="scatter", density=density)


def _edge(name):
    """(scene, maxdepth, spp): the inputs of tests/test_gpu_edges.py."""
    films = {"1x1": (1, 1, 1), "ragged7x3": (7, 3, 5), "row65": (65, 1, 3)}
    if name in films:
        Wf, Hf, spp = films[name]
        dens = (0.2 + np.random.default_rng(Wf * 31 + Hf).random((6, 6, 6), dtype=np.float32)).astype(np.float32)
        return _edge_scene(Wf, Hf, dens), 6, spp
    if name.startswith("maxdepth"):
        return _edge_scene(8, 6, np.full((4, 4, 4), 2.0, np.float32)), int(name[len("maxdepth"):]), 4
    if name == "empty":
        dens = np.zeros((5, 5, 5), np.float32)
    elif name == "single_voxel":
        dens = np.full((1, 1, 1), 1.5, np.float32)
    else:
        dens = np.random.default_rng(3).random((8, 8, 8), dtype=np.float32)
        dens[4:] = 0
    return _edge_scene(9, 7, dens), 5, 4


EDGES = ["1x1", "ragged7x3", "row65", "maxdepth0", "maxdepth1", "maxdepth1000", "empty", "single_voxel", "half_empty"]


@functools.lru_cache(maxsize=None)
def _edge_ref(name):
    scene, maxdepth, spp = _edge(name)
    return Ref(scene, maxdepth, 0, spp)


@pytest.mark.parametrize("name", EDGES)
def test_edge_inputs_pass_the_film_cap_by_the_oracle_alone(name):
    """No device: the canonical oracle's film passes the correlated criterion on every edge
    shape whose two-seed noise is non-zero."""
    ref = _edge_ref(name)
    assert np.array_equal(ref.canonical_film["w"], ref.seed0["w"])
    print(f"edge inputs {name}: noise {ref.noise:.3e}")
    if ref.noise > 0:
        _assert_film_correlated(ref, ref.canonical_film, f"edge {name} (canonical oracle)")


@device
@pytest.mark.parametrize("name", EDGES)
def test_fast_edge_shapes(name):
    ref = _edge_ref(name)
    scene, spp = ref.scene, ref.spp
    npix = scene.film.width * scene.film.height
    integ = _integ(scene, ref.maxdepth, spp)
    try:
        film = _device_film(integ, ref, 0, spp)
        assert integ.ctx.last_kernel() == "k_paths<false, true, 0, 0, false, true>"
        lookups = integ.stats()["medium_lookups"]
        _, ns, L, lam, _ = integ.ctx.last_pass_samples(npix, spp)
        assert ns == spp
        assert np.array_equal(film["w"], ref.seed0["w"])
        assert np.all(np.isfinite(L)) and np.all(L >= 0)
        err = _rel_rms(ref.image(film), ref.image(ref.seed0))
        print(f"fast edge {name}: film rel RMS {err:.3e} (MC noise {ref.noise:.3e})")
        if ref.noise > 0:
            _assert_film_correlated(ref, film, f"fast edge {name}")
        if name == "empty":
            # no medium event exists: only lambda's last bits differ from the replay render
            assert lookups == 0
            integ.ctx.set_render_mode("replay")
            integ.render()
            _, _, L_r, _, _ = integ.ctx.last_pass_samples(npix, spp)
            assert float(L_r.min()) > 0
            worst = float(np.max(np.abs(L.astype(np.float64) - L_r) / L_r))
            print(f"fast edge empty: max relative |L - L_replay| {worst:.2e}")
            assert worst <= 1e-5
    finally:
        integ.close()
