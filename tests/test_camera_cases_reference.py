"""CPU checks of tests/camera_cases.py: scene.py's camera matrices and the oracle's ray code against
the reference's own transforms, the oracle's Gaussian filter sampling against the reference's at
the new radii, the conditions that make the device tests mean something, and how little of a camera
ray the per-sample replay sees.

Why avr_last_pass_rays exists. The suite's per-sample comparison looks at (L, lambda, filter
weight). Measured here (test_replay_sees_little_of_the_ray; 20 x 12, 4 samples, maxdepth 6) with
ONE float32 entry of a camera matrix moved by one ulp, the oracle against itself:

  camera        entry nudged               rays bit-identical   (L, lambda, weight) bit-identical
  persp-roll    render_from_camera[2][2]        13.3 %                 92.4 %   (lit samples: 92.1 %)
  ortho-back    render_from_camera[2][2]         0.0 %                 97.6 %   (lit samples: 97.3 %)
  persp-inside  render_from_camera[2][2]        27.9 %                 78.9 %   (lit samples: 75.1 %)
  persp-roll    camera_from_raster[1][1]        55.9 %                 96.5 %   (lit samples: 96.4 %)
  ortho-back    camera_from_raster[1][1]        22.9 %                 86.9 %   (lit samples: 85.0 %)
  persp-inside  camera_from_raster[1][1]        30.2 %                 77.0 %   (lit samples: 73.0 %)

Most samples return the same radiance whichever of two neighbouring rays they follow (rays that
miss the box, paths whose first collision falls in the same voxel neighbourhood round the same
way), so a rounding difference in the camera stage that touches few rays stays below what
(L, lambda, weight) can show. The ray itself shows it: the device tests compare o, d and the first
free-flight draw bit for bit."""
import ctypes
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_cases as cc   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


@pytest.fixture(autouse=True)
def _platform_libm_afterwards():
    """The oracle's libm mode is process-wide and the canonical runs here set it: hand the process
    back in the platform mode that tests calling the library directly expect."""
    yield
    from oracle import binding
    binding.set_libm("platform")


# ---------------------------------------------------------------------------
# conditions on the inputs

@pytest.mark.parametrize("camera", list(cc.CAMERAS))
def test_hit_shares(camera):
    scene = cc.scene_for(camera)
    share = float(cc.hit_mask(scene).mean())
    lo, hi = cc.HIT_SHARE[camera]
    print(f"{camera}: {share:.3f} of the pixel-centre rays cross the box")
    assert lo <= share <= hi


def test_cameras_are_what_they_claim():
    """Direction signs, roll, mirror, the portrait film and the frame < 1 branch."""
    d = cc.pixel_centre_rays(cc.scene_for("persp-roll"))[1]
    assert (d < 0).all()
    rfc = np.asarray(cc.scene_for("persp-roll").render_from_camera, np.float64)
    assert np.abs(rfc[:3, :3]).min() > 0.01              # rolled: no entry of the rotation is zero
    m = np.asarray(cc.scene_for("persp-mirrored").render_from_camera, np.float64)[:3, :3]
    assert abs(np.linalg.det(m) + 1) < 1e-6 and abs(np.linalg.det(rfc[:3, :3]) - 1) < 1e-6
    assert np.allclose(np.linalg.norm(cc.pixel_centre_rays(cc.scene_for("persp-mirrored"))[1], axis=1), 1, atol=1e-6)
    d = cc.pixel_centre_rays(cc.scene_for("persp-inside"))[1]
    assert all((d[:, k] < 0).any() and (d[:, k] > 0).any() for k in range(3))
    pos = np.array(cc.CAMERAS["persp-inside"][1]["pos"])
    assert np.all((pos > 0) & (pos < 1))
    c, r = cc.CAMERAS["persp-inside-sphere"][1]["sphere"]
    assert np.linalg.norm(pos - np.array(c)) < r
    d = cc.pixel_centre_rays(cc.scene_for("ortho-oblique"))[1]
    assert np.abs(d).min() > 0.5 and np.ptp(d, axis=0).max() < 1e-6
    d = cc.pixel_centre_rays(cc.scene_for("ortho-back"))[1]
    assert np.array_equal(np.abs(d), np.tile([0.0, 0.0, 1.0], (len(d), 1))) and (d[:, 2] == -1).all()
    assert cc.film_size("portrait") == (12, 20)
    for name in ("portrait", "persp-frame"):     # frame < 1: the window's x is +-1
        cam = cc.make_camera(name)
        assert cam._screen(*cc.film_size(name))[:2] == [-1.0, 1.0]
    assert cc.make_camera("persp-roll")._screen(cc.W, cc.H)[2:] == [-1.0, 1.0]
    sw = cc.CAMERAS["persp-shifted"][1]["screenwindow"]
    assert sw[0] + sw[1] != 0 and sw[2] + sw[3] != 0


def test_interface_sphere_leaves_inside_origins_alone():
    """"persp-inside-sphere": the camera sits inside the interface sphere, so interface_entry
    returns every origin as it is, while the sphere is the active boundary."""
    from oracle import binding
    scene = cc.scene_for("persp-inside-sphere")
    run = binding.OracleRun(scene, max_depth=cc.MAXDEPTH, seed=0, libm="canonical")
    assert run.s.boundary == 1
    w, h = cc.film_size("persp-inside-sphere")
    moved = 0
    for pix in range(w * h):
        for s in range(2):
            o, d, u, pf, wt = run.camera_ray(pix % w, pix // w, s)
            o0, d0 = run.camera_rays_at(pf)
            moved += not (cc.same_bits(o[None], o0).all() and cc.same_bits(d[None], d0).all())
    assert moved == 0
    # and the sphere cuts paths short: without it the same camera returns other radiance
    free = binding.OracleRun(cc.scene_for("persp-inside"), max_depth=cc.MAXDEPTH, seed=0, libm="canonical")
    differ = sum(not np.array_equal(run.pixel_sample(p % w, p // w, 0)[0], free.pixel_sample(p % w, p // w, 0)[0])
                 for p in range(w * h))
    assert differ > w * h // 4


def test_needle_table_has_zero_rows():
    """"gauss-needle": FastExp underflows beyond |x| = 0.66, so whole rows (and columns) of f are
    zero and their conditional CDFs fall back to uniform; the rows through the middle are not."""
    t = cc.gaussian_table("gauss-needle")
    zero = (t == 0).all(axis=1)
    print(f"gauss-needle: {int(zero.sum())} of {len(zero)} rows all zero")
    assert zero.any() and not zero.all()
    assert int(zero.sum()) == 26
    # no other Gaussian filter of the module has such rows
    for name in cc.FILTER_TABLES:
        if name != "gauss-needle":
            assert not (cc.gaussian_table(name) == 0).all(axis=1).any(), name


def test_filter_table_sizes_and_branches(tmp_path):
    """The table sizes the cases are chosen for, from smp::filter_blob_floats of the header itself,
    against the camera stage's LDS limit: which filters take the global-memory branch."""
    src = tmp_path / "shim.cpp"
    src.write_text("#define AVR_HD inline\n"
                   f'#include "{ROOT}/acceleratedvolrenderer_amd/csrc/avr_sampling.h"\n'
                   'extern "C" int blob(int nx, int ny) { return avr::smp::filter_blob_floats(nx, ny); }\n'
                   'extern "C" int guide_k() { return avr::smp::kFilterGuideK; }\n')
    so = tmp_path / "shim.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    assert L.guide_k() == cc.filter_guide_k()
    limit = cc.filter_lds_limit()
    assert 48 * 48 + 1 <= limit            # the default filter (1.5, 1.5) is staged
    for name, (nx, ny, floats, staged) in cc.FILTER_TABLES.items():
        assert cc.filter_table_size(name) == (nx, ny)
        behind_f = L.blob(nx, ny) - nx * ny
        assert behind_f == cc.filter_blob_floats(nx, ny) - nx * ny
        print(f"{name}: {nx} x {ny}, {behind_f} floats behind f (LDS limit {limit}): {cc.filter_branch(name)}")
        if floats is not None:
            assert behind_f == floats
        assert cc.filter_staged(name) == staged, (
            f"{name}: kFiltLds = {limit} no longer puts this filter's tables in "
            f"{'LDS' if staged else 'global memory'}; the branch it was chosen for is not covered")
    assert L.blob(48, 48) - 48 * 48 == 6335
    assert sum(1 for v in cc.FILTER_TABLES.values() if not v[3]) >= 4 and any(v[3] for v in cc.FILTER_TABLES.values())


# ---------------------------------------------------------------------------
# rays against the reference's own transforms

@pytest.fixture(scope="module")
def ray_golden():
    with open(os.path.join(GOLDEN, "camera_ray_vectors.json")) as fh:
        cases = json.load(fh)["cases"]
    return {c["name"]: c for c in cases}


def test_golden_cameras_are_the_module_s(ray_golden):
    lines = cc.harness_camera_lines().splitlines()
    assert [c["line"] for c in ray_golden.values()] == lines
    assert list(ray_golden) == list(cc.CAMERAS)


RAY_TOL = 2e-5      # rad and length units: about 300 float epsilons against ~30 float operations


def _ray_deviation(scene, case):
    """(angle between directions, distance between origins) per golden ray: scene.py's float32
    matrices through the oracle's ray code against the reference's rays."""
    from oracle import binding
    rows = np.array(case["rays"], np.uint32).view(np.float32)
    run = binding.OracleRun(scene, max_depth=cc.MAXDEPTH, seed=0, libm="canonical")
    o, d = run.camera_rays_at(rows[:, :2])
    o, d = o.astype(np.float64), d.astype(np.float64)
    ro, rd = rows[:, 2:5].astype(np.float64), rows[:, 5:8].astype(np.float64)
    assert np.allclose(np.linalg.norm(rd, axis=1), 1, atol=1e-5)
    # atan2 of |a x b| and a . b: exact for small angles, where arccos of the dot product is not
    ang = np.arctan2(np.linalg.norm(np.cross(d, rd), axis=1), np.einsum("ij,ij->i", d, rd))
    return ang, np.linalg.norm(o - ro, axis=1)


def _check_rays(scene, case, label):
    ang, dist = _ray_deviation(scene, case)
    print(f"{label}: max angle {ang.max():.2e} rad, max origin distance {dist.max():.2e} over {len(ang)} rays")
    assert ang.max() <= RAY_TOL and dist.max() <= RAY_TOL
    return ang, dist


def _wrong_camera(camera, how):
    """The camera of a case with one formula wrong: "flip_y" maps raster y upwards over the screen
    window, "fov_long_axis" gives the fov to the film's longer axis, "no_roll" looks with up = +y."""
    from acceleratedvolrenderer_amd import transform as xf
    if how == "no_roll":
        return cc.make_camera(camera, up=(0.0, 1.0, 0.0))
    cam = cc.make_camera(camera)
    if how == "flip_y":
        def camera_from_raster(self, xres, yres):
            x0, x1, y0, y1 = self._screen(xres, yres)
            ndc_from_screen = xf.scale(1 / (x1 - x0), 1 / (y1 - y0), 1) @ xf.translate([-x0, -y0, 0])
            screen_from_raster = np.linalg.inv(xf.scale(xres, yres, 1) @ ndc_from_screen)
            return np.linalg.inv(self.screen_from_camera()) @ screen_from_raster
        cam.camera_from_raster = types.MethodType(camera_from_raster, cam)
    elif how == "fov_long_axis":
        def _screen(self, xres, yres):
            frame = self.frameaspectratio if self.frameaspectratio is not None else xres / yres
            return [-1.0, 1.0, -1.0 / frame, 1.0 / frame] if frame > 1 else [-frame, frame, -1.0, 1.0]
        cam._screen = types.MethodType(_screen, cam)
    else:
        raise ValueError(how)
    return cam


def _wrong_formulas(camera):
    """The wrong formulas that change a camera: the fov's axis matters to a perspective camera
    without a screen window, the roll to a camera whose up is not +y."""
    kind, kw = cc.CAMERAS[camera]
    out = ["flip_y"]
    if kind == "perspective" and "screenwindow" not in kw:
        out.append("fov_long_axis")
    if tuple(kw["up"]) != (0.0, 1.0, 0.0):
        out.append("no_roll")
    return out


def test_every_wrong_formula_is_tried():
    tried = {how for c in cc.CAMERAS for how in _wrong_formulas(c)}
    assert tried == {"flip_y", "fov_long_axis", "no_roll"}
    assert "no_roll" in _wrong_formulas("persp-roll") and "no_roll" in _wrong_formulas("ortho-oblique")
    assert "fov_long_axis" in _wrong_formulas("portrait") and "fov_long_axis" in _wrong_formulas("persp-frame")


@pytest.mark.parametrize("camera", list(cc.CAMERAS))
def test_rays_match_the_reference(camera, ray_golden):
    """scene.py's camera_from_raster and render_from_camera, handed as float32 to the oracle's
    GenerateRay, against rays the reference's LookAt / Perspective / Orthographic / Inverse give at
    the film's corners, its centre and 16 raster points; and the same check fails, with a corner ray
    off by more than 1e-2, for each wrong formula that applies to the camera."""
    case = ray_golden[camera]
    assert (case["width"], case["height"]) == cc.film_size(camera)
    assert len(case["rays"]) == 21
    _check_rays(cc.scene_for(camera), case, camera)
    for how in _wrong_formulas(camera):
        wrong = cc.scene_for(camera, cam=_wrong_camera(camera, how))
        ang, dist = _ray_deviation(wrong, case)
        worst = max(ang[:4].max(), dist[:4].max())
        print(f"{camera} with {how}: a corner ray moves by {worst:.3f}")
        assert worst > 1e-2
        with pytest.raises(AssertionError):
            _check_rays(wrong, case, f"{camera} with {how}")


# ---------------------------------------------------------------------------
# GaussianFilter::Sample at the new radii

def test_gaussian_filter_sampling_at_the_new_radii():
    """oracle_gaussian_filter_sample against the reference's GaussianFilter::Sample, position and
    weight bit for bit, for every Gaussian filter of the module: u = (0, 0), (1 - 2^-24, 1 - 2^-24),
    (0.5, 0.5) and 93 random points each."""
    from oracle import binding as ob
    with open(os.path.join(GOLDEN, "gaussian_filter_vectors.json")) as fh:
        golden = json.load(fh)["gaussian_filter"]
    want = sorted((np.float32(r[0]), np.float32(r[1]), np.float32(s)) for k, r, s in cc.FILTERS.values()
                  if k == "gaussian")
    have = sorted(tuple(f32([c[k]])[0] for k in ("rx", "ry", "sigma")) for c in golden)
    assert have == want
    for c in golden:
        rx, ry, sigma = (float(f32([c[k]])[0]) for k in ("rx", "ry", "sigma"))
        rows = np.array(c["samples"], np.uint32)
        u = rows[:, :2].view(np.float32)
        assert u[0].tolist() == [0.0, 0.0] and u[2].tolist() == [0.5, 0.5]
        assert (u[1] == np.float32(0.99999994)).all()
        got = ob.gaussian_filter_samples(rx, ry, sigma, u)
        assert not np.isnan(got).any()
        assert got.view(np.uint32).tolist() == rows[:, 2:].tolist(), (rx, ry, sigma)


@pytest.mark.parametrize("filt", [f for f in cc.FILTERS if f != "box"])
def test_oracle_runs_every_filter_without_nan_weights(filt):
    from oracle import binding
    scene = cc.scene_for("persp-roll", filt)
    run = binding.OracleRun(scene, max_depth=cc.MAXDEPTH, seed=0, libm="canonical")
    w = np.array([run.camera_ray(p % cc.W, p // cc.W, s)[4] for p in range(cc.W * cc.H) for s in range(2)])
    print(f"{filt}: filter weights {w.min():.5f} .. {w.max():.5f}")
    assert np.isfinite(w).all()
    if cc.FILTERS[filt][0] == "box":
        assert (w == 1).all()


# ---------------------------------------------------------------------------
# what the per-sample replay sees of the ray

def _nudged_runs(camera, matrix, entry):
    """The oracle of a camera (4 samples per pixel) and the same with one float32 matrix entry one
    ulp up."""
    from oracle import binding
    scene = cc.scene_for(camera, spp=4)
    base = binding.OracleRun(scene, max_depth=cc.MAXDEPTH, seed=0, libm="canonical")
    m = getattr(scene, matrix)
    assert m.dtype == np.float32 and m[entry] != 0
    m[entry] = np.nextafter(m[entry], np.float32(np.inf))
    return base, binding.OracleRun(scene, max_depth=cc.MAXDEPTH, seed=0, libm="canonical")


def _nudge_entry(camera, matrix):
    """render_from_camera: the entry with the largest magnitude in column 2, which the camera-space z of
    the direction multiplies. An orthographic direction IS that column, so every ray changes; a
    perspective direction has z >= cos(fov / 2 diagonal) > 0.5 in camera space, so the product moves by
    more than half an ulp of the entry, and the component it is summed into is no larger than the entry's
    binade allows (|d_i| <= 1): the sum rounds differently for most rays. camera_from_raster: [1][1], the
    entry the issue measured (recorded only)."""
    if matrix == "camera_from_raster":
        return (1, 1)
    m = np.asarray(cc.scene_for(camera).render_from_camera)
    return (int(np.argmax(np.abs(m[:3, 2]))), 2)


@pytest.mark.parametrize("matrix", ["render_from_camera", "camera_from_raster"])
@pytest.mark.parametrize("camera", cc.SENSITIVITY)
def test_replay_sees_little_of_the_ray(camera, matrix):
    """One ulp on one entry of a camera matrix (_nudge_entry): through camera_ray more than half of
    the rays change (render_from_camera); through (L, lambda, weight) most samples stay bit-identical
    (recorded, no bound: the module docstring and DESIGN.md hold the figures)."""
    entry = _nudge_entry(camera, matrix)
    a, b = _nudged_runs(camera, matrix, entry)
    w, h = cc.film_size(camera)
    ray_same, rec_same, lit = [], [], []
    for s in range(4):
        for pix in range(w * h):
            px, py = pix % w, pix // w
            ra, rb = a.camera_ray(px, py, s), b.camera_ray(px, py, s)
            ray_same.append(cc.same_bits(ra[0][None], rb[0][None]).all() and cc.same_bits(ra[1][None], rb[1][None]).all())
            sa, sb = a.pixel_sample(px, py, s, with_weight=True), b.pixel_sample(px, py, s, with_weight=True)
            rec_same.append(all(cc.same_bits(np.atleast_1d(x)[None], np.atleast_1d(y)[None]).all()
                                for x, y in ((sa[0], sb[0]), (sa[1], sb[1]), (sa[4], sb[4]))))
            lit.append(bool((sa[0] > 0).any()))
    ray_same, rec_same, lit = np.array(ray_same), np.array(rec_same), np.array(lit)
    print(f"{camera}, {matrix}[{entry[0]}][{entry[1]}] + 1 ulp: rays bit-identical {ray_same.mean():.3f}, "
          f"(L, lambda, weight) bit-identical {rec_same.mean():.3f}, among the {int(lit.sum())} lit samples "
          f"{rec_same[lit].mean():.3f}")
    if matrix == "render_from_camera":
        assert ray_same.mean() < 0.5
    assert ray_same.mean() < 1.0
    assert lit.sum() > 100
