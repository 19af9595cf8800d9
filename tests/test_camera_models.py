"""Thin-lens depth of field and SphericalCamera on the CPU (tests/camera_model_cases.py;
tests/test_gpu_camera_models.py holds the device side):

  * csrc/avr_camera.h, host-compiled, against tests/camera_model_ref.py's numpy restatement of
    pbrt's formulas. Per component the header may differ from the float64 restatement by at most
    4 x the largest difference between the float32 and the float64 restatement on the same inputs
    (the formulas' own rounding, measured on the reference's arithmetic; the 4 allows for
    canon::sincos_f against libm). A wrong formula moves a component by 1e-3 or more;
  * direct calls for what a sampler cannot be made to produce: the lens centre, |x| = |y|, the
    square's corners and creases, the poles of the equirectangular map;
  * the equal-area directions equal the oracle's canonical EqualAreaSquareToSphere bit for bit after
    the y/z swap; the truth chain with a pinhole equals the oracle's camera rays bit for bit;
  * host logic: constructors, argument errors of the two ABI calls, entry_cell_order, the bake tool;
  * the conditions on the cases' inputs."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_cases as cc          # noqa: E402
import camera_model_cases as cm    # noqa: E402
import camera_model_ref as ref     # noqa: E402

N = 100000
F32, F64 = np.float32, np.float64


def _bound(a32, a64, what):
    """4 x the largest |float32 - float64| of the restatement."""
    own = float(np.abs(a32.astype(F64) - a64).max())
    print(f"{what}: the restatement's own rounding {own:.3g}, bound {4 * own:.3g}")
    assert 0 < own < 1e-5, (what, own)
    return 4 * own


def _lens_inputs(rng, n):
    u = rng.random((n, 2)).astype(F32)
    radius = rng.uniform(0.01, 0.5, n).astype(F32)
    focal = rng.uniform(0.5, 5.0, n).astype(F32)
    persp = rng.random(n) < 0.5
    d = np.where(persp[:, None], rng.normal(size=(n, 3)) * [0.4, 0.4, 0.05] + [0, 0, 1], [0.0, 0.0, 1.0])
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    o = np.where(persp[:, None], 0.0, rng.uniform(-1, 1, (n, 3)) * [1, 1, 0]).astype(F32)
    return radius, focal, u, o, d


def test_thin_lens_header_against_the_restatement():
    rng = np.random.default_rng(11)
    radius, focal, u, o, d = _lens_inputs(rng, N)
    ho, hd = cm.hdr_lens(radius, focal, u, o, d)
    o32, d32 = ref.thin_lens(radius, focal, u, o, d, F32)
    o64, d64 = ref.thin_lens(radius, focal, u, o, d, F64)
    # origins scale with the lens radius: measured on o / R
    r64 = radius.astype(F64)[:, None]
    bo = _bound(o32 / radius[:, None], o64 / r64, "lens origins / R")
    bd = _bound(d32, d64, "lens directions")
    eo, ed = np.abs(ho.astype(F64) / r64 - o64 / r64).max(), np.abs(hd.astype(F64) - d64).max()
    print(f"header: origins / R {eo:.3g}, directions {ed:.3g}")
    assert eo <= bo and ed <= bd
    assert (ho[:, 2] == 0).all() and np.abs(np.linalg.norm(hd.astype(F64), axis=1) - 1).max() < 1e-6
    # the disc itself, and that the lens is not a no-op (ft = focalDistance / d.z, not focalDistance)
    hx = cm.hdr_disk(u)
    assert np.abs(hx.astype(F64) - ref.concentric_disk(u, F64)).max() <= _bound(
        ref.concentric_disk(u, F32), ref.concentric_disk(u, F64), "concentric disc")
    assert (np.linalg.norm(hx.astype(F64), axis=1) <= 1 + 1e-6).all()
    wrong_ft = np.abs(ref.thin_lens(radius, focal * d[:, 2], u, o, d, F64)[1] - d64).max()
    assert wrong_ft > 1e-3


def test_thin_lens_direct_cases():
    one = np.ones(1, F32)
    # u = (0.5, 0.5): the lens centre exactly, so the pinhole's ray (perspective) / origin 0 (orthographic)
    d = np.array([[0.3, -0.2, 0.9]], F32)
    d /= np.linalg.norm(d)
    ho, hd = cm.hdr_lens(0.3 * one, 2.0 * one, [[0.5, 0.5]], [[0, 0, 0]], d)
    assert (ho == 0).all() and np.abs(hd - d).max() < 2e-7
    assert (cm.hdr_disk([[0.5, 0.5]]) == 0).all()
    # |x| = |y| takes the second branch: theta = pi/2 - pi/4 (x / y)
    u = np.array([[0.75, 0.75], [0.25, 0.75], [0.75, 0.25], [0.25, 0.25], [1.0, 1.0], [0.0, 0.0]], F32)
    got, want = cm.hdr_disk(u), ref.concentric_disk(u, F64)
    assert np.abs(got - want).max() < 2e-7
    r = np.hypot(got[:, 0], got[:, 1])
    assert np.allclose(r, [0.5, 0.5, 0.5, 0.5, 1, 1], atol=2e-7)
    # an axis of the square: x = 0 (second branch, theta = pi/2) and y = 0 (first branch, theta = 0)
    got = cm.hdr_disk([[0.5, 1.0], [1.0, 0.5]])
    assert np.abs(got - [[0, 1], [1, 0]]).max() < 1e-7


def _film_points(rng, n, res):
    """Raster points over and around a film: uv in [-0.45, 1.45]^2, about a quarter of them inside,
    the rest outside on every side and corner (every wrap branch and pairs of them)."""
    pf = rng.uniform(-0.45, 1.45, (n, 2)) * res
    return pf.astype(F32)


@pytest.mark.parametrize("mapping", ["equalarea", "equirectangular"])
def test_spherical_header_against_the_restatement(mapping):
    rng = np.random.default_rng(12)
    res = (cm.W, cm.H)
    pf = _film_points(rng, N, res)
    if mapping == "equalarea":
        br = ref.wrap_branches(pf, res)
        assert br.any(axis=0).all() and (br[:, 0] & br[:, 2]).any(), "a wrap branch is not taken"
    h = cm.hdr_spherical(mapping, pf, res)
    d32, d64 = ref.spherical_dir(mapping, pf, res, F32), ref.spherical_dir(mapping, pf, res, F64)
    b = _bound(d32, d64, mapping)
    err = float(np.abs(h.astype(F64) - d64).max())
    print(f"header {mapping}: {err:.3g}")
    assert err <= b
    assert np.abs(np.linalg.norm(h.astype(F64), axis=1) - 1).max() < 2e-6
    # wrong formulas move a component by far more than the bound: no y/z swap, the other mapping,
    # no wrap
    assert np.abs(d64[:, [0, 2, 1]] - d64).max() > 1e-3
    other = "equirectangular" if mapping == "equalarea" else "equalarea"
    assert np.abs(ref.spherical_dir(other, pf, res, F64) - d64).max() > 1e-3
    if mapping == "equalarea":
        u, v = pf[:, 0].astype(F64) / res[0], pf[:, 1].astype(F64) / res[1]
        nowrap = ref.square_to_sphere(u, v, F64)[:, [0, 2, 1]]
        out = ref.wrap_branches(pf, res).any(axis=1)
        assert np.nanmax(np.abs(nowrap[out] - d64[out])) > 1e-3


def test_spherical_direct_cases():
    res = (8, 8)
    # the square's corners (the -z pole), centre (+z), edge midpoints and the creases |u| + |v| = 1
    pts = np.array([[0, 0], [8, 0], [0, 8], [8, 8], [4, 4], [4, 0], [0, 4], [8, 4], [4, 8], [2, 2], [6, 2], [2, 6],
                    [6, 6], [1, 3], [5, 7]], F32)
    got, want = cm.hdr_spherical("equalarea", pts, res), ref.spherical_dir("equalarea", pts, res, F64)
    assert np.abs(got - want).max() < 5e-7
    assert np.abs(got[:4] - [0, -1, 0]).max() < 1e-7 and np.abs(got[4] - [0, 1, 0]).max() < 1e-7   # y is the pole axis
    assert np.abs(got[9:, 1]).max() < 1e-7          # creases: the equator
    # a point mirrored across an edge of the square is the same direction as its wrap
    a = cm.hdr_spherical("equalarea", [[-1.5, 3.0], [9.5, 3.0], [3.0, -1.5], [3.0, 9.5]], res)
    b = cm.hdr_spherical("equalarea", [[1.5, 5.0], [6.5, 5.0], [5.0, 1.5], [5.0, 6.5]], res)
    assert np.array_equal(a, b)
    # equirectangular: v = 0 and v = 1 are the poles (+y and -y after the swap), whatever u
    pts = np.array([[0, 0], [3, 0], [8, 0], [0, 8], [5, 8], [0, 4], [2, 4], [4, 4]], F32)
    got, want = cm.hdr_spherical("equirectangular", pts, res), ref.spherical_dir("equirectangular", pts, res, F64)
    assert np.abs(got - want).max() < 5e-7
    assert np.abs(got[:3] - [0, 1, 0]).max() < 1e-6 and np.abs(got[3:5] - [0, -1, 0]).max() < 1e-6
    assert np.abs(got[5] - [1, 0, 0]).max() < 1e-6 and np.abs(got[6] - [0, 0, 1]).max() < 1e-6
    assert np.abs(got[7] - [-1, 0, 0]).max() < 1e-6


def test_equal_area_directions_equal_the_oracle_bit_for_bit():
    from oracle import binding
    rng = np.random.default_rng(13)
    uv = np.concatenate([rng.random((3000, 2)), [[0, 0], [1, 1], [0.5, 0.5], [1, 0], [0, 1], [0.25, 0.75]]]).astype(F32)
    # raster points whose pFilm / res is exactly uv's float32 (res * uv need not round-trip: use a film of 1 x 1)
    h = cm.hdr_spherical("equalarea", uv, (1, 1))
    binding.set_libm("canonical")
    L = binding.lib()
    ora = np.zeros((len(uv), 3), F32)
    try:
        for i, (u, v) in enumerate(uv):
            L.oracle_equal_area_square_to_sphere(float(u), float(v), ora[i].ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    finally:
        binding.set_libm("platform")
    assert np.array_equal(h.view(np.uint32), ora[:, [0, 2, 1]].view(np.uint32))


@pytest.mark.parametrize("camera", ["persp-roll", "ortho-oblique", "persp-inside"])
def test_truth_chain_with_a_pinhole_equals_the_oracle(camera):
    """camera_model_cases.chain restates the kernels' pinhole and xf_ray around avr_camera.h: with a
    pinhole it gives the oracle's camera rays bit for bit."""
    from oracle import binding
    scene = cc.scene_for(camera, "box", "independent")
    run = binding.OracleRun(scene, max_depth=cm.MAXDEPTH, seed=0, libm="canonical")
    try:
        pf = (np.random.default_rng(14).random((500, 2)) * [cm.W, cm.H]).astype(F32)
        o, d = run.camera_rays_at(pf)
    finally:
        binding.set_libm("platform")
    co, cd = cm.chain(scene, pf, np.zeros_like(pf))
    assert cc.same_bits(co, o).all() and cc.same_bits(cd, d).all()


# ---------------------------------------------------------------------------
# host logic

def test_constructor_defaults_and_errors():
    from acceleratedvolrenderer_amd import SphericalCamera
    from acceleratedvolrenderer_amd.scene import OrthographicCamera, PerspectiveCamera
    for cam in (PerspectiveCamera(fov=40.0), OrthographicCamera()):
        assert cam.lensradius == 0.0 and cam.focaldistance == 1e6
    cam = PerspectiveCamera(fov=40.0, lensradius=0.05, focaldistance=2.2)
    assert (cam.lensradius, cam.focaldistance, cam.type_id) == (0.05, 2.2, 1)
    for bad in (dict(lensradius=-0.1), dict(lensradius=float("nan")), dict(lensradius=float("inf")),
                dict(lensradius=0.1, focaldistance=0.0), dict(lensradius=0.1, focaldistance=float("nan"))):
        with pytest.raises(ValueError):
            PerspectiveCamera(**bad)
    sph = SphericalCamera()
    assert (sph.type_id, sph.mapping, sph.mapping_id) == (2, "equalarea", 0)
    sph = SphericalCamera(mapping="equirectangular", pos=(0.5, 0.5, -0.2), look=(0.5, 0.5, 0.5), lensradius=0.3,
                          focaldistance=2.0)
    assert (sph.mapping_id, sph.lensradius) == (1, 0.0)      # accepted and ignored, as pbrt's Create
    assert SphericalCamera(lensradius=-1.0, focaldistance=float("nan")).lensradius == 0.0      # ... whatever they are
    with pytest.raises(ValueError, match="mapping"):
        SphericalCamera(mapping="fisheye")
    # a scene takes it like the others
    scene = cm.scene_for("sph-ea-outside")
    assert scene.render_from_camera.shape == (4, 4) and np.isfinite(scene.camera_from_raster).all()


def test_abi_argument_errors_without_a_gpu():
    """Without a device there is no context: only the null-context and null-matrix branches can be
    reached here. The argument matrix of both calls (radius, focal distance, state, a spherical
    camera) is tests/test_gpu_camera_models.py::test_lens_call_errors_on_a_context."""
    from acceleratedvolrenderer_amd import capi
    lib = capi.load()
    eye = np.eye(4, dtype=F32)
    fp = eye.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.avr_camera_lens(None, 0.1, 1.0) != 0
    assert b"context" in lib.avr_last_error()
    assert lib.avr_camera_spherical(None, 0, fp) != 0
    assert b"spherical" in lib.avr_last_error()
    assert lib.avr_camera_spherical(None, 7, None) != 0


@pytest.mark.parametrize("case", ["lens-persp", "lens-ortho", "sph-ea-outside", "sph-er-outside", "sph-ea-inside"])
def test_entry_cell_order_on_the_host(case):
    from acceleratedvolrenderer_amd import integrator
    scene = cm.scene_for(case)
    npix = cm.W * cm.H
    order = integrator.entry_cell_order(scene)
    assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(npix))
    o, d = cm.pixel_centre_rays(scene)
    share = cm.hit_share(scene)
    nhit = int(round(share * npix))
    # the hit mask in scanline order, by camera_cases' float64 slab test on this module's own rays
    mfr = np.asarray(scene.medium_from_render, F64)
    om, dm = o @ mfr[:3, :3].T + mfr[:3, 3], d @ mfr[:3, :3].T
    b = np.asarray(scene.medium.bounds, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (b[:3] - om) / dm, (b[3:] - om) / dm
    hit = np.maximum(np.nanmax(np.minimum(t0, t1), axis=1), 0.0) < np.nanmin(np.maximum(t0, t1), axis=1)
    assert int(hit.sum()) == nhit
    assert hit[order[:nhit]].all() and not hit[order[nhit:]].any()
    if share < 1:
        assert not np.array_equal(order, np.arange(npix))
    if case == "lens-persp":        # the lens centre's ray: the pinhole's order
        assert np.array_equal(order, integrator.entry_cell_order(cm.scene_for(case, cam=cm.make_camera(case, lens=False))))


def test_bake_tool_light_transform_undoes_the_swap():
    """tools/bake_envmap.py: for every pixel centre of an 8 x 8 film the camera's render-space
    direction equals the printed world_from_light applied to the direction env::square_to_sphere
    gives the light for that pixel (three float32 products and two sums per component, |d| <= 1:
    3e-7)."""
    sys.path.insert(0, os.path.join(cm.ROOT, "tools"))
    import bake_envmap
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import RGBFilm, Scene
    cam = bake_envmap.bake_camera((0.2, 0.7, -0.4), (0.9, 0.1, 0.6), (0.2, 1.0, 0.1))
    base = scenes.s_uniform(n=4, width=8, height=8, variant="scatter")
    scene = Scene(cam, RGBFilm(8, 8), base.medium, base.lights)
    y, x = np.mgrid[0:8, 0:8]
    pf = np.stack([x.ravel() + 0.5, y.ravel() + 0.5], 1).astype(F32)
    _, d = cm.chain(scene, pf, np.zeros_like(pf))
    # the light's direction for pixel (x, y): square_to_sphere((x + 0.5) / res, (y + 0.5) / res), the
    # header's own function (a 1 x 1 film hands uv through; swapped back to the light's axes)
    s = cm.hdr_spherical("equalarea", (pf / F32(8)).astype(F32), (1, 1))[:, [0, 2, 1]]
    wfl = bake_envmap.world_from_light(cam)
    assert np.allclose(wfl[:3, :3] @ wfl[:3, :3].T, np.eye(3), atol=1e-12) and not wfl[:3, 3].any()
    err = np.abs(s.astype(F64) @ wfl[:3, :3].T - d).max()
    print(f"bake: camera direction against world_from_light x light direction {err:.3g}")
    assert err < 3e-7
    # and the scene resolves that matrix for an ImageInfiniteLight as its render_from_light
    assert np.abs(wfl[:3, :3] @ bake_envmap.SWAP_YZ[:3, :3] - np.asarray(scene.render_from_camera, F64)[:3, :3]).max() < 1e-7


# ---------------------------------------------------------------------------
# the conditions on the inputs

@pytest.mark.parametrize("case", list(cm.CASES))
def test_case_conditions(case):
    scene = cm.scene_for(case)
    share = cm.hit_share(scene)
    lo, hi = cm.HIT_SHARE[case]
    print(f"{case}: {share:.3f} of the pixel-centre rays cross the box")
    assert lo <= share <= hi
    kind, pose, kw, filt, sphere = cm.CASES[case]
    if case == "lens-inside":       # the lens disc stays inside the box
        pos = np.array(cc.CAMERAS[pose][1]["pos"])
        assert min(pos.min(), (1 - pos).min()) > kw["lensradius"]
    if sphere:                      # the camera, lens included, is outside the interface sphere
        pos = np.array(pose["pos"])
        assert np.linalg.norm(pos - sphere[0]) - kw["lensradius"] > sphere[1]


def test_sphere_case_is_as_well_conditioned_as_its_margin():
    """"lens-sphere-outside": the margin of the device test is 4 x the pinhole's largest distance from
    the float64 first crossing, measured here on the canonical oracle's interface entry, and no lens
    ray of either sampler is nearer the tangent (discriminant over its scale) than the nearest ray
    of that measurement."""
    from oracle import binding
    case, pin_min, lens_min, dev = "lens-sphere-outside", [], [], []
    try:
        for sampler in cm.SAMPLERS:
            scene, o, d, u, w, pf, lens = cm.truth(case, sampler)
            pin = cm.pinhole_scene(case, sampler)
            run = binding.OracleRun(pin, max_depth=cm.MAXDEPTH, seed=0, libm="canonical")
            po, pd, _, _ = cc.oracle_rays(run, cm.W, cm.H, 0, cm.SPP)
            o0, d0 = cm.chain(pin, pf, lens)                       # the pinhole's rays before the entry
            assert cc.same_bits(pd, d0).all()
            hit, p, rel = cm.sphere_crossing(pin, o0, d0)
            assert hit.mean() > 0.2 and cc.same_bits(po[~hit], o0[~hit]).all()
            dev.append(float(np.abs(po.astype(F64) - p)[hit].max()))
            pin_min.append(float(np.abs(rel).min()))
            lhit, _, lrel = cm.sphere_crossing(scene, o, d)
            assert lhit.mean() > 0.2
            lens_min.append(float(np.abs(lrel).min()))
            print(f"{case}/{sampler}: pinhole deviation {dev[-1]:.3g}, nearest the tangent: pinhole "
                  f"{pin_min[-1]:.3g}, lens {lens_min[-1]:.3g}")
    finally:
        binding.set_libm("platform")
    assert abs(max(dev) - cm.SPHERE_PINHOLE_DEVIATION) < 1e-8
    assert min(lens_min) >= min(pin_min)


def test_float64_shares_of_the_outside_pose():
    assert round(cm.hit_share(cm.scene_for("sph-ea-outside")), 3) == 0.342
    assert round(cm.hit_share(cm.scene_for("sph-er-outside")), 3) == 0.267


@pytest.mark.parametrize("sampler", cm.SAMPLERS)
def test_wide_filter_takes_every_wrap_branch(sampler):
    """"sph-ea-wide": through gauss-64 (radius 2) film points leave [0, res] on all four sides, and
    every one of WrapEqualAreaSquare's four branches is taken by at least one sample."""
    scene, o, d, u, w, pf, lens = cm.truth("sph-ea-wide", sampler)
    br = ref.wrap_branches(pf, (cm.W, cm.H))
    print(f"sph-ea-wide/{sampler}: samples per wrap branch {br.sum(axis=0).tolist()}")
    assert (br.sum(axis=0) >= 1).all()
    assert np.isfinite(d).all() and np.abs(np.linalg.norm(d.astype(F64), axis=1) - 1).max() < 2e-6
