"""PointLight, SpotLight and pbrt's whole BVHLightSampler on the CPU (tests/local_light_cases.py;
tests/test_gpu_local_lights.py holds the device side). The oracle knows no local lights, so
csrc/avr_local_light.h, host-compiled, is held against tests/local_light_ref.py, an independent
numpy restatement of the reference's text:

  * SampleLi of both lights under every transform of light_cases.TRANSFORMS at points inside,
    outside, on the cone's edges, on the axis, at the light and 1e-6 / 1e6 from it: wi, the
    distance (relative) and Li (relative to scale I / r^2, so that the cone's edge, where Li -> 0,
    is measured on the falloff) within 4 x the restatement's own float32 rounding, measured against
    its float64 evaluation. Measured: the restatement's own rounding is at most 1.1e-7 (wi), 1.5e-7
    (distance) and 1.1e-6 (Li: the spot light's falloff near the cone's edge); the header reproduces the
    float32 restatement to the last bit at every probe, so the margin of 4 of
    test_camera_models.py is kept. (A cone with conedeltaangle 0 is a step: the probes on its
    edge are compared with the float32 restatement alone, bit for bit);
  * the light BVH of lists of 1, 2, 3 and 8 lights equals the restatement's in topology, leaf
    indices, quantised boxes and cosines (exactly), directions and phi (within rounding);
  * BVHLightSampler::Sample over a lattice through and around the box with light_cases.PICK_U:
    index and "no light" equal outside 1e-5 of a bin edge (float64 restatement; at most 2 % of a
    case's draws), the pmf within 4 x the restatement's own rounding;
  * Create's scales, power= and cosines; the spot light aimed away has importance 0 over the box;
  * every mutation of the restatement misses: no 1/r^2, the transforms swapped, unquantised bounds
    in Importance, pInfinite without the + 1;
  * argument errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import light_cases as lc            # noqa: E402
import local_light_cases as ll      # noqa: E402
import local_light_ref as ref       # noqa: E402

F32, F64 = np.float32, np.float64
SAMPLE_LIGHTS = ("p-inside", "p-far", "s-in", "s-wide", "s-sharp")


def _kind(light):
    return "spot" if light.type_id == 4 else "point"


def _sample_errors(scene, mut=None):
    """(errors of the header, the float32 restatement's own rounding) for light 0 of a scene, each as
    (wi absolute, distance relative, Li relative to scale I / r^2), over the finite probes."""
    light = scene.lights[0]
    p = ll.probe_points(scene, 0)
    lam = lc.probe_lambdas(len(p))
    wi, Li, dist, I4 = ll.hdr_sample(scene, 0, p, lam)
    args = (_kind(light), scene.light_rfl[0], scene.light_lfr[0], light.cos_falloff_start, light.cos_falloff_end, light.scale,
            I4, p)
    w32, L32, d32 = ref.sample_li(*args, T=F32)
    w64, L64, d64 = ref.sample_li(*args, T=F64)
    ok = np.isfinite(w64).all(axis=1) & np.isfinite(L64).all(axis=1) & (d64 > 0)
    # at the light itself 0 / 0: neither side has a finite answer
    assert (~np.isfinite(wi[~ok])).any(axis=1).all() if (~ok).any() else True
    assert (~ok).sum() <= 2 and ok.sum() > 60
    if light.type_id == 4 and light.cos_falloff_start == light.cos_falloff_end:
        # SmoothStep's a == b branch is a step: a probe that float64 puts within 1e-6 of it may fall
        # on either side in float32. There the header must equal the float32 restatement itself.
        m = np.asarray(scene.light_lfr[0], F64)[:3, :3]
        wl = (-w64) @ m.T
        edge = np.abs(wl[:, 2] / np.linalg.norm(wl, axis=1) - F64(light.cos_falloff_end)) < 1e-6
        assert (edge & ok).sum() <= 4
        assert np.array_equal(Li[edge & ok], L32[edge & ok])
        ok &= ~edge
    with np.errstate(all="ignore"):
        base = np.abs(F64(light.scale) * I4.astype(F64) / (d64 * d64)[:, None])

    def errs(w, L, d, want):
        ww, wl, wd = want
        return (np.abs(w[ok].astype(F64) - ww[ok]).max(), np.abs(d[ok].astype(F64) / wd[ok] - 1).max(),
                np.nanmax(np.abs((L[ok].astype(F64) - wl[ok]) / base[ok])))
    # (a mutation replaces what the header is held against; the own rounding stays the clean one)
    want = (w64, L64, d64) if mut is None else ref.sample_li(*args, T=F64, mut=mut)
    return errs(wi, Li, dist, want), errs(w32, L32, d32, (w64, L64, d64)), (wi, Li, dist, ok)


@pytest.mark.parametrize("xform", lc.TRANSFORMS)
@pytest.mark.parametrize("name", SAMPLE_LIGHTS)
def test_sample_li_header_against_the_restatement(name, xform):
    scene = ll.scene_of([(name, xform)])
    got, own, (wi, Li, dist, ok) = _sample_errors(scene)
    print(f"{name}/{xform}: header wi {got[0]:.3g} dist {got[1]:.3g} Li {got[2]:.3g}; the restatement's own rounding "
          f"wi {own[0]:.3g} dist {own[1]:.3g} Li {own[2]:.3g}")
    for g, o in zip(got, own):
        assert 0 < o < 1e-5
        assert g <= 4 * o
    assert np.abs(np.linalg.norm(wi[ok].astype(F64), axis=1) - 1).max() < 1e-6
    if scene.lights[0].type_id == 4:      # probes on both sides of the cone: some lit, some not
        lit = Li[ok].any(axis=1)
        assert lit.any() and (~lit).any()
    else:
        assert Li[ok].all()


@pytest.mark.parametrize("mut,name", [("no-r2", "p-inside"), ("no-r2", "s-in"), ("swapped", "s-in"), ("swapped", "s-wide")])
def test_a_wrong_sample_li_shows(mut, name):
    """The restatement with the 1 / r^2 dropped, or renderFromLight and lightFromRender swapped,
    is outside the header's bound (under a rotation, so that the two transforms differ)."""
    scene = ll.scene_of([(name, "rot-axis")])
    got, own, _ = _sample_errors(scene, mut=mut)
    print(f"{mut}/{name}: header vs the mutated restatement wi {got[0]:.3g} dist {got[1]:.3g} Li {got[2]:.3g}")
    assert max(g / o for g, o in zip(got, own)) > 1e3


# ---------------------------------------------------------------------------
# the tree

def _assert_same_tree(got, tree, label):
    assert len(got["leaf"]) == len(tree.nodes), label
    assert got["n_infinite"] == len(tree.infinite), label
    if tree.nodes:
        assert np.array_equal(got["all_bounds"], np.concatenate([tree.all_lo, tree.all_hi])), label
    for i, node in enumerate(tree.nodes):
        assert bool(got["leaf"][i]) == node["leaf"], (label, i)
        assert int(got["link"][i]) == node["link"], (label, i)
        assert np.array_equal(got["qb"][i], node["qb"]), (label, i, got["qb"][i], node["qb"])
        assert tuple(int(v) for v in got["qcos"][i]) == tuple(node["qcos"]), (label, i)
        w = ref._oct_decode(node["w"][0], node["w"][1], F32)
        assert np.abs(got["w"][i] - w).max() < 1e-6, (label, i, got["w"][i], w)
        assert abs(float(got["phi"][i]) - float(node["phi"])) <= 4e-7 * float(node["phi"]), (label, i)


@pytest.mark.parametrize("case", list(ll.BVH))
def test_bvh_equals_the_restatement(case):
    scene = ll.scene_of(ll.BVH[case])
    tree, bounds = ll.ref_tree(scene)
    got = ll.hdr_build(scene)
    live = sum(1 for b in bounds if b is not None and b.phi > 0)
    print(f"{case}: {len(tree.nodes)} nodes over {live} lights with power, {len(tree.infinite)} infinite")
    assert len(tree.nodes) == (2 * live - 1 if live else 0)
    _assert_same_tree(got, tree, case)
    leaves = sorted(n["link"] for n in tree.nodes if n["leaf"])
    assert leaves == [i for i, b in enumerate(bounds) if b is not None and b.phi > 0]


def test_the_cases_cover_the_build():
    """Sizes 1, 2, 3 and 8; a split by cost (two populated dimensions) and the mid fallback
    (collinear: every bucket box has no area); degenerate and zero-phi lists."""
    sizes = {len(v) for v in ll.BVH.values()}
    assert {1, 2, 3, 8} <= sizes
    line, _ = ll.ref_tree(ll.scene_of(ll.BVH["eight-collinear"]))
    # the fallback halves the list: a balanced tree, root's second child after 7 nodes
    assert line.nodes[0]["link"] == 8 and [n["link"] for n in line.nodes if n["leaf"]] == list(range(8))
    spread, _ = ll.ref_tree(ll.scene_of(ll.BVH["eight-spread"]))
    assert [n["link"] for n in spread.nodes if n["leaf"]] != list(range(8)), "no cost split reorders the lights"
    none, _ = ll.ref_tree(ll.scene_of(ll.BVH["three-all-zero"]))
    assert none.nodes == [] and none.infinite == []


# ---------------------------------------------------------------------------
# picks

def _pick_report(scene, mut=None):
    tree, _ = ll.ref_tree(scene)
    p, u = ll.pick_inputs()
    hi, hp = ll.hdr_pick(scene, p, u)
    i32, p32, _ = ref.bvh_sample(tree, p, u, F32)
    i64, p64, margin = ref.bvh_sample(tree, p, u, F64, mut=mut)
    near = margin < 1e-5
    # a lattice point on a light: 0 / 0 in Importance, and the pmf is NaN on every side
    assert np.array_equal(np.isnan(hp), np.isnan(p32))
    fin = np.isfinite(p64) & np.isfinite(p32) & (p64 > 0)
    with np.errstate(all="ignore"):
        same = (i64 == i32) & (i64 >= 0) & ~near & fin
        own = float(np.abs(p32[same].astype(F64) / p64[same] - 1).max()) if same.any() else 0.0
        cmp = (hi == i64) & (i64 >= 0) & ~near & fin
        err = float(np.abs(hp[cmp].astype(F64) / p64[cmp] - 1).max()) if cmp.any() else 0.0
    wrong = float(((hi != i64) & ~near).mean())
    return dict(excluded=float(near.mean()), own=own, err=err, wrong=wrong, none=float((i64 < 0).mean()), hi=hi, hp=hp)


@pytest.mark.parametrize("case", list(ll.BVH))
def test_picks_equal_the_restatement(case):
    scene = ll.scene_of(ll.BVH[case])
    r = _pick_report(scene)
    print(f"{case}: excluded near a bin edge {r['excluded']:.4f}, no light {r['none']:.3f}, index mismatches "
          f"{r['wrong']:.5f}, pmf error {r['err']:.3g} (the restatement's own rounding {r['own']:.3g})")
    assert r["excluded"] <= 0.02
    assert r["wrong"] == 0.0
    assert r["err"] <= 4 * max(r["own"], 2.0 ** -24)
    assert (r["hp"][r["hi"] < 0] == 0).all()
    tree, _ = ll.ref_tree(scene)
    assert ll.hdr_pmf_infinite(scene) == ref.pmf_infinite(tree)


@pytest.mark.parametrize("mut,case", [("unquantised", "eight-collinear"), ("unquantised", "point+spot"),
                                      ("no-plus-one", "infinite+locals")])
def test_a_wrong_pick_shows(mut, case):
    scene = ll.scene_of(ll.BVH[case])
    good, bad = _pick_report(scene), _pick_report(scene, mut=mut)
    print(f"{mut}/{case}: index mismatches {bad['wrong']:.4f}, pmf error {bad['err']:.3g} (own {good['own']:.3g})")
    # it misses the pick test's own assertions, and by a wide margin
    assert bad["wrong"] > 0.001 or bad["err"] > 10 * 4 * max(good["own"], 2.0 ** -24)
    if mut == "no-plus-one":
        tree, _ = ll.ref_tree(scene)
        assert ll.hdr_pmf_infinite(scene) != ref.pmf_infinite(tree, mut=mut)


def test_the_spot_light_aimed_away_has_no_importance_in_the_box():
    """The anchor case is what it claims: [X, s-away] has a root leaf whose importance is 0 at every
    lattice point of the box, faces and corners included (the restatement alone)."""
    scene = ll.scene_of(["distant-base", "s-away"])
    tree, _ = ll.ref_tree(scene)
    assert len(tree.nodes) == 1 and tree.nodes[0]["leaf"] and tree.infinite == [0]
    for T in (F32, F64):
        imp = ref.importance(tree.nodes[0], tree.all_lo, tree.all_hi, ll.box_lattice(7), T)
        assert (imp == 0).all()
    idx, pmf, _ = ref.bvh_sample(tree, np.repeat(ll.box_lattice(3), len(lc.PICK_U), 0), np.tile(lc.PICK_U, 27), F32)
    assert set(np.unique(idx)) == {-1, 0} and (pmf[idx == 0] == F32(0.5)).all()
    assert ref.pmf_infinite(tree) == F32(0.5)
    # and it does light something elsewhere: behind the camera plane
    assert ref.importance(tree.nodes[0], tree.all_lo, tree.all_hi, np.array([[0.0, 0.0, -1.5]], F32), F32)[0] > 0


# ---------------------------------------------------------------------------
# Create

@pytest.mark.parametrize("L", [None, ("blackbody", 3200.0), 0.7])
def test_create_scales(L):
    from acceleratedvolrenderer_amd import spectra
    from acceleratedvolrenderer_amd.scene import PointLight, SpotLight
    kw = {} if L is None else dict(I=lc._spectrum(L))
    table = spectra.TABLES["D65"] if L is None else spectra.as_table(lc._spectrum(L), 1.0)
    phot = spectra.spectrum_to_photometric(table)
    for power in (None, -1.0, 40.0):
        assert PointLight(scale=1.5, power=power, **kw).scale == ref.point_scale(1.5, phot, power)
        s = SpotLight(scale=1.5, power=power, coneangle=35.0, conedeltaangle=10.0, **kw)
        assert s.scale == ref.spot_scale(1.5, phot, 35.0, 10.0, power)
        cs, ce = ref.spot_cosines(35.0, 10.0)
        assert (s.cos_falloff_start, s.cos_falloff_end) == (cs, ce)
    # power is not a no-op, and the two lights normalise differently
    assert PointLight(power=40.0, **kw).scale != PointLight(**kw).scale
    assert abs(float(PointLight(power=4 * np.pi, **kw).scale) * float(phot) - 1) < 1e-6


def test_transforms_follow_create():
    """renderFromLight: Translate(from) for the point light; for the spot light +z maps onto
    Normalize(to - from), through an orthonormal frame."""
    sc = ll.scene_of(["p-inside", "s-wide"])
    assert np.allclose(sc.light_rfl[0][:3, 3], np.array([0.3, 0.7, 0.4]) - ll.CAM, atol=1e-7)
    m = np.asarray(sc.light_rfl[1], F64)
    d = np.array([0.9, 0.8, 0.7]) - np.array([0.2, 0.2, 0.2])
    assert np.allclose(m[:3, :3] @ [0, 0, 1], d / np.linalg.norm(d), atol=1e-6)
    assert np.allclose(m[:3, :3] @ m[:3, :3].T, np.eye(3), atol=1e-6)
    assert np.allclose(m @ np.asarray(sc.light_lfr[1], F64), np.eye(4), atol=1e-6)
    assert np.allclose(m[:3, 3], np.array([0.2, 0.2, 0.2]) - ll.CAM, atol=1e-7)


# ---------------------------------------------------------------------------
# errors

def test_errors_without_a_gpu():
    from acceleratedvolrenderer_amd import capi
    from acceleratedvolrenderer_amd.scene import SpotLight
    with pytest.raises(ValueError):
        SpotLight(coneangle=20.0, conedeltaangle=-5.0)      # falloffStart > totalWidth
    with pytest.raises(ValueError):
        ll.scene_of(["p-inside"] * 9)
    lib = capi.load()
    assert lib.avr_light_local(None, 0, None, None, 1.0, -1.0) != 0
    assert lib.avr_light_probe_at(None, 0, 0, None, None, None, None, None, None, None) != 0
    assert lib.avr_light_pick_at(None, 0, None, None, None, None) != 0
    assert lib.avr_light_bvh(None, None, None, None, None, None, None, None, None, None) != 0
    assert lib.avr_light_sampler(None, 2) != 0
