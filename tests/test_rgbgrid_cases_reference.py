"""RGBGridMedium's lookup on real colours, without a device (tests/rgbgrid_cases.py; the device
side is tests/test_gpu_rgbgrid.py).

* tests/golden/rgbgrid_vectors.json holds what the reference's own
  SampledGrid<RGBUnboundedSpectrum> / SampledGrid<RGBIlluminantSpectrum> give for
  Lookup(p, convert) (convert = Sample(lambda), media.h:381-397) and MaxValue(bounds, convert)
  (convert = MaxValue(), media.cpp:364-377) over the colour grids. The oracle's SamplePoint
  (OracleRun.medium_sample), a float32 numpy restatement (taps by oracle_rsp_eval, lerps as
  a (1 - t) + b t) and oracle_rgb_majorant reproduce them bit for bit, the colours converted on
  the host through the fixture table on the way in. Where the reference sources are present, the
  harness is compiled from its source as it stands and must print the fixture again, and the
  fixture table is compared with the full one; elsewhere those two tests skip.
* every (grid, combination, box): finite, non-negative, within `tolerance` of the float64
  reference, below the cell's majorant.

The tolerance (rgbgrid_cases.tolerance). u = 2^-24 is float32's unit roundoff. The reference
starts from the lookup's own float32 voxel offsets and lerp weights (they define which lookup is
meant) and the float32 coefficients; after them it is float64. For one tap with coefficients
c0, c1, c2, scale S and wavelength l:

  x = fma(l, fma(l, c0, c1), c2): two roundings. The inner one errs by at most u |l c0 + c1|,
      which the outer multiplies by l; the outer one by u |x|. With P = |c0| l^2 + |c1| l + |c2|
      both are at most u P: |dx| <= 2 P u.
  s(x) = .5 + x / (2 sqrt(1 + x^2)) has slope 1 / (2 (1 + x^2)^1.5) <= 1/2, decreasing in |x|:
      dx moves it by at most s'(max(|x| - |dx|, 0)) |dx| <= P u, and by at most 1 (its range).
      That is `cond`. Its own roundings: x^2, 1 + ., sqrt (halves what came before), the
      division: 3 u relative on |x / (2 sqrt)| <= 1/2; the final sum, u on a value <= 1: 3 u
      in all (the two results that are not approximations, +-inf -> 1 / 0 and 1 + x^2 = inf ->
      0.5, are reproduced by the reference itself: _sigmoid64).
  S s: one rounding, u S. For Le the product with the illuminant sample I: one more, and every
      term carries the factor I: with M = S I the tap errs by at most M (cond + 5 u).
  The seven lerps are three levels deep for every output. A level computes 1 - t, two products
  and a sum: at most 3 u times the larger operand, M; the weights are convex, so the taps'
  errors do not grow: 9 u M, 10 u M with the second-order terms.
  The medium's scale (sigmaScale, LeScale): one rounding more, u M.

  |float32 - float64| <= scale M (max over taps of cond + 16 u)

an absolute bound, proportional to the largest scale among the eight taps (M) and not to the
result: a black tap next to a bright one is held to the bright one's rounding, and eight black
taps to exactly 0. Largest observed error / bound over all cases: 0.213 (printed by
test_float32_lookup_within_the_float64_bound).

The majorant bound. SampledGrid::MaxValue of a cell covers every tap of every point in it. A
float32 lerp can exceed both ends: (a (1 - t)(1 + u)^2 + b t (1 + u)) (1 + u) <= max(a, b)
(1 + u)^3; three levels and the scale give sigma <= scale max_tap (1 + u)^10 for sigma_a and for
sigma_s. The majorant is fl(scale fl(max_a + max_s)) >= scale (max_a + max_s) (1 - u)^2, so

  scale (sigma_a + sigma_s) <= majorant (1 + u)^10 / (1 - u)^2 <= majorant (1 + K 2^-23), K = 6

(12 u = 6 x 2^-23; the second-order terms, 68 u^2, are added as 1e-12). This takes each tap
below its voxel's MaxValue, which holds exactly at 360, 830 and the vertex wavelength as
MaxValue computes it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgbgrid_cases as rc   # noqa: E402
from oracle import binding   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MAJORANT = 6


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vectors():
    with open(rc.VECTORS) as f:
        return json.load(f)


def _golden(vectors, grid, key):
    return np.array(vectors["lookup"][grid][key], np.uint32).view(np.float32)


def _reference_medium(grid):
    """The grid as sigma_a and as Le, both scales 1: what the goldens hold."""
    from acceleratedvolrenderer_amd.scene import RGBGridMedium
    return RGBGridMedium(sigma_a_coeffs=rc.coeffs(grid, "a"), Le_coeffs=rc.coeffs(grid, "a"))


# ---------------------------------------------------------------------------
# the goldens

@pytest.mark.parametrize("grid", rc.GOLDEN_GRIDS)
def test_golden_inputs_are_the_cases(vectors, grid):
    u, lam = rc.golden_probes(grid)
    assert _bits(_golden(vectors, grid, "p")).tolist() == _bits(u).reshape(-1).tolist()
    assert _bits(_golden(vectors, grid, "lambda")).tolist() == _bits(lam).reshape(-1).tolist()
    assert len(u) == rc.GOLDEN_LOOKUPS and all(len(set(r)) == 4 for r in lam.tolist())


@pytest.mark.parametrize("grid", rc.GOLDEN_GRIDS)
def test_oracle_medium_sample_reproduces_the_reference(vectors, grid):
    u, lam = rc.golden_probes(grid)
    scene = rc.probe_scene(grid, None, "unit", med=_reference_medium(grid))
    assert np.array_equal(rc.render_points(scene, u), u)
    for libm in ("platform", "canonical"):
        sa, ss, le = binding.OracleRun(scene, libm=libm).medium_sample(u, lam)
        assert _bits(sa).reshape(-1).tolist() == _bits(_golden(vectors, grid, "sigma")).tolist()
        assert _bits(le).reshape(-1).tolist() == _bits(_golden(vectors, grid, "Le")).tolist()
        assert np.all(ss == 1)                              # no sigma_s grid (media.h:389)
    if grid not in ("black",):
        assert np.unique(_golden(vectors, grid, "sigma")).size > 4 and _golden(vectors, grid, "Le").max() > 0
    else:
        assert not _golden(vectors, grid, "sigma").any() and not _golden(vectors, grid, "Le").any()


def lookup32(c4, u, lam, illuminant=None):
    """SampledGrid<RGB*Spectrum>::Lookup(p, convert) restated in float32 numpy: the taps'
    sigmoid by oracle_rsp_eval, scale * s [* illuminant], lerps a (1 - t) + b t."""
    F = np.float32
    L = binding.lib()
    nz, ny, nx, _ = c4.shape
    out = np.zeros((len(u), 4), np.float32)
    for r, (p, lm) in enumerate(zip(np.asarray(u, np.float32), np.asarray(lam, np.float32))):
        ps = [F(F(p[0] * F(nx)) - F(.5)), F(F(p[1] * F(ny)) - F(.5)), F(F(p[2] * F(nz)) - F(.5))]
        i = [int(np.floor(v)) for v in ps]
        t = [F(v - F(k)) for v, k in zip(ps, i)]
        ill = np.ones(4, np.float32)
        if illuminant is not None:
            off = [int(np.floor(float(l) + 0.5)) - 360 for l in lm]
            ill = np.array([illuminant[o] if 0 <= o < 471 else 0 for o in off], np.float32)

        def tap(dx, dy, dz):
            x, y, z = i[0] + dx, i[1] + dy, i[2] + dz
            if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
                return np.zeros(4, np.float32)
            c = c4[z, y, x]
            s = np.array([L.oracle_rsp_eval(float(c[0]), float(c[1]), float(c[2]), float(l)) for l in lm], np.float32)
            s = (c[3] * s).astype(np.float32)
            return (s * ill).astype(np.float32) if illuminant is not None else s

        lerp = lambda w, a, b: ((a * F(F(1) - w)).astype(np.float32) + (b * w).astype(np.float32)).astype(np.float32)
        d00 = lerp(t[0], tap(0, 0, 0), tap(1, 0, 0))
        d10 = lerp(t[0], tap(0, 1, 0), tap(1, 1, 0))
        d01 = lerp(t[0], tap(0, 0, 1), tap(1, 0, 1))
        d11 = lerp(t[0], tap(0, 1, 1), tap(1, 1, 1))
        out[r] = lerp(t[2], lerp(t[1], d00, d10), lerp(t[1], d01, d11))
    return out


@pytest.mark.parametrize("grid", rc.GOLDEN_GRIDS)
def test_float32_restatement_reproduces_the_reference(vectors, grid):
    from acceleratedvolrenderer_amd import spectra
    u, lam = rc.golden_probes(grid)
    c4 = rc.coeffs(grid, "a")
    with np.errstate(invalid="ignore"):
        assert _bits(lookup32(c4, u, lam)).reshape(-1).tolist() == _bits(_golden(vectors, grid, "sigma")).tolist()
        got = lookup32(c4, u, lam, spectra.TABLES["D65"].astype(np.float32))
    assert _bits(got).reshape(-1).tolist() == _bits(_golden(vectors, grid, "Le")).tolist()


@pytest.mark.parametrize("res", rc.GOLDEN_MAX_RES, ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("grid", rc.GOLDEN_GRIDS)
def test_oracle_rgb_majorant_reproduces_the_reference(vectors, grid, res):
    """oracle_rgb_majorant with the grid as sigma_a and as sigma_s and scale 1 is m + m = 2 m,
    exactly, m the reference's MaxValue of the cell."""
    want = np.array(vectors["max_value"][f"{grid}@{res[0]}x{res[1]}x{res[2]}"], np.uint32).view(np.float32)
    a = np.ascontiguousarray(rc.coeffs(grid, "a"))
    nz, ny, nx = rc.SHAPES[grid]
    out = np.zeros(int(np.prod(res)), np.float32)
    binding.lib().oracle_rgb_majorant(binding.fp(a), binding.fp(a), nx, ny, nz, 1.0, res[0], res[1], res[2],
                                      binding.fp(out))
    assert _bits(out / np.float32(2)).tolist() == _bits(want).tolist()
    assert (want.max() > 0) == (grid != "black")
    # and through the medium object (binding.rgb_majorant): sigma_s missing is 1
    med = rc.medium(grid, "a", scale=1.0)
    med.majorant_res = tuple(res)
    assert _bits(binding.rgb_majorant(med)).tolist() == _bits(want + np.float32(1)).tolist()


def test_srgb_subset_fixture_converts_the_palette_like_the_full_table(srgb_table):
    full = srgb_table.spectrum_coeffs(rc.palette_rgb())
    assert _bits(full).tolist() == _bits(rc.table().spectrum_coeffs(rc.palette_rgb())).tolist()


def _write_table_inc(table, path):
    """The fixture table in the text layout of rgb2spec_opt's output, which the harness reads."""
    with open(path, "w") as f:
        f.write("ToSpectrumTable_Scale = { " + ", ".join(repr(float(v)) for v in table.z_nodes) + " };\n")
        f.write("ToSpectrumTable_Data = { " + ", ".join("0" if v == 0 else repr(float(v)) for v in table.coeffs.reshape(-1).tolist()) + " };\n")


def test_fixtures_regenerate_from_the_reference(vectors, tmp_path):
    """With the reference sources and the objects of oracle/_ref present: the harness, compiled
    from oracle/ref/ref_harness.cpp as it stands (a binary left in oracle/_ref may be older than
    its source), prints the committed rgbgrid_vectors.json again. It reads the fixture table, which
    converts the palette as the full table does (the test above), so nothing here depends on a
    table generated on this machine."""
    refdir = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.isdir("/root/reference/src/pbrt") or not os.path.exists(os.path.join(refdir, "spectrum.o")):
        pytest.skip("reference sources or their objects under oracle/_ref absent")
    exe = tmp_path / "ref_harness"
    subprocess.check_call(["make", "-s", f"COPY={tmp_path}", str(exe)], cwd=os.path.join(ROOT, "oracle", "ref"))
    inc = tmp_path / "srgb_subset.inc"
    _write_table_inc(rc.table(), inc)
    run = subprocess.run([str(exe), "--rgbtable", str(inc), "--rgb-grid"], input=rc.harness_lines().encode(),
                         capture_output=True)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    got = json.loads(run.stdout)
    assert sorted(got) == sorted(vectors) == ["lookup", "max_value"]
    for section in ("lookup", "max_value"):
        assert sorted(got[section]) == sorted(vectors[section])
        for name, want in vectors[section].items():
            rows = want.items() if isinstance(want, dict) else [("", want)]
            for key, w in rows:
                g = got[section][name][key] if key else got[section][name]
                differ = int(np.sum(np.array(g, np.uint32) != np.array(w, np.uint32))) if len(g) == len(w) else -1
                assert differ == 0, f"{section}/{name}/{key}: {differ} of {len(w)} values differ (-1: another length)"


def test_palette_coefficients_are_the_edges_they_claim():
    c = dict(zip(rc.NAMES, rc.table().spectrum_coeffs(rc.palette_rgb())))
    assert c["black"].tolist() == [0, 0, -np.inf, 0]
    for g in ("grey0.01", "grey0.5", "grey1", "grey7.5"):
        assert c[g][0] == 0 and c[g][1] == 0 and c[g][2] == 0 and c[g][3] == 2 * rc.PALETTE[g][0]   # rgb / scale = .5
    for name in ("red", "green", "blue", "cyan", "magenta", "yellow", "neargrey", "tiny", "large", "hdr", "leaf", "rust"):
        assert c[name][0] != 0 and np.all(np.isfinite(c[name])), name
    assert c["hdr"][3] == 60 and c["large"][3] == 100
    L = binding.lib()
    x = rc.DIRECT[1]
    assert [L.oracle_rsp_eval(*map(float, x[:3]), l) for l in (360.0, 555.0, 830.0)] == [0.5, 0.5, 0.5]
    assert L.oracle_rsp_eval(0.0, 0.0, float("inf"), 555.0) == 1.0 and L.oracle_rsp_max(0.0, 0.0, float("inf")) == 1.0
    assert L.oracle_rsp_eval(0.0, 0.0, float("-inf"), 555.0) == 0.0 and L.oracle_rsp_max(0.0, 0.0, float("-inf")) == 0.0


# ---------------------------------------------------------------------------
# every case

_IDS = [f"{g}-{c}-{b}" for g, c, b in rc.ALL_CASES]
_worst = {"frac": 0.0}


@pytest.mark.parametrize("grid,combo,box", rc.ALL_CASES, ids=_IDS)
def test_float32_lookup_within_the_float64_bound(grid, combo, box):
    k = rc.case(grid, combo, box)
    worst = 0.0
    for name, got, ref, tol in zip(("sigma_a", "sigma_s", "Le"), k["oracle"], k["ref"], k["tol"]):
        assert np.all(np.isfinite(got)), name                  # black next to colours, all-black
        assert np.all(got >= 0), name
        err = np.abs(got.astype(np.float64) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(err == 0, 0.0, err / tol)
        worst = max(worst, float(frac.max()))
        bad = np.argwhere(err > tol)
        assert len(bad) == 0, (name, k["p"][bad[0][0]], k["lam"][bad[0][0]], got[tuple(bad[0])], ref[tuple(bad[0])],
                               tol[tuple(bad[0])])
    _worst["frac"] = max(_worst["frac"], worst)
    print(f"{grid}/{combo}/{box}: {len(k['p'])} probes, largest error / bound {worst:.3f} (so far {_worst['frac']:.3f})")


def test_probe_sets_hold_what_they_claim():
    """Faces hit exactly, black taps next to coloured ones, outside points with every tap outside."""
    for box in rc.BOXES:
        k = rc.case("plume", "a+s+Le", box)
        u = rc.grid_coordinates(k["scene"], k["p"])
        faces = 0
        for axis in range(3):
            for side in (0.0, 1.0):
                n = int(np.sum(u[:, axis] == side))
                print(f"plume/{box}: {n} probes with grid coordinate {axis} exactly {side}")
                faces += n >= 1
                # behind the transform a face may have no float32 point that maps onto it exactly
                # (media_cases.on_face): the probes then lie within ulps of it, on both sides
                near = np.abs(u[:, axis].astype(np.float64) - side) < 1e-5
                assert np.any(near & (u[:, axis] >= side)) and np.any(near & (u[:, axis] <= side))
        assert faces == 6 if box == "unit" else faces >= 4
        sa = k["oracle"][0]
        assert np.any(sa == 0) and np.any(sa > 0)
        # outside the box: the edge voxels still weigh in within half a voxel, nothing farther out
        k = rc.case("g798", "a+s", box)
        u, sa = rc.grid_coordinates(k["scene"], k["p"]), k["oracle"][0]
        outside = ((u < 0) | (u > 1)).any(axis=1)
        assert outside.sum() >= 32 and np.any(sa[outside] > 0) and np.any((sa[outside] == 0).all(axis=1))
    ids = rc.voxel_ids("plume", "a")
    black = ids == rc.NAMES.index("black")
    assert 0.3 < black.mean() < 0.95
    edge = black[:, :, 1:] != black[:, :, :-1]
    assert edge.any()
    k = rc.case("black", "a+s+Le", "unit")
    assert not k["oracle"][0].any() and not k["oracle"][1].any() and not k["oracle"][2].any()
    k = rc.case("black", "s", "affine")
    assert np.all(k["oracle"][0] == np.float32(1.3))           # sigma_a missing: scale * 1
    for combo, which in (("scale0", (0, 1)), ("Lescale0", (2,))):
        k = rc.case("g798", combo, "unit")
        for w in which:
            assert not k["oracle"][w].any()


@pytest.mark.parametrize("grid,combo,box", rc.ALL_CASES, ids=_IDS)
def test_majorant_is_conservative(grid, combo, box):
    """scale (sigma_a + sigma_s) at every probe inside the box and every wavelength is at most
    the majorant of the probe's cell times (1 + K 2^-23); all-black grids: majorant exactly 0."""
    k = rc.case(grid, combo, box)
    maj = k["run"].majorant
    res = k["scene"].medium.majorant_res
    assert maj.shape == (int(np.prod(res)),) and np.all(np.isfinite(maj)) and np.all(maj >= 0)
    if grid == "black" and combo not in ("s", "a"):
        assert not maj.any()
    cell = rc.cell_majorant(k["scene"], k["p"], maj, res)
    inside = ~np.isnan(cell)
    st = k["oracle"][0].astype(np.float64) + k["oracle"][1].astype(np.float64)
    bound = cell * (1 + K_MAJORANT * 2.0 ** -23 + 1e-12)
    over = st[inside] - bound[inside, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(st[inside] > 0, st[inside] / cell[inside, None] - 1, -1.0)
    print(f"{grid}/{combo}/{box}: {int(inside.sum())} probes inside, largest sigma_t / majorant - 1 = {rel.max() / 2.0 ** -23:+.2f} x 2^-23")
    assert inside.sum() > 0.7 * len(inside) or grid == "g111"
    assert np.all(over <= 0), (k["p"][inside][np.argmax(over.max(axis=1))], float(over.max()))
