"""CPU checks of tests/vdb_cases.py with the oracle alone standing in for the device: the points
meet the conditions that make the device tests mean something, the oracle's tree stays within
the float64 reference's tolerance, csrc/avr_vdb.h compiled for the host (base layout, apron layout
without and with the fat copy, get_value) equals the oracle bit for bit on every tree, the oracle's
block key keeps all 32 bits of a block coordinate, and avr_vdb_fetch's state errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vdb_cases as vc   # noqa: E402
import vdb_shim   # noqa: E402

ALL = vc.TREES + ("temperature",)


def _grid(name):
    return vc.temperature() if name == "temperature" else vc.grid(name)


def _pts(name):
    return vc.temperature_points() if name == "temperature" else vc.points(name)


def _want(name):
    if name == "temperature":
        return vc.oracle_tree(name).sample_world(_pts(name))
    return vc.oracle_values(name)


@pytest.fixture(scope="module")
def hdr(tmp_path_factory):
    return vdb_shim.build(tmp_path_factory.mktemp("vdb_cases"))


# ---------------------------------------------------------------------------
# conditions on the inputs

@pytest.mark.parametrize("name", vc.TREES)
def test_points_meet_the_conditions(name):
    g, p = vc.grid(name), vc.points(name)
    assert p.dtype == np.float32 and p.shape == (vc.N_POINTS, 3)
    varied, per_box, minus1 = vc.conditions(g, p)
    print(f"{name}: {len(g.leaf_origins)} leaves, {len(g.tile_values)} tiles; non-constant stencils {varied:.3f}; "
          f"fewest points with a tap in one leaf / tile {int(per_box.min())}; points in the -1 extended block {minus1}; "
          f"distinct oracle values {len(np.unique(vc.oracle_values(name)))}")
    assert varied >= 0.5
    assert per_box.min() >= 100
    assert minus1 >= 1000
    # inside the probe's domain: within 2^24 index units of the tree
    assert np.abs(vc.index_coordinates(g, p)).max() < 2 ** 24 - 2 ** 21


@pytest.mark.parametrize("name", vc.TREES)
def test_structured_values_cover_every_face_and_the_extent_ends(name):
    """Identity trees: every structured value of every axis occurs among the points (the face
    integers, their float neighbours, k + 0.5, k + 0.37 and +-10^6); mapped trees: the same in the
    index-space points before the map."""
    g = vc.grid(name)
    q = vc.index_points(name)
    if name in vc.IDENTITY:
        assert np.array_equal(q.astype(np.float32), vc.points(name))
    lo, hi = vc.extent(g)
    for a in range(3):
        have = set(q[:, a].tolist())
        vals = vc._axis_values(g, a)
        assert set(vals.astype(np.float64).tolist()) <= have
        for k in (lo[a] - 10, lo[a] - 1, lo[a], hi[a], hi[a] + 10):
            assert np.float32(k) in vals and np.nextafter(np.float32(k), np.float32(-np.inf)) in vals
        assert np.float32(1e6) in vals and np.float32(-1e6) in vals


@pytest.mark.parametrize("name", ALL)
def test_vectorised_values_are_the_grids_values(name):
    """vdb_cases.values (the float64 reference's getValue) equals NanoVDBGrid.values at the taps of
    every 25th point."""
    g = _grid(name)
    x = vc.index_coordinates(g, _pts(name)[::25])
    ijk = np.floor(x).astype(np.int64)
    for c in ((0, 0, 0), (1, 1, 1), (1, 0, 1)):
        q = ijk + np.array(c)
        assert np.array_equal(vc.values(g, q).view(np.uint32), g.values(q).view(np.uint32))


def test_trees_are_what_the_cases_say():
    h = vc.grid("holes128")
    assert sorted(h.tile_sizes.tolist()) == [8, 8, 128] and len(h.leaf_origins) == 4 and h.background == np.float32(0.05)
    for name in ("thin-z", "thin-y", "thin-x"):
        lo, hi = vc.extent(vc.grid(name))
        assert np.all(lo < 0) and sorted(((hi - lo) // 8).tolist()) == [1, 1, 6]
        assert np.all(vc.grid(name).index_bbox[:3] < 0)
    b = vc.grid("background")
    assert b.background == np.float32(0.25) and 0.0 in b.tile_values.tolist() and len(b.leaf_origins) == 1
    s = vc.grid("single-leaf")
    assert len(s.leaf_origins) == 8 and s.index_bbox.tolist() == [7, 7, 7, 9, 9, 9]
    t, d = vc.temperature(), vc.grid("mapped-holes128")
    assert np.all(t.index_bbox[:3] < 0)
    assert not np.allclose(t.index_to_world, d.index_to_world)
    assert np.allclose(np.linalg.norm(t.index_to_world[:, :3], axis=0), 0.5 * np.linalg.norm(d.index_to_world[:, :3], axis=0))
    for name in vc.MAPPED:   # the world box is about unit size
        p0, p1 = vc.grid(name).world_bbox()
        assert 0.5 < float(np.max(p1 - p0)) < 2.0


# ---------------------------------------------------------------------------
# references

@pytest.mark.parametrize("name", vc.IDENTITY)
def test_oracle_is_within_the_float64_tolerance(name):
    g = vc.grid(name)
    ref = vc.trilinear64(g, vc.points(name))
    dev = float(np.max(np.abs(vc.oracle_values(name).astype(np.float64) - ref)))
    unit = vc.f64_tolerance(g) / vc.F64_TOL_ULPS
    print(f"{name}: oracle - float64 reference: {dev / unit:.3f} x 2^-23 x the largest value (tolerance {vc.F64_TOL_ULPS})")
    assert dev <= vc.f64_tolerance(g)
    assert float(ref.max()) > 0.5 * unit * 2 ** 23     # the points see the tree's values


@pytest.mark.parametrize("name", ALL)
def test_host_compiled_header_equals_oracle(hdr, name):
    """csrc/avr_vdb.h on the host: sample_world of the base layout and of the apron layout without
    and with the fat copy equal the oracle bit for bit at every point; get_value(Apron) equals
    get_value(Grid) over the extent +-10 voxels."""
    g, p, want = _grid(name), _pts(name), _want(name).view(np.uint32)
    assert np.array_equal(vdb_shim.sample(hdr, g, p).view(np.uint32), want)
    for fat in (0, 1):
        out, nblk, vals = vdb_shim.sample_apron(hdr, g, p, fat)
        assert np.array_equal(out.view(np.uint32), want), (name, fat)
        assert np.all(vals == 0)
    print(f"{name}: {nblk} apron blocks")
    assert nblk >= len(g.leaf_origins)


# ---------------------------------------------------------------------------
# the oracle's block key

def test_oracle_tree_keeps_all_bits_of_a_block_coordinate():
    """A voxel a multiple of 2^24 away from a leaf along an axis (its block coordinate equal to the
    leaf's in the low 21 bits) is the background, not the leaf's value."""
    from acceleratedvolrenderer_amd import NanoVDBGrid
    from oracle import binding
    rng = np.random.default_rng(5)
    g = NanoVDBGrid([(0, 0, 0)], vc._random(rng, (1, 8, 8, 8)), background=0.125, tile_origins=[(8, 0, 0)],
                    tile_sizes=[8], tile_values=[0.875])
    tree = binding.VdbTree(g)
    for x, y, z in ((0, 0, 0), (3, 5, 7), (7, 7, 7)):
        assert tree.value(x, y, z) == g.leaf_values[0, x, y, z]
        assert tree.value(x + 8, y, z) == np.float32(0.875)
        for k in (1, -1, 2, -2, 64, -64):
            for a in range(3):
                q = [x, y, z]
                q[a] += k * 2 ** 24
                assert tree.value(*q) == np.float32(0.125), (q, "leaf")
                q[0] += 8
                assert tree.value(*q) == np.float32(0.125), (q, "tile")
    far = np.float32(2.0 ** 30)
    pts = np.array([[sx * far if a == 0 else 3.5, sx * far if a == 1 else 3.5, sx * far if a == 2 else 3.5]
                    for a in range(3) for sx in (1, -1)] + [[far, -far, far]], np.float32)
    assert np.array_equal(tree.sample_world(pts), np.full(len(pts), 0.125, np.float32))
    # the case that showed it: thin-z's leaves alias at z = 2^30 under a 21-bit key
    t = vc.oracle_tree("thin-z")
    assert t.sample_world(np.array([[-0.5, -9.0, 2.0 ** 30]], np.float32))[0] == vc.grid("thin-z").background


# ---------------------------------------------------------------------------
# avr_vdb_fetch without a device

def test_vdb_fetch_state_error_without_a_gpu():
    """No context (so no NanoVDB medium): AVR_ERR_STATE, reported before any argument check."""
    from acceleratedvolrenderer_amd import capi
    lib = capi.load()
    for grid in (0, 1):
        assert lib.avr_vdb_fetch(None, grid, None, 0, None, None) == 3
        assert b"NanoVDBMedium" in lib.avr_last_error()
        assert lib.avr_vdb_fetch(None, grid, None, -1, None, None) == 3
