"""The voxel boundary, graph::VoxelBoundary (graph/voxels/voxel_boundary.cpp), on the CPU: the
sphere points and ray bundles against float32 restatements written here; the two floods
(ToSingleLayerAndSaveCast :122-181, FillInside :183-225) against the reference's own loops
restated with Python sets (the three-set flood, the FIFO fill); the ids of the graphs that come
out; the vertex-count bisection (:64-95) against a float32 restatement over host counts; argument
errors; the kernels' resources; the host code under ASan + UBSan as a stand-alone program
(tests/sanitize_voxels_main.cpp). The device side is tests/test_gpu_graph_voxels.py.
"""
import collections
import ctypes
import math
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from acceleratedvolrenderer_amd import capi, graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---------------------------------------------------------------------------- sphere points

CENTER, RADIUS = np.array([0.25, -0.5, 0.125], f32), f32(2.0)


def test_sphere_point_counts():
    assert len(graph.sphere_surface_points(CENTER, RADIUS, 90)) == 6
    p = graph.sphere_surface_points(CENTER, RADIUS, 45)
    assert len(p) == 8 + 6 * 2 + 2 and p.dtype == np.float32


@pytest.mark.parametrize("step", [90, 45, 30, 10])
def test_sphere_points_lie_on_the_sphere_and_mirror(step):
    p = graph.sphere_surface_points(CENTER, RADIUS, step).astype(np.float64)
    r = np.sqrt(((p - CENTER.astype(np.float64)) ** 2).sum(axis=1))
    ulp = float(np.spacing(RADIUS))
    print(f"step {step}: {len(p)} points, |r - radius| max {np.abs(r - float(RADIUS)).max() / ulp:.2f} ulp")
    assert np.abs(r - float(RADIUS)).max() <= 4 * ulp
    # the equator ring has ratio 1: 360 / step points; every later point is followed by its
    # mirror (the same theta measured from the other pole, the same phi)
    n0 = 360 // step
    rest = p[n0:]
    assert len(rest) % 2 == 0 and len(rest) > 0
    up, down = rest[0::2], rest[1::2]
    mirrored = up.copy()
    mirrored[:, 1] = 2 * float(CENTER[1]) - up[:, 1]
    assert np.all(up[:, 1] > float(CENTER[1])) and np.all(down[:, 1] < float(CENTER[1]))
    assert np.abs(down - mirrored).max() <= 2.0 ** -20 * float(RADIUS)
    assert np.allclose(p[:n0, 1], float(CENTER[1]), atol=2.0 ** -20 * float(RADIUS))


@pytest.mark.parametrize("step", [0, 91, -5, float("nan")])
def test_sphere_points_refuse_a_bad_step(step):
    with pytest.raises(ValueError):
        graph.sphere_surface_points(CENTER, RADIUS, step)


# ---------------------------------------------------------------------------- bundles

def _md(pmin, pmax):
    """What VoxelBoundary reads of a MediumData (util.h:45-59), from the primitive's bounds."""
    pmin, pmax = np.asarray(pmin, f32), np.asarray(pmax, f32)
    half = ((pmax - pmin).astype(f32) / f32(2)).astype(f32)
    ln = f32(np.sqrt(f32(f32(f32(half[0] * half[0]) + f32(half[1] * half[1])) + f32(half[2] * half[2]))))
    return types.SimpleNamespace(pmin=pmin, pmax=pmax, bounds_center=(pmin + half).astype(f32), max_dist_to_center=ln,
                                 geometry=None)


def _coordinate_system(v):   # vecmath.h:1007-1013 in float32
    sign = f32(math.copysign(1.0, float(v[2])))
    a = f32(f32(-1) / f32(sign + v[2]))
    b = f32(f32(v[0] * v[1]) * a)
    return (np.array([f32(f32(1) + f32(f32(sign * f32(v[0] * v[0])) * a)), f32(sign * b), f32(-sign * v[0])], f32),
            np.array([b, f32(sign + f32(f32(v[1] * v[1]) * a)), f32(-v[1])], f32))


@pytest.mark.parametrize("frame", ["reference", "orthonormal"])
def test_bundles_equal_a_float32_restatement(frame):
    md = _md([-0.3, 0.1, 0.2], [0.9, 1.0, 1.7])
    vb = graph.VoxelBoundary(None, md, num_steps=7, frame=frame, device=False)
    o, d, xv, yv = vb.bundles(30)
    pts = graph.sphere_surface_points(md.bounds_center, f32(md.max_dist_to_center * f32(2)), 30)
    assert np.array_equal(o, pts) and len(o) > 30
    step = f32(md.max_dist_to_center / f32(7))
    for k in range(len(o)):
        dk = (md.bounds_center - pts[k]).astype(f32)
        basis = dk
        if frame == "orthonormal":
            basis = (dk / f32(np.sqrt(f32(f32(f32(dk[0] * dk[0]) + f32(dk[1] * dk[1])) + f32(dk[2] * dk[2]))))).astype(f32)
        x, y = _coordinate_system(basis)
        assert np.array_equal(d[k], dk)
        assert np.array_equal(xv[k], (x * step).astype(f32)) and np.array_equal(yv[k], (y * step).astype(f32))
    if frame == "orthonormal":
        d64, x64, y64 = d.astype(np.float64), xv.astype(np.float64), yv.astype(np.float64)
        ln = lambda v: np.sqrt((v * v).sum(axis=1))
        assert np.all(np.abs((x64 * d64).sum(axis=1)) <= 1e-5 * ln(x64) * ln(d64))
        assert np.all(np.abs((y64 * d64).sum(axis=1)) <= 1e-5 * ln(y64) * ln(d64))
        assert np.all(np.abs((x64 * y64).sum(axis=1)) <= 1e-5 * ln(x64) * ln(y64))
        assert np.allclose(ln(x64), float(step), rtol=1e-5) and np.allclose(ln(y64), float(step), rtol=1e-5)
    else:
        # CoordinateSystem of a vector of length 2 R: not a unit frame
        assert not np.allclose(np.sqrt((xv.astype(np.float64) ** 2).sum(axis=1)), float(step), rtol=1e-3)
    with pytest.raises(ValueError):
        graph.VoxelBoundary(None, md, frame="unit")


# ---------------------------------------------------------------------------- flood cases

def _ball_shell(center, r0, r1, lo, hi):
    g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    r = np.sqrt(((g - np.asarray(center, np.float64)) ** 2).sum(axis=1))
    return g[(r >= r0) & (r < r1)]


def flood_cases():
    """name -> (pmin, pmax, spacing, coors (m, 3) int32): the primitive's bounds, from which
    FitBounds makes the lattice, and the boundary vertices in id order (shuffled)."""
    rng = np.random.default_rng(11)
    cases = {}

    def add(name, pmin, pmax, spacing, coors):
        coors = np.asarray(coors, np.int64)
        coors = coors[rng.permutation(len(coors))]
        cases[name] = (np.asarray(pmin, f32) * f32(spacing), np.asarray(pmax, f32) * f32(spacing), f32(spacing),
                       np.ascontiguousarray(coors, np.int32))

    shell = _ball_shell((5.5, 5.5, 5.5), 3.6, 4.7, (0, 0, 0), (11, 11, 11))
    add("shell", (0, 0, 0), (11, 11, 11), 1.0, shell)                       # lattice -1..12: 14^3
    solid = [(x, y, z) for x in range(1, 9) for y in range(1, 9) for z in range(1, 5) if not (x >= 5 and y >= 5)]
    add("L", (0, 0, 0), (9, 9, 5), 0.25, solid)
    two = np.concatenate([_ball_shell((3, 3, 3), 1.6, 2.7, (0, 0, 0), (6, 6, 6)),
                          _ball_shell((11, 3, 3), 1.6, 2.7, (8, 0, 0), (14, 6, 6))])
    add("two", (0, 0, 0), (14, 6, 6), 1.0, two)
    hole = shell[~np.all(shell == shell[np.argmax(shell[:, 0] * 10000 - np.abs(shell[:, 1] - 5) - np.abs(shell[:, 2] - 5))],
                         axis=1)]
    assert len(hole) == len(shell) - 1
    add("hole", (0, 0, 0), (11, 11, 11), 1.0, hole)
    box = [(x, y, z) for x in range(1, 6) for y in range(1, 11) for z in range(0, 3)
           if x in (1, 5) or y in (1, 10) or z in (0, 2)]
    add("noncubic", (0, 0, 0), (6, 11, 2), 0.5, box)                        # lattice 9 x 14 x 5
    add("negative", (-26, -13, -9), (-15, -2, 2), 0.5, shell + np.array([-26, -13, -9]))
    return cases


CASES = flood_cases()


def _lattice(pmin, pmax, spacing):
    """FitBounds (util.h:313-317): FitToGraph of the two corners, widened by one."""
    fit = lambda p: np.array([int(np.trunc(q + math.copysign(0.5, q))) for q in (np.asarray(p, f32) / f32(spacing)).astype(f32)])
    return tuple(fit(pmin) - 1), tuple(fit(pmax) + 1)


def _neighbours(p, lo, hi):
    """GetNeighbours (:106-120) with Inside(Point3i, Bounds3i), both corners inclusive."""
    out = []
    for i in range(6):
        q = list(p)
        q[i // 2] += -1 if i % 2 == 0 else 1
        if all(lo[a] <= q[a] <= hi[a] for a in range(3)):
            out.append(tuple(q))
    return out


def ref_single_layer(lo, hi, verts):
    """ToSingleLayerAndSaveCast (:122-181) with its three sets; verts: {coors: id}. Returns the
    single-layer ids, the cast set and numVisited."""
    single, cast, visited = set(), set(), 0
    prev, cur, nxt = set(), {tuple(lo)}, set()
    while True:
        for p in cur:
            visited += 1
            for nb in _neighbours(p, lo, hi):
                if nb in verts:
                    single.add(verts[nb])
                    cast.add(p)
                elif nb not in prev and nb not in cur:
                    nxt.add(nb)
        if not nxt:
            break
        prev.clear()
        prev, cur, nxt = cur, nxt, prev
    return single, cast, visited


def ref_fill(lo, hi, cast, start):
    """FillInside (:195-219): the FIFO flood from `start`; the filled coordinates in queue order."""
    visited, order = set(), []
    queue, queued = collections.deque([start]), {start}
    while queue:
        p = queue.popleft()
        queued.discard(p)
        visited.add(p)
        order.append(p)
        for nb in _neighbours(p, lo, hi):
            if nb not in cast and nb not in visited and nb not in queued:
                queue.append(nb)
                queued.add(nb)
    return order


_REF = {}


def reference(name):
    """The restatement's results for a case, computed once: lattice, single-layer ids, cast,
    visited, and the filled sets from the lowest survivor and from all of them."""
    if name not in _REF:
        pmin, pmax, spacing, coors = CASES[name]
        lo, hi = _lattice(pmin, pmax, spacing)
        verts = {tuple(int(v) for v in c): i for i, c in enumerate(coors)}
        single, cast, visited = ref_single_layer(lo, hi, verts)
        first = set(ref_fill(lo, hi, cast, tuple(int(v) for v in coors[min(single)])))
        every = set()
        for i in sorted(single):
            c = tuple(int(v) for v in coors[i])
            if c not in every:
                every |= set(ref_fill(lo, hi, cast, c))
        _REF[name] = types.SimpleNamespace(lo=lo, hi=hi, single=single, cast=cast, visited=visited, first=first, every=every)
    return _REF[name]


def _as_set(coors):
    return {tuple(int(v) for v in c) for c in np.asarray(coors)}


def run_case(name, ctx=None):
    """The case through VoxelBoundary (host floods without a context): the boundary graph and
    the two filled graphs, with the state bytes after each step."""
    pmin, pmax, spacing, coors = CASES[name]
    vb = graph.VoxelBoundary(ctx, _md(pmin, pmax), device=ctx is not None)
    full = graph.UniformGraph(capi.GraphUniform(coors, np.zeros(len(coors), f32), spacing))
    g = vb.to_single_layer(full)
    s0 = g.voxels.state().copy()
    lowest = vb.fill_inside(g)
    s1 = g.voxels.state().copy()
    every = vb.fill_inside(g, start="all")
    s2 = g.voxels.state().copy()
    return types.SimpleNamespace(vb=vb, full=full, g=g, lowest=lowest, every=every, states=(s0, s1, s2))


_RUN = {}


def host_run(name):
    if name not in _RUN:
        _RUN[name] = run_case(name)
    return _RUN[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_floods_follow_the_reference_loops(name):
    ref, run = reference(name), host_run(name)
    vox = run.g.voxels
    assert tuple(vox.lo) == ref.lo and tuple(vox.lo + vox.n - 1) == ref.hi
    if name == "shell":
        assert tuple(vox.n) == (14, 14, 14)
    if name == "noncubic":
        assert tuple(vox.n) == (9, 14, 5)
    if name == "negative":
        assert all(h < 0 for h in ref.hi[:2]) and ref.lo[2] < 0
    s0 = run.states[0]
    assert set(run.g.old_ids.tolist()) == ref.single
    z, y, x = np.nonzero(s0 & capi.VOXEL_CAST)
    assert _as_set(np.stack([x, y, z], axis=1) + vox.lo) == ref.cast
    assert run.g.visited == ref.visited == int(np.count_nonzero(s0 & capi.VOXEL_OUTSIDE))
    assert _as_set(run.lowest.coors) == ref.first
    assert _as_set(run.every.coors) == ref.every
    print(f"{name}: {len(run.full.coors)} vertices, {len(ref.single)} single layer, {len(ref.cast)} cast, "
          f"{ref.visited} visited of {vox.cells}, filled {len(ref.first)} / {len(ref.every)}")
    # the steps only add their own bits
    assert np.array_equal(run.states[1] & ~np.uint8(capi.VOXEL_FILLED), s0)
    assert np.array_equal(run.states[2] & ~np.uint8(capi.VOXEL_FILLED), s0)
    assert vox.counts() == (ref.visited, len(ref.cast), len(ref.single), len(ref.every))


def test_closed_shapes_fill_their_inside_and_a_hole_leaks():
    shell, hole, solid = reference("shell"), reference("hole"), reference("L")
    n = len(CASES["shell"][3])
    inside = 14 ** 3 - shell.visited - n
    assert inside > 0 and len(shell.single) < n          # a thick shell: some vertices touch no outside cell
    assert len(shell.first) == n + inside and shell.first == shell.every
    # the flood enters through the hole: every cell is visited or a vertex, and nothing but
    # vertices is left to fill
    assert hole.visited + (n - 1) == 14 ** 3
    verts = _as_set(CASES["hole"][3])
    assert _as_set(host_run("hole").every.coors) == hole.every == verts
    assert _as_set(host_run("hole").lowest.coors) == hole.first <= verts   # those the start reaches over vertices alone
    # the L is solid: the fill is the vertex set itself, the concave corner included
    assert _as_set(host_run("L").lowest.coors) == _as_set(CASES["L"][3])
    assert len(solid.single) < len(CASES["L"][3])


def test_two_shells_fill_one_blob_from_one_start_and_both_from_all():
    ref, run = reference("two"), host_run("two")
    coors = CASES["two"][3]
    left, right = _as_set(coors[coors[:, 0] <= 6]), _as_set(coors[coors[:, 0] >= 8])
    low = _as_set(run.lowest.coors)
    assert (left <= low) != (right <= low) and not ((left & low) and (right & low))
    assert left | right <= _as_set(run.every.coors)
    assert len(run.every.coors) == 2 * len(run.lowest.coors)
    # an explicit start in the other shell fills the other blob
    other = [i for i, o in enumerate(run.g.old_ids) if tuple(int(v) for v in coors[o]) not in low][0]
    blob = _as_set(run.vb.fill_inside(run.g, start=other).coors)
    assert blob | low == ref.every and not (blob & low)


@pytest.mark.parametrize("name", sorted(CASES))
def test_ids_of_the_graphs(name):
    run = host_run(name)
    g, coors = run.g, CASES[name][3]
    assert np.all(np.diff(g.old_ids) > 0)
    assert np.array_equal(g.coors, coors[g.old_ids])
    assert np.array_equal(g.old_to_new[g.old_ids], np.arange(len(g.old_ids)))
    assert np.count_nonzero(g.old_to_new < 0) == len(coors) - len(g.old_ids)
    assert g.num_vertices == len(g.old_ids) and g.num_captured == len(coors)
    for filled in (run.lowest, run.every):
        c = filled.coors.astype(np.int64)
        key = (c[:, 2] * 4096 + c[:, 1]) * 4096 + c[:, 0]
        assert np.all(np.diff(key) > 0)
        assert np.array_equal(filled.points, (filled.coors.astype(f32) * g.spacing).astype(f32))
        assert np.all(filled.light_scalar == 0) and filled.spacing == g.spacing


def test_fill_runs_the_single_layer_first_on_a_fresh_graph():
    pmin, pmax, spacing, coors = CASES["shell"]
    vb = graph.VoxelBoundary(None, _md(pmin, pmax), device=False)
    full = graph.UniformGraph(capi.GraphUniform(coors, np.zeros(len(coors), f32), spacing))
    start = int(min(reference("shell").single))
    assert _as_set(vb.fill_inside(full, start=start).coors) == reference("shell").first
    vox = capi.GraphVoxels(pmin, pmax, spacing, coors)
    vox.fill(None)                                       # avr_graph_voxels_fill alone does too
    assert np.array_equal(vox.state(), host_run("shell").states[1])


# ---------------------------------------------------------------------------- bisection

def _cloud():
    rng = np.random.default_rng(4)
    v = rng.normal(size=(3000, 3))
    v *= (rng.uniform(2.0, 4.5, size=(3000, 1)) / np.linalg.norm(v, axis=1, keepdims=True))
    return np.ascontiguousarray(v, f32)


_COUNTS = {}


def _host_count(points, spacing):
    key = float(f32(spacing))
    if key not in _COUNTS:
        _COUNTS[key] = capi.GraphUniform.from_points(points, np.zeros(len(points), f32), f32(spacing)).num_vertices
    return _COUNTS[key]


def ref_bisection(count, wanted):
    """CaptureBoundary(wantedVertices) :67-91 in float32; (spacingGTE1, the spacings tried)."""
    gte1 = count(f32(1)) >= wanted
    lo, hi, tried = f32(1), f32(1000), []
    steps_needed = int(math.ceil(math.log2(1000))) + 1
    for _ in range(steps_needed - 1):
        middle = f32(lo + f32(f32(hi - lo) / f32(2)))
        tried.append(f32(middle / (f32(1) if gte1 else f32(1000))))
        if count(tried[-1]) > wanted:
            lo = middle
        else:
            hi = middle
    return gte1, tried


@pytest.mark.parametrize("wanted, gte1", [(150, True), (2500, False)])
def test_bisection_follows_the_float32_restatement(wanted, gte1):
    pts = _cloud()
    branch, tried = ref_bisection(lambda s: _host_count(pts, s), wanted)
    assert branch == gte1 and len(tried) == 10 and len(set(float(t) for t in tried)) == 10
    vb = graph.VoxelBoundary(None, _md([-5, -5, -5], [5, 5, 5]), device=False)
    g = vb.capture_boundary(wanted_vertices=wanted, points=pts)
    print(f"wanted {wanted}: count(1) = {_host_count(pts, 1)}, spacings {[float(t) for t in tried]}, "
          f"{g.num_captured} vertices before thinning")
    assert g.spacing == tried[-1] and [float(t) for t in g.spacings_tried] == [float(t) for t in tried]
    assert g.num_captured == _host_count(pts, tried[-1])
    # the same graph as the spacing form at that spacing
    h = vb.capture_boundary(spacing=tried[-1], points=pts)
    assert np.array_equal(h.coors, g.coors) and h.spacings_tried is None
    with pytest.raises(ValueError):
        vb.capture_boundary(points=pts)
    with pytest.raises(ValueError):
        vb.capture_boundary(spacing=1.0, wanted_vertices=5, points=pts)


# ---------------------------------------------------------------------------- errors

def _err():
    return capi.load().avr_last_error().decode()


def test_argument_errors():
    lib = capi.load()
    pmin, pmax, spacing, coors = CASES["shell"]
    h = ctypes.c_void_p()
    cp = coors.ctypes.data_as(capi.c_int_p)
    fp = lambda a: a.ctypes.data_as(capi.c_float_p)
    # null buffers
    assert lib.avr_graph_voxels_create(fp(pmin), fp(pmax), 1.0, len(coors), cp, None) != 0 and "null" in _err()
    assert lib.avr_graph_voxels_create(None, fp(pmax), 1.0, len(coors), cp, ctypes.byref(h)) != 0 and "null" in _err()
    assert lib.avr_graph_voxels_create(fp(pmin), fp(pmax), 1.0, len(coors), None, ctypes.byref(h)) != 0
    assert lib.avr_graph_voxels_create(fp(pmin), fp(pmax), 1.0, 0, cp, ctypes.byref(h)) != 0 and "at least one" in _err()
    for fn in (lib.avr_graph_voxels_single_layer, ):
        assert fn(None, None, None) != 0 and "null voxels" in _err()
    assert lib.avr_graph_voxels_fill(None, None, -1, None) != 0 and "null voxels" in _err()
    assert lib.avr_graph_voxels_state(None, None, None, None, 0) != 0
    assert lib.avr_graph_voxels_visited(None, None, None, None, None) != 0
    # the device entry points refuse a null context before they touch a GPU
    cnt = ctypes.c_longlong(0)
    pts = np.zeros((4, 3), f32)
    assert lib.avr_graph_capture(None, 1, fp(pts), fp(pts), fp(pts), fp(pts), 1, fp(np.zeros(36, f32)), ctypes.byref(cnt)) != 0
    assert "null context" in _err()
    assert lib.avr_graph_uniform_count_device(None, 4, fp(pts), 1.0, ctypes.byref(cnt)) != 0 and "null context" in _err()
    assert lib.avr_graph_uniform_count_device(None, 4, fp(pts), 1.0, None) != 0 and "null" in _err()
    assert lib.avr_graph_uniform_from_points_device(None, 4, fp(pts), 1.0, None, None) != 0 and "null" in _err()
    assert lib.avr_graph_uniform_from_points_device(None, 4, fp(pts), 1.0, ctypes.byref(h), None) != 0
    # a short state buffer
    vox = capi.GraphVoxels(pmin, pmax, spacing, coors)
    short = np.zeros(vox.cells - 1, np.uint8)
    assert lib.avr_graph_voxels_state(vox.h, None, None, short.ctypes.data_as(ctypes.c_void_p), len(short)) != 0
    assert "shorter" in _err()
    # spacing, cell cap, vertices
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="spacing must be positive"):
            capi.GraphVoxels(pmin, pmax, s, coors)
    with pytest.raises(RuntimeError, match="2\\^31 - 1 cells"):
        capi.GraphVoxels([0, 0, 0], [1300, 1300, 1300], 1.0, coors)
    for bad in ([13, 5, 5], [5, -2, 5], [5, 5, 2 ** 31 - 1]):
        with pytest.raises(RuntimeError, match="vertex 1: outside the bounds"):
            capi.GraphVoxels(pmin, pmax, spacing, np.array([coors[0], bad], np.int64))
    with pytest.raises(RuntimeError, match="vertex 2: repeated"):
        capi.GraphVoxels(pmin, pmax, spacing, coors[[0, 1, 0]])
    with pytest.raises(ValueError):
        capi.GraphVoxels(pmin, pmax, spacing, coors.astype(f32))
    # start ids
    vox.single_layer(None)
    thinned = sorted(set(range(len(coors))) - reference("shell").single)
    for bad in (thinned[0], len(coors), 2 ** 31 - 1):
        with pytest.raises(RuntimeError, match="no single-layer vertex"):
            vox.fill(None, bad)
    for bad in (-3, 1.5, True, "first"):
        with pytest.raises(ValueError):
            vox.fill(None, bad)
    run = host_run("shell")
    for bad in (-1, len(run.g.old_ids), 2.0):
        with pytest.raises(ValueError):
            run.vb.fill_inside(run.g, start=bad)
    with pytest.raises(ValueError):
        graph.VoxelBoundary(None, _md(pmin, pmax), num_steps=0)


def test_tool_arguments():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import graph_maker
        a = graph_maker.parser().parse_args(["--out", "x", "--voxels", "0.05", "--fill-start", "all"])
        b = graph_maker.parser().parse_args(["--out", "x", "--wanted-vertices", "500", "--equator-step", "30",
                                             "--capture-steps", "20", "--fill-start", "7"])
        none = graph_maker.parser().parse_args(["--out", "x"])
        import graph_render_demo
        assert graph_render_demo.parser().parse_args(["--graph-file", "x_voxels.txt"]).graph_file == "x_voxels.txt"
        assert graph_render_demo.parser().parse_args([]).graph_file is None
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    assert a.voxels == 0.05 and a.fill_start == "all" and a.equator_step == 10 and a.capture_steps == 100
    assert b.voxels is None and b.wanted_vertices == 500 and b.equator_step == 30 and b.capture_steps == 20
    assert graph_maker.fill_start(b.fill_start) == 7 and graph_maker.fill_start(a.fill_start) == "all"
    assert graph_maker.fill_start(none.fill_start) is None and none.voxels is None and none.wanted_vertices is None
    with pytest.raises(ValueError):
        graph_maker.fill_start("some")


# ---------------------------------------------------------------------------- resources

@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """The graph kernels alone, cross-compiled for gfx950 with the build's flags; {mangled name:
    figures} from the -Rpass-analysis=kernel-resource-usage remarks, as
    tests/test_graph_uniform.py reads them."""
    from acceleratedvolrenderer_amd import build as avr_build
    if not os.path.exists(avr_build.HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("voxel_resources")
    inst = [f"template __global__ void k_graph_capture<{g}>(DevMedium, long long, int, const float *, const float *, "
            "const float *, const float *, float4 *, int *);" for g in (0, 1)]
    inst += [f"template __global__ void k_graph_voxels_level<{f}>(graph::VoxelDims, unsigned *, const int *, int, int *, "
             "int *);" for f in (0, 1)]
    src = tmp / "voxels.hip"
    src.write_text('#define AVR_KPATHS_TU\n#include "avr_kernels.hip"\n#include "avr_graph.hip"\n'
                   "namespace avr {\n" + "\n".join(inst) + "\n}\n")
    cmd = ([avr_build.HIPCC] + avr_build.FLAGS +
           ["-I" + avr_build.CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
            "-c", str(src), "-o", str(tmp / "voxels.o")])
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for block in p.stderr.split("Function Name: ")[1:]:
        out[block.split()[0]] = {key: int(re.search(pat, block).group(1)) for key, pat in (
            ("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
            ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))}
    return out


def test_voxel_kernel_resources(resources):
    """No scratch in the capture, dedupe and flood kernels; the capture stages the majorant in
    LDS (16 KiB), the others use none."""
    def one(tag):
        match = [v for k, v in resources.items() if tag in k]
        assert len(match) == 1, tag
        return match[0]
    for tag, lds in (("15k_graph_captureILi0EE", 16384), ("15k_graph_captureILi1EE", 16384),
                     ("20k_graph_voxels_levelILi0EE", 0), ("20k_graph_voxels_levelILi1EE", 0),
                     ("22k_graph_uniform_insertE", 0), ("21k_graph_uniform_firstE", 0)):
        r = one(tag)
        print(f"{tag}: {r}")
        assert r["scratch"] == 0 and r["lds"] == lds


# ---------------------------------------------------------------------------- sanitizers

@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/sanitize_voxels_main.cpp: the host floods and FromPoints on the shell, L and hole
    recipes in one instrumented executable (no runtime is preloaded into anything)."""
    exe = tmp_path / "sanitize_voxels_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "sanitize_voxels_main.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sanitize ok" in r.stdout
    assert "runtime error" not in r.stderr
