"""Uniform (voxel) lighting graphs: UniformGraph (graph.h:195, graph.cpp:545-577), FitToGraph
(graph/util.h:302-311), FreeGraph::ToUniform's vertex part (graph.cpp:597-604) and
GraphIntegrator's uniform branch with --graph-debug's voxel view (graph_integrator.cpp:89-178).

CPU (not gpu): the coordinates and the hashed lookup against a numpy restatement written here
and a Python dict; the conversion from points against np.unique and a sequential float32 sum;
the file round trip; the first-lit-voxel search against a brute-force numpy IntersectP over
every lit voxel; argument errors; the Python surface; the kernels' resources; the host code
under ASan + UBSan as a stand-alone program (tests/sanitize_uniform_main.cpp).

GPU (gpu): device lookup and trace bitwise against the host; the render's samples replayed by
the oracle's graph walks on the read-back camera rays, count and L bitwise from the host
lookup; the voxel view bitwise from the host trace + lookup; the interface primitive; the
pipeline end to end; the state errors.
"""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
LIMIT = 1 << 20
SEED = 3
LIGHT_DIR = np.array([0.3, -0.5, 0.81], f32)


# ---------------------------------------------------------------------------- reference

def ref_coors(points, spacing):
    """FitToGraph: float32 division, then round half away from zero; (coors as float64, valid)."""
    with np.errstate(all="ignore"):
        q = (np.asarray(points, f32) / f32(spacing)).astype(f32)
        q64 = q.astype(np.float64)
        r = np.trunc(q64 + np.copysign(0.5, q64))
        valid = np.all(np.abs(r) < LIMIT, axis=-1)      # NaN compares false
    return r, valid


def ref_lookup(table, points, spacing):
    """(ids, light) from a dict {(cx, cy, cz): (id, light)}."""
    r, valid = ref_coors(points, spacing)
    ids = np.full(len(r), -1, np.int32)
    light = np.zeros(len(r), f32)
    for i in np.nonzero(valid)[0]:
        hit = table.get((int(r[i, 0]), int(r[i, 1]), int(r[i, 2])))
        if hit is not None:
            ids[i], light[i] = hit
    return ids, light


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ref_intersect(lo, hi, o, d):
    """Bounds3::IntersectP(o, d, Infinity, &hit0, &hit1) in float32 for boxes (m, 3) and one
    ray: (hit (m,), hit0, hit1), t0 from 0 and tFar widened by 1 + 2 gamma(3)."""
    eps = f32(5.96046448e-08)
    gamma3 = f32(f32(3) * eps) / f32(f32(1) - f32(3) * eps)
    widen = f32(f32(1) + f32(2) * gamma3)
    m = len(lo)
    t0 = np.zeros(m, f32)
    t1 = np.full(m, np.inf, f32)
    alive = np.ones(m, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = f32(1) / d[a]
            near = ((lo[:, a] - o[a]) * inv).astype(f32)
            far = ((hi[:, a] - o[a]) * inv).astype(f32)
            swap = near > far
            near, far = np.where(swap, far, near), np.where(swap, near, far)
            far = (far * widen).astype(f32)
            t0 = np.where(near > t0, near, t0)
            t1 = np.where(far < t1, far, t1)
            alive &= ~(t0 > t1)
    return alive, t0, t1


def ref_trace(coors, light, spacing, o, d):
    """The brute force over every lit voxel: (id, hit0, hit1, ambiguous) per ray; ties of hit0
    to the lower id."""
    s = f32(spacing)
    lit = np.nonzero(np.asarray(light, f32) != 0)[0]
    mid = (coors[lit].astype(f32) * s).astype(f32)
    half = f32(s / f32(2))
    lo, hi = (mid - half).astype(f32), (mid + half).astype(f32)
    n = len(o)
    ids = np.full(n, -1, np.int32)
    h0, h1 = np.zeros(n, f32), np.zeros(n, f32)
    amb = np.zeros(n, bool)
    for i in range(n):
        hit, t0, t1 = ref_intersect(lo, hi, o[i], d[i])
        k = np.nonzero(hit & (t0 < np.inf))[0]           # hit0 < minHit0 starts from Infinity
        if len(k) == 0:
            continue
        order = k[np.argsort(t0[k], kind="stable")]     # lit is ascending, so ties keep the lower id
        w = order[0]
        ids[i], h0[i], h1[i] = lit[w], t0[w], t1[w]
        tol = 1e-5 * max(1.0, float(t0[w]))
        gap = float(t0[order[1]]) - float(t0[w]) if len(order) > 1 else np.inf
        amb[i] = gap <= tol or float(t1[w]) - float(t0[w]) <= tol
    return ids, h0, h1, amb


# ---------------------------------------------------------------------------- inputs

_CASES = {}


def _lattice_graph():
    """Spacing 1/12: a random 2500 of the lattice points -3..15 per axis, random lights, and the
    extreme valid coordinates; the dict the lookups are checked against."""
    if "lattice" not in _CASES:
        rng = np.random.default_rng(5)
        allc = np.stack(np.meshgrid(*[np.arange(-3, 16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        coors = allc[rng.permutation(len(allc))[:2500]].astype(np.int32)
        coors = np.concatenate([coors, np.array([[LIMIT - 1, 0, 0], [0, -(LIMIT - 1), 2]], np.int32)])
        light = (rng.random(len(coors), dtype=f32) + f32(0.05)).astype(f32)
        table = {tuple(int(v) for v in c): (i, light[i]) for i, c in enumerate(coors)}
        _CASES["lattice"] = (coors, light, f32(1) / f32(12), table)
    return _CASES["lattice"]


def _lookup_queries():
    if "queries" not in _CASES:
        coors, light, s, _ = _lattice_graph()
        rng = np.random.default_rng(6)
        q = [(f32(-0.3) + f32(1.6) * rng.random((4000, 3), dtype=f32)).astype(f32)]
        k = np.arange(-9, 20).astype(f32)
        half = ((k + f32(0.5)) * s).astype(f32)                   # (k + 1/2) spacing, both signs
        q.append(np.stack([half, half[::-1], np.roll(half, 3)], axis=1))
        q.append((coors[-2:].astype(f32) * s).astype(f32))        # the extreme vertices' own points
        big = f32(LIMIT) * s
        q.append(np.array([[np.nan, 0.5, 0.5], [0.5, np.nan, 0.5], [0.5, 0.5, np.nan], [big, 0.5, 0.5], [-big, 0.5, 0.5],
                           [0.5, 2 * big, 0.5], [0.5, 0.5, -1e30], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5],
                           [-0.0, 0.0, -0.04]], f32))
        _CASES["queries"] = np.concatenate(q).astype(f32)
    return _CASES["queries"]


def _ball_graph(all_lit=False):
    """The voxel view's recipe: lattice points 0..12 per axis at spacing 1/12 whose centre is
    within 0.42 of (0.5, 0.5, 0.5), a random third dropped (default_rng(7)), some survivors dark."""
    key = "ball_lit" if all_lit else "ball"
    if key not in _CASES:
        s = f32(1) / f32(12)
        allc = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
        centre = (allc.astype(f32) * s).astype(f32)
        allc = allc[np.linalg.norm(centre.astype(np.float64) - 0.5, axis=1) <= 0.42]
        rng = np.random.default_rng(7)
        coors = allc[rng.random(len(allc)) >= 1 / 3]
        light = (rng.random(len(coors), dtype=f32) + f32(0.05)).astype(f32)
        if not all_lit:
            light[rng.random(len(coors)) < 0.12] = 0
        _CASES[key] = (np.ascontiguousarray(coors), light, s)
    return _CASES[key]


def _trace_rays():
    """4096 orthographic rays along +z from z = -1 and 4096 perspective rays from (0.5, 0.5, -1.5)."""
    if "rays" not in _CASES:
        rng = np.random.default_rng(9)
        o1 = np.concatenate([rng.random((4096, 2), dtype=f32), np.full((4096, 1), -1, f32)], axis=1)
        d1 = np.tile(np.array([0, 0, 1], f32), (4096, 1))
        target = np.concatenate([(f32(-0.1) + f32(1.2) * rng.random((4096, 2), dtype=f32)), np.full((4096, 1), 0.5, f32)], axis=1)
        o2 = np.tile(np.array([0.5, 0.5, -1.5], f32), (4096, 1))
        d2 = (target - o2).astype(f32)
        d2 = (d2 / np.linalg.norm(d2, axis=1)[:, None].astype(f32)).astype(f32)
        _CASES["rays"] = (np.concatenate([o1, o2]).astype(f32), np.concatenate([d1, d2]).astype(f32))
    return _CASES["rays"]


def _trace_reference():
    """The brute force for the ball graph and the rays, computed once."""
    if "trace_ref" not in _CASES:
        coors, light, s = _ball_graph()
        o, d = _trace_rays()
        _CASES["trace_ref"] = ref_trace(coors, light, s, o, d)
    return _CASES["trace_ref"]


# ---------------------------------------------------------------------------- CPU

def test_coordinates_and_lookup_match_numpy_and_a_dict():
    from acceleratedvolrenderer_amd import capi
    coors, light, s, table = _lattice_graph()
    q = _lookup_queries()
    u = capi.GraphUniform(coors, light, s)
    assert u.num_vertices == len(coors) and u.spacing == s
    assert np.array_equal(u.coors, coors) and same_bits(u.light_scalar, light)
    assert same_bits(u.points, (coors.astype(f32) * s).astype(f32))
    ids, got = u.lookup(q)
    rid, rlight = ref_lookup(table, q, s)
    assert np.array_equal(ids, rid) and same_bits(got, rlight)
    r, valid = ref_coors(q, s)
    print(f"{len(q)} queries: found {np.mean(rid >= 0):.3f}, invalid {np.sum(~valid)}, negative coordinates "
          f"{np.sum(valid & np.any(r < 0, axis=1))}")
    assert 0.2 < np.mean(rid >= 0) < 0.8 and np.sum(~valid) == 9 and np.sum(valid & np.any(r < 0, axis=1)) > 500
    assert np.all(ids[~valid] == -1) and np.all(got[~valid] == 0)
    assert ids[-12:-10].tolist() == [len(coors) - 2, len(coors) - 1]       # the extreme vertices are found
    # half-way points proper: at a power-of-two spacing (k + 1/2) spacing / spacing is k + 1/2 exactly
    k = np.arange(-6, 7)
    c2 = np.stack([k, k, k], axis=1).astype(np.int32)
    l2 = (np.arange(len(k)) + 1).astype(f32)
    u2 = capi.GraphUniform(c2, l2, 0.25)
    h = ((k.astype(f32) + f32(0.5)) * f32(0.25)).astype(f32)
    assert np.array_equal((h / f32(0.25)).astype(np.float64), k + 0.5)
    away = np.where(k >= 0, k + 1, k)                                      # half away from zero
    for sign in (1, -1):
        pts = np.stack([sign * h] * 3, axis=1).astype(f32)
        want = np.array([np.nonzero(k == v)[0][0] if v in k else -1 for v in (sign * away if sign > 0 else -away)])
        got_ids, got_l = u2.lookup(pts)
        assert np.array_equal(got_ids, want)
        assert np.array_equal(got_ids, ref_lookup({(int(v),) * 3: (i, l2[i]) for i, v in enumerate(k)}, pts, 0.25)[0])


def _points_case():
    if "points" not in _CASES:
        rng = np.random.default_rng(13)
        _CASES["points"] = (rng.random((4000, 3), dtype=f32), (rng.random(4000, dtype=f32) + f32(0.01)).astype(f32))
    return _CASES["points"]


@pytest.mark.parametrize("reduce", ["first", "mean"])
def test_from_points_matches_numpy(reduce):
    from acceleratedvolrenderer_amd import capi
    pts, light = _points_case()
    s = f32(0.08)
    u = capi.GraphUniform.from_points(pts, light, s, reduce=reduce)
    r, valid = ref_coors(pts, s)
    assert valid.all()
    c = r.astype(np.int64)
    keys = (c[:, 0] + LIMIT) | ((c[:, 1] + LIMIT) << 21) | ((c[:, 2] + LIMIT) << 42)
    uniq, first, inverse, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first)                 # new ids in the order of first appearance
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    vertex_of = rank[inverse]
    assert u.num_vertices == len(uniq)
    assert np.array_equal(u.vertex_of, vertex_of)
    assert np.array_equal(u.coors, c[first[order]])
    if reduce == "first":
        want = light[first[order]]
    else:
        total = np.zeros(len(uniq), f32)
        for i in range(len(pts)):             # the sequential float32 sum in ascending id
            total[vertex_of[i]] = f32(total[vertex_of[i]] + light[i])
        want = (total / counts[order].astype(f32)).astype(f32)
    assert same_bits(u.light_scalar, want)
    shared = np.mean(counts >= 2)
    print(f"{len(uniq)} voxels from 4000 vertices, {shared:.3f} of them hold two or more")
    assert shared > 0.5
    ids, l = u.lookup(pts)
    assert np.array_equal(ids, vertex_of) and same_bits(l, want[vertex_of])


def test_files_round_trip(tmp_path):
    from acceleratedvolrenderer_amd import capi, graph, graph_io
    coors, light, s, _ = _lattice_graph()
    light = light.copy()
    light[:5] = np.array([0.0, 1e-30, 3.4e38, 1 / 3, 2.5], f32)
    u = graph.UniformGraph(capi.GraphUniform(coors, light, s))
    path = str(tmp_path / "u.txt")
    u.save(path)
    head = open(path).read().split("\n")[:5]
    assert head[0] == "basic" and head[1] == "uniform %.9g" % float(s) and head[2] == "True False False True False"
    assert head[3] == f"{len(coors)} 0 0 {len(coors)} 0 0"
    assert head[4].endswith(" %d %d %d " % tuple(coors[0])) and len(head[4].split()) == 8
    g = graph_io.read_graph(path)
    assert g.kind == "uniform" and g.spacing == s and g.radius is None
    assert np.array_equal(g.coors, coors) and same_bits(g.light_scalar, light) and same_bits(g.points, u.points)
    assert graph_io.read_kind(path) == "uniform"
    back = graph.load_uniform(path)
    assert back.spacing == s and np.array_equal(back.coors, coors) and same_bits(back.light_scalar, light)
    graph_io.write_uniform_graph(str(tmp_path / "u6.txt"), u, precision=6)        # the reference's own precision
    g6 = graph.load_uniform(str(tmp_path / "u6.txt"))
    assert np.array_equal(g6.coors, coors) and np.allclose(g6.light_scalar, light, rtol=1e-5)
    # two vertices in one voxel: the first in file order stays (the coors column is not the key)
    edited = tmp_path / "two.txt"
    edited.write_text("basic\nuniform 0.25\nTrue False False True False\n3 0 0 3 0 0\n"
                      "1 0.26 0.5 0.75 7 9 9 9 \n0 0.25 0.5 0.75 5 1 2 3 \n2 1 1 1 6 4 4 4 \n")
    two = graph.load_uniform(str(edited))
    assert two.num_vertices == 2 and two.coors.tolist() == [[1, 2, 3], [4, 4, 4]] and two.light_scalar.tolist() == [7, 6]
    # a free graph, and a file without lighting
    free = os.path.join(ROOT, "tests", "golden", "graph_free_small.txt")
    assert graph_io.read_kind(free) == "free"
    with pytest.raises(ValueError, match="free graph"):
        graph.load_uniform(free)
    dark = tmp_path / "dark.txt"
    dark.write_text("basic\nuniform 0.25\nTrue False False False False\n1 0 0 1 0 0\n0 0.25 0.5 0.75 1 2 3 \n")
    with pytest.raises(ValueError, match="without lighting"):
        graph.load_uniform(str(dark))
    with pytest.raises(ValueError, match="uniform graph"):
        graph.load_index(path)


def test_trace_matches_the_brute_force():
    from acceleratedvolrenderer_amd import capi
    coors, light, s = _ball_graph()
    o, d = _trace_rays()
    rid, r0, r1, amb = _trace_reference()
    u = capi.GraphUniform(coors, light, s)
    ids, h0, h1 = u.trace(o, d)
    hit = rid >= 0
    print(f"{len(coors)} voxels, {np.sum(light == 0)} dark; {hit.sum()} of {len(o)} rays hit "
          f"(orthographic {hit[:4096].sum()}, perspective {hit[4096:].sum()}), ambiguous {amb.sum()}")
    assert np.sum(light == 0) > 20 and hit[:4096].sum() > 1000 and hit[4096:].sum() > 1000
    assert amb.mean() <= 0.005
    ok = ~amb
    assert np.array_equal(ids[ok], rid[ok])
    assert same_bits(h0[ok], r0[ok]) and same_bits(h1[ok], r1[ok])
    assert np.all(light[ids[ids >= 0]] != 0)                      # a dark voxel is never the answer
    # rays that start inside the bounds, run backwards, or have no direction
    inside = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.52, 0.47, 0.9], [0.5, 0.5, 2.0]], f32)
    dirs = np.array([[0.6, 0.0, 0.8], [0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]], f32)
    gi, g0, g1 = u.trace(inside, dirs)
    bi, b0, b1, bamb = ref_trace(coors, light, s, inside, dirs)
    assert not bamb.any() and np.array_equal(gi, bi) and same_bits(g0, b0) and same_bits(g1, b1)
    assert gi[3] == -1 and gi[2] >= 0


def test_argument_errors():
    import ctypes
    from acceleratedvolrenderer_amd import capi
    lib = capi.load()
    c = np.array([[0, 0, 0], [1, 2, 3]], np.int32)
    l = np.array([1.0, 2.0], f32)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(RuntimeError, match="avr error 1.*spacing"):
            capi.GraphUniform(c, l, bad)
        with pytest.raises(RuntimeError, match="avr error 1.*spacing"):
            capi.GraphUniform.from_points(c.astype(f32), l, bad)
    with pytest.raises(RuntimeError, match="avr error 1.*at least one vertex"):
        capi.GraphUniform(np.zeros((0, 3), np.int32), np.zeros(0, f32), 0.1)
    with pytest.raises(RuntimeError, match="avr error 1.*at least one vertex"):
        capi.GraphUniform.from_points(np.zeros((0, 3), f32), np.zeros(0, f32), 0.1)
    for v in (LIMIT, -LIMIT, 2 ** 40):
        with pytest.raises(RuntimeError, match=r"avr error 1.*vertex 1: coordinate outside"):
            capi.GraphUniform(np.array([[0, 0, 0], [1, v, 3]], np.int64), l, 0.1)
    capi.GraphUniform(np.array([[0, 0, 0], [1, LIMIT - 1, 1 - LIMIT]], np.int64), l, 0.1).close()
    with pytest.raises(RuntimeError, match="avr error 1.*vertex 1: NaN light"):
        capi.GraphUniform(c, np.array([1.0, np.nan], f32), 0.1)
    with pytest.raises(RuntimeError, match="avr error 1.*vertex 1: repeated coordinate"):
        capi.GraphUniform(np.array([[1, 2, 3], [1, 2, 3]], np.int32), l, 0.1)
    with pytest.raises(ValueError):
        capi.GraphUniform(c, l[:1], 0.1)
    with pytest.raises(ValueError, match="integer"):
        capi.GraphUniform(c.astype(f32), l, 0.1)
    for bad in (np.nan, np.inf, 0.1 * LIMIT):
        with pytest.raises(RuntimeError, match="avr error 1.*vertex 1: coordinate outside"):
            capi.GraphUniform.from_points(np.array([[0, 0, 0], [0, bad, 0]], f32), l, 0.1)
    with pytest.raises(RuntimeError, match="avr error 1.*vertex 0: NaN light"):
        capi.GraphUniform.from_points(c.astype(f32), np.array([np.nan, 1.0], f32), 0.1)
    with pytest.raises(ValueError, match="first.*mean"):
        capi.GraphUniform.from_points(c.astype(f32), l, 0.1, reduce="max")
    h = ctypes.c_void_p()
    pf = c.astype(f32)
    fp = lambda a: a.ctypes.data_as(capi.c_float_p)
    ip = lambda a: a.ctypes.data_as(capi.c_int_p)
    assert lib.avr_graph_uniform_from_points(2, fp(pf), fp(l), 0.1, 2, None, ctypes.byref(h)) == 1
    assert b"reduce" in lib.avr_last_error() and not h.value
    assert lib.avr_graph_uniform_from_points(2, fp(pf), fp(l), 0.1, 0, None, None) == 1
    assert lib.avr_graph_uniform_create(2, ip(c), fp(l), 0.1, None) == 1
    assert lib.avr_graph_uniform_create(2, None, fp(l), 0.1, ctypes.byref(h)) == 1 and not h.value
    u = capi.GraphUniform(c, l, 0.1)
    ids, out = np.zeros(2, np.int32), np.zeros(2, f32)
    assert lib.avr_graph_uniform_size(None, None, None) == 1 and lib.avr_graph_uniform_get(None, None, None) == 1
    assert lib.avr_graph_uniform_lookup(None, 2, fp(pf), ip(ids), fp(out)) == 1
    assert lib.avr_graph_uniform_lookup(u.h, -1, fp(pf), ip(ids), fp(out)) == 1
    assert lib.avr_graph_uniform_lookup(u.h, 2, None, ip(ids), fp(out)) == 1 and b"null buffer" in lib.avr_last_error()
    assert lib.avr_graph_uniform_lookup(u.h, 0, None, None, None) == 0
    assert lib.avr_graph_uniform_trace(None, 2, fp(pf), fp(pf), ip(ids), fp(out), fp(out)) == 1
    assert lib.avr_graph_uniform_trace(u.h, 2, fp(pf), None, ip(ids), fp(out), fp(out)) == 1
    assert lib.avr_graph_uniform_trace(u.h, 2, fp(pf), fp(pf), None, None, None) == 0     # any output may be null
    with pytest.raises(ValueError, match="one direction per origin"):
        u.trace(pf, pf[:1])
    # the device entry points refuse a null context before they touch a GPU
    assert lib.avr_graph_uniform_lookup_device(None, u.h, 2, fp(pf), ip(ids), fp(out)) == 1
    assert lib.avr_graph_uniform_trace_device(None, u.h, 2, fp(pf), fp(pf), ip(ids), fp(out), fp(out)) == 1
    assert lib.avr_graph_render_uniform(None, u.h, None, 0, 1, 0, 0, 1.0) == 1
    assert b"null context or uniform graph" in lib.avr_last_error()
    assert lib.avr_graph_uniform_destroy(None) == 0


class _StubContext:
    """Stands in for capi.Context where only the Python side is under test."""
    calls = []

    def __init__(self, device=0, max_paths=0):
        pass

    def set_scene(self, scene):
        pass

    def set_graph_geometry(self, primitive):
        pass

    def graph_render(self, index, *a, **kw):
        self.calls.append(("free", index, a, kw))

    def graph_render_uniform(self, uniform, *a, **kw):
        self.calls.append(("uniform", uniform, a, kw))

    def close(self):
        pass


def test_python_surface_without_a_gpu(tmp_path, monkeypatch):
    import acceleratedvolrenderer_amd as avr
    from acceleratedvolrenderer_amd import capi, graph, integrator
    assert avr.GraphUniform is capi.GraphUniform
    assert integrator.INTEGRATOR_NAMES == ("volpath", "volpathcustom", "volpath_mi355x")
    params = inspect.signature(graph.GraphIntegrator.__init__).parameters
    assert params["voxel_view"].default is False and params["light_scale"].default is None
    assert capi.INV_4PI == float(f32(1 / (4 * np.pi)))
    coors, light, s = _ball_graph()
    u = capi.GraphUniform(coors, light, s)
    with pytest.raises(ValueError, match="GBufferFilm"):
        graph.GraphIntegrator(_graph_scene(gbuffer=True), u)
    monkeypatch.setattr(capi, "Context", _StubContext)
    _StubContext.calls.clear()
    scene = _graph_scene()
    integ = graph.GraphIntegrator(scene, u, spp=2, seed=SEED)
    assert integ.index is u and integ.light_scale == capi.INV_4PI and integ.voxel_view is False
    integ._render_range(0, 2)
    wrapped = graph.GraphIntegrator(scene, graph.UniformGraph(u), voxel_view=True, light_scale=1)
    assert wrapped.index is u
    wrapped._render_range(1, 2)
    # from_file dispatches on the file's kind
    graph.UniformGraph(u).save(str(tmp_path / "u.txt"))
    from_u = graph.GraphIntegrator.from_file(scene, str(tmp_path / "u.txt"), spp=1)
    assert isinstance(from_u.index, capi.GraphUniform) and np.array_equal(from_u.index.coors, coors)
    from_f = graph.GraphIntegrator.from_file(scene, os.path.join(ROOT, "tests", "golden", "graph_free_small.txt"))
    assert isinstance(from_f.index, capi.GraphIndex)
    from_f._render_range(0, 1)
    kinds = [(c[0], c[3]) for c in _StubContext.calls]
    assert kinds == [("uniform", dict(view=0, light_scale=capi.INV_4PI)), ("uniform", dict(view=1, light_scale=1.0)),
                     ("free", {})]
    # the conversion of a free graph's vertices
    pts, l = _points_case()

    class _Free(graph.FreeGraph):
        def __init__(self):
            self.points = pts
    ug = _Free().to_uniform(0.08, l, reduce="mean")
    assert isinstance(ug, graph.UniformGraph) and ug.table.num_vertices == ug.num_vertices == len(ug.light_scalar)
    assert len(ug.vertex_of) == len(pts) and ug.spacing == f32(0.08)


def test_tools_take_the_uniform_options():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import graph_maker
        import graph_render_demo
        a = graph_maker.parser().parse_args(["--out", "x", "--uniform", "0.02", "--uniform-reduce", "mean"])
        none = graph_maker.parser().parse_args(["--out", "x"])
        b = graph_render_demo.parser().parse_args(["--uniform", "1r", "--voxel-view"])
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    assert a.uniform == 0.02 and a.uniform_reduce == "mean" and none.uniform is None and none.uniform_reduce == "first"
    assert b.uniform == "1r" and b.voxel_view
    assert graph_render_demo.uniform_spacing("2r", f32(0.0125)) == float(f32(0.025))
    assert graph_render_demo.uniform_spacing("0.03", f32(0.0125)) == 0.03


# ---------------------------------------------------------------------------- resources

def _kernel_resources(tmp, geom):
    from acceleratedvolrenderer_amd import build as avr_build
    inst = []
    for z in ("false", "true"):
        inst.append(f"template __global__ void k_graph_render<{z}, {geom}>(Params, graph::IndexView, Xf, float4 *);")
        for view in (0, 1):
            inst.append(f"template __global__ void k_graph_render_uniform<{z}, {geom}, {view}>(Params, graph::UniformView, "
                        "Xf, float, float4 *);")
    src = tmp / f"uniform_g{geom}.hip"
    src.write_text('#define AVR_KPATHS_TU\n#include "avr_kernels.hip"\n#include "avr_graph.hip"\n'
                   "namespace avr {\n" + "\n".join(inst) + "\n}\n")
    cmd = ([avr_build.HIPCC] + avr_build.FLAGS +
           ["-I" + avr_build.CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
            "-c", str(src), "-o", str(tmp / f"uniform_g{geom}.o")])
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """The graph kernels alone, cross-compiled for gfx950 with the build's flags, one translation
    unit per geometry (side by side); {mangled name: figures} from the
    -Rpass-analysis=kernel-resource-usage remarks, as tests/test_graph_interface.py reads them."""
    from acceleratedvolrenderer_amd import build as avr_build
    if not os.path.exists(avr_build.HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("uniform_resources")
    procs = [_kernel_resources(tmp, g) for g in (0, 1)]
    out = {}
    for p in procs:
        _, log = p.communicate()
        assert p.returncode == 0, log[-2000:]
        for block in log.split("Function Name: ")[1:]:
            name = block.split()[0]
            out[name] = {key: int(re.search(pat, block).group(1)) for key, pat in (
                ("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))}
    return out


def test_uniform_kernel_resources(resources):
    """No scratch anywhere; every k_graph_render_uniform instantiation runs at least as many
    waves/SIMD as k_graph_render with the same sampler and geometry; no connect buffer in LDS
    (the majorant staging alone for view 0, nothing for view 1)."""
    def one(tag):
        match = [v for k, v in resources.items() if tag in k]
        assert len(match) == 1, tag
        return match[0]
    seen = 0
    for geom in (0, 1):
        for z in (0, 1):
            free = one(f"14k_graph_renderILb{z}ELi{geom}EE")
            for view in (0, 1):
                r = one(f"22k_graph_render_uniformILb{z}ELi{geom}ELi{view}EE")
                print(f"k_graph_render_uniform<{bool(z)}, {geom}, {view}>: {r}; k_graph_render: {free}")
                assert r["scratch"] == 0 and r["occ"] >= free["occ"]
                assert r["lds"] == (16384 if view == 0 else 0)
                seen += 1
    assert seen == 8
    for kernel in ("k_graph_uniform_lookup", "k_graph_uniform_trace"):
        r = one(f"{len(kernel)}{kernel}E")
        print(f"{kernel}: {r}")
        assert r["scratch"] == 0 and r["lds"] == 0


# ---------------------------------------------------------------------------- sanitizers

@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/sanitize_uniform_main.cpp: create, from_points, lookup and trace on this file's
    recipes in one instrumented executable (no runtime is preloaded into anything)."""
    exe = tmp_path / "sanitize_uniform_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "sanitize_uniform_main.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sanitize ok" in r.stdout
    assert "runtime error" not in r.stderr


# ---------------------------------------------------------------------------- GPU

def _graph_scene(shape=(12, 12, 12), seed=5, sampler=0, one_light=True, gbuffer=False, sphere=False, spp=4):
    """tests/test_graph_render.py's _graph_scene recipe (gray GridMedium, 16x16 film), with the
    distant light alone (the graph render takes exactly one) unless one_light is False."""
    from acceleratedvolrenderer_amd import scenes, GridMedium, GBufferFilm, IndependentSampler, ZSobolSampler
    from acceleratedvolrenderer_amd.scene import Scene
    base = scenes.s_uniform(n=2, width=16, height=16, variant="scatter")
    dens = (0.2 + 0.8 * np.random.default_rng(seed).random(shape, dtype=np.float32)).astype(np.float32)
    med = GridMedium(dens, sigma_a=0.4, sigma_s=6.0, g=0.5)
    film = GBufferFilm(16, 16) if gbuffer else base.film
    smp = (ZSobolSampler if sampler else IndependentSampler)(pixelsamples=spp)
    return Scene(base.camera, film, med, base.lights[:1] if one_light else base.lights, sampler=smp,
                 interface_sphere=((0.5, 0.5, 0.5), 0.45) if sphere else None)


def _render_offset(scene):
    """Render space is world space moved by this translation (CameraWorld)."""
    m = np.asarray(scene.render_from_world, np.float64)
    assert np.array_equal(m[:3, :3], np.eye(3))
    return m[:3, 3]


def _render_graph(scene):
    """The render tests' graph, in render space at spacing 0.08: a random 60 % of the lattice
    points over the medium's box (a scatter point finds a vertex or does not, both often),
    random positive lights."""
    if "render" not in _CASES:
        rng = np.random.default_rng(21)
        first = np.floor(_render_offset(scene) / 0.08).astype(np.int64) - 1
        allc = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + first
        coors = np.ascontiguousarray(allc[rng.random(len(allc)) < 0.6].astype(np.int32))
        light = (rng.random(len(coors), dtype=f32) + f32(0.05)).astype(f32)
        _CASES["render"] = (coors, light, f32(0.08))
    return _CASES["render"]


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def rendered(gpu):
    """Per (grid shape, sampler): the scene and the two renders of sample indices [0, 4) from the
    render graph, in passes of 3 + 1 samples and in one pass."""
    from acceleratedvolrenderer_amd import GraphIntegrator, capi
    coors, light, s = _render_graph(_graph_scene())
    uni = capi.GraphUniform(coors, light, s)
    out = {}
    for shape in ((12, 12, 12), (9, 12, 5)):
        for kind in (0, 1):
            scene = _graph_scene(shape, sampler=kind)
            split = GraphIntegrator(scene, uni, spp=4, seed=SEED, max_paths=3 * 256)
            rgb_s, w_s = split.render()
            last_s = split.last_pass()
            whole = GraphIntegrator(scene, uni, spp=4, seed=SEED)
            rgb_w, w_w = whole.render()
            out[shape, kind] = dict(scene=scene, uniform=uni, split=split, whole=whole, rgb_split=rgb_s, w_split=w_s,
                                    last_split=last_s, rgb=rgb_w, w=w_w, last=whole.last_pass())
    yield out
    for r in out.values():
        r["split"].close()
        r["whole"].close()


@pytest.mark.gpu
def test_device_lookup_and_trace_match_the_host(gpu):
    from acceleratedvolrenderer_amd import capi
    coors, light, s, _ = _lattice_graph()
    q = _lookup_queries()
    u = capi.GraphUniform(coors, light, s)
    bc, bl, bs = _ball_graph()
    ball = capi.GraphUniform(bc, bl, bs)
    o, d = _trace_rays()
    ctx = capi.Context(0)
    try:
        ids, l = ctx.graph_uniform_lookup(u, q)
        # a second object at once: the cached device copy must follow the object, not its address
        t_ids, t0, t1 = ctx.graph_uniform_trace(ball, o, d)
        b_ids, b_l = ctx.graph_uniform_lookup(ball, q)
        again_ids, again_l = ctx.graph_uniform_lookup(u, q)
    finally:
        ctx.close()
    h_ids, h_l = u.lookup(q)
    assert np.array_equal(ids, h_ids) and same_bits(l, h_l)
    assert np.array_equal(again_ids, h_ids) and same_bits(again_l, h_l)
    hb_ids, hb_l = ball.lookup(q)
    assert np.array_equal(b_ids, hb_ids) and same_bits(b_l, hb_l) and not np.array_equal(b_ids, h_ids)
    ht_ids, ht0, ht1 = ball.trace(o, d)
    assert np.array_equal(t_ids, ht_ids) and same_bits(t0, ht0) and same_bits(t1, ht1)
    assert np.sum(t_ids >= 0) > 2000 and np.sum(ids >= 0) > 1000


def _light_spectrum(scene, lam):
    """lightSpectrum.Sample(lambda): DistantLight's scale * Lemit at lround(lambda) (DenselySampled)."""
    off = np.floor(lam.astype(np.float64) + 0.5).astype(np.int64) - 360
    table = np.asarray(scene.light_L[0], f32)
    val = np.where((off >= 0) & (off < len(table)), table[np.clip(off, 0, len(table) - 1)], f32(0)).astype(f32)
    return (val * f32(scene.light_scale[0])).astype(f32)


def _start_rays(md, lp):
    """Where each sample's walk starts (graph_camera_start): (rows that hit the primitive, ro,
    tMax), by the box model's host mirror."""
    rows, ro, tmax = [], [], []
    for i in range(len(lp["o"])):
        ty, t0, t1 = md.box_hits(lp["o"][i], lp["d"][i])
        if ty == 2:
            continue
        oo = lp["o"][i]
        if ty == 0:
            oo = (oo + (lp["d"][i] * t0).astype(f32)).astype(f32)
            t = f32(t1 - t0)
        else:
            t = t0
        rows.append(i); ro.append(oo); tmax.append(t)
    return np.array(rows), np.array(ro, f32), np.array(tmax, f32)


def _replay(r, lp, sampler_kind, light_scale):
    """Check one pass (lp = GraphIntegrator.last_pass()) sample by sample; returns (scattered,
    found) per sample."""
    from acceleratedvolrenderer_amd import graph
    from oracle import binding
    scene = r["scene"]
    W, H = scene.film.width, scene.film.height
    npix = W * H
    md = graph.MediumData(scene)
    run = binding.OracleRun(scene, seed=SEED, libm="canonical")
    n = npix * lp["samples"]
    assert len(lp["o"]) == len(lp["L"]) == n
    rows, ro, tmax = _start_rays(md, lp)
    scat_o = np.zeros(n, bool)
    pts_o = np.zeros((n, 3), f32)
    for s in range(lp["samples"]):
        sel = (rows >= s * npix) & (rows < (s + 1) * npix)
        assert sel.sum() > npix // 2
        pts, cnt = run.graph_walks(ro[sel], lp["d"][rows[sel]], tmax[sel], (rows[sel] - s * npix).astype(np.int64), 1,
                                   lp["first"] + s, W, 1, skip_dims=6,
                                   sampler=(sampler_kind, SEED, scene.sampler.pixelsamples, W, H))
        scat_o[rows[sel]] = cnt == 1
        pts_o[rows[sel]] = pts[:, 0]
    scat = lp["count"] >= 0
    # scatter or not, and the point, bit-identical for every sample
    assert np.array_equal(scat, scat_o)
    assert same_bits(lp["p"][scat], pts_o[scat])
    assert np.all(lp["p"][~scat] == 0)
    # count and L against the host lookup at the read-back point (identity graph_from_render)
    ids, light = r["uniform"].lookup(lp["p"][scat])
    assert np.array_equal(lp["count"][scat], (ids >= 0).astype(np.int32))
    spec = _light_spectrum(scene, lp["lam"])
    want = np.zeros((n, 4), f32)
    want[scat] = ((spec[scat] * light[:, None]).astype(f32) * f32(light_scale)).astype(f32)
    want[np.nonzero(scat)[0][ids < 0]] = 0
    assert same_bits(lp["L"], want)
    assert np.all(spec > 0)
    found = np.zeros(n, bool)
    found[scat] = ids >= 0
    return scat, found


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
@pytest.mark.parametrize("shape", [(12, 12, 12), (9, 12, 5)], ids=["12x12x12", "5x12x9"])
def test_render_replays_oracle_walks(rendered, shape, kind):
    from acceleratedvolrenderer_amd import capi
    r = rendered[shape, kind]
    # the split render's last pass is the 1-sample pass of sample index 3
    assert (r["last_split"]["first"], r["last_split"]["samples"]) == (3, 1)
    assert (r["last"]["first"], r["last"]["samples"]) == (0, 4)
    _replay(r, r["last_split"], kind, capi.INV_4PI)
    scat, found = _replay(r, r["last"], kind, capi.INV_4PI)
    # the split render's pass holds the same samples as the one-pass render's last quarter
    for key in ("L", "lam", "o", "d", "p", "count"):
        a, b = r["last_split"][key], r["last"][key][3 * 256:]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), key
    print(f"{shape} sampler {kind}: scattered {scat.mean():.3f}, of those a vertex found {found[scat].mean():.3f}")
    assert scat.mean() >= 0.5
    assert 0.25 <= found[scat].mean() < 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
def test_film(rendered, kind):
    from acceleratedvolrenderer_amd import GraphIntegrator, capi
    r = rendered[(12, 12, 12), kind]
    scene = r["scene"]
    # passes of 3 + 1 samples add up to the one-pass film
    assert np.array_equal(r["rgb"], r["rgb_split"]) and np.array_equal(r["w"], r["w_split"]) and np.all(r["w"] == 4)
    # zero exactly where every sample's L is zero, positive elsewhere
    L = r["last"]["L"].reshape(4, 256, 4)
    lit = np.any((L > 0).any(axis=2), axis=0)
    rgb = r["rgb"].reshape(256, 3)
    assert 0 < lit.sum() <= 256
    assert np.all(rgb[~lit] == 0) and np.all(rgb[lit] > 0)
    # light scalars x 2 -> film x 2, exactly; light_scale 1 against Inv4Pi: not the same film
    coors, light, s = _render_graph(scene)
    twice = GraphIntegrator(scene, capi.GraphUniform(coors, (light * f32(2)).astype(f32), s), spp=4, seed=SEED)
    rgb2, _ = twice.render()
    # [0, 4) in one call == [0, 2) then [2, 4)
    twice.index = r["uniform"]
    twice.render(0, 2)
    rgb_ab, w_ab = twice.render(2, 4, clear=False)
    twice.light_scale = 1.0
    rgb_one, _ = twice.render()
    one_pass = twice.last_pass()
    twice.close()
    assert np.array_equal(rgb2, 2.0 * r["rgb"])
    assert np.array_equal(rgb_ab, r["rgb"]) and np.array_equal(w_ab, r["w"])
    _replay(r, one_pass, kind, 1.0)
    assert rgb_one.sum() > 10 * r["rgb"].sum()


def _xf(m, v, point):
    """Transform::operator() on (n, 3) points or vectors in float32, sums left to right (xf_point_lr,
    xf_vector); m None: the identity."""
    m = np.eye(4, dtype=f32) if m is None else np.asarray(m, f32).reshape(4, 4)
    out = np.zeros_like(v)
    for r in range(3):
        acc = (m[r, 0] * v[:, 0]).astype(f32)
        acc = (acc + (m[r, 1] * v[:, 1]).astype(f32)).astype(f32)
        acc = (acc + (m[r, 2] * v[:, 2]).astype(f32)).astype(f32)
        out[:, r] = (acc + m[r, 3]).astype(f32) if point else acc
    return out


def _voxel_view_check(integ, uni, m):
    """One voxel-view pass against the host: rays from the read-back camera records, mapped by
    the translation m (None: identity), trace + lookup at the chord's middle."""
    from acceleratedvolrenderer_amd import graph
    lp = integ.last_pass()
    n = len(lp["o"])
    rows, ro, _ = _start_rays(graph.MediumData(integ.scene), lp)
    og, dg = _xf(m, ro, True), _xf(m, lp["d"][rows], False)
    ids, h0, h1 = uni.trace(og, dg)
    hit = ids >= 0
    tm = ((h0 + h1).astype(f32) / f32(2)).astype(f32)
    middle = (og + (dg * tm[:, None]).astype(f32)).astype(f32)
    mid_ids, mid_light = uni.lookup(middle)
    count = np.full(n, -1, np.int32)
    count[rows[hit]] = (mid_ids[hit] >= 0).astype(np.int32)
    p = np.zeros((n, 3), f32)
    p[rows[hit]] = middle[hit]
    spec = _light_spectrum(integ.scene, lp["lam"])
    want = np.zeros((n, 4), f32)
    sel = rows[hit & (mid_ids >= 0)]
    want[sel] = (spec[sel] * mid_light[hit & (mid_ids >= 0)][:, None]).astype(f32)
    assert np.array_equal(lp["count"], count)
    assert same_bits(lp["p"], p)
    assert same_bits(lp["L"], want)
    return lp, rows, hit, ids


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
def test_voxel_view(gpu, kind):
    from acceleratedvolrenderer_amd import GraphIntegrator, capi
    coors, light, s = _ball_graph()
    uni = capi.GraphUniform(coors, light, s)
    scene = _graph_scene(sampler=kind)
    m = np.eye(4, dtype=f32)
    m[:3, 3] = -_render_offset(scene)        # the ball graph is in world space: graph_from_render = world_from_render
    integ = GraphIntegrator(scene, uni, spp=4, seed=SEED, voxel_view=True, max_paths=3 * 256, graph_from_render=m)
    rgb_split, w = integ.render()
    lp, rows, hit, ids = _voxel_view_check(integ, uni, m)
    assert (lp["first"], lp["samples"]) == (3, 1)
    integ.close()
    whole = GraphIntegrator(scene, uni, spp=4, seed=SEED, voxel_view=True, graph_from_render=m,
                            light_scale=123.0)                                                  # light_scale plays no part
    rgb, _ = whole.render()
    lp, rows, hit, ids = _voxel_view_check(whole, uni, m)
    whole.close()
    print(f"sampler {kind}: {len(rows)} of {len(lp['o'])} rays cross the primitive, {hit.sum()} hit a lit voxel, "
          f"{np.sum(lp['count'] == 1)} find a vertex at the middle")
    assert np.array_equal(rgb, rgb_split) and rgb.sum() > 0
    assert hit.mean() > 0.3 and np.sum(lp["count"] == 1) > 0.9 * hit.sum() and np.all(light[ids[hit]] != 0)


@pytest.mark.gpu
def test_voxel_view_with_a_translated_graph(gpu):
    """The voxel view through a graph_from_render translation, and graph and translation moved
    together: the medium sits in [1.25, 1.75]^3 of render space, the spacing is 1/16 and the
    translation a multiple of 1/8 that keeps every coordinate's binade or lowers it, so each
    translated coordinate is exact in float, the lattice coordinates move by whole numbers and
    the box differences lo - o, hi - o, hence hit0 and hit1, are the same bits."""
    from acceleratedvolrenderer_amd import GraphIntegrator, GridMedium, DistantLight, OrthographicCamera, RGBFilm, capi
    from acceleratedvolrenderer_amd.scene import Scene
    rng = np.random.default_rng(8)
    dens = (0.2 + 0.8 * rng.random((7, 6, 5), dtype=f32)).astype(f32)
    med = GridMedium(dens, p0=(1.25, 1.25, 1.25), p1=(1.75, 1.75, 1.75), sigma_a=0.4, sigma_s=12.0, g=0.5)
    cam = OrthographicCamera(pos=(0.0, 0.0, 0.0), look=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0),
                             screenwindow=(1.25, 1.75, 1.25, 1.75))
    scene = Scene(cam, RGBFilm(16, 16), med, [DistantLight(from_=(-1.0, 1.0, -1.0), to=(0.0, 0.0, 0.0), scale=2.0)])
    assert np.array_equal(np.asarray(scene.render_from_world), np.eye(4))
    s = f32(1) / f32(16)
    allc = np.stack(np.meshgrid(*[np.arange(20, 29)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    centre = allc.astype(np.float64) / 16
    keep = (np.linalg.norm(centre - 1.5, axis=1) <= 0.24) & (rng.random(len(allc)) < 0.7)
    coors = np.ascontiguousarray(allc[keep])
    light = (rng.random(len(coors), dtype=f32) + f32(0.1)).astype(f32)
    t = np.array([0.125, -0.25, 0.25], f32)
    shift = np.array([2, -4, 4], np.int32)
    m = np.eye(4, dtype=f32)
    m[:3, 3] = t
    ua, ub = capi.GraphUniform(coors, light, s), capi.GraphUniform(coors + shift, light, s)
    a = GraphIntegrator(scene, ua, spp=2, seed=SEED, voxel_view=True)
    b = GraphIntegrator(scene, ub, spp=2, seed=SEED, voxel_view=True, graph_from_render=m)
    rgb_a, _ = a.render()
    rgb_b, _ = b.render()
    la, rows, hit_a, ids_a = _voxel_view_check(a, ua, None)
    lb, _, hit_b, ids_b = _voxel_view_check(b, ub, m)
    a.close(); b.close()
    print(f"{len(coors)} voxels, {hit_a.sum()} of {len(rows)} rays hit one")
    assert hit_a.mean() > 0.3
    assert np.array_equal(ids_a, ids_b) and np.array_equal(la["count"], lb["count"])
    assert same_bits(la["L"], lb["L"]) and np.array_equal(rgb_a, rgb_b) and rgb_a.sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
def test_interface_primitive(gpu, kind):
    from acceleratedvolrenderer_amd import GraphIntegrator, capi
    scene = _graph_scene(sampler=kind, sphere=True)
    coors, light, s = _render_graph(scene)
    uni = capi.GraphUniform(coors, light, s)
    integ = GraphIntegrator(scene, uni, spp=4, seed=SEED, primitive="interface", light_scale=0.5)
    rgb, w = integ.render()
    lp = integ.last_pass()
    integ.close()
    scat = lp["count"] >= 0
    dist = np.linalg.norm(lp["p"][scat].astype(np.float64) - (0.5 + _render_offset(scene)), axis=1)
    print(f"sampler {kind}: scattered {scat.mean():.3f}, farthest scatter point {dist.max():.5f} of 0.45")
    assert scat.mean() > 0.3 and np.all(dist <= 0.45 * (1 + 1e-4))
    ids, l = uni.lookup(lp["p"][scat])
    assert np.array_equal(lp["count"][scat], (ids >= 0).astype(np.int32)) and 0 < np.mean(ids >= 0) < 1
    spec = _light_spectrum(scene, lp["lam"])
    want = np.zeros((len(scat), 4), f32)
    want[scat] = ((spec[scat] * l[:, None]).astype(f32) * f32(0.5)).astype(f32)
    assert same_bits(lp["L"], want)
    assert np.all(np.isfinite(rgb)) and rgb.sum() > 0


@pytest.mark.gpu
def test_pipeline_end_to_end(gpu):
    """build_graph -> compute_final_light -> to_uniform(spacing = 2 x vertex radius, "mean") ->
    render with light_scale=1, against the free-graph render of the same lit graph: a sanity
    bound (the factor of 3 on the image mean that the free pipeline test uses against
    VolPathIntegrator), not parity: a voxel answers only where one of its own vertices lies,
    the free render also from neighbours within the search ranges. Measured on an MI355X:
    ratio 0.931 (image means 0.1260 uniform, 0.1353 free; 186 vertices in 108 voxels of 0.2078;
    87.5 % of the last pass's scatters find a vertex)."""
    from acceleratedvolrenderer_amd import GraphIntegrator, graph
    scene = _graph_scene(spp=16)
    bounces = 6
    integ = GraphIntegrator(scene, None, spp=16, seed=SEED)
    cfg = graph.GraphBuilderConfig(radius_modifier=60.0, max_depth=12, dimension_steps=8, iterations_per_step=6,
                                   render_search_range={"active": True, "neighboursToUse": 4})
    in_dir = (-np.asarray(scene.light_w[0], f32)).astype(f32)      # the way the light travels
    smp = graph.GraphSampling(sampler=0, seed=SEED, samples_per_pixel=16, resolution=(64, 64))
    md = graph.MediumData(scene)
    g = graph.FreeGraphBuilder(integ.ctx, md, in_dir, smp, cfg).build_graph()
    lc = graph.LightingCalculator(integ.ctx, g, md, in_dir, smp,
                                  graph.LightingCalculatorConfig(light_iterations=8, points_on_radius_light=1,
                                                                 bounces=[bounces]))
    assert lc.compute_final_light() == bounces
    integ.index = g.index(lc.light_scalar)
    img_free = integ.get_image(*integ.render())
    ug = g.to_uniform(f32(2) * g.radius, lc.light_scalar, reduce="mean")
    integ.index = ug.table
    integ.light_scale = 1.0
    img = integ.get_image(*integ.render())
    found = integ.last_pass()["count"]
    integ.close()
    print(f"uniform render mean {img.mean():.5e}, free render mean {img_free.mean():.5e}, ratio "
          f"{img.mean() / img_free.mean():.3f}; {g.num_vertices} vertices in {ug.num_vertices} voxels of "
          f"{float(ug.spacing):.4f}; scatters finding a vertex {np.mean(found[found >= 0] > 0):.3f}")
    assert np.all(np.isfinite(img)) and img.mean() > 0
    assert img_free.mean() / 3 <= img.mean() <= img_free.mean() * 3


@pytest.mark.gpu
def test_state_errors(gpu):
    from acceleratedvolrenderer_amd import capi, UniformInfiniteLight
    from acceleratedvolrenderer_amd.scene import Scene
    uni = capi.GraphUniform(np.array([[6, 6, 6]], np.int32), np.array([1.0], f32), 0.08)
    ctx = capi.Context(0)
    try:
        with pytest.raises(RuntimeError, match="avr error 3.*film required"):      # nothing set: no film
            ctx.graph_render_uniform(uni, 0, 1, 0)
        one = _graph_scene()
        ctx.set_scene(one)
        for view in (-1, 2):
            with pytest.raises(RuntimeError, match="avr error 1.*view must be"):
                ctx.graph_render_uniform(uni, 0, 1, 0, view=view)
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(RuntimeError, match="avr error 1.*light_scale"):
                ctx.graph_render_uniform(uni, 0, 1, 0, light_scale=bad)
        ctx.set_scene(_graph_scene(one_light=False))                              # two lights
        with pytest.raises(RuntimeError, match="avr error 3.*one distant light"):
            ctx.graph_render_uniform(uni, 0, 1, 0)
        ctx.set_scene(Scene(one.camera, one.film, one.medium, [UniformInfiniteLight(scale=0.25)]))
        with pytest.raises(RuntimeError, match="avr error 3.*one distant light"):
            ctx.graph_render_uniform(uni, 0, 1, 0)
        ctx.set_scene(_graph_scene(sphere=True))                                  # a boundary sphere at geometry 0
        with pytest.raises(RuntimeError, match="avr error 3.*bounds box"):
            ctx.graph_render_uniform(uni, 0, 1, 0)
        with pytest.raises(RuntimeError, match="avr error 3.*not avr_graph_render"):
            ctx.graph_last_pass(256, 1)
        ctx.set_scene(one)
        with pytest.raises(RuntimeError, match="avr error 1.*sample range"):
            ctx.graph_render_uniform(uni, 2, 1, 0)
        ctx.graph_render_uniform(uni, 0, 1, 0, view=1)
        assert ctx.graph_last_pass(256, 1)[3].shape == (256,)
    finally:
        ctx.close()
