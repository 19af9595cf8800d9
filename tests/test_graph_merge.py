"""The vertex merge in data-parallel rounds (csrc/avr_graph_merge.h; avr_graph_merge_assign,
avr_graph_merge_assign_device, avr_graph_add_walks_assigned, avr_graph_add_walks_device)
against the sequential builder (avr_graph_add_walks / _from), which stays the reference.

CPU (not gpu): the host rounds plus the replay give the builder's graph bit for bit on random
walks with heavy, moderate and almost no merging and on a clumped input, with existing
vertices and start vertices, against the Python restatement on one seed, and on constructed
cases (the d2 == r2 fallback, ties, nearest-not-first, a dependence chain); argument errors
leave the graph unchanged; the merge kernels' compiler-reported resources.
GPU (gpu): the device assignment is bitwise the host's on the same inputs and on a 20 000-walk
input that needs several rounds; FreeGraphBuilder(merge="device") builds the graph
merge="host" builds, with reinforcement, for the box and the interface sphere.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _random_walks(seed, n_walks, max_depth):
    """Uniform scatter points in the unit cube, 0..max_depth per walk."""
    rng = np.random.default_rng(seed)
    pts = rng.random((n_walks, max_depth, 3), dtype=f32)
    counts = rng.integers(0, max_depth + 1, n_walks).astype(np.int32)
    return pts, counts


def _clumped_walks(seed, n_walks, max_depth, radius):
    """Walks whose step (0.4 radius per axis at most) is below the radius, from 40 seeds."""
    rng = np.random.default_rng(seed)
    seeds = rng.random((40, 3), dtype=f32)
    step = (rng.random((n_walks, max_depth, 3), dtype=f32) - f32(0.5)) * f32(0.8 * radius)
    pts = (seeds[rng.integers(0, 40, n_walks)][:, None, :] + np.cumsum(step, axis=1, dtype=f32)).astype(f32)
    counts = rng.integers(0, max_depth + 1, n_walks).astype(np.int32)
    return pts, counts


@functools.lru_cache(maxsize=None)
def _case(name):
    """name -> (radius, points, counts, max_depth)."""
    if name == "clumped":
        return (0.05,) + _clumped_walks(11, 2000, 8, 0.05) + (8,)
    if name == "large":
        return (0.02,) + _random_walks(13, 20000, 8) + (8,)
    radius = {"heavy": 0.2, "moderate": 0.035, "sparse": 0.0035}[name]
    return (radius,) + _random_walks(12, 2000, 8) + (8,)


CASES = ["heavy", "moderate", "sparse", "clumped"]


def _state(g):
    """Everything the builder holds, in comparable form."""
    xyz, smp = g.vertices()
    fr, to, es = g.edges()
    rp, col, val = g.transport()
    return (xyz.view(np.uint32).tolist(), smp.tolist(), fr.tolist(), to.tolist(), es.tolist(),
            g.in_node_path_length(), rp.tolist(), col.tolist(), val.view(np.uint32).tolist())


def _same_graph(a, b):
    sa, sb = _state(a), _state(b)
    for what, x, y in zip(("vertices", "vertex samples", "edge from", "edge to", "edge samples", "in-node path length",
                           "transport row_ptr", "transport col", "transport val"), sa, sb):
        assert x == y, what


@functools.lru_cache(maxsize=None)
def _sequential(name):
    """The sequential builder's graph of a case."""
    from acceleratedvolrenderer_amd import capi
    radius, pts, counts, md = _case(name)
    g = capi.Graph(radius)
    g.add_walks(pts, counts, md)
    return g


@functools.lru_cache(maxsize=None)
def _host_assign(name):
    from acceleratedvolrenderer_amd import capi
    radius, pts, counts, md = _case(name)
    return capi.Graph(radius).merge_assign(pts, counts, md)


# ---------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", CASES)
def test_host_merge_matches_builder(name):
    from acceleratedvolrenderer_amd import capi
    radius, pts, counts, md = _case(name)
    ref = _sequential(name)
    vop, rounds = _host_assign(name)
    n_pts, n_v = int(counts.sum()), ref.size()[0]
    print(f"{name}: {n_pts} points -> {n_v} vertices, {rounds} host rounds")
    assert vop.shape == (len(counts), md)
    assert np.all(vop[np.arange(md)[None, :] >= counts[:, None]] == -1)
    assert rounds >= 1
    # the three regimes the radii are chosen for
    assert {"heavy": n_v < n_pts / 20, "moderate": n_pts / 20 < n_v < 0.95 * n_pts, "sparse": n_v > 0.99 * n_pts,
            "clumped": n_v < n_pts / 4}[name]
    g = capi.Graph(radius)
    g.add_walks_assigned(pts, counts, md, vop)
    _same_graph(g, ref)


def test_builder_searches_after_a_replay():
    """The replayed vertices are in the builder's own radius search afterwards: the host merge
    and CountInRadius go on from a replayed graph as from a merged one."""
    from acceleratedvolrenderer_amd import capi
    radius, pts, counts, md = _case("moderate")
    g, ref = capi.Graph(radius), capi.Graph(radius)
    half = len(counts) // 2
    ref.add_walks(pts, counts, md)
    g.add_walks_assigned(pts[:half], counts[:half], md, _host_assign("moderate")[0][:half])
    ids = np.arange(0, g.size()[0], 7, dtype=np.int32)
    part = capi.Graph(radius)
    part.add_walks(pts[:half], counts[:half], md)
    assert g.count_in_radius(ids, 3 * radius).tolist() == part.count_in_radius(ids, 3 * radius).tolist()
    g.add_walks(pts[half:], counts[half:], md)
    _same_graph(g, ref)


def test_host_merge_matches_restatement():
    """The clustered generator of the assembly tests (merges, revisits, self-edges) on one
    seed, against oracle/graph_builder.py."""
    from acceleratedvolrenderer_amd import capi
    from oracle.graph_builder import OracleGraph
    rng = np.random.default_rng(4)
    radius, md, n = 0.04, 6, 300
    centers = rng.random((12, 3), dtype=f32)
    pts = (centers[rng.integers(0, 12, (n, md))] + (rng.random((n, md, 3), dtype=f32) - f32(0.5)) * f32(2.2 * radius)).astype(f32)
    counts = rng.integers(0, md + 1, n).astype(np.int32)
    g = capi.Graph(radius)
    vop, _ = g.merge_assign(pts, counts, md)
    assert g.size() == (0, 0)   # assigning leaves the graph alone
    g.add_walks_assigned(pts, counts, md, vop)
    ref = OracleGraph(radius)
    ref.add_walks(pts, counts, md)
    xyz, smp = g.vertices()
    assert np.array_equal(xyz, np.array(ref.xyz, f32)) and smp.tolist() == ref.samples
    fr, to, es = g.edges()
    assert list(zip(fr.tolist(), to.tolist(), es.tolist())) == [(a, b, s) for (a, b), s in ref.edges.items()]
    avg, cnt = g.in_node_path_length()
    assert cnt == ref.pl_count and avg == pytest.approx(ref.pl_sum / ref.pl_count, rel=1e-6)


def _incremental():
    """A first batch, and a second with start vertices (some -1) and some walks of count 0."""
    radius, md = 0.05, 6
    p1, c1 = _clumped_walks(21, 600, md, radius)
    p2, c2 = _clumped_walks(22, 500, md, radius)
    p2[::2] = _random_walks(23, 250, md)[0]
    rng = np.random.default_rng(24)
    c2 = np.minimum(c2, md - 1).astype(np.int32)   # a start vertex takes one path slot
    c2[rng.integers(0, 500, 40)] = 0
    return radius, md, p1, c1, p2, c2, rng


def _incremental_graphs():
    from acceleratedvolrenderer_amd import capi
    radius, md, p1, c1, p2, c2, rng = _incremental()
    ref, g = capi.Graph(radius), capi.Graph(radius)
    ref.add_walks(p1, c1, md)
    g.add_walks(p1, c1, md)
    start = rng.integers(0, ref.size()[0], 500).astype(np.int32)
    start[rng.integers(0, 500, 120)] = -1
    assert (start == -1).any() and (c2 == 0).any() and (c2[start == -1] > 0).any()
    ref.add_walks_from(p2, c2, md, start)
    return ref, g, (p2, c2, md, start)


def test_incremental_merge_matches_add_walks_from():
    ref, g, (p2, c2, md, start) = _incremental_graphs()
    before = _state(g)
    vop, rounds = g.merge_assign(p2, c2, md, start)
    assert _state(g) == before
    n0 = g.size()[0]
    assert (vop[vop >= 0] < n0).any() and (vop >= n0).any()   # joins old vertices and makes new ones
    g.add_walks_assigned(p2, c2, md, vop, start)
    _same_graph(g, ref)


def _assign_both(radius, walks, max_depth, existing=None):
    """Constructed walks (lists of points) through merge_assign and through the builder; the
    two must agree. Returns (ids per walk, rounds). existing: one-point walks added first."""
    from acceleratedvolrenderer_amd import capi
    pts = np.zeros((len(walks), max_depth, 3), f32)
    counts = np.array([len(w) for w in walks], np.int32)
    for i, w in enumerate(walks):
        pts[i, :len(w)] = np.array(w, f32).reshape(-1, 3)
    g, ref = capi.Graph(radius), capi.Graph(radius)
    if existing:
        e = np.array(existing, f32).reshape(-1, 1, 3)
        for gg in (g, ref):
            gg.add_walks(e, np.ones(len(e), np.int32), 1)
    vop, rounds = g.merge_assign(pts, counts, max_depth)
    g.add_walks_assigned(pts, counts, max_depth, vop)
    ref.add_walks(pts, counts, max_depth)
    _same_graph(g, ref)
    return [vop[i, :len(w)].tolist() for i, w in enumerate(walks)], rounds, (pts, counts)


def _chain(n=64):
    """Points 0.4 apart along x in one walk, r = 0.5: each is decided after its predecessor
    (odd points merge into the even point before them, which must first be known new)."""
    return [[(float(f32(0.4) * f32(k)), 0.0, 0.0) for k in range(n)]]


CONSTRUCTED = {
    # d2 == r2 exactly: the fallback joins the walk's previous vertex ...
    "equal_in_walk": (0.5, [[(0, 0, 0), (0.5, 0, 0)]], 2, None, [[0, 0]]),
    # ... which two one-point walks do not have ...
    "equal_two_walks": (0.5, [[(0, 0, 0)], [(0.5, 0, 0)]], 1, None, [[0], [1]]),
    # ... and the previous vertex is the far one here
    "equal_far_previous": (0.5, [[(0, 0, 0), (3, 0, 0), (0.5, 0, 0)]], 3, None, [[0, 1, 2]]),
    "tie_lowest_id": (0.5, [[(0, 0, 0)]], 1, [(-0.25, 0, 0), (0.25, 0, 0)], [[0]]),
    "tie_lowest_id_in_batch": (0.5, [[(-0.25, 0, 0)], [(2, 0, 0)], [(0.25, 0, 0)], [(0, 0, 0)]], 1, None,
                               [[0], [1], [2], [0]]),
    # vertex 1 (created later) is nearer than vertex 0
    "nearest_not_first": (0.5, [[(0, 0, 0)], [(0.75, 0, 0)], [(0.4375, 0, 0)]], 1, None, [[0], [1], [1]]),
    "nearest_existing": (0.5, [[(0.4375, 0, 0)]], 1, [(0, 0, 0), (0.75, 0, 0)], [[1]]),
}


@pytest.mark.parametrize("name", sorted(CONSTRUCTED))
def test_constructed_cases(name):
    radius, walks, md, existing, want = CONSTRUCTED[name]
    ids, rounds, _ = _assign_both(radius, walks, md, existing)
    assert ids == want, (ids, rounds)


def test_chain_needs_rounds():
    ids, rounds, _ = _assign_both(0.5, _chain(), 64)
    assert ids == [[k // 2 for k in range(64)]]
    # the host's rounds are synchronous (states of the round before): the chain resolves one
    # link per round, so nothing below 64 is asserted here
    print(f"chain of 64: {rounds} host rounds")
    assert rounds >= 2


def test_empty_batches():
    from acceleratedvolrenderer_amd import capi
    g = capi.Graph(0.1)
    vop, rounds = g.merge_assign(np.zeros((0, 4, 3), f32), np.zeros(0, np.int32), 4)
    assert vop.shape == (0, 4) and rounds == 0
    g.add_walks_assigned(np.zeros((0, 4, 3), f32), np.zeros(0, np.int32), 4, vop)
    vop, rounds = g.merge_assign(np.zeros((3, 4, 3), f32), np.zeros(3, np.int32), 4)
    assert np.all(vop == -1) and rounds == 0
    g.add_walks_assigned(np.zeros((3, 4, 3), f32), np.zeros(3, np.int32), 4, vop)
    assert g.size() == (0, 0)


def test_argument_errors_leave_the_graph_unchanged():
    from acceleratedvolrenderer_amd import capi
    g = capi.Graph(0.5)
    g.add_walks(np.array([[[0, 0, 0], [2, 0, 0]]], f32), np.array([2], np.int32), 2)
    before = _state(g)
    pts = np.array([[[4, 0, 0], [6, 0, 0], [0, 0, 0]]], f32)
    one = np.array([3], np.int32)
    for call in (g.merge_assign, lambda *a: g.add_walks_assigned(*a[:3], np.zeros((1, 3), np.int32), *a[3:])):
        with pytest.raises(RuntimeError, match="count out of range"):
            call(pts, np.array([4], np.int32), 3)
        with pytest.raises(RuntimeError, match="count out of range"):
            call(pts, np.array([-1], np.int32), 3)
        with pytest.raises(RuntimeError, match="count out of range"):   # a start vertex takes a slot
            call(pts, one, 3, np.array([0], np.int32))
        with pytest.raises(RuntimeError, match="start vertex"):
            call(pts, np.array([2], np.int32), 3, np.array([2], np.int32))
        with pytest.raises(RuntimeError, match="start vertex"):
            call(pts, np.array([2], np.int32), 3, np.array([-2], np.int32))
    bad = pts.copy()
    bad[0, 1, 1] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        g.merge_assign(bad, one, 3)
    # ids: 2 and 3 are new at their turns, 0 exists; 4 is above the count at its turn, -1 negative
    for ids in ([2, 4, 0], [3, 2, 0], [2, 3, -1], [2, 3, 5]):
        with pytest.raises(RuntimeError, match="vertex id"):
            g.add_walks_assigned(pts, one, 3, np.array([ids], np.int32))
    assert _state(g) == before
    g.add_walks_assigned(pts, one, 3, np.array([[2, 3, 0]], np.int32))
    assert g.size()[0] == 4
    with pytest.raises(ValueError):
        g.add_walks_assigned(pts, one, 3, np.zeros((1, 2), np.int32))
    from acceleratedvolrenderer_amd import graph
    with pytest.raises(ValueError, match="merge"):
        graph.FreeGraphBuilder(None, None, [0, 0, 1], None, graph.GraphBuilderConfig(), node_radius=0.1, merge="gpu")
    assert graph.FreeGraphBuilder(None, None, [0, 0, 1], None, graph.GraphBuilderConfig(), node_radius=0.1).merge == "host"


def test_merge_kernel_resources(tmp_path):
    """The merge kernels compile without scratch. Observed (hipcc -Rpass-analysis, gfx950), which
    is the floor asserted: k_graph_merge_round 46 VGPRs, k_graph_merge_round_wave 56, both 8
    waves/SIMD and no LDS; the id-scan kernels 9-14 VGPRs, 8 waves/SIMD (k_graph_merge_scan: 1 KiB
    of LDS)."""
    from acceleratedvolrenderer_amd import build as avr_build
    if not os.path.exists(avr_build.HIPCC):
        pytest.skip("no hipcc")
    src = tmp_path / "merge.hip"
    src.write_text('#define AVR_KPATHS_TU\n#include "avr_kernels.hip"\n#include "avr_graph.hip"\n')
    cmd = ([avr_build.HIPCC] + avr_build.FLAGS +
           ["-I" + avr_build.CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
            "-c", str(src), "-o", str(tmp_path / "merge.o")])
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    seen = {}
    for block in p.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        if "k_graph_merge_" in name:
            seen[name] = {key: int(re.search(pat, block).group(1)) for key, pat in (
                ("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))}
    floors = {"k_graph_merge_round": 8, "k_graph_merge_round_wave": 8, "k_graph_merge_flags": 8,
              "k_graph_merge_scan": 8, "k_graph_merge_ids": 8}
    found = {}
    for kernel in floors:
        match = [v for k, v in seen.items() if f"{len(kernel)}{kernel}" in k]   # the mangled name's own length
        assert len(match) == 1, (kernel, sorted(seen))
        print(f"{kernel}: {match[0]}")
        found[kernel] = match[0]
    for kernel, floor in floors.items():
        assert found[kernel]["scratch"] == 0 and found[kernel]["occ"] >= floor, kernel
    assert found["k_graph_merge_round"]["lds"] == 0 and found["k_graph_merge_round_wave"]["lds"] == 0


# ---------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu_ctx():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from acceleratedvolrenderer_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES + ["large"])
def test_device_assignment_is_the_hosts(gpu_ctx, name):
    from acceleratedvolrenderer_amd import capi
    radius, pts, counts, md = _case(name)
    want, host_rounds = _host_assign(name)
    g = capi.Graph(radius)
    vop, rounds = g.merge_assign_device(gpu_ctx, pts, counts, md)
    print(f"{name}: {int(counts.sum())} points, device rounds {rounds}, host rounds {host_rounds}")
    assert np.array_equal(vop, want)
    assert g.size() == (0, 0)
    assert 1 <= rounds <= host_rounds
    if name == "large":
        assert rounds >= 2
        ref = capi.Graph(radius)
        ref.add_walks(pts, counts, md)
        stats = g.add_walks_device(gpu_ctx, pts, counts, md)
        print(stats)
        _same_graph(g, ref)
        assert stats["points"] == int(counts.sum()) and stats["new_vertices"] == ref.size()[0]
        assert stats["rounds"] >= 2


@pytest.mark.gpu
def test_device_incremental_merge(gpu_ctx):
    ref, g, (p2, c2, md, start) = _incremental_graphs()
    want, _ = g.merge_assign(p2, c2, md, start)
    vop, rounds = g.merge_assign_device(gpu_ctx, p2, c2, md, start)
    assert np.array_equal(vop, want) and rounds >= 1
    stats = g.add_walks_device(gpu_ctx, p2, c2, md, start)
    _same_graph(g, ref)
    assert stats["points"] == int(c2.sum())


@pytest.mark.gpu
def test_device_constructed_cases(gpu_ctx):
    from acceleratedvolrenderer_amd import capi
    cases = dict(CONSTRUCTED, chain=(0.5, _chain(), 64, None, [[k // 2 for k in range(64)]]))
    for name, (radius, walks, md, existing, want) in sorted(cases.items()):
        pts = np.zeros((len(walks), md, 3), f32)
        counts = np.array([len(w) for w in walks], np.int32)
        for i, w in enumerate(walks):
            pts[i, :len(w)] = np.array(w, f32).reshape(-1, 3)
        g = capi.Graph(radius)
        if existing:
            e = np.array(existing, f32).reshape(-1, 1, 3)
            g.add_walks(e, np.ones(len(e), np.int32), 1)
        vop, rounds = g.merge_assign_device(gpu_ctx, pts, counts, md)
        assert [vop[i, :len(w)].tolist() for i, w in enumerate(walks)] == want, name
        if name == "chain":
            # every link waits for the one before it, and the waves of one launch run side by
            # side: how many links a round resolves depends on their timing, so only >= 2
            print(f"chain of 64: {rounds} device rounds")
            assert rounds >= 2
    g = capi.Graph(0.1)
    vop, rounds = g.merge_assign_device(gpu_ctx, np.zeros((3, 4, 3), f32), np.zeros(3, np.int32), 4)
    assert np.all(vop == -1) and rounds == 0
    assert g.add_walks_device(gpu_ctx, np.zeros((0, 4, 3), f32), np.zeros(0, np.int32), 4)["points"] == 0


def _graph_scene(interface=None):
    """tests/test_graph.py's 12^3 graph scene, optionally bounded by a sphere."""
    from acceleratedvolrenderer_amd import scenes, GridMedium
    from acceleratedvolrenderer_amd.scene import Scene
    base = scenes.s_uniform(n=2, width=16, height=16, variant="scatter")
    dens = (f32(0.2) + f32(0.8) * np.random.default_rng(5).random((12, 12, 12), dtype=f32)).astype(f32)
    med = GridMedium(dens, sigma_a=0.4, sigma_s=6.0, g=0.5)
    kw = {"interface_sphere": interface} if interface is not None else {}
    return Scene(base.camera, base.film, med, base.lights[:1], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("primitive", ["box", "interface"])
def test_build_graph_device_merge_is_host_merge(primitive):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from acceleratedvolrenderer_amd import capi, graph
    scene = _graph_scene(((0.5, 0.5, 0.5), 0.45) if primitive == "interface" else None)
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    d = np.array([0.3, -0.5, 0.81], f32)
    d = (d / f32(np.linalg.norm(d))).astype(f32)
    built = {}
    for merge in ("device", "host"):
        cfg = graph.GraphBuilderConfig(
            radius_modifier=60.0, max_depth=12, dimension_steps=8, iterations_per_step=6,
            render_search_range={"active": True, "neighboursToUse": 4},
            edge_reinforcement={"active": True, "unsatisfiedAllowedRatio": 0.3, "reinforcementRays": 4,
                                "edgesForNotSparse": 3},
            neighbour_reinforcement={"active": True, "unsatisfiedAllowedRatio": 0.3, "reinforcementRays": 3,
                                     "neighboursForNotSparse": 3, "neighbourRangeModifier": 2.0})
        md = graph.MediumData(scene, primitive=primitive)
        sampling = graph.GraphSampling(sampler=0, seed=3, samples_per_pixel=16, resolution=(64, 64))
        b = graph.FreeGraphBuilder(ctx, md, d, sampling, cfg, search_ranges="host", merge=merge)
        built[merge] = (b, b.build_graph())
    ctx.close()
    (bd, gd), (bh, gh) = built["device"], built["host"]
    print(f"{primitive}: {gd.num_vertices} vertices, {len(gd.edge_from)} edges, {bd.reinforce_cycles} cycles, "
          f"{bd.merge_rounds} merge rounds, last {bd.merge_stats}")
    assert bd.reinforce_cycles == bh.reinforce_cycles >= 1
    assert gd.num_vertices > 50
    assert np.array_equal(gd.points.view(np.uint32), gh.points.view(np.uint32))
    assert gd.samples.tolist() == gh.samples.tolist()
    for a in ("edge_from", "edge_to", "edge_samples"):
        assert getattr(gd, a).tolist() == getattr(gh, a).tolist(), a
    assert np.array_equal(gd.search_range.view(np.uint32), gh.search_range.view(np.uint32))
    assert (gd.in_node_path_length, gd.in_node_path_count) == (gh.in_node_path_length, gh.in_node_path_count)
    assert bd.merge_stats is not None and bd.merge_rounds >= 1 and bh.merge_stats is None
