"""k nearest neighbours and ComputeSearchRanges over the vertex index
(free_graph_builder.cpp:473-548; avr_graph_index_knn / _search_ranges, avr_graph_knn /
_search_ranges, include/avr.h).

The reference is a brute-force numpy restatement written here: float32 throughout, nanoflann's
L2_Simple_Adaptor distance ((dx² + dy²) + dz²), the neighbours ordered by (d2, id) with the
vertex itself removed by id, and the two sequential float Averager levels. It resolves ties as
the index does, so no case and no vertex is skipped: ids, d2 bits and range bits are compared
for every vertex.

CPU (not gpu): the host routine against the restatement. GPU (gpu): the device bitwise
against the host, and FreeGraphBuilder's three search_ranges modes on a small S-cloud graph.
"""
import ctypes

import numpy as np
import pytest

f32 = np.float32


# ---------------------------------------------------------------------------- reference

def _d2(verts, p):
    d = (p[None, :] - verts).astype(f32)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(f32) + d[:, 2] * d[:, 2]).astype(f32)


def ref_knn(verts, k):
    """(ids, d2, ranges): GetNClosest and ComputeSearchRanges by brute force."""
    verts = np.asarray(verts, f32)
    n = len(verts)
    all_ids = np.arange(n)
    ids = np.zeros((n, k), np.int32)
    d2 = np.zeros((n, k), f32)
    for v in range(n):
        d = _d2(verts, verts[v])
        order = np.lexsort((all_ids, d))
        order = order[order != v][:k]
        ids[v], d2[v] = order, d[order]
    avg = np.zeros(n, f32)
    for v in range(n):
        s = f32(0)
        for i in range(k):
            s = f32(s + f32(np.sqrt(d2[v, i])))
        avg[v] = f32(s / f32(k))
    ranges = np.zeros(n, f32)
    for v in range(n):
        s = f32(f32(0) + avg[v])
        for i in range(k):
            s = f32(s + avg[ids[v, i]])
        ranges[v] = f32(s / f32(k + 1))
    return ids, d2, ranges


def _random(seed=11, n=4000):
    return np.random.default_rng(seed).random((n, 3), dtype=f32)


def _points(name):
    if name == "random":
        return _random(), 0.05
    if name == "cluster":      # more than 16 vertices in one cell
        rng = np.random.default_rng(5)
        d = rng.normal(size=(300, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        ball = (0.5 + 1e-3 * d * rng.random((300, 1)) ** (1 / 3)).astype(f32)
        return np.concatenate([ball, rng.random((50, 3), dtype=f32)]), 0.05
    if name == "outlier":      # many radius doublings, a radius beyond the grid
        return np.concatenate([_random(), np.array([[50.0, 50.0, 50.0]], f32)]), 0.05
    if name == "lattice":      # exact ties everywhere
        g = np.arange(6, dtype=f32)
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).copy(), 0.5
    if name == "minimal":
        return np.random.default_rng(2).random((5, 3), dtype=f32), 0.3
    if name == "tail257":      # one past a block
        return np.random.default_rng(257).random((257, 3), dtype=f32), 0.1
    if name == "tail65":       # one past a wave
        return np.random.default_rng(65).random((65, 3), dtype=f32), 0.1
    raise KeyError(name)


CASES = [("random", 4), ("random", 15), ("cluster", 15), ("outlier", 4), ("lattice", 6), ("minimal", 4),
         ("tail257", 4), ("tail65", 4)]
IDS = [f"{n}-k{k}" for n, k in CASES]
_REF = {}


def _case(name, k):
    """(points, radius, reference), the reference computed once per case."""
    if (name, k) not in _REF:
        pts, radius = _points(name)
        _REF[name, k] = (pts, radius, ref_knn(pts, k))
    return _REF[name, k]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _index(pts, radius):
    from acceleratedvolrenderer_amd import capi
    return capi.GraphIndex(pts, np.zeros(len(pts), f32), None, radius=radius)


# ---------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name,k", CASES, ids=IDS)
def test_host_knn_and_ranges_match_brute_force(name, k):
    pts, radius, (ref_ids, ref_d2, ref_rng) = _case(name, k)
    idx = _index(pts, radius)
    ids, d2 = idx.knn(k)
    rng = idx.search_ranges(k)
    ties = int(np.sum(ref_d2[:, 1:] == ref_d2[:, :-1]))
    print(f"{name} k={k}: n={len(pts)}, tied neighbour pairs {ties}, mean range {rng.mean():.6g}")
    assert ids.shape == d2.shape == (len(pts), k) and rng.shape == (len(pts),)
    assert np.array_equal(ids, ref_ids)
    assert np.array_equal(_bits(d2), _bits(ref_d2))
    assert np.array_equal(_bits(rng), _bits(ref_rng))
    assert np.all(np.isfinite(rng)) and np.all(rng > 0)
    if name == "lattice":
        assert ties > 200          # the lower id wins every one of them
    if name == "outlier":
        assert d2[-1, 0] > 7000    # 3 * 49² from the far vertex to the cube


def test_knn_one_output_only():
    pts, radius, (ref_ids, ref_d2, _) = _case("tail65", 4)
    idx = _index(pts, radius)
    n = len(pts)
    ids = np.zeros((n, 4), np.int32)
    d2 = np.zeros((n, 4), f32)
    ip, fp = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), d2.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert idx.lib.avr_graph_index_knn(idx.h, 4, ip, None) == 0
    assert idx.lib.avr_graph_index_knn(idx.h, 4, None, fp) == 0
    assert np.array_equal(ids, ref_ids) and np.array_equal(_bits(d2), _bits(ref_d2))


def test_knn_argument_errors():
    from acceleratedvolrenderer_amd import capi
    pts, radius = _points("tail65")
    idx = _index(pts, radius)
    for bad in (0, -1, 16):
        with pytest.raises(RuntimeError, match="avr error 1.*k must be 1..15"):
            idx.knn(bad)
        with pytest.raises(RuntimeError, match="avr error 1.*k must be 1..15"):
            idx.search_ranges(bad)
    small = _index(pts[:5], radius)
    for call in (small.knn, small.search_ranges):
        with pytest.raises(RuntimeError, match="avr error 1.*enough vertices"):
            call(5)                      # k == n: the reference reads neighbours[-1]
    assert small.knn(4)[0].shape == (5, 4)
    lib = capi.load()
    assert lib.avr_graph_index_knn(idx.h, 4, None, None) == 1 and b"null buffer" in lib.avr_last_error()
    assert lib.avr_graph_index_search_ranges(idx.h, 4, None) == 1 and b"null buffer" in lib.avr_last_error()
    assert lib.avr_graph_index_knn(None, 4, None, None) == 1 and b"null graph index" in lib.avr_last_error()
    # the device entry points check their arguments before they touch a device
    assert lib.avr_graph_knn(None, idx.h, 4, None, None) == 1
    assert lib.avr_graph_search_ranges(None, idx.h, 4, None) == 1


def test_host_ranges_agree_with_the_scipy_form():
    """The legacy float64 k-d tree form differs from the float routine in rounding only."""
    from acceleratedvolrenderer_amd import graph
    pts, radius, (_, _, ref_rng) = _case("random", 4)
    host = graph.compute_search_ranges_host(pts, radius, 4)
    assert np.array_equal(_bits(host), _bits(ref_rng))
    legacy = graph.compute_search_ranges(pts, 4)
    rel = np.abs(host.astype(np.float64) - legacy) / legacy
    print(f"host vs scipy: max relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-5
    with pytest.raises(ValueError, match="enough vertices"):
        graph.compute_search_ranges_host(pts[:3], radius, 4)
    with pytest.raises(ValueError, match="search_ranges"):
        graph.FreeGraphBuilder(None, None, [0, 0, 1], None, graph.GraphBuilderConfig(), node_radius=0.1,
                               search_ranges="gpu")


# ---------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from acceleratedvolrenderer_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", CASES, ids=IDS)
def test_device_knn_and_ranges_are_the_hosts(ctx, name, k):
    pts, radius, (ref_ids, ref_d2, ref_rng) = _case(name, k)
    idx = _index(pts, radius)
    host_ids, host_d2 = idx.knn(k)
    host_rng = idx.search_ranges(k)
    ids, d2 = ctx.graph_knn(idx, k)
    rng = ctx.graph_search_ranges(idx, k)
    assert np.array_equal(ids, host_ids)
    assert np.array_equal(_bits(d2), _bits(host_d2))
    assert np.array_equal(_bits(rng), _bits(host_rng))
    assert np.array_equal(ids, ref_ids) and np.array_equal(_bits(rng), _bits(ref_rng))


@pytest.mark.gpu
def test_device_knn_argument_errors(ctx):
    pts, radius = _points("minimal")
    idx = _index(pts, radius)
    for bad in (0, 16, 5):
        with pytest.raises(RuntimeError, match="avr error 1"):
            ctx.graph_knn(idx, bad)
        with pytest.raises(RuntimeError, match="avr error 1"):
            ctx.graph_search_ranges(idx, bad)
    assert ctx.lib.avr_graph_knn(ctx.h, idx.h, 4, None, None) == 1
    assert ctx.lib.avr_graph_search_ranges(ctx.h, idx.h, 4, None) == 1


def _cloud_scene(ctx, n=32):
    """S-cloud's n³ GridMedium with its distant light alone (tools/graph_render_demo.py's scene)."""
    import torch
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import Scene
    density = torch.empty((n, n, n), dtype=torch.float32, device="cuda:0")
    ctx.generate_cloud(density.data_ptr(), n, 0, n ** 3)
    ctx.sync()
    cloud = scenes.s_cloud(density, width=64, height=48, spp=1)
    return Scene(cloud.camera, cloud.film, cloud.medium, cloud.lights[:1], sampler=cloud.sampler)


@pytest.mark.gpu
def test_builder_search_range_modes(ctx):
    """FreeGraphBuilder on the S-cloud 32³ scene with test_graph_render's small configuration:
    "device" is bitwise "host", and the default is still the scipy form's values."""
    from acceleratedvolrenderer_amd import graph
    scene = _cloud_scene(ctx)
    ctx.set_scene(scene)
    cfg = graph.GraphBuilderConfig(radius_modifier=60.0, max_depth=12, dimension_steps=8, iterations_per_step=6,
                                   render_search_range={"active": True, "neighboursToUse": 4})
    in_dir = (-np.asarray(scene.light_w[0], f32)).astype(f32)
    smp = graph.GraphSampling(sampler=0, seed=3, samples_per_pixel=16, resolution=(64, 64))
    md = graph.MediumData(scene)
    out = {}
    for mode in ("device", "host", None):
        kw = {} if mode is None else {"search_ranges": mode}
        g = graph.FreeGraphBuilder(ctx, md, in_dir, smp, cfg, **kw).build_graph()
        out[mode] = g
    dev, host, default = out["device"], out["host"], out[None]
    assert dev.num_vertices > 4 and np.array_equal(dev.points, host.points) and np.array_equal(dev.points, default.points)
    assert np.array_equal(_bits(dev.search_range), _bits(host.search_range))
    legacy = graph.compute_search_ranges(default.points, 4)
    assert np.array_equal(_bits(default.search_range), _bits(legacy))
    rel = np.abs(host.search_range.astype(np.float64) - legacy) / legacy
    print(f"{dev.num_vertices} vertices, host vs scipy max relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-5
