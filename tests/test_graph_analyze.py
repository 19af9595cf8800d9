"""The analyzer integrator: IntegrationAnalyzer (graph/analysis/integration_analyzer.cpp).

CPU (not gpu): the host coverage search (avr_graph_index_coverage, include/avr.h) against a
brute-force numpy restatement of Analyze written here: float32 throughout, nanoflann's
L2_Simple_Adaptor distance ((dx² + dy²) + dz²), node = some d2 < Sqr(vertexRadius), the search
result d2 < the largest squared range with d2 > Sqr(range[v]) dropped, sorted by (d2, id), the
sequential float sum of sqrt(d2). Counts equal, sums bit-identical.

GPU (gpu): avr_graph_coverage bitwise against the host routine; the analysis' scatters
replayed by the oracle's graph walks (canonical libm) on the camera rays read back from the
pass; the per-pixel sums against the detail; passes and calls; the render at maxdepth 1; the
state and argument errors.
"""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---------------------------------------------------------------------------- reference

def _d2(verts, p):
    d = (p[None, :] - verts).astype(f32)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(f32) + d[:, 2] * d[:, 2]).astype(f32)


def ref_coverage(verts, ranges, radius, queries):
    """Analyze by brute force: (node, in_range, range_sum, tie) per query. `tie`: two vertices
    in range share a distance (nanoflann's order is then unspecified; the index takes the lower id)."""
    verts = np.asarray(verts, f32)
    r2 = f32(f32(radius) * f32(radius))
    rng2 = None
    if ranges is not None:
        rng2 = (np.asarray(ranges, f32) * np.asarray(ranges, f32)).astype(f32)
    nq = len(queries)
    node, cnt = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
    rsum, tie = np.zeros(nq, f32), np.zeros(nq, bool)
    for k, p in enumerate(np.asarray(queries, f32)):
        d2 = _d2(verts, p)
        node[k] = int(np.any(d2 < r2))
        if rng2 is None:
            continue
        ids = np.nonzero((d2 < rng2.max()) & ~(d2 > rng2))[0]
        ids = ids[np.lexsort((ids, d2[ids]))]
        s = f32(0)
        for v in ids:
            s = f32(s + np.sqrt(d2[v]))
        cnt[k], rsum[k] = len(ids), s
        tie[k] = len(ids) > 1 and bool(np.any(np.diff(d2[ids]) == 0))
    return node, cnt, rsum, tie


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.uint64)


def _inputs(seed=11, n=4000, radius=0.05, nq=1500):
    """tests/test_graph_render.py's recipe."""
    rng = np.random.default_rng(seed)
    verts = rng.random((n, 3), dtype=f32)
    light = (rng.random(n, dtype=f32) + f32(1e-3)).astype(f32)
    q = (f32(-0.1) + f32(1.2) * rng.random((nq, 3), dtype=f32)).astype(f32)
    q[:8] = verts[:8]
    ranges = (f32(radius) * (f32(0.5) + f32(3) * rng.random(n, dtype=f32))).astype(f32)
    return verts, light, q, ranges


_REF = {}


def _case(name):
    """The inputs of one case and their reference, computed once:
    (verts, light, ranges, radius, queries, ref)."""
    if name not in _REF:
        if name == "ranges":
            verts, light, q, ranges = _inputs()
            radius = 0.05
        elif name == "plain":
            verts, light, q, _ = _inputs()
            ranges, radius = None, 0.05
        elif name == "hand":
            # one vertex inside the vertex radius of the query but with a range below its
            # distance; a second one far away with the largest range, out of its reach
            verts = np.array([[0.5, 0.5, 0.5], [3.0, 0.5, 0.5]], f32)
            light = np.array([1.0, 1.0], f32)
            ranges = np.array([0.01, 0.5], f32)
            radius = 0.1
            q = np.array([[0.55, 0.5, 0.5], [0.505, 0.5, 0.5], [2.75, 0.5, 0.5], [0.5, 0.5, 0.5]], f32)
        elif name == "one":
            verts = np.array([[0.25, 0.5, 0.75]], f32)
            light = np.array([2.0], f32)
            ranges = np.array([0.12], f32)
            radius = 0.1
            q = np.array([[0.25, 0.5, 0.8], [0.25, 0.5, 0.75], [0.25, 0.5, 0.86], [0.25, 0.5, 0.9],
                          [1e6, -1e6, 3.0]], f32)
        else:   # "far": a flat graph, ranges far larger than the grid, queries far outside the box
            rng = np.random.default_rng(3)
            verts = rng.random((500, 3), dtype=f32)
            verts[:, 2] = f32(0.5)
            light = np.ones(500, f32)
            ranges = np.full(500, 100.0, f32)
            radius = 0.02
            q = (f32(-0.2) + f32(1.4) * rng.random((40, 3), dtype=f32)).astype(f32)
            q[-3:] = np.array([[50.0, 0.5, 0.5], [-40.0, -40.0, -40.0], [0.5, 0.5, 1e9]], f32)
        _REF[name] = (verts, light, ranges, radius, q, ref_coverage(verts, ranges, radius, q))
    return _REF[name]


def _check_against_ref(got, ref, ties_allowed=True):
    """ties_allowed: skip the queries with a tie (next to none may have one); else compare
    every query, ties in the index's own order (the lower id first) on both sides."""
    node, cnt, rsum = got
    ref_node, ref_cnt, ref_sum, tie = ref
    if ties_allowed:
        assert tie.mean() <= 0.001
    ok = ~tie if ties_allowed else np.ones(len(tie), bool)
    assert np.array_equal(node[ok], ref_node[ok])
    assert np.array_equal(cnt[ok], ref_cnt[ok])
    assert np.array_equal(bits(rsum[ok]), bits(ref_sum[ok]))


# ---------------------------------------------------------------------------- CPU

def test_index_coverage_against_brute_force():
    from acceleratedvolrenderer_amd import capi
    verts, light, ranges, radius, q, ref = _case("ranges")
    idx = capi.GraphIndex(verts, light, ranges, radius=radius)
    got = idx.coverage(q)
    _check_against_ref(got, ref)
    node, cnt, rsum, tie = ref
    print(f"coverage: node {node.mean():.4f}, search {np.mean(cnt > 0):.4f}, max {cnt.max()} in range, "
          f"above 16: {np.sum(cnt > 16)}, ties {tie.sum()}")
    # the figures of these inputs: well beyond the 16-key buffer, so the rescans run
    assert tie.sum() == 0 and abs(node.mean() - 0.564) < 5e-4 and abs(np.mean(cnt > 0) - 0.959) < 5e-4
    assert cnt.max() == 43 and np.sum(cnt > 32) > 0
    # a query on a vertex: distance 0 is in range and adds 0
    assert np.all(node[:8] == 1) and np.all(got[1][:8] >= 1)
    # the random inputs hold no query with a vertex in the radius and none in range
    assert not np.any((node == 1) & (cnt == 0))


def test_index_coverage_node_without_a_vertex_in_range():
    from acceleratedvolrenderer_amd import capi
    verts, light, ranges, radius, q, ref = _case("hand")
    node, cnt, rsum = capi.GraphIndex(verts, light, ranges, radius=radius).coverage(q)
    _check_against_ref((node, cnt, rsum), ref, ties_allowed=False)
    # 0.05 from vertex 0: inside its radius 0.1, beyond its range 0.01 (and far from vertex 1)
    assert (node[0], cnt[0], rsum[0]) == (1, 0, 0)
    # 0.005 from it: in range too
    assert (node[1], cnt[1]) == (1, 1) and rsum[1] == np.sqrt(_d2(verts[:1], q[1]))[0]
    # 0.25 from vertex 1: outside the radius, inside its range 0.5
    assert (node[2], cnt[2], rsum[2]) == (0, 1, f32(0.25))
    # on vertex 0: distance 0 counts and adds nothing
    assert (node[3], cnt[3], rsum[3]) == (1, 1, 0)


def test_index_coverage_without_search_ranges():
    from acceleratedvolrenderer_amd import capi
    verts, light, ranges, radius, q, ref = _case("plain")
    node, cnt, rsum = capi.GraphIndex(verts, light, None, radius=radius).coverage(q)
    _check_against_ref((node, cnt, rsum), ref, ties_allowed=False)
    assert np.all(cnt == 0) and np.all(rsum == 0) and abs(node.mean() - 0.564) < 5e-4
    # node is the first question alone: the same with ranges
    assert np.array_equal(node, _case("ranges")[5][0])


def test_index_coverage_single_vertex_and_far_queries():
    from acceleratedvolrenderer_amd import capi
    verts, light, ranges, radius, q, ref = _case("one")
    node, cnt, rsum = capi.GraphIndex(verts, light, ranges, radius=radius).coverage(q)
    _check_against_ref((node, cnt, rsum), ref, ties_allowed=False)
    assert node.tolist() == [1, 1, 0, 0, 0] and cnt.tolist() == [1, 1, 1, 0, 0]
    # the far queries' large distances tie; both sides order ties by vertex id
    verts, light, ranges, radius, q, ref = _case("far")
    idx = capi.GraphIndex(verts, light, ranges, radius=radius)
    node, cnt, rsum = idx.coverage(q)
    _check_against_ref((node, cnt, rsum), ref, ties_allowed=False)
    assert ref[3].any()
    # ranges of 100 reach from 50 and from (-40, -40, -40), not from z = 1e9
    assert cnt[-3:].tolist() == [500, 500, 0] and np.all(cnt[:-3] == 500) and node[-3:].tolist() == [0, 0, 0]


def test_index_coverage_argument_errors():
    from acceleratedvolrenderer_amd import capi
    lib = capi.load()
    idx = capi.GraphIndex(np.zeros((1, 3), f32), np.ones(1, f32), None, radius=0.1)
    out = np.zeros(1, np.int32)
    p = np.zeros(3, f32)
    assert lib.avr_graph_index_coverage(None, 1, capi._fp(p), None, None, None) == 1
    assert lib.avr_graph_index_coverage(idx.h, -1, capi._fp(p), None, None, None) == 1
    assert lib.avr_graph_index_coverage(idx.h, 1, None, None, None, None) == 1 and b"null" in lib.avr_last_error()
    # no points is no error, and any output may be left out
    assert lib.avr_graph_index_coverage(idx.h, 0, None, None, None, None) == 0
    assert lib.avr_graph_index_coverage(idx.h, 1, capi._fp(p), out.ctypes.data_as(capi.c_int_p), None, None) == 0
    assert out[0] == 1
    # the device calls check their arguments before they touch a GPU
    assert lib.avr_graph_coverage(None, idx.h, 1, capi._fp(p), None, None, None) == 1
    assert lib.avr_graph_analyze(None, idx.h, None, 0, 1, 0, 1, 0) == 1
    assert lib.avr_graph_analysis_read(None, None, None, None, None, None) == 3
    assert lib.avr_graph_analysis_clear(None) == 3
    assert lib.avr_graph_analyze_last_pass(None, None, None, None, None, None, None, None, 0, 1) == 1


def test_python_surface_without_a_gpu():
    import acceleratedvolrenderer_amd as avr
    from acceleratedvolrenderer_amd import graph, integrator
    assert avr.IntegrationAnalyzer is graph.IntegrationAnalyzer
    assert integrator.INTEGRATOR_NAMES == ("volpath", "volpathcustom", "volpath_mi355x")
    cp = graph.IntegrationAnalyzer.create_params
    # IntegrationAnalyzer::Create: maxdepth defaults to 1; --maxdepth replaces it whenever given
    assert cp("analyzer", {}) == dict(maxdepth=1, spp=16, seed=0)
    assert cp("analyzer", {"maxdepth": 4, "pixelsamples": 8, "seed": 2}) == dict(maxdepth=4, spp=8, seed=2)
    assert cp("analyzer", {"maxdepth": 4}, maxdepth_override=2)["maxdepth"] == 2
    assert cp("analyzer", {"maxdepth": 4}, maxdepth_override=0)["maxdepth"] == 0
    for name in ("graph", "volpath", "analyser"):
        with pytest.raises(ValueError, match="integrator type unknown"):
            cp(name, {})
    for fn in ("from_file", "create", "analyze", "last_pass", "result", "close"):
        assert callable(getattr(graph.IntegrationAnalyzer, fn))
    # the result's figures and the reference's line (integration_analyzer.cpp:40-44)
    res = graph.GraphAnalysis(2, 1, 1, 4, [4, 0], [1, 0], [3, 0], [6, 0], [1.5, 0.0])
    assert res.total.shape == (1, 2) and res.total.dtype == np.uint64 and res.range_sum.dtype == np.float64
    px = res.pixel(0, 0)
    assert (px["total"], px["node"], px["search"], px["in_range"]) == (4, 1, 3, 6)
    assert (px["node_ratio"], px["search_ratio"], px["mean_range"]) == (0.25, 0.75, 0.25)
    assert res.format_line(0, 0) == "[ 0, 0 ], 1 / 4 (0.25) | 3 / 4 (0.75), 0.25"
    empty = res.pixel(1, 0)
    assert np.isnan(empty["node_ratio"]) and np.isnan(empty["search_ratio"]) and empty["mean_range"] == 0
    assert res.summary() == px
    nr, sr, mr = res.ratio_maps()
    assert nr.tolist() == [[0.25, 0.0]] and sr.tolist() == [[0.75, 0.0]] and mr.tolist() == [[0.25, 0.0]]


# ---------------------------------------------------------------------------- GPU

def _graph_scene(shape=(12, 12, 12), seed=5, sampler=0, one_light=True, sphere=False, spp=4):
    """tests/test_graph_render.py's _graph_scene recipe (gray GridMedium, 16x16 film)."""
    from acceleratedvolrenderer_amd import scenes, GridMedium, IndependentSampler, ZSobolSampler
    from acceleratedvolrenderer_amd.scene import Scene
    base = scenes.s_uniform(n=2, width=16, height=16, variant="scatter")
    dens = (0.2 + 0.8 * np.random.default_rng(seed).random(shape, dtype=np.float32)).astype(np.float32)
    med = GridMedium(dens, sigma_a=0.4, sigma_s=6.0, g=0.5)
    smp = (ZSobolSampler if sampler else IndependentSampler)(pixelsamples=spp)
    return Scene(base.camera, base.film, med, base.lights[:1] if one_light else base.lights, sampler=smp,
                 interface_sphere=((0.5, 0.5, 0.5), 0.45) if sphere else None)


SEED = 3
SPP = 4
NPIX = 256
LIGHT_DIR = np.array([0.3, -0.5, 0.81], f32)
SHAPES = [(12, 12, 12), (9, 12, 5)]
DEPTHS = [1, 3]


def _build_graph(scene, ctx, kind, radius_modifier=60.0):
    from acceleratedvolrenderer_amd import graph
    cfg = graph.GraphBuilderConfig(radius_modifier=radius_modifier, max_depth=12, dimension_steps=8,
                                   iterations_per_step=6,
                                   render_search_range={"active": True, "neighboursToUse": 4})
    d = (LIGHT_DIR / f32(np.linalg.norm(LIGHT_DIR))).astype(f32)
    smp = graph.GraphSampling(sampler=kind, seed=SEED, samples_per_pixel=16, resolution=(64, 64))
    b = graph.FreeGraphBuilder(ctx, graph.MediumData(scene), d, smp, cfg)
    return b, b.build_graph()


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _maps(res):
    return (res.total, res.node, res.search, res.in_range, res.range_sum)


@pytest.fixture(scope="module")
def analysed(gpu):
    """Per (grid shape, sampler): the scene, its graph and index, and per maxdepth the analyses
    of sample indices [0, 4): in one pass with its detail, in passes of 3 + 1 samples with the
    last pass's detail, and in two calls [0, 2) then [2, 4) without clearing."""
    from acceleratedvolrenderer_amd import IntegrationAnalyzer
    out, open_ = {}, []
    for shape in SHAPES:
        for kind in (0, 1):
            scene = _graph_scene(shape, sampler=kind)
            whole = IntegrationAnalyzer(scene, None, spp=SPP, seed=SEED)
            split = IntegrationAnalyzer(scene, None, spp=SPP, seed=SEED, max_paths=3 * NPIX)
            open_ += [whole, split]
            _, g = _build_graph(scene, whole.ctx, kind)
            light = (np.random.default_rng(21).random(g.num_vertices, dtype=f32) + f32(0.05)).astype(f32)
            whole.index = split.index = g.index(light)
            r = dict(scene=scene, graph=g, light=light, index=whole.index, whole=whole)
            for md in DEPTHS:
                whole.maxdepth = split.maxdepth = md
                res = whole.analyze(detail=True)
                last = whole.last_pass()
                res_split = split.analyze(detail=True)
                last_split = split.last_pass()
                whole.analyze(0, 2)
                res_ab = whole.analyze(2, 4, clear=False)
                r[md] = dict(res=res, last=last, res_split=res_split, last_split=last_split, res_ab=res_ab)
            out[shape, kind] = r
    yield out
    for a in open_:
        a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ranges", "plain", "hand", "one", "far"])
def test_device_coverage_matches_host_routine(gpu, name):
    from acceleratedvolrenderer_amd import capi
    verts, light, ranges, radius, q, ref = _case(name)
    idx = capi.GraphIndex(verts, light, ranges, radius=radius)
    host = idx.coverage(q)
    ctx = capi.Context(0)
    try:
        dev = ctx.graph_coverage(idx, q)
        # connect and coverage share the context's copy of the index
        assert np.array_equal(ctx.graph_connect(idx, q)[1], idx.connect(q)[1])
        again = ctx.graph_coverage(idx, q)
    finally:
        ctx.close()
    for got in (dev, again):
        assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])
        assert np.array_equal(bits(got[2]), bits(host[2]))
    _check_against_ref(dev, ref, ties_allowed=name == "ranges")


def _replay(r, lp, sampler_kind, md_):
    """One pass (lp = IntegrationAnalyzer.last_pass()) against the oracle's walks, sample by
    sample: the number of analysed scatters and every scatter point."""
    from acceleratedvolrenderer_amd import graph
    from oracle import binding
    scene = r["scene"]
    W, H = scene.film.width, scene.film.height
    npix = W * H
    md = graph.MediumData(scene)
    run = binding.OracleRun(scene, seed=SEED, libm="canonical")
    n = npix * lp["samples"]
    assert len(lp["o"]) == len(lp["count"]) == n and lp["p"].shape == (n, md_, 3)
    cnt_o = np.zeros(n, np.int32)
    pts_o = np.zeros((n, md_, 3), f32)
    for s in range(lp["samples"]):
        o, d, t, idx, rows = [], [], [], [], []
        for pix in range(npix):
            i = s * npix + pix
            ty, t0, t1 = md.box_hits(lp["o"][i], lp["d"][i])
            if ty == 2:
                continue
            oo = lp["o"][i]
            if ty == 0:
                oo = (oo + (lp["d"][i] * t0).astype(f32)).astype(f32)
                tmax = f32(t1 - t0)
            else:
                tmax = t0
            o.append(oo); d.append(lp["d"][i]); t.append(tmax); idx.append(pix); rows.append(i)
        assert len(rows) > npix // 2
        pts, cnt = run.graph_walks(np.array(o, f32), np.array(d, f32), np.array(t, f32), np.array(idx, np.int64), 1,
                                   lp["first"] + s, W, md_, skip_dims=6,
                                   sampler=(sampler_kind, SEED, scene.sampler.pixelsamples, W, H))
        rows = np.array(rows)
        cnt_o[rows] = cnt
        for k in range(md_):
            pts_o[rows, k] = np.where((cnt > k)[:, None], pts[:, k], f32(0))
    # the count and every point, bit-identical for every sample (entries past the count: zero)
    assert np.array_equal(lp["count"], cnt_o)
    assert np.array_equal(bits(lp["p"]), bits(pts_o))
    return cnt_o


@pytest.mark.gpu
@pytest.mark.parametrize("md", DEPTHS)
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
@pytest.mark.parametrize("shape", SHAPES, ids=["12x12x12", "5x12x9"])
def test_analysis_replays_oracle_walks(analysed, shape, kind, md):
    r = analysed[shape, kind]
    a = r[md]
    last, last_split = a["last"], a["last_split"]
    # the split analysis' last pass is the 1-sample pass of sample index 3
    assert (last_split["first"], last_split["samples"]) == (3, 1)
    assert (last["first"], last["samples"]) == (0, SPP)
    _replay(r, last_split, kind, md)
    cnt = _replay(r, last, kind, md)
    for key in ("o", "d", "count", "p", "node", "in_range", "range_sum"):
        x, y = last_split[key], last[key][3 * NPIX:]
        assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y), key
    # each scatter's answer is the host routine's at the read-back point (identity graph_from_render)
    used = np.arange(md)[None, :] < last["count"][:, None]
    node, in_range, range_sum = r["index"].coverage(last["p"][used])
    assert np.array_equal(last["node"][used], node) and np.array_equal(last["in_range"][used], in_range)
    assert np.array_equal(bits(last["range_sum"][used]), bits(range_sum))
    for key in ("node", "in_range", "range_sum"):
        assert np.all(last[key][~used] == 0)
    print(f"{shape} sampler {kind} maxdepth {md}: {r['graph'].num_vertices} vertices, scatters per sample "
          f"{cnt.mean():.3f}, node {node.mean():.3f}, search {np.mean(in_range > 0):.3f}, max in range {in_range.max()}")
    assert cnt.max() == md and np.mean(cnt > 0) >= 0.5
    assert 0 < node.sum() and 0 < np.sum(in_range > 0)
    if md > 1:
        assert 0 < np.sum(cnt == 1) and 0 < np.sum(cnt == 2)     # paths that end between two scatters


def _sums_from_detail(lp, md):
    """The per-pixel sums of one pass, in the stated order: per sample the scatters' range_sum
    added in double in scatter order, then the samples' records in sample-index order."""
    n = len(lp["count"])
    rec = np.zeros(n, np.float64)
    for i in range(n):
        acc = np.float64(0)
        for k in range(lp["count"][i]):
            acc = acc + np.float64(lp["range_sum"][i, k])
        rec[i] = acc
    used = np.arange(md)[None, :] < lp["count"][:, None]
    per = dict(total=lp["count"].astype(np.uint64), node=(lp["node"] * used).sum(1).astype(np.uint64),
               search=((lp["in_range"] > 0) & used).sum(1).astype(np.uint64),
               in_range=(lp["in_range"] * used).sum(1).astype(np.uint64))
    out = {k: v.reshape(lp["samples"], NPIX).sum(0, dtype=np.uint64) for k, v in per.items()}
    acc = np.zeros(NPIX, np.float64)
    for s in range(lp["samples"]):
        for pix in range(NPIX):
            acc[pix] = acc[pix] + rec[s * NPIX + pix]
    out["range_sum"] = acc
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("md", DEPTHS)
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
@pytest.mark.parametrize("shape", SHAPES, ids=["12x12x12", "5x12x9"])
def test_per_pixel_sums(analysed, shape, kind, md):
    a = analysed[shape, kind][md]
    res = a["res"]
    want = _sums_from_detail(a["last"], md)
    for key in ("total", "node", "search", "in_range"):
        got = getattr(res, key)
        assert got.shape == (16, 16) and got.dtype == np.uint64
        assert np.array_equal(got.ravel(), want[key]), key
    assert np.array_equal(bits(res.range_sum.ravel()), bits(want["range_sum"]))
    assert res.total.sum() > 0 and res.range_sum.sum() > 0
    # passes of 3 + 1 samples, and [0, 2) then [2, 4) without clearing: the same bits
    for other in (a["res_split"], a["res_ab"]):
        for x, y in zip(_maps(res), _maps(other)):
            assert np.array_equal(bits(x), bits(y))
    # the reference's figures
    s = res.summary()
    assert s["total"] == int(res.total.sum()) and 0 < s["node_ratio"] <= 1 and 0 < s["search_ratio"] <= 1
    assert s["mean_range"] == float(f32(np.add.reduce(res.range_sum.ravel()) / res.in_range.sum()))
    y, x = np.unravel_index(np.argmax(res.total), res.total.shape)
    px = res.pixel(x, y)
    assert px["total"] == res.total[y, x] and res.format_line(x, y).startswith(f"[ {x}, {y} ], {px['node']} / {px['total']} (")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
def test_against_the_render_at_maxdepth_1(analysed, kind):
    from acceleratedvolrenderer_amd import GraphIntegrator
    r = analysed[(12, 12, 12), kind]
    last = r[1]["last"]
    integ = GraphIntegrator(r["scene"], r["index"], spp=SPP, seed=SEED)
    try:
        rgb, w = integ.render()
        lp = integ.last_pass()
        # an analysis on the render's context leaves the film as it is
        integ.ctx.graph_analyze(r["index"], 0, SPP, SEED, 3)
        total = integ.ctx.graph_analysis_read(NPIX)[0]
        rgb2, w2 = integ.film_sums()
    finally:
        integ.close()
    assert np.array_equal(bits(lp["o"]), bits(last["o"])) and np.array_equal(bits(lp["d"]), bits(last["d"]))
    assert np.array_equal(last["count"], (lp["count"] >= 0).astype(np.int32))
    scat = lp["count"] >= 0
    assert np.array_equal(bits(lp["p"][scat]), bits(last["p"][scat, 0]))
    assert np.array_equal((last["node"][:, 0] > 0) | (last["in_range"][:, 0] > 0), lp["count"] > 0)
    assert np.array_equal(bits(rgb2), bits(rgb)) and np.array_equal(bits(w2), bits(w)) and rgb.sum() > 0
    assert np.array_equal(total.reshape(16, 16), r[3]["res"].total)


@pytest.mark.gpu
def test_state_and_argument_errors(gpu):
    from acceleratedvolrenderer_amd import capi
    from acceleratedvolrenderer_amd.scene import Scene
    idx = capi.GraphIndex(np.array([[0.5, 0.5, 0.5]], f32), np.array([1.0], f32), np.array([0.3], f32), radius=0.1)
    ctx = capi.Context(0, NPIX)
    try:
        with pytest.raises(RuntimeError, match="avr error 3.*film required"):      # nothing set
            ctx.graph_analyze(idx, 0, 1, 0, 1)
        with pytest.raises(RuntimeError, match="avr error 3.*no film"):
            ctx.graph_analysis_read(NPIX)
        ctx.set_scene(_graph_scene(sphere=True))                                  # a boundary sphere
        with pytest.raises(RuntimeError, match="avr error 3.*bounds box"):
            ctx.graph_analyze(idx, 0, 1, 0, 1)
        with pytest.raises(RuntimeError, match="avr error 3.*not avr_graph_analyze"):
            ctx.graph_analyze_last_pass(NPIX, 1, 1)
        one = _graph_scene()
        ctx.set_scene(one)
        with pytest.raises(RuntimeError, match="avr error 1.*sample range"):
            ctx.graph_analyze(idx, 2, 1, 0, 1)
        with pytest.raises(RuntimeError, match="avr error 1.*sample range"):
            ctx.graph_analyze(idx, -1, 1, 0, 1)
        with pytest.raises(RuntimeError, match="avr error 1.*max_depth"):
            ctx.graph_analyze(idx, 0, 1, 0, -1)
        # the detail buffer is refused, not allocated, beyond the path state's bound:
        # 256 samples x 100000 x 24 B against 256 paths x 252 B
        with pytest.raises(RuntimeError, match="avr error 1.*detail buffer.*exceeds"):
            ctx.graph_analyze(idx, 0, 1, 0, 100000, detail=True)
        ctx.graph_analyze(idx, 0, 1, 0, 100000)                                   # without detail: fine
        # graph state: an analysis is no render, a render no analysis, no detail is no detail
        with pytest.raises(RuntimeError, match="avr error 3.*not avr_graph_render"):
            ctx.graph_last_pass(NPIX, 1)
        with pytest.raises(RuntimeError, match="avr error 3.*not avr_graph_analyze"):
            ctx.graph_analyze_last_pass(NPIX, 1, 100000)
        ctx.graph_analyze(idx, 0, 1, 0, 2, detail=True)
        assert ctx.graph_analyze_last_pass(NPIX, 1, 2)[2].shape == (NPIX,)
        with pytest.raises(RuntimeError, match="avr error 1.*max_depth"):
            ctx.graph_analyze_last_pass(NPIX, 1, 3)
        ctx.graph_render(idx, 0, 1, 0)
        with pytest.raises(RuntimeError, match="avr error 3.*not avr_graph_analyze"):
            ctx.graph_analyze_last_pass(NPIX, 1, 2)
        assert ctx.graph_last_pass(NPIX, 1)[3].shape == (NPIX,)
        # max_depth 0 analyses nothing; no light is needed; a new film clears the sums
        ctx.graph_analysis_clear()
        ctx.graph_analyze(idx, 0, 2, 0, 0, detail=True)
        assert all(np.all(a == 0) for a in ctx.graph_analysis_read(NPIX))
        assert np.all(ctx.graph_analyze_last_pass(NPIX, 2, 0)[2] == 0)
        ctx.set_scene(Scene(one.camera, one.film, one.medium, [], sampler=one.sampler))
        ctx.graph_analyze(idx, 0, 2, 0, 2)
        total = ctx.graph_analysis_read(NPIX)[0]
        assert total.sum() > 0
        ctx.graph_analyze(idx, 0, 2, 0, 2)
        assert np.array_equal(ctx.graph_analysis_read(NPIX)[0], 2 * total)
        ctx.set_scene(one)
        assert all(np.all(a == 0) for a in ctx.graph_analysis_read(NPIX))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_graph_analyze_tool(analysed, tmp_path, capsys):
    """tools/graph_analyze.py over a graph file: the reference's line per pixel and depth, the
    frame summary, the JSON and the three maps, equal to IntegrationAnalyzer.from_file's."""
    import json
    import sys
    from acceleratedvolrenderer_amd import IntegrationAnalyzer, imageio
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import graph_analyze
    finally:
        sys.path.pop(0)
    r = analysed[(12, 12, 12), 0]
    path = str(tmp_path / "graph.txt")
    r["graph"].save(path, r["light"])
    prefix = str(tmp_path / "out" / "uni")
    preset = ["--scene", "s-uniform", "--n", "4", "--width", "16", "--height", "16", "--sampler", "independent",
              "--filter", "box", "--spp", "4", "--seed", str(SEED)]
    assert graph_analyze.main(preset + ["--graph", path, "--maxdepth", "1,2", "--pixels", "8,8", "3,12",
                                        "--out", prefix]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert sorted(os.listdir(tmp_path / "out")) == sorted(
        ["uni_analysis.json"] + [f"uni_d{d}_{m}.exr" for d in (1, 2) for m in ("node_ratio", "search_ratio", "mean_range")])
    out = json.loads(open(prefix + "_analysis.json").read())
    assert [e["maxdepth"] for e in out["depths"]] == [1, 2] and out["graph"]["vertices"] == r["graph"].num_vertices
    an = IntegrationAnalyzer.from_file(graph_analyze.make_scene("s-uniform", 4, 16, 16, "independent", 4, "box"), path,
                                       maxdepth=2, spp=4, seed=SEED)
    try:
        res = an.analyze()
    finally:
        an.close()
    assert res.total.sum() > 0 and out["depths"][1]["frame"] == res.summary()
    assert out["depths"][0]["frame"]["total"] < out["depths"][1]["frame"]["total"]
    assert out["depths"][1]["pixels"][0] == dict(x=8, y=8, **res.pixel(8, 8))
    # per depth: the two pixels' lines, the frame's, a blank line
    assert lines[4] == res.format_line(8, 8) and lines[5] == res.format_line(3, 12) and lines[6] == res.format_summary()
    assert lines[0].startswith("[ 8, 8 ], ") and lines[2].startswith("frame, ") and lines[3] == ""
    for name, img in zip(("node_ratio", "search_ratio", "mean_range"), res.ratio_maps()):
        got, channels, _ = imageio.read_exr(f"{prefix}_d2_{name}.exr")
        assert channels == ["Y"] and np.array_equal(got[:, :, 0], img)
