"""Graph files in the reference's text format (graph_io.py; graph.cpp:15-24, 237-416, 644-663).

tests/golden/graph_free_small.txt is a hand-written file of a 4-vertex free graph with
lighting and search ranges at precision 6, laid out after graph.cpp's stream code
(FreeGraph::WriteToStream, Graph::WriteToStream, WriteVertexData, operator<<(Point3)). The
reference did not produce it (its tools need NanoVDB to build, which this project does not carry).

CPU (not gpu): the fixture's bytes and values, round trips, id order, the uniform header, the
error messages, the tool's --help. GPU (gpu): a graph saved and rendered from its file, and
tools/graph_maker.py end to end.
"""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_free_small.txt")
f32 = np.float32

POINTS = np.array([[0, 0, 0], [0.1, 0.2, 0.3], [-1.5, 2.5e-05, 1e+10], [0.123457, 100, 1e-07]], f32)
LIGHT = np.array([1, 0.5, 0.333333, 2], f32)
RANGES = np.array([0.25, 0.125, 0.0625, 0.1], f32)


def _graph(points, radius, search_range=None, **kw):
    return types.SimpleNamespace(points=points, radius=radius, search_range=search_range, **kw)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------------------- CPU

def test_golden_fixture_layout():
    """The fixture itself: header lines without a trailing space, vertex lines with one."""
    lines = open(GOLDEN, newline="").read().split("\n")
    assert lines[:4] == ["basic", "free 0.05", "False False False True True", "4 0 0 4 0 0"]
    assert lines[-1] == "" and len(lines) == 9
    assert all(l.endswith(" ") and not l.endswith("  ") and len(l.split()) == 6 for l in lines[4:8])


def test_read_golden():
    from acceleratedvolrenderer_amd import graph_io
    g = graph_io.read_graph(GOLDEN)
    assert (g.description, g.kind) == ("basic", "free")
    assert g.radius == f32(0.05) and g.spacing is None
    assert g.flags == dict(use_coors=False, use_samples=False, use_ray_vertex_types=False, use_lighting=True,
                           use_render_search_range=True)
    assert (g.cur_vertex_id, g.cur_edge_id, g.cur_path_id, g.num_vertices) == (4, 0, 0, 4)
    assert g.points.dtype == f32 and np.array_equal(_bits(g.points), _bits(POINTS))
    assert np.array_equal(_bits(g.light_scalar), _bits(LIGHT)) and np.array_equal(_bits(g.search_range), _bits(RANGES))
    assert g.vertex_type is None and g.samples is None and g.coors is None
    assert len(g.edge_from) == 0 and g.edge_samples is None and g.paths == []


def test_write_reproduces_golden(tmp_path):
    from acceleratedvolrenderer_amd import graph_io
    want = open(GOLDEN, "rb").read()
    out = tmp_path / "g.txt"
    graph_io.write_graph(str(out), _graph(POINTS, f32(0.05), RANGES), LIGHT, precision=6)
    assert out.read_bytes() == want
    # and from the record read back (its own light_scalar)
    graph_io.write_graph(str(out), graph_io.read_graph(GOLDEN), precision=6)
    assert out.read_bytes() == want
    # without ranges / without light the flags and the columns go
    graph_io.write_graph(str(out), _graph(POINTS, f32(0.05)), LIGHT, precision=6)
    lines = out.read_text().split("\n")
    assert lines[2] == "False False False True False" and lines[5] == "1 0.1 0.2 0.3 0.5 "
    graph_io.write_graph(str(out), _graph(POINTS, f32(0.05)), None, precision=6, description="other")
    lines = out.read_text().split("\n")
    assert lines[0] == "other" and lines[2] == "False False False False False" and lines[5] == "1 0.1 0.2 0.3 "
    with pytest.raises(ValueError, match="one light_scalar per vertex"):
        graph_io.write_graph(str(out), _graph(POINTS, f32(0.05)), LIGHT[:3])
    with pytest.raises(ValueError, match="one token"):
        graph_io.write_graph(str(out), _graph(POINTS, f32(0.05)), LIGHT, description="two words")


def _random_graph(n=1000, seed=4):
    rng = np.random.default_rng(seed)
    # float32 values of every magnitude: random bit patterns of finite, normal floats
    def floats(count):
        bits = rng.integers(0, 2 ** 32, size=count, dtype=np.uint64).astype(np.uint32)
        exp = (bits >> 23) & 0xFF
        bits[(exp == 0) | (exp == 255)] = np.float32(1.5).view(np.uint32)
        return bits.view(f32)
    pts = floats(3 * n).reshape(n, 3)
    pts[: n // 2] = rng.random((n // 2, 3), dtype=f32)
    return pts, np.abs(floats(n)), np.abs(floats(n))


def test_round_trips(tmp_path):
    from acceleratedvolrenderer_amd import graph_io
    pts, light, ranges = _random_graph()
    radius = f32(0.0123456789)
    path = str(tmp_path / "g.txt")
    graph_io.write_graph(path, _graph(pts, radius, ranges), light)           # precision 9
    g = graph_io.read_graph(path)
    assert np.array_equal(_bits(g.points), _bits(pts)) and np.array_equal(_bits(g.light_scalar), _bits(light))
    assert np.array_equal(_bits(g.search_range), _bits(ranges)) and _bits(g.radius) == _bits(radius)
    graph_io.write_graph(path, _graph(pts, radius, ranges), light, precision=6)
    g6 = graph_io.read_graph(path)
    assert not np.array_equal(_bits(g6.points), _bits(pts)) and not np.array_equal(_bits(g6.light_scalar), _bits(light))
    np.testing.assert_allclose(g6.points, pts, rtol=1e-5)      # 6 significant digits: 5e-6, plus the float rounding
    assert _bits(g6.radius) != _bits(radius)


def test_edges_round_trip(tmp_path):
    from acceleratedvolrenderer_amd import graph_io
    pts, light, _ = _random_graph(50)
    g = _graph(pts, f32(0.1), samples=np.arange(50, dtype=np.int32) + 1,
               edge_from=np.array([0, 3, 7], np.int32), edge_to=np.array([3, 7, 49], np.int32),
               edge_samples=np.array([2, 1, 5], np.int32))
    path = str(tmp_path / "g.txt")
    graph_io.write_graph(path, g, light, edges=True)
    lines = open(path).read().split("\n")
    assert lines[2] == "False True False True False" and lines[3] == "50 3 0 50 3 0"
    assert lines[4 + 50] == "0 0 3 2 " and lines[4 + 52] == "2 7 49 5 "
    r = graph_io.read_graph(path)
    assert np.array_equal(r.samples, g.samples) and np.array_equal(r.edge_id, [0, 1, 2])
    assert np.array_equal(r.edge_from, g.edge_from) and np.array_equal(r.edge_to, g.edge_to)
    assert np.array_equal(r.edge_samples, g.edge_samples) and np.array_equal(_bits(r.light_scalar), _bits(light))
    # without edges=True the edge count still shows in curEdgeId
    graph_io.write_graph(path, g, light)
    assert open(path).read().split("\n")[2:4] == ["False False False True False", "50 3 0 50 0 0"]


def test_every_flag_and_paths_are_read(tmp_path):
    """A stream with all five flags, edges and paths, as Graph::WriteToStream lays it out."""
    from acceleratedvolrenderer_amd import graph_io
    path = tmp_path / "full.txt"
    path.write_text("dbg\nfree 0.5\nTrue True True True True\n2 1 1 2 1 1\n"
                    "1 1 2 3 0 0.5 7 0.25 4 5 6 \n0 0 0 0 1 1.5 9 0.75 -1 0 2 \n"
                    "0 0 1 3 \n0 2 0 1 \n")
    g = graph_io.read_graph(str(path))
    assert g.vertex_type.tolist() == [1, 0] and g.light_scalar.tolist() == [1.5, 0.5]
    assert g.samples.tolist() == [9, 7] and g.search_range.tolist() == [0.75, 0.25]
    assert g.coors.tolist() == [[-1, 0, 2], [4, 5, 6]] and g.points.tolist() == [[0, 0, 0], [1, 2, 3]]
    assert (g.edge_from.tolist(), g.edge_to.tolist(), g.edge_samples.tolist()) == ([0], [1], [3])
    assert len(g.paths) == 1 and g.paths[0][0] == 0 and g.paths[0][1].tolist() == [0, 1]


def test_vertex_lines_in_any_order(tmp_path):
    from acceleratedvolrenderer_amd import graph_io
    lines = open(GOLDEN).read().split("\n")
    shuffled = lines[:4] + [lines[6], lines[4], lines[7], lines[5]] + [""]
    path = tmp_path / "s.txt"
    path.write_text("\n".join(shuffled))
    g = graph_io.read_graph(str(path))
    assert np.array_equal(_bits(g.points), _bits(POINTS)) and np.array_equal(_bits(g.light_scalar), _bits(LIGHT))
    # tokens, not lines: the same stream on one line reads the same
    path.write_text(" ".join(shuffled))
    assert np.array_equal(_bits(graph_io.read_graph(str(path)).search_range), _bits(RANGES))


def test_uniform_header_reads_but_does_not_load(tmp_path):
    from acceleratedvolrenderer_amd import graph, graph_io
    text = open(GOLDEN).read().replace("free 0.05", "uniform 0.25")
    path = tmp_path / "u.txt"
    path.write_text(text)
    g = graph_io.read_graph(str(path))
    assert g.kind == "uniform" and g.spacing == f32(0.25) and g.radius is None and g.num_vertices == 4
    with pytest.raises(ValueError, match="uniform graph"):
        graph.load_index(str(path))


def test_malformed_files_are_rejected(tmp_path):
    from acceleratedvolrenderer_amd import graph, graph_io
    lines = open(GOLDEN).read().split("\n")
    path = tmp_path / "bad.txt"

    def expect(new_lines, pattern, load=graph_io.read_graph):
        path.write_text("\n".join(new_lines))
        with pytest.raises(ValueError, match=pattern):
            load(str(path))

    expect(lines[:7] + [""], r"line 7: file ends where a vertex line is expected")            # truncated
    expect(lines[:7] + ["3 0.123457 100"], r"line 8: file ends where a vertex line is expected")
    expect(lines[:3], r"line 3: file ends where curVertexId is expected")
    expect([], r"line 1: file ends where the description is expected")
    expect(lines[:6] + ["3" + lines[6][1:]] + lines[7:], r"line 7: vertex id 2 is missing.*sequential vertex ids 0..3")
    expect(lines[:6] + ["1" + lines[6][1:]] + lines[7:], r"line 7: vertex id 1 is out of place or repeated")
    expect(lines[:5] + ["1 0.1 zwei 0.3 0.5 0.125 "] + lines[6:], r"line 6: a number expected, found 'zwei'")
    expect(lines[:5] + ["1.5 0.1 0.2 0.3 0.5 0.125 "] + lines[6:], r"line 6: an integer expected, found '1.5'")
    expect(lines[:1] + ["tree 0.05"] + lines[2:], r'line 2: "free" or "uniform" expected, found \'tree\'')
    expect(lines[:2] + ["False False False Yes True"] + lines[3:], r"line 3: True or False expected, found 'Yes'")
    expect(lines[:3] + ["4 0 0 -4 0 0"] + lines[4:], r"line 4: the vertex count expected")
    # a readable file that cannot be rendered: no lighting
    no_light = lines[:2] + ["False False False False True"] + lines[3:4] + \
        [" ".join(l.split()[:4] + l.split()[5:]) + " " for l in lines[4:8]] + [""]
    path.write_text("\n".join(no_light))
    g = graph_io.read_graph(str(path))
    assert g.light_scalar is None and np.array_equal(_bits(g.search_range), _bits(RANGES))
    with pytest.raises(ValueError, match="without lighting .useLighting False."):
        graph.load_index(str(path))


def test_load_index_and_save(tmp_path):
    """load_index builds the host index of the file's vertices: the same connect results as
    the index of the arrays; FreeGraph.save is write_graph."""
    from acceleratedvolrenderer_amd import capi, graph
    rng = np.random.default_rng(6)
    pts = rng.random((500, 3), dtype=f32)
    light = (rng.random(500, dtype=f32) + f32(0.1)).astype(f32)
    ranges = (f32(0.05) + f32(0.2) * rng.random(500, dtype=f32)).astype(f32)
    q = rng.random((200, 3), dtype=f32)
    g = _graph(pts, f32(0.08), ranges)
    path = str(tmp_path / "g.txt")
    graph.FreeGraph.save(g, path, light)
    idx = graph.load_index(path)
    assert idx.num_vertices == 500 and idx.has_search_range and idx.radius == float(f32(0.08))
    a_l, a_c = idx.connect(q)
    b_l, b_c = capi.GraphIndex(pts, light, ranges, radius=f32(0.08)).connect(q)
    assert np.array_equal(a_c, b_c) and np.array_equal(_bits(a_l), _bits(b_l)) and a_c.max() > 0
    assert hasattr(graph.GraphIntegrator, "from_file")


def test_graph_maker_help_runs_without_a_gpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "graph_maker.py"), "--help"],
                         capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0, out.stderr
    assert "--out" in out.stdout and "--config" in out.stdout and "PREFIX_stats.json" in out.stdout


# ---------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _cloud_scene(torch, n=32):
    """S-cloud's n³ GridMedium with its distant light alone, 64x48, 1 spp."""
    from acceleratedvolrenderer_amd import capi, scenes
    from acceleratedvolrenderer_amd.scene import Scene
    density = torch.empty((n, n, n), dtype=torch.float32, device="cuda:0")
    gen = capi.Context(0)
    gen.generate_cloud(density.data_ptr(), n, 0, n ** 3)
    gen.sync()
    gen.close()
    cloud = scenes.s_cloud(density, width=64, height=48, spp=1)
    return Scene(cloud.camera, cloud.film, cloud.medium, cloud.lights[:1], sampler=cloud.sampler)


@pytest.mark.gpu
def test_render_from_file_is_the_in_memory_render(gpu, tmp_path):
    from acceleratedvolrenderer_amd import GraphIntegrator, graph
    scene = _cloud_scene(gpu)
    integ = GraphIntegrator(scene, None, spp=1, seed=3)
    cfg = graph.GraphBuilderConfig(radius_modifier=60.0, max_depth=12, dimension_steps=8, iterations_per_step=6,
                                   render_search_range={"active": True, "neighboursToUse": 4})
    in_dir = (-np.asarray(scene.light_w[0], f32)).astype(f32)
    smp = graph.GraphSampling(sampler=0, seed=3, samples_per_pixel=16, resolution=(64, 64))
    md = graph.MediumData(scene)
    g = graph.FreeGraphBuilder(integ.ctx, md, in_dir, smp, cfg, search_ranges="device").build_graph()
    lc = graph.LightingCalculator(integ.ctx, g, md, in_dir, smp,
                                  graph.LightingCalculatorConfig(light_iterations=8, points_on_radius_light=1, bounces=[4]))
    assert lc.compute_final_light() == 4
    integ.index = g.index(lc.light_scalar)
    rgb, w = integ.render()
    integ.close()
    assert rgb.sum() > 0 and np.all(np.isfinite(rgb))
    p9, p6 = str(tmp_path / "g9.txt"), str(tmp_path / "g6.txt")
    g.save(p9, lc.light_scalar)
    g.save(p6, lc.light_scalar, precision=6)
    sums = {}
    for path in (p9, p6):
        fi = GraphIntegrator.from_file(scene, path, spp=1, seed=3)
        sums[path] = fi.render()
        fi.close()
    assert np.array_equal(sums[p9][0].view(np.uint32), rgb.view(np.uint32)) and np.array_equal(sums[p9][1], w)
    assert np.all(np.isfinite(sums[p6][0])) and sums[p6][0].sum() > 0
    assert not np.array_equal(sums[p6][0], rgb)
    print(f"{g.num_vertices} vertices; film sum {rgb.sum():.6e} in memory and at precision 9, "
          f"{sums[p6][0].sum():.6e} at precision 6")


@pytest.mark.gpu
def test_graph_maker_tool(gpu, tmp_path):
    from acceleratedvolrenderer_amd import graph
    cfg = {"graphBuilder": {"radiusModifier": 60.0, "maxDepth": 12, "dimensionSteps": 8, "iterationsPerStep": 6,
                            "renderSearchRange": {"active": True, "neighboursToUse": 4}},
           "lightingCalculator": {"lightIterations": 8, "pointsOnRadiusLight": 1, "bounces": [1, 3]}}
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    prefix = str(tmp_path / "out" / "cloud")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "graph_maker.py"), "--scene", "s-cloud", "--n", "32",
                          "--config", str(tmp_path / "cfg.json"), "--out", prefix], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Depth 2 (1 bounces)" in out.stdout and "Depth 4 (3 bounces)" in out.stdout
    assert sorted(os.listdir(tmp_path / "out")) == ["cloud_d2.txt", "cloud_d4.txt", "cloud_stats.json"]
    stats = json.loads(open(prefix + "_stats.json").read())
    assert stats["amounts"]["vertices"] > 4 and stats["amounts"]["edges"] > 0       # 4 neighbours need 5 vertices
    assert stats["in_node_path_length"]["avg"] >= 0 and stats["render_search_range"]["avg"] > 0
    assert 0 < stats["sizes"]["node_radius"] < stats["sizes"]["scene_radius"]
    for stage in ("build_graph", "search_ranges", "light_vector", "transport_matrix", "final_light", "write"):
        assert stage in stats["seconds"]
    assert [f["depth"] for f in stats["files"]] == [2, 4]
    idx = graph.load_index(prefix + "_d2.txt")
    assert idx.num_vertices == stats["amounts"]["vertices"] and idx.has_search_range
