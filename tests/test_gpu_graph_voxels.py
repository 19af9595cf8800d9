"""The voxel boundary on the device (graph::VoxelBoundary, graph/voxels/voxel_boundary.cpp):
k_graph_capture bit for bit against the CPU oracle's crossings and majorant DDA; the direction
is not normalised; the reference's own bundles; the device conversion from points and the
device floods against the host's, byte for byte; the pipeline from the medium to a rendered
uniform graph; the state and argument errors that need a context. The host side and the flood
cases are tests/test_graph_voxels.py.

avr_graph_walks takes every medium type (it has no refusal of its own), and so does
avr_graph_capture: there is no medium type to refuse, and no test of one.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SEED = 3


def _cpu_file():
    """tests/test_graph_voxels.py as a module: its flood cases, host runs and restatements."""
    spec = importlib.util.spec_from_file_location("avr_test_graph_voxels", os.path.join(ROOT, "tests", "test_graph_voxels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def cpu():
    return _cpu_file()


def _density():
    """32^3, zero but for two overlapping balls (radius 9 voxels at the centre, radius 5 offset
    by (7, 3, -4)), values in [0.5, 1] inside: the 16^3 majorant has empty cells all round."""
    rng = np.random.default_rng(8)
    z, y, x = np.meshgrid(*[np.arange(32) + 0.5] * 3, indexing="ij")
    ball = lambda cx, cy, cz, r: (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r
    inside = ball(16, 16, 16, 9) | ball(16 + 7, 16 + 3, 16 - 4, 5)
    return np.where(inside, 0.5 + 0.5 * rng.random((32, 32, 32)), 0.0).astype(f32)


def _scene(majorant_res=(16, 16, 16), sphere=False, spp=4):
    """tests/test_graph_uniform.py's _graph_scene recipe with the two-ball medium."""
    from acceleratedvolrenderer_amd import scenes, GridMedium, IndependentSampler
    from acceleratedvolrenderer_amd.scene import Scene
    base = scenes.s_uniform(n=2, width=16, height=16, variant="scatter")
    med = GridMedium(_density(), sigma_a=0.4, sigma_s=6.0, g=0.5, majorant_res=majorant_res)
    return Scene(base.camera, base.film, med, base.lights[:1], sampler=IndependentSampler(pixelsamples=spp),
                 interface_sphere=((0.5, 0.5, 0.5), 0.45) if sphere else None)


def _length(v):
    return f32(np.sqrt(f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))))


def _unit_directions():
    """The six axis directions and 18 random unit vectors whose float32 length is exactly 1, so
    that the oracle's Normalize is the identity on them."""
    dirs = [np.array(v, f32) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    rng = np.random.default_rng(5)
    while len(dirs) < 24:
        v = rng.normal(size=3)
        v = (v / np.linalg.norm(v)).astype(f32)
        if _length(v) == f32(1) and np.all(v != 0):
            dirs.append(v)
    return np.array(dirs, f32)


NUM_STEPS = 8


def _bundles(md, cpu, dirs):
    """Orthonormal bundles along `dirs`: origin = center - dir * 2 R, (xv, yv) =
    CoordinateSystem(dir) * (R / NUM_STEPS), in float32."""
    R = md.max_dist_to_center
    step = f32(R / f32(NUM_STEPS))
    o, xs, ys = [], [], []
    for d in dirs:
        o.append((md.bounds_center - (d * f32(R * f32(2))).astype(f32)).astype(f32))
        x, y = cpu._coordinate_system(d)
        xs.append((x * step).astype(f32))
        ys.append((y * step).astype(f32))
    return np.array(o, f32), np.array(xs, f32), np.array(ys, f32)


def _expected(run, hits, o, d, xv, yv):
    """Per ray of the bundles, in ray order: (captured, point, kind) from the oracle: the
    crossing `hits(p, d)`, the skip to the entry in float32, dda_segments from there and the
    first segment with sigma_maj != 0. kind: 0 missed the primitive, 1 started inside, 2 crossed
    only empty cells, 3 captured."""
    flags, pts, kinds = [], [], []
    for b in range(len(o)):
        assert run_normalize_is_identity(d[b])
        for i in range(-NUM_STEPS, NUM_STEPS + 1):
            for j in range(-NUM_STEPS, NUM_STEPS + 1):
                p = ((o[b] + (xv[b] * f32(i)).astype(f32)).astype(f32) + (yv[b] * f32(j)).astype(f32)).astype(f32)
                ty, t0, _ = hits(p, d[b])
                flag, q, kind = False, np.zeros(3, f32), 0
                if ty == 3:
                    kind = 1
                elif ty == 0:
                    kind = 2
                    p = (p + (d[b] * f32(t0)).astype(f32)).astype(f32)
                    for seg in run.dda_segments(p, d[b], lambda_u=0.0):
                        if seg[2] != 0:
                            flag, q, kind = True, (p + (d[b] * seg[0]).astype(f32)).astype(f32), 3
                            break
                flags.append(flag)
                pts.append(q)
                kinds.append(kind)
    return np.array(flags), np.array(pts, f32), np.array(kinds)


def run_normalize_is_identity(d):
    """Normalize(d) = d / Length(d) with Length = sqrt((x^2 + y^2) + z^2) in float32."""
    return _length(d) == f32(1) and np.array_equal((d / _length(d)).astype(f32), d)


def _capture_against_oracle(cpu, scene, primitive, majorant_res=None):
    from acceleratedvolrenderer_amd import capi, graph
    from oracle import binding
    md = graph.MediumData(scene, primitive)
    dirs = _unit_directions()
    o, xv, yv = _bundles(md, cpu, dirs)
    ctx = capi.Context(0)
    try:
        ctx.set_scene(scene)
        ctx.set_graph_geometry(md.geometry)
        if majorant_res is not None:
            ctx.set_majorant_res(majorant_res)
        pts, flag, n = ctx.graph_capture(o, dirs, xv, yv, NUM_STEPS)
        pts4, flag4, n4 = ctx.graph_capture(o, (dirs * f32(4)).astype(f32), xv, yv, NUM_STEPS)
    finally:
        ctx.close()
    run = binding.OracleRun(scene, max_depth=1, seed=0)
    if primitive == "interface":
        sph = np.asarray(scene.interface_sphere_render, f32)
        hits = lambda p, d: binding.graph_sphere_hits(sph[:3], sph[3], p, d)
    else:
        hits = run.graph_box_hits
    eflag, epts, kinds = _expected(run, hits, o, dirs, xv, yv)
    counts = [int(np.count_nonzero(kinds == k)) for k in range(4)]
    print(f"{primitive}, majorant {scene.medium.majorant_res}: {len(flag)} rays: {counts[0]} miss the primitive, "
          f"{counts[1]} start inside, {counts[2]} cross only empty cells, {counts[3]} capture")
    assert len(flag) == 24 * 289 == 6936 == len(eflag)
    assert counts[0] > 0 and counts[2] > 0 and counts[3] > 0
    assert np.array_equal(flag, eflag) and n == counts[3]
    assert np.array_equal(pts.view(np.uint32), epts.view(np.uint32))
    # the direction is used as given: scaled by 4 (exact through the slab test and the DDA) the
    # same rays capture the same points; a kernel that normalised would still pass this, one that
    # normalised only the DDA's direction and not the segment bounds would not
    assert np.array_equal(flag4, flag) and n4 == n
    assert np.array_equal(pts4.view(np.uint32), pts.view(np.uint32))


def test_capture_matches_the_oracle_bit_for_bit(gpu, cpu):
    _capture_against_oracle(cpu, _scene(), "box")


def test_capture_with_another_majorant_resolution(gpu, cpu):
    _capture_against_oracle(cpu, _scene(majorant_res=(5, 8, 3)), "box", majorant_res=(5, 8, 3))


def test_capture_with_an_interface_sphere(gpu, cpu):
    _capture_against_oracle(cpu, _scene(sphere=True), "interface")


def test_reference_bundles_capture_reproducibly_inside_the_bounds(gpu):
    from acceleratedvolrenderer_amd import capi, graph
    scene = _scene()
    md = graph.MediumData(scene)
    ctx = capi.Context(0)
    try:
        ctx.set_scene(scene)
        vb = graph.VoxelBoundary(ctx, md, num_steps=NUM_STEPS, frame="reference")
        o, d, xv, yv = vb.bundles(45)
        a = ctx.graph_capture(o, d, xv, yv, NUM_STEPS)
        b = ctx.graph_capture(o, d, xv, yv, NUM_STEPS)
        pts = vb.capture_points(45)
    finally:
        ctx.close()
    assert len(o) == 22 and len(a[1]) == 22 * 289 == vb.last_rays
    assert np.array_equal(a[1], b[1]) and a[2] == b[2] == int(a[1].sum()) > 0
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(pts, a[0][a[1]])
    pad = 1e-4 * float(np.linalg.norm(md.pmax.astype(np.float64) - md.pmin.astype(np.float64)))
    assert np.all(pts >= md.pmin - pad) and np.all(pts <= md.pmax + pad)
    print(f"reference bundles: {a[2]} of {len(a[1])} rays capture")


@pytest.fixture(scope="module")
def captured(gpu):
    """The two-ball medium's boundary points from 62 bundles of 33 x 33 rays, once."""
    from acceleratedvolrenderer_amd import capi, graph
    scene = _scene()
    md = graph.MediumData(scene)
    ctx = capi.Context(0)
    try:
        ctx.set_scene(scene)
        pts = graph.VoxelBoundary(ctx, md, num_steps=16).capture_points(30)
    finally:
        ctx.close()
    assert len(pts) > 5000
    return scene, md, pts


def test_device_conversion_equals_the_host(captured):
    from acceleratedvolrenderer_amd import capi, graph
    scene, md, pts = captured
    zeros = np.zeros(len(pts), f32)
    ctx = capi.Context(0)
    try:
        vb = graph.VoxelBoundary(ctx, md)
        tried = vb.bisect_spacing(pts, 300)
        host_tried = graph.VoxelBoundary(None, md, device=False).bisect_spacing(pts, 300)
        assert [float(t) for t in tried] == [float(t) for t in host_tried] and len(set(float(t) for t in tried)) == 10
        for spacing in [f32(1 / 16), f32(0.05)] + tried:
            host = capi.GraphUniform.from_points(pts, zeros, spacing)
            dev = capi.GraphUniform.from_points_device(ctx, pts, spacing)
            assert ctx.graph_uniform_count(pts, spacing) == host.num_vertices == dev.num_vertices
            assert np.array_equal(dev.coors, host.coors) and np.array_equal(dev.vertex_of, host.vertex_of)
            assert np.all(dev.light_scalar == 0) and dev.spacing == host.spacing
            print(f"spacing {float(spacing):.6f}: {len(pts)} points in {host.num_vertices} voxels")
        # the host's errors, the lowest bad point named
        bad = pts.copy()
        bad[[700, 41, 3000], 1] = [np.nan, 3e6, -np.inf]
        for call in (lambda: capi.GraphUniform.from_points(bad, zeros, 0.05), lambda: ctx.graph_uniform_count(bad, 0.05),
                     lambda: capi.GraphUniform.from_points_device(ctx, bad, 0.05)):
            with pytest.raises(RuntimeError, match="vertex 41: coordinate outside"):
                call()
        for spacing in (0.0, -1.0, np.nan, np.inf):
            with pytest.raises(RuntimeError, match="spacing must be positive"):
                ctx.graph_uniform_count(pts, spacing)
        with pytest.raises(RuntimeError, match="at least one vertex"):
            ctx.graph_uniform_count(np.zeros((0, 3), f32), 0.05)
    finally:
        ctx.close()


def test_device_floods_equal_the_host(captured, cpu):
    from acceleratedvolrenderer_amd import capi, graph
    scene, md, pts = captured
    ctx = capi.Context(0)
    try:
        for name in sorted(cpu.CASES):
            host, dev = cpu.host_run(name), cpu.run_case(name, ctx)
            for h, d in zip(host.states, dev.states):
                assert np.array_equal(h, d), name
            assert np.array_equal(host.g.coors, dev.g.coors) and np.array_equal(host.every.coors, dev.every.coors)
            assert host.g.visited == dev.g.visited and host.g.levels == dev.g.levels
            assert host.lowest.levels == dev.lowest.levels
        # the captured medium at spacing 1/16
        full = graph.UniformGraph(capi.GraphUniform.from_points(pts, np.zeros(len(pts), f32), f32(1 / 16)))
        out = []
        for c in (None, ctx):
            vb = graph.VoxelBoundary(c, md, device=c is not None)
            g = vb.to_single_layer(full)
            states = [g.voxels.state().copy()]
            for start in (None, "all", len(g.old_ids) - 1):
                filled = vb.fill_inside(g, start=start)
                states.append(g.voxels.state().copy())
            out.append((g, states, filled))
        (gh, sh, fh), (gd, sd, fd) = out
        for h, d in zip(sh, sd):
            assert np.array_equal(h, d)
        assert np.array_equal(gh.coors, gd.coors) and np.array_equal(fh.coors, fd.coors)
        assert gh.levels == gd.levels and gh.visited == gd.visited
        print(f"captured: {full.num_vertices} vertices, {gd.num_vertices} single layer, {gd.visited} of {gd.voxels.cells} "
              f"cells visited in {gd.levels} levels, {fd.num_vertices} filled")
    finally:
        ctx.close()


def test_end_to_end_from_the_medium_to_a_rendered_uniform_graph(gpu):
    """capture -> single layer -> fill -> light vector -> uniform render. Measured on an MI355X:
    582 voxels captured at spacing 1/16, 413 in the single layer, 1117 filled, 5742 of 6859
    cells visited; 217 of the 1024 samples scatter in a voxel, all 217 in a lit one; image mean
    1.98e-2."""
    from acceleratedvolrenderer_amd import GraphIntegrator, capi, graph
    scene = _scene(spp=4)
    md = graph.MediumData(scene)
    integ = GraphIntegrator(scene, None, spp=4, seed=SEED)
    try:
        vb = graph.VoxelBoundary(integ.ctx, md, num_steps=16)
        boundary = vb.capture_boundary(spacing=f32(1 / 16), equator_step=30)
        filled = vb.fill_inside(boundary)
        as_set = lambda c: {tuple(int(v) for v in p) for p in c}
        single, inside = as_set(boundary.coors), as_set(filled.coors)
        cast = as_set(boundary.voxels.cells_with(capi.VOXEL_CAST))
        assert single <= inside and not (cast & inside) and len(inside) >= len(single) > 0
        assert len(inside) > 2 * len(single)           # two solid balls: far more inside than on the surface
        in_dir = (-np.asarray(scene.light_w[0], f32)).astype(f32)
        smp = graph.GraphSampling(sampler=0, seed=SEED, samples_per_pixel=8, resolution=(1024, 1024))
        radius = f32(graph.same_spot_radius(md) * f32(20))
        light = integ.ctx.graph_light(smp.struct(), filled.points, in_dir, radius, 1, 8, md.max_dist_to_center)
        assert np.all(np.isfinite(light)) and np.count_nonzero(light) > len(light) // 2
        lit = capi.GraphUniform(filled.coors, light, filled.spacing)
        integ.index = lit
        integ.light_scale = 1.0
        img = integ.get_image(*integ.render())
        last = integ.last_pass()
    finally:
        integ.close()
    found = last["count"] == 1
    ids, l = lit.lookup(last["p"][found])
    print(f"{boundary.num_captured} captured, {len(single)} single layer, {len(inside)} filled, {boundary.visited} cells "
          f"visited; {int(found.sum())} of {len(found)} samples scatter in a voxel, {int(np.count_nonzero(l))} in a lit one; "
          f"image mean {img.mean():.4e}")
    assert np.all(ids >= 0) and np.count_nonzero(l) >= 1
    assert np.all(np.isfinite(img)) and img.mean() > 0


def test_state_and_argument_errors(gpu):
    from acceleratedvolrenderer_amd import capi
    lib = capi.load()
    fp = lambda a: a.ctypes.data_as(capi.c_float_p)
    v = np.zeros((2, 3), f32)
    v[:, 2] = 1
    out = np.zeros((2 * 9, 4), f32)
    cnt = ctypes.c_longlong(0)
    err = lambda: lib.avr_last_error().decode()
    ctx = capi.Context(0)
    try:
        with pytest.raises(RuntimeError, match="avr error 3.*medium required"):     # capture before a medium is set
            ctx.graph_capture(v, v, v, v, 1)
        ctx.set_scene(_scene())
        assert ctx.graph_capture(v, v, v, v, 1)[0].shape == (18, 3)
        assert ctx.graph_capture(v, v, v, v, 0)[0].shape == (2, 3)
        for args in ((None, fp(v), fp(v), fp(v)), (fp(v), None, fp(v), fp(v)), (fp(v), fp(v), None, fp(v)),
                     (fp(v), fp(v), fp(v), None)):
            assert lib.avr_graph_capture(ctx.h, 2, *args, 1, fp(out), ctypes.byref(cnt)) == 1 and "null" in err()
        assert lib.avr_graph_capture(ctx.h, 2, fp(v), fp(v), fp(v), fp(v), 1, None, ctypes.byref(cnt)) == 1
        assert lib.avr_graph_capture(ctx.h, 2, fp(v), fp(v), fp(v), fp(v), 1, fp(out), None) == 1
        for nb, steps in ((0, 1), (-1, 1), (2, -1)):
            assert lib.avr_graph_capture(ctx.h, nb, fp(v), fp(v), fp(v), fp(v), steps, fp(out), ctypes.byref(cnt)) == 1
            assert "bad capture arguments" in err()
        for nb, steps in ((1, 30000), (3, 16383), (2, 2 ** 30)):                     # 2^31 - 1 rays at the most
            assert lib.avr_graph_capture(ctx.h, nb, fp(v), fp(v), fp(v), fp(v), steps, fp(out), ctypes.byref(cnt)) == 1
            assert "2^31 - 1 rays" in err()
        with pytest.raises(ValueError):
            ctx.graph_capture(v, v[:1], v, v, 1)
        bad = v.copy()
        bad[1, 0] = np.nan
        for args in ((bad, v, v, v), (v, bad, v, v), (v, v, bad, v), (v, v, v, bad), (v, np.zeros((2, 3), f32), v, v)):
            with pytest.raises(RuntimeError, match="avr error 1.*capture: bundle"):
                ctx.graph_capture(*args, 1)
    finally:
        ctx.close()
