"""The lighting-graph tools with the medium's interface as their primitive (graph geometry 1:
avr_graph_set_geometry, MediumData(scene, "interface")).

The oracle's graph routines know the bounds box only. They still pin the interface model,
because a smaller tMax only ends a delta-tracking segment earlier: every tentative collision
before it is unchanged. So, for a ray started at the interface entry with t_first = the
interface chord, the interface-model walk is the oracle's box-model walk (same o, d, t_first,
index0, skip_dims) cut off before its first scatter point outside the interface (`_prefix_check`).
A walk with a point within 1e-4 of the surface (relative to the sphere's radius, or the mesh's
half-diagonal) is ambiguous and left out; at most 1 % may be.

CPU (not gpu): MediumData's primitive bounds, the Python surface and the tools' arguments, the
reference side of the prefix rule (what is cut, how many), and the compiler-reported resources
of the graph kernels for both geometries.
GPU (gpu): start rays, walks, reinforcement rays, render, analyzer, light vector and the
pipeline end to end on the 12^3 / 16x16 scenes of tests/test_graph.py.
"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

SEED = 3
LIGHT_DIR = np.array([0.3, -0.5, 0.81], f32)
IN_DIR = (LIGHT_DIR / f32(np.linalg.norm(LIGHT_DIR))).astype(f32)
SPHERE = ((0.5, 0.5, 0.5), 0.45)          # inscribed in the unit medium box
OFF_SPHERE = ((0.35, 0.5, 0.5), 0.4)      # sticks out of the box: the medium clips it
SMALL_SPHERE = ((0.5, 0.5, 0.5), 0.4)
NPIX = 256


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _scene(interface=None, sampler=0, spp=4, dens=None, sigma_a=0.4, sigma_s=6.0, g=0.5):
    """tests/test_graph.py's _graph_scene recipe (12^3 gray GridMedium of density 0.2-1, 16x16
    film, the distant light alone) bounded by `interface`: None, "mesh" (scenes.s_mesh_interface's
    rotated box) or a world-space sphere ((cx, cy, cz), r)."""
    from acceleratedvolrenderer_amd import scenes, GridMedium, IndependentSampler, ZSobolSampler
    from acceleratedvolrenderer_amd.scene import Scene
    base = scenes.s_uniform(n=2, width=16, height=16, variant="scatter")
    if dens is None:
        dens = (0.2 + 0.8 * np.random.default_rng(5).random((12, 12, 12), dtype=f32)).astype(f32)
    med = GridMedium(dens, sigma_a=sigma_a, sigma_s=sigma_s, g=g)
    kw = {}
    if interface == "mesh":
        kw["interface_mesh"] = scenes.box_mesh((0.2, 0.15, 0.2), (0.8, 0.85, 0.8), rotate_deg=30.0)
    elif interface is not None:
        kw["interface_sphere"] = interface
    smp = (ZSobolSampler if sampler else IndependentSampler)(pixelsamples=spp)
    return Scene(base.camera, base.film, med, base.lights[:1], sampler=smp, **kw)


def _sampling(kind):
    from acceleratedvolrenderer_amd import graph
    return graph.GraphSampling(sampler=kind, seed=SEED, samples_per_pixel=16, resolution=(64, 64))


def _oracle_sampler(s):
    return (s.sampler, s.seed, s.samples_per_pixel, s.resolution[0], s.resolution[1])


def _builder(scene, ctx, kind, primitive="interface", steps=24, iters=6, max_depth=12, **cfg):
    from acceleratedvolrenderer_amd import graph
    c = graph.GraphBuilderConfig(radius_modifier=60.0, max_depth=max_depth, dimension_steps=steps,
                                 iterations_per_step=iters, **cfg)
    return graph.FreeGraphBuilder(ctx, graph.MediumData(scene, primitive), IN_DIR, _sampling(kind), c,
                                  search_ranges="device")


def _convex_hits(planes, o, d):
    """The plane clip in float32, the oracle's ConvexHits order: dots left to right, one
    division per plane; (type, t0, t1) as graph_sphere_hits."""
    t0, t1 = f32(-np.inf), f32(np.inf)
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    for pl in np.asarray(planes, f32):
        denom = f32(f32(f32(pl[0] * d[0]) + f32(pl[1] * d[1])) + f32(pl[2] * d[2]))
        num = f32(pl[3] - f32(f32(f32(pl[0] * o[0]) + f32(pl[1] * o[1])) + f32(pl[2] * o[2])))
        if denom == 0:
            if num < 0:
                return 2, f32(0), f32(0)
            continue
        t = f32(num / denom)
        if denom > 0:
            t1 = t if t < t1 else t1
        else:
            t0 = t if t > t0 else t0
    if not (t0 <= t1) or t1 <= 0:
        return 2, f32(0), f32(0)
    if t0 <= 0:
        return 3, t1, f32(0)
    return 0, t0, t1


class _Shape:
    """The scene's interface in render space: its hits as the device has to give them (one
    solve from the ray's origin) and on which side of it a point lies (float64)."""

    def __init__(self, scene):
        sph = scene.interface_sphere_render
        if sph is not None:
            self.c, self.r = np.asarray(sph[:3], f32), f32(sph[3])
            self.planes = None
        else:
            self.planes = np.asarray(scene.interface_planes_render, f32)
            v = np.asarray(scene.interface_vertices_render, np.float64)
            self.half_diagonal = float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)) / 2)

    def hits(self, o, d):
        if self.planes is None:
            from oracle import binding
            return binding.graph_sphere_hits(self.c, self.r, o, d)
        return _convex_hits(self.planes, o, d)

    def entry(self, o, d):
        """(type, origin after SkipIntersection, first tMax) of the graph tools' convention."""
        o, d = np.asarray(o, f32), np.asarray(d, f32)
        ty, t0, t1 = self.hits(o, d)
        if ty == 0:
            return ty, (o + (d * f32(t0)).astype(f32)).astype(f32), f32(f32(t1) - f32(t0))
        if ty == 3:
            return ty, o, f32(t0)
        return ty, o, f32(0)

    def side(self, pts):
        """(outside, in the ambiguous band) per point."""
        p = np.asarray(pts, np.float64).reshape(-1, 3)
        if self.planes is None:
            dist = np.linalg.norm(p - self.c.astype(np.float64), axis=1)
            r = float(self.r)
            return dist >= r, np.abs(dist - r) < 1e-4 * r
        pl = self.planes.astype(np.float64)
        s = p @ pl[:, :3].T - pl[:, 3]
        return (s >= 0).any(axis=1), (np.abs(s) < 1e-4 * self.half_diagonal).any(axis=1)


def _prefix_check(shape, pts, counts, pts_o, counts_o):
    """The prefix rule for every walk: (walks cut, walks left out). Asserts that every walk
    kept is bit-identical (count and points) and that at most 1 % are left out."""
    n = len(counts_o)
    assert len(counts) == n
    cut = left_out = 0
    for w in range(n):
        po = pts_o[w, :counts_o[w]]
        outside, band = shape.side(po)
        if band.any():
            left_out += 1
            continue
        k = int(np.argmax(outside)) if outside.any() else int(counts_o[w])
        cut += k < counts_o[w]
        assert counts[w] == k, (w, counts[w], k, counts_o[w])
        assert np.array_equal(bits(pts[w, :k]), bits(po[:k])), w
    assert left_out <= 0.01 * n
    return cut, left_out


def _expected_start_rays(b, shape):
    """The grid rays' (type, origin after the skip, t_first) from the builder's grid points."""
    grid = b.grid_points()
    ty = np.zeros(len(grid), np.int32)
    o = np.zeros((len(grid), 3), f32)
    t = np.zeros(len(grid), f32)
    for i, p in enumerate(grid):
        ty[i], o[i], t[i] = shape.entry(p, b.in_dir)
    return ty, o, t


# ---------------------------------------------------------------------------- CPU

def test_medium_data_primitives():
    from acceleratedvolrenderer_amd import graph
    plain = _scene()
    box, same = graph.MediumData(plain), graph.MediumData(plain, "interface")
    assert (box.primitive, box.geometry, box.shape) == ("box", 0, "box")
    assert (same.primitive, same.geometry, same.shape) == ("interface", 1, "box")
    for key in ("pmin", "pmax", "bounds_center"):
        assert np.array_equal(bits(getattr(box, key)), bits(getattr(same, key))), key
    assert bits(box.max_dist_to_center) == bits(same.max_dist_to_center)
    assert bits(graph.same_spot_radius(box)) == bits(graph.same_spot_radius(same))

    sph = _scene(SPHERE)
    md = graph.MediumData(sph, "interface")
    c, r = np.asarray(sph.interface_sphere_render[:3], f32), f32(sph.interface_sphere_render[3])
    assert md.shape == "sphere" and md.geometry == 1
    assert np.array_equal(bits(md.pmin), bits(c - r)) and np.array_equal(bits(md.pmax), bits(c + r))
    half = ((md.pmax - md.pmin) / f32(2)).astype(f32)
    assert np.array_equal(bits(md.bounds_center), bits(md.pmin + half))
    assert md.max_dist_to_center == pytest.approx(0.45 * math.sqrt(3), rel=1e-6)
    assert graph.same_spot_radius(md) == pytest.approx(0.45 * math.sqrt(3) * 2 / 1000, rel=1e-6)
    # the default stays the box, whatever the scene's interface
    assert np.array_equal(bits(graph.MediumData(sph).pmin), bits(box.pmin))
    assert graph.MediumData(sph).shape == "box"

    mesh = _scene("mesh")
    mm = graph.MediumData(mesh, "interface")
    v = mesh.interface_vertices_render
    assert v.shape == (8, 3) and v.dtype == np.float32 and mm.shape == "mesh"
    assert np.array_equal(bits(mm.pmin), bits(v.min(axis=0))) and np.array_equal(bits(mm.pmax), bits(v.max(axis=0)))
    # the vertices lie on the planes the device intersects
    s = v.astype(np.float64) @ mesh.interface_planes_render[:, :3].T.astype(np.float64) - mesh.interface_planes_render[:, 3]
    assert np.all(s < 1e-5) and np.all(np.sum(np.abs(s) < 1e-5, axis=1) == 3)
    # rotated by 30 degrees about y: wider than the unrotated box in x and z, as high in y
    ext = (mm.pmax - mm.pmin).astype(np.float64)
    assert ext[1] == pytest.approx(0.7, abs=1e-6) and ext[0] == pytest.approx(0.6 * (math.cos(math.pi / 6) + 0.5), abs=1e-6)
    assert plain.interface_vertices_render is None and sph.interface_vertices_render is None


class _FakeCtx:
    def __init__(self, steps=0):
        self.geometry, self.steps = None, steps

    def set_graph_geometry(self, g):
        self.geometry = g

    def graph_start_rays(self, center, max_dist, in_dir, steps):
        self.args = (np.asarray(center, f32), f32(max_dist), np.asarray(in_dir, f32), steps)
        n = steps * steps
        ty = np.array([0, 2, 3, 2] * (n // 4), np.int32)
        return ty, np.arange(3 * n, dtype=f32).reshape(n, 3), np.arange(n, dtype=f32)


def test_python_surface_without_a_gpu():
    from acceleratedvolrenderer_amd import capi, graph
    assert capi.GRAPH_GEOMETRY == {"box": 0, "interface": 1}
    for name, nargs in (("avr_graph_set_geometry", 2), ("avr_graph_start_rays", 8)):
        assert len(capi.SIGNATURES[name][1]) == nargs
    assert hasattr(capi.Context, "set_graph_geometry") and hasattr(capi.Context, "graph_start_rays")
    with open(os.path.join(ROOT, "include", "avr.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        doc = fh.read()
    for name in ("avr_graph_set_geometry", "avr_graph_start_rays"):
        assert re.search(r"\bint " + name + r"\(avr_context \*ctx", header) and name in doc

    sph = _scene(SPHERE)
    with pytest.raises(ValueError, match="primitive"):
        graph.MediumData(sph, "sphere")
    with pytest.raises(ValueError, match="primitive"):
        graph.GraphIntegrator(sph, None, primitive="sphere")
    with pytest.raises(ValueError, match="primitive"):
        graph.IntegrationAnalyzer(sph, None, primitive=1)
    md_i, md_b = graph.MediumData(sph, "interface"), graph.MediumData(sph)
    lcc = graph.LightingCalculatorConfig(light_iterations=4)
    with pytest.raises(ValueError, match="differs"):
        graph.LightingCalculator(None, None, md_b, IN_DIR, _sampling(0), lcc, primitive="interface")
    assert graph.LightingCalculator(None, None, md_i, IN_DIR, _sampling(0), lcc, primitive="interface").md is md_i

    # the builder sets its context's geometry from its MediumData, and an interface's grid is the device's
    ctx = _FakeCtx()
    b = _builder(sph, ctx, 0, steps=4, iters=3)
    assert ctx.geometry == 1
    assert _builder(sph, _FakeCtx(), 0, primitive="box").ctx.geometry == 0
    with pytest.raises(ValueError, match="device"):
        b.start_rays(device=False)
    o, d, t, idx = b.start_rays()
    assert np.array_equal(bits(ctx.args[0]), bits(md_i.bounds_center)) and bits(ctx.args[1]) == bits(md_i.max_dist_to_center)
    assert ctx.args[3] == 4 and np.array_equal(ctx.args[2], IN_DIR)
    keep = np.array([0, 2] * 4) + np.repeat(np.arange(4) * 4, 2)
    assert idx.tolist() == (keep * 3).tolist() and t.tolist() == keep.tolist()
    assert np.array_equal(o, np.arange(48, dtype=f32).reshape(16, 3)[keep]) and np.array_equal(d, np.tile(IN_DIR, (8, 1)))
    # the box's grid on the host: the points the loop always used
    bb = _builder(sph, _FakeCtx(), 0, primitive="box", steps=4)
    assert bb.grid_points().shape == (16, 3) and len(bb.start_rays()[0]) > 0


def test_interface_sphere_argument():
    from acceleratedvolrenderer_amd import graph
    assert graph.parse_interface_sphere("0.5,0.5,0.5,0.45") == ((0.5, 0.5, 0.5), 0.45)
    assert graph.parse_interface_sphere(" 1, -2 ,3e-1, 4") == ((1.0, -2.0, 0.3), 4.0)
    for bad in ("0.5,0.5,0.5", "0.5,0.5,0.5,0", "0.5,0.5,0.5,-1", "a,b,c,d", "0,0,0,inf", "0,0,0,1,2"):
        with pytest.raises(ValueError):
            graph.parse_interface_sphere(bad)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import graph_analyze
        import graph_maker
        import graph_render_demo
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    for tool, argv in ((graph_maker, ["--out", "x"]), (graph_analyze, ["--out", "x"]), (graph_render_demo, [])):
        p = tool.parser()
        assert p.parse_args(argv).interface_sphere is None
        assert p.parse_args(argv + ["--interface-sphere", "0.5,0.5,0.5,0.45"]).interface_sphere == ((0.5, 0.5, 0.5), 0.45)
        with pytest.raises(SystemExit):
            p.parse_args(argv + ["--interface-sphere", "0.5,0.5,0.45"])


@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
def test_prefix_rule_reference(kind):
    """The reference side of the walk test, on the host alone: the sphere scene's grid rays that
    cross the sphere, the oracle's box-model walks from them, and what the prefix rule cuts: a
    third of the walks (which the box model gets wrong), none of them ambiguous."""
    from oracle import binding
    scene = _scene(SPHERE, sampler=kind)
    shape = _Shape(scene)
    b = _builder(scene, _FakeCtx(), kind)
    ty, o, t = _expected_start_rays(b, shape)
    sel = ty != 2
    assert len(ty) == 576 and sel.sum() == 164 and np.all(ty[sel] == 0)
    idx = np.arange(576, dtype=np.int64)[sel] * 6
    run = binding.OracleRun(scene, libm="canonical")
    pts_o, cnt_o = run.graph_walks(o[sel], np.tile(IN_DIR, (164, 1)), t[sel], idx, 6, 0, 64, 12,
                                   sampler=_oracle_sampler(b.sampling))
    assert len(cnt_o) == 984
    cut = left_out = 0
    kept = np.zeros(984, np.int64)
    nearest = np.inf
    for w in range(984):
        po = pts_o[w, :cnt_o[w]]
        outside, band = shape.side(po)
        left_out += band.any()
        kept[w] = int(np.argmax(outside)) if outside.any() else cnt_o[w]
        cut += kept[w] < cnt_o[w]
        if len(po):
            dist = np.linalg.norm(po.astype(np.float64) - shape.c.astype(np.float64), axis=1)
            nearest = min(nearest, np.min(np.abs(dist - float(shape.r))) / float(shape.r))
    print(f"sampler {kind}: mean scatters {cnt_o.mean():.2f} -> {kept.mean():.2f}, cut {cut / 984:.3f}, "
          f"left out {left_out}, nearest point {nearest:.1e} r from the surface")
    assert left_out == 0 and nearest > 1e-4
    assert cut >= 0.3 * 984
    assert cnt_o.mean() > 2.5 and 1.9 < kept.mean() < 2.2


def _kernel_resources(tmp, geom):
    from acceleratedvolrenderer_amd import build as avr_build
    inst = []
    for z in ("false", "true"):
        inst.append(f"template __global__ void k_graph_walks<{z}, {geom}>(Params, long long, int, const float *, "
                    "const float *, const float *, const long long *, int, int, int, int, float *, int *);")
        inst.append(f"template __global__ void k_graph_render<{z}, {geom}>(Params, graph::IndexView, Xf, float4 *);")
        inst.append(f"template __global__ void k_graph_analyze<{z}, {geom}>(Params, graph::IndexView, Xf, int, "
                    "graph::AnalyzeRec *, graph::AnalyzeDetail *);")
    inst.append(f"template __global__ void k_graph_start_rays<{geom}>(DevMedium, V3, float, V3, int, int *, float *, float *);")
    src = tmp / f"graph_g{geom}.hip"
    src.write_text('#define AVR_KPATHS_TU\n#include "avr_kernels.hip"\n#include "avr_graph.hip"\n'
                   "namespace avr {\n" + "\n".join(inst) + "\n}\n")
    cmd = ([avr_build.HIPCC] + avr_build.FLAGS +
           ["-I" + avr_build.CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
            "-c", str(src), "-o", str(tmp / f"graph_g{geom}.o")])
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """The graph kernels alone, cross-compiled for gfx950 with the build's flags, one
    translation unit per geometry (side by side); {mangled name: figures} from the
    -Rpass-analysis=kernel-resource-usage remarks, as tests/test_kpaths_resources.py reads them."""
    from acceleratedvolrenderer_amd import build as avr_build
    if not os.path.exists(avr_build.HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("graph_resources")
    procs = [_kernel_resources(tmp, g) for g in (0, 1)]
    out = {}
    for p in procs:
        _, log = p.communicate()
        assert p.returncode == 0, log[-2000:]
        for block in log.split("Function Name: ")[1:]:
            name = block.split()[0]
            out[name] = {key: int(re.search(pat, block).group(1)) for key, pat in (
                ("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"))}
    return out


@pytest.mark.parametrize("geom", [0, 1], ids=["box", "interface"])
def test_graph_kernel_resources(resources, geom):
    """No scratch, and the 2 waves/SIMD of the box-only kernels, for both geometries."""
    seen = 0
    for z in (0, 1):
        for kernel in ("k_graph_walks", "k_graph_render", "k_graph_analyze"):
            tag = f"{len(kernel)}{kernel}ILb{z}ELi{geom}EE"
            match = [v for k, v in resources.items() if tag in k]
            assert len(match) == 1, tag
            print(f"{kernel}<{bool(z)}, {geom}>: {match[0]}")
            assert match[0]["scratch"] == 0 and match[0]["occ"] >= 2
            seen += 1
    match = [v for k, v in resources.items() if f"k_graph_start_raysILi{geom}EE" in k]
    assert len(match) == 1 and match[0]["scratch"] == 0
    print(f"k_graph_start_rays<{geom}>: {match[0]}")
    assert seen == 6


# ---------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def contexts(gpu):
    """One context per (interface, sampler kind, geometry) asked for, made on first use."""
    from acceleratedvolrenderer_amd import capi
    made = {}

    def get(interface, kind=0, geometry=1):
        key = (interface, kind, geometry)
        if key not in made:
            scene = _scene(interface, sampler=kind)
            ctx = capi.Context(0)
            ctx.set_scene(scene)
            ctx.set_graph_geometry(geometry)
            made[key] = (scene, ctx)
        return made[key]

    yield get
    for _, ctx in made.values():
        ctx.close()


@pytest.mark.gpu
def test_start_rays_box_matches_host_loop(contexts):
    """Geometry 0, and geometry 1 without an interface: avr_graph_start_rays is the Python loop
    bit for bit (which rays cross, o, t_first) at 24 steps."""
    scene, ctx = contexts(None, 0, 0)
    b = _builder(scene, ctx, 0, primitive="box")
    o_h, d_h, t_h, idx_h = b.start_rays(device=False)
    assert len(o_h) > 100
    for primitive in ("box", "interface"):
        bd = _builder(scene, ctx, 0, primitive=primitive)
        o, d, t, idx = bd.start_rays(device=True)
        assert np.array_equal(idx, idx_h) and np.array_equal(bits(d), bits(d_h))
        assert np.array_equal(bits(o), bits(o_h)) and np.array_equal(bits(t), bits(t_h))
    md = b.md
    ty, o_all, t_all = ctx.graph_start_rays(md.bounds_center, md.max_dist_to_center, IN_DIR, 24)
    grid = b.grid_points()
    want = np.array([md.box_hits(p, IN_DIR)[0] for p in grid], np.int32)
    assert np.array_equal(ty, want) and set(ty.tolist()) == {0, 2}
    miss = ty == 2
    assert np.array_equal(bits(o_all[miss]), bits(grid[miss])) and np.all(t_all[miss] == 0)
    # a sphere on the context changes nothing while its geometry is 0
    scene_s, ctx_s = contexts(SPHERE, 0, 0)
    o, d, t, idx = _builder(scene_s, ctx_s, 0, primitive="box").start_rays(device=True)
    assert np.array_equal(idx, idx_h) and np.array_equal(bits(o), bits(o_h)) and np.array_equal(bits(t), bits(t_h))


@pytest.mark.gpu
@pytest.mark.parametrize("interface", [SPHERE, OFF_SPHERE, "mesh"], ids=["sphere", "off-centre", "mesh"])
def test_start_rays_interface(contexts, interface):
    """Type, t0-moved origin and t1 - t0 per grid ray: the oracle's graph_sphere_hits for a
    sphere, the float32 plane clip restated above for the mesh."""
    scene, ctx = contexts(interface)
    b = _builder(scene, ctx, 0)
    md = b.md
    ty, o, t = ctx.graph_start_rays(md.bounds_center, md.max_dist_to_center, IN_DIR, 24)
    ty_w, o_w, t_w = _expected_start_rays(b, _Shape(scene))
    print(f"{md.shape}: {np.sum(ty == 0)} of {len(ty)} grid rays cross")
    assert np.array_equal(ty, ty_w) and set(ty.tolist()) == {0, 2}
    assert np.array_equal(bits(o), bits(o_w)) and np.array_equal(bits(t), bits(t_w))
    if interface == SPHERE:
        assert np.sum(ty == 0) == 164
    o_s, d_s, t_s, idx_s = b.start_rays()
    sel = ty != 2
    assert np.array_equal(bits(o_s), bits(o[sel])) and np.array_equal(bits(t_s), bits(t[sel]))
    assert np.array_equal(idx_s, np.arange(576)[sel] * 6) and np.array_equal(d_s, np.tile(IN_DIR, (sel.sum(), 1)))


WALK_CASES = [(SPHERE, 0), (SPHERE, 1), ("mesh", 0), (OFF_SPHERE, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("interface,kind", WALK_CASES, ids=["sphere-independent", "sphere-zsobol", "mesh", "off-centre"])
def test_walks_follow_the_interface(contexts, interface, kind):
    """The prefix rule for every walk of the grid rays that cross the interface; a context left
    at geometry 0 with the same interface walks on through the box, as before."""
    from oracle import binding
    scene, ctx = contexts(interface, kind)
    b = _builder(scene, ctx, kind)
    o, d, t, idx = b.start_rays()
    c = b.config
    smp = b.sampling
    pts, counts = ctx.graph_walks(smp.struct(), o, d, t, idx, c.iterations_per_step, 0, c.max_depth)
    run = binding.OracleRun(scene, libm="canonical")
    pts_o, counts_o = run.graph_walks(o, d, t, idx, c.iterations_per_step, 0, smp.resolution[0], c.max_depth,
                                      sampler=_oracle_sampler(smp))
    cut, left_out = _prefix_check(_Shape(scene), pts, counts, pts_o, counts_o)
    print(f"{len(counts)} walks, mean scatters {counts_o.mean():.2f} in the box model, {counts.mean():.2f} in the "
          f"interface, cut {cut / len(counts):.3f}, left out {left_out}")
    assert len(counts) > 300 and cut > 0.1 * len(counts) and counts.mean() > 1.0
    _, ctx0 = contexts(interface, kind, 0)
    pts0, counts0 = ctx0.graph_walks(smp.struct(), o, d, t, idx, c.iterations_per_step, 0, c.max_depth)
    assert np.array_equal(counts0, counts_o)
    used = np.arange(c.max_depth)[None, :] < counts_o[:, None]
    assert np.array_equal(bits(pts0[used]), bits(pts_o[used]))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
def test_reinforce_rays_cross_the_sphere(contexts, kind):
    """Sphere-volume points of vertices near the sphere's surface: the directions are the
    oracle's, and valid, o, t_first follow graph_sphere_hits from each point. Every point lies
    inside the medium box (0.4 + 0.09 < 0.5), so the oracle's box-model origin is the point."""
    from oracle import binding
    scene, ctx = contexts(SMALL_SPHERE, kind)
    shape = _Shape(scene)
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(40, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    verts = (shape.c + (dirs * rng.uniform(0.3, 0.4, (40, 1))).astype(f32)).astype(f32)
    ids = rng.permutation(200)[:40].astype(np.int32)
    s = _sampling(kind)
    radius = 0.09
    o, d, t, valid = ctx.graph_reinforce_rays(s.struct(), ids, verts, radius, 7, 2)
    ro, rd, rt, rv = binding.OracleRun(scene, libm="canonical").graph_reinforce_rays(
        ids, verts, radius, 7, 2, s.resolution[0], sampler=_oracle_sampler(s))
    assert np.all(rv == 1)                                   # inside the box: the origin is the point itself
    assert np.all(np.linalg.norm(ro.reshape(-1, 3) - verts.repeat(7, axis=0), axis=1) < radius * (1 + 1e-6))
    assert np.array_equal(bits(d), bits(rd))
    kinds = []
    for i, (p, dr) in enumerate(zip(ro.reshape(-1, 3), rd.reshape(-1, 3))):
        ty, ow, tw = shape.entry(p, dr)
        kinds.append(ty)
        assert valid.ravel()[i] == (ty != 2), i
        assert np.array_equal(bits(o.reshape(-1, 3)[i]), bits(ow)) and bits(t.ravel()[i]) == bits(tw), (i, ty)
    print(f"rays from outside {kinds.count(0)}, from inside {kinds.count(3)}, missing {kinds.count(2)}")
    assert kinds.count(0) > 0 and kinds.count(3) > 0


def _light_spectrum(scene, lam):
    """lightSpectrum.Sample(lambda): DistantLight's scale * Lemit at lround(lambda) (DenselySampled)."""
    off = np.floor(lam.astype(np.float64) + 0.5).astype(np.int64) - 360
    table = np.asarray(scene.light_L[0], f32)
    val = np.where((off >= 0) & (off < len(table)), table[np.clip(off, 0, len(table) - 1)], f32(0)).astype(f32)
    return (val * f32(scene.light_scale[0])).astype(f32)


def _camera_entries(shape, lp, s):
    """The pass's sample-index-s records that cross the interface: rows, entry points,
    directions and chords from the read-back camera rays."""
    o, d, t, pix_, rows = [], [], [], [], []
    for pix in range(NPIX):
        i = s * NPIX + pix
        ty, oo, tmax = shape.entry(lp["o"][i], lp["d"][i])
        if ty == 2:
            continue
        o.append(oo); d.append(lp["d"][i]); t.append(tmax); pix_.append(pix); rows.append(i)
    return np.array(rows), np.array(o, f32), np.array(d, f32), np.array(t, f32), np.array(pix_, np.int64)


RENDER_CASES = [(SPHERE, 0), (SPHERE, 1), ("mesh", 0)]
RENDER_IDS = ["sphere-independent", "sphere-zsobol", "mesh"]


def _interface_graph(scene, ctx, kind):
    """The interface-model graph of the scene (8 steps x 6 walks, device search ranges) with
    random positive light: (graph, light, index)."""
    b = _builder(scene, ctx, kind, steps=8, render_search_range={"active": True, "neighboursToUse": 4})
    g = b.build_graph()
    light = (np.random.default_rng(21).random(g.num_vertices, dtype=f32) + f32(0.05)).astype(f32)
    return g, light, g.index(light)


@pytest.fixture(scope="module")
def rendered(gpu):
    """Per case: the scene, its graph and index, and the renders of sample indices [0, 4) in
    passes of 3 + 1 samples and in one pass (tests/test_graph_render.py's set-up)."""
    from acceleratedvolrenderer_amd import GraphIntegrator
    out = {}
    for interface, kind in RENDER_CASES:
        scene = _scene(interface, sampler=kind)
        split = GraphIntegrator(scene, None, spp=4, seed=SEED, max_paths=3 * NPIX, primitive="interface")
        g, light, index = _interface_graph(scene, split.ctx, kind)
        split.index = index
        rgb_s, w_s = split.render()
        last_s = split.last_pass()
        whole = GraphIntegrator(scene, index, spp=4, seed=SEED, primitive="interface")
        rgb_w, w_w = whole.render()
        out[interface, kind] = dict(scene=scene, graph=g, index=index, split=split, whole=whole, rgb_split=rgb_s,
                                    w_split=w_s, last_split=last_s, rgb=rgb_w, w=w_w, last=whole.last_pass())
    yield out
    for r in out.values():
        r["split"].close()
        r["whole"].close()


def _replay_render(r, lp, kind):
    """One pass against the oracle sample by sample: (crosses the interface, scattered)."""
    from oracle import binding
    scene = r["scene"]
    shape = _Shape(scene)
    W, H = scene.film.width, scene.film.height
    run = binding.OracleRun(scene, seed=SEED, libm="canonical")
    n = NPIX * lp["samples"]
    assert len(lp["o"]) == len(lp["L"]) == n
    cross = np.zeros(n, bool)
    scat_o = np.zeros(n, bool)
    pts_o = np.zeros((n, 3), f32)
    for s in range(lp["samples"]):
        rows, o, d, t, pix = _camera_entries(shape, lp, s)
        assert 0 < len(rows) < NPIX               # the corners look past the interface
        pts, cnt = run.graph_walks(o, d, t, pix, 1, lp["first"] + s, W, 1, skip_dims=6,
                                   sampler=(kind, SEED, scene.sampler.pixelsamples, W, H))
        cross[rows] = True
        scat_o[rows] = cnt == 1
        pts_o[rows] = pts[:, 0]
    scat = lp["count"] >= 0
    # scatter or not, and the point, bit-identical for every sample
    assert np.array_equal(scat, scat_o)
    assert np.array_equal(bits(lp["p"][scat]), bits(pts_o[scat]))
    assert np.all(lp["p"][~scat] == 0)
    outside, _ = shape.side(lp["p"][scat])
    assert not outside.any()
    # count and L against the host index at the read-back point (identity graph_from_render)
    conn, cnt = r["index"].connect(lp["p"][scat])
    assert np.array_equal(lp["count"][scat], cnt)
    spec = _light_spectrum(scene, lp["lam"])
    with np.errstate(all="ignore"):
        want = np.zeros((n, 4), f32)
        want[scat] = (spec[scat] * conn[:, None]).astype(f32)
    for ch in range(4):
        assert np.array_equal(bits(lp["L"][:, ch]), bits(want[:, ch])), ch
    return cross, scat


@pytest.mark.gpu
@pytest.mark.parametrize("interface,kind", RENDER_CASES, ids=RENDER_IDS)
def test_render_replays_oracle_walks(rendered, interface, kind):
    r = rendered[interface, kind]
    assert (r["last_split"]["first"], r["last_split"]["samples"]) == (3, 1)
    assert (r["last"]["first"], r["last"]["samples"]) == (0, 4)
    _replay_render(r, r["last_split"], kind)
    cross, scat = _replay_render(r, r["last"], kind)
    # split passes are one pass: the last pass's records and the film
    for key in ("L", "lam", "o", "d", "p", "count"):
        a, b = r["last_split"][key], r["last"][key][3 * NPIX:]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), key
    assert np.array_equal(r["rgb"], r["rgb_split"]) and np.array_equal(r["w"], r["w_split"])
    print(f"{r['graph'].num_vertices} vertices, samples crossing {cross.mean():.3f}, of them scattered "
          f"{scat[cross].mean():.3f}, connected {np.mean(r['last']['count'][scat] > 0):.3f}")
    assert scat[cross].mean() >= 0.5 and not scat[~cross].any()
    assert np.mean(r["last"]["count"][scat] > 0) > 0.25 and r["rgb"].sum() > 0


@pytest.mark.gpu
def test_render_and_analysis_refuse_an_interface_at_geometry_0(rendered):
    """The default stays the bounds box: the same scene and index at geometry 0 are refused,
    with the hint at the new call; geometry 1 again takes them."""
    r = rendered[SPHERE, 0]
    ctx = r["whole"].ctx
    ctx.set_graph_geometry(0)
    try:
        with pytest.raises(RuntimeError, match="avr error 3.*bounds box.*avr_graph_set_geometry"):
            ctx.graph_render(r["index"], 0, 1, SEED)
        with pytest.raises(RuntimeError, match="avr error 3.*bounds box.*avr_graph_set_geometry"):
            ctx.graph_analyze(r["index"], 0, 1, SEED, 1)
        for bad in (2, -1):
            with pytest.raises(RuntimeError, match="avr error 1.*geometry"):
                ctx.set_graph_geometry(bad)
    finally:
        ctx.set_graph_geometry("interface")
    # the setting outlives avr_medium_* calls
    ctx.set_scene(r["scene"])
    rgb, w = r["whole"].render()
    assert np.array_equal(rgb, r["rgb"]) and np.array_equal(w, r["w"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
def test_analysis_follows_the_interface(gpu, kind):
    """detail=True at maxdepth 3 on the sphere scene: every sample's scatters follow the prefix
    rule against the oracle (skip_dims 6), each scatter's answer is the host index_coverage's,
    and the per-pixel sums are the detail summed in order."""
    from acceleratedvolrenderer_amd import IntegrationAnalyzer
    from oracle import binding
    md_ = 3
    scene = _scene(SPHERE, sampler=kind)
    shape = _Shape(scene)
    an = IntegrationAnalyzer(scene, None, maxdepth=md_, spp=4, seed=SEED, primitive="interface")
    try:
        _, _, an.index = _interface_graph(scene, an.ctx, kind)
        res = an.analyze(detail=True)
        lp = an.last_pass()
        index = an.index
    finally:
        an.close()
    W, H = scene.film.width, scene.film.height
    n = NPIX * 4
    assert (lp["first"], lp["samples"]) == (0, 4) and lp["p"].shape == (n, md_, 3)
    run = binding.OracleRun(scene, seed=SEED, libm="canonical")
    cross = np.zeros(n, bool)
    cut = left_out = walks = 0
    for s in range(4):
        rows, o, d, t, pix = _camera_entries(shape, lp, s)
        assert 0 < len(rows) < NPIX
        pts_o, cnt_o = run.graph_walks(o, d, t, pix, 1, s, W, md_, skip_dims=6,
                                       sampler=(kind, SEED, scene.sampler.pixelsamples, W, H))
        c, l = _prefix_check(shape, lp["p"][rows], lp["count"][rows], pts_o, cnt_o)
        cut, left_out, walks = cut + c, left_out + l, walks + len(rows)
        cross[rows] = True
    assert left_out <= 0.01 * walks and cut > 0
    assert np.all(lp["count"][~cross] == 0)
    used = np.arange(md_)[None, :] < lp["count"][:, None]
    assert np.all(lp["p"][~used] == 0)
    node, in_range, range_sum = index.coverage(lp["p"][used])
    assert np.array_equal(lp["node"][used], node) and np.array_equal(lp["in_range"][used], in_range)
    assert np.array_equal(bits(lp["range_sum"][used]), bits(range_sum))
    for key in ("node", "in_range", "range_sum"):
        assert np.all(lp[key][~used] == 0)
    print(f"sampler {kind}: scatters per crossing sample {lp['count'][cross].mean():.3f}, walks cut {cut / walks:.3f}, "
          f"node {node.mean():.3f}, search {np.mean(in_range > 0):.3f}")
    assert lp["count"].max() == md_ and 0 < node.sum() and 0 < np.sum(in_range > 0)
    # the per-pixel sums: per sample the scatters' range_sum added in double in scatter order,
    # then the samples in sample-index order
    rec = np.zeros(n, np.float64)
    for i in range(n):
        acc = np.float64(0)
        for k in range(lp["count"][i]):
            acc = acc + np.float64(lp["range_sum"][i, k])
        rec[i] = acc
    per = dict(total=lp["count"], node=(lp["node"] * used).sum(1), search=((lp["in_range"] > 0) & used).sum(1),
               in_range=(lp["in_range"] * used).sum(1))
    for key, v in per.items():
        got = getattr(res, key)
        assert got.dtype == np.uint64 and np.array_equal(got.ravel(), v.astype(np.uint64).reshape(4, NPIX).sum(0)), key
    acc = np.zeros(NPIX, np.float64)
    for s in range(4):
        acc = acc + rec[s * NPIX:(s + 1) * NPIX]
    assert np.array_equal(res.range_sum.ravel().view(np.uint64), acc.view(np.uint64)) and res.total.sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["independent", "zsobol"])
def test_light_vector_starts_at_the_interface(gpu, kind):
    """GetLightVector in a constant medium (16^3 of density 1, sigma_a 1, sigma_s 2: kappa = 3)
    inside the sphere ((0.5, 0.5, 0.5), 0.4), whose rays stay more than half a voxel from the
    box's faces. Per disk ray, with u0 and u1 the distances from the interface entry to the
    start and the end of the vertex-sphere chord, the estimate's mean over the uniform chord
    point is E = (exp(-kappa u0) - exp(-kappa u1)) / (kappa (u1 - u0)); light[v] = Inv4Pi x the
    mean of E over the vertex's valid disk rays. The measured mean must agree within 4 standard
    errors; the expectation from the box entry (a path longer by >= 0.1) must be missed by more."""
    from acceleratedvolrenderer_amd import capi, graph
    from oracle import binding
    kappa = 3.0
    scene = _scene(SMALL_SPHERE, sampler=kind, dens=np.ones((16, 16, 16), f32), sigma_a=1.0, sigma_s=2.0)
    shape = _Shape(scene)
    md, md_box = graph.MediumData(scene, "interface"), graph.MediumData(scene)
    rng = np.random.default_rng(9)
    dirs = rng.normal(size=(200, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    verts = (shape.c + (dirs * (0.3 * rng.random((200, 1)) ** (1 / 3))).astype(f32)).astype(f32)
    # vertex 200: its disk rays all pass the sphere at 0.5 from the centre
    xv, _ = graph.coordinate_system(IN_DIR)
    verts = np.concatenate([verts, (shape.c + xv * f32(0.5)).astype(f32)[None]]).astype(f32)
    radius, n_r, iters = f32(0.05), 2, 8
    s = _sampling(kind)
    ctx = capi.Context(0)
    try:
        ctx.set_scene(scene)
        ctx.set_graph_geometry(1)
        light = ctx.graph_light(s.struct(), verts, IN_DIR, radius, n_r, iters, md.max_dist_to_center)
    finally:
        ctx.close()

    def mean_e(u0, u1):
        return (np.exp(-kappa * u0) - np.exp(-kappa * u1)) / (kappa * (u1 - u0))

    want = np.zeros(201)
    want_box = np.zeros(201)
    for v in range(201):
        origin = (verts[v] - ((IN_DIR * md.max_dist_to_center).astype(f32) * f32(2)).astype(f32)).astype(f32)
        es, eb = [], []
        for p in binding.graph_disk_points(origin, radius, n_r, IN_DIR):
            mty, m0, m1 = shape.hits(p, IN_DIR)
            sty, s0, s1 = binding.graph_sphere_hits(verts[v], radius, p, IN_DIR)
            if mty != 0 or sty != 0:
                continue
            m0, m1, s0, s1 = float(m0), float(m1), float(s0), float(s1)
            start, end = max(m0, s0), min(m1, s1)
            if end < start:
                continue
            es.append(mean_e(start - m0, end - m0) if end > start else math.exp(-kappa * (start - m0)))
            bty, b0, _ = md_box.box_hits(p, IN_DIR)
            assert bty == 0 and float(b0) < m0 - 0.1
            eb.append(mean_e(start - float(b0), end - float(b0)) if end > start else math.exp(-kappa * (start - float(b0))))
        if v < 200:
            assert len(es) >= 9
        want[v] = np.mean(es) / (4 * math.pi) if es else 0.0
        want_box[v] = np.mean(eb) / (4 * math.pi) if eb else 0.0
    assert light[200] == 0 and want[200] == 0
    diff = light[:200].astype(np.float64) - want[:200]
    diff_box = light[:200].astype(np.float64) - want_box[:200]
    se = diff.std() / math.sqrt(200)
    z, z_box = diff.mean() / se, diff_box.mean() / (diff_box.std() / math.sqrt(200))
    print(f"sampler {kind}: light mean {light[:200].mean():.5e}, expected {want[:200].mean():.5e} (z = {z:.2f}), "
          f"from the box entry {want_box[:200].mean():.5e} (z = {z_box:.2f})")
    assert light[:200].mean() > 0
    assert abs(diff.mean()) <= 4 * se
    assert abs(diff_box.mean()) > 4 * diff_box.std() / math.sqrt(200)


@pytest.mark.gpu
def test_pipeline_end_to_end_in_the_sphere(gpu, tmp_path):
    """FreeGraphBuilder(MediumData(scene, "interface")) with reinforcement and device search
    ranges, LightingCalculator, FreeGraph.save, GraphIntegrator.from_file(primitive="interface"):
    a finite film, exactly 0 outside the sphere's silhouette, from a graph inside the sphere."""
    from acceleratedvolrenderer_amd import GraphIntegrator, capi, graph
    scene = _scene(SPHERE, spp=4)
    shape = _Shape(scene)
    ctx = capi.Context(0)
    try:
        ctx.set_scene(scene)
        b = _builder(scene, ctx, 0, steps=8, max_depth=8,
                     render_search_range={"active": True, "neighboursToUse": 4},
                     edge_reinforcement={"active": True, "unsatisfiedAllowedRatio": 0.3, "reinforcementRays": 4,
                                         "edgesForNotSparse": 3})
        g = b.build_graph()
        lc = graph.LightingCalculator(ctx, g, b.md, b.in_dir, b.sampling,
                                      graph.LightingCalculatorConfig(light_iterations=8, points_on_radius_light=1,
                                                                     bounces=[6]), primitive="interface")
        assert lc.compute_final_light() == 6
    finally:
        ctx.close()
    assert b.reinforce_cycles >= 1 and g.num_vertices > 50 and g.search_range is not None
    outside, _ = shape.side(g.points)
    assert not outside.any()
    assert np.all(np.isfinite(lc.light_scalar)) and lc.light_scalar.min() >= 0 and lc.light_scalar.max() > 0
    path = str(tmp_path / "sphere_graph.txt")
    g.save(path, lc.light_scalar)
    integ = GraphIntegrator.from_file(scene, path, spp=4, seed=SEED, primitive="interface")
    try:
        rgb, w = integ.render()
        lp = integ.last_pass()
        img = integ.get_image(rgb, w)
    finally:
        integ.close()
    assert lp["samples"] == 4
    misses = np.array([shape.hits(o, d)[0] == 2 for o, d in zip(lp["o"], lp["d"])]).reshape(4, NPIX)
    off = misses.all(axis=0)                      # pixels whose every sample looks past the sphere
    rgb = np.asarray(rgb).reshape(NPIX, 3)
    print(f"{g.num_vertices} vertices after {b.reinforce_cycles} reinforcement cycles; {off.sum()} pixels outside the "
          f"silhouette, image mean {img.mean():.4e}")
    assert 0 < off.sum() < NPIX
    assert np.all(np.isfinite(img)) and np.all(rgb[off] == 0) and rgb[~misses.any(axis=0)].sum() > 0
