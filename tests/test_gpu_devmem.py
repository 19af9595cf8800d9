"""Ownership of device memory in the C-ABI host code (csrc/avr_devmem.h): one context cycled
through every kind of state that owns device buffers, and one call of every entry point that
takes scratch, with the library's live-memory counters (avr_debug_live_device_bytes, bound by
hand: it is not in include/avr.h) the same after everything is closed as before. The sequences
are measured against their own start, since other tests of the process may hold contexts.

Between the steps the context renders 1 spp in both kernel modes, and the films must equal
(array_equal) those of a fresh context given the same state at once: a view struct left
pointing at a freed or stale buffer shows there. Everything on 16 x 12 films and 6^3 grids."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, H, MAXDEPTH, N = 16, 12, 5, 6


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()


def live():
    from acceleratedvolrenderer_amd import capi
    lib = capi.load()
    fn = lib.avr_debug_live_device_bytes
    fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)] * 2
    fn.restype = ctypes.c_int
    b, k = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    assert fn(ctypes.byref(b), ctypes.byref(k)) == 0
    return b.value, k.value


def _density():
    return (0.3 + np.random.default_rng(3).random((N, N, N), dtype=np.float32)).astype(np.float32)


def _camera(w=W, h=H):
    from acceleratedvolrenderer_amd.scene import PerspectiveCamera
    return PerspectiveCamera(fov=40.0, pos=(0.5, 0.5, -1.6), look=(0.5, 0.5, 0.5), up=(0, 1, 0),
                             frameaspectratio=w / h)


def _lights(image=False):
    import light_cases
    from acceleratedvolrenderer_amd.scene import DistantLight, UniformInfiniteLight
    ls = [DistantLight(from_=(-1.0, 1.0, -1.0), to=(0.0, 0.0, 0.0), scale=2.0), UniformInfiniteLight(scale=0.25)]
    # (the image light's map is square, res x res: the 8 x 8 one of tests/light_cases.py)
    return ls + [light_cases.map_light("half-black-8")] if image else ls


def _rgb_coeffs(rng, hi):
    c = np.empty((N, N, N, 4), np.float32)
    c[..., 0] = rng.uniform(-2e-5, 2e-5, (N, N, N))
    c[..., 1] = rng.uniform(-0.02, 0.02, (N, N, N))
    c[..., 2] = rng.uniform(-5, 5, (N, N, N))
    c[..., 3] = rng.uniform(0.2, hi, (N, N, N))
    return c


def _vdb_medium():
    """Two leaves and one tile, with a temperature grid of one leaf."""
    from acceleratedvolrenderer_amd.scene import NanoVDBMedium
    from acceleratedvolrenderer_amd.vdb import NanoVDBGrid
    rng = np.random.default_rng(5)
    m = np.diag([1 / 16, 1 / 16, 1 / 8, 1.0])
    dens = NanoVDBGrid([(0, 0, 0), (8, 0, 0)], (0.2 + rng.random((2, 8, 8, 8))).astype(np.float32),
                       tile_origins=[(0, 8, 0)], tile_sizes=[8], tile_values=[0.5], index_to_world=m)
    temp = NanoVDBGrid([(0, 0, 0)], (900 + 2500 * rng.random((1, 8, 8, 8))).astype(np.float32), index_to_world=m)
    return NanoVDBMedium(dens, temperature=temp, sigma_a=0.5, sigma_s=2.0, g=0.3, Lescale=0.01)


def _medium(kind):
    from acceleratedvolrenderer_amd.scene import CloudMedium, GridMedium, HomogeneousMedium, RGBGridMedium
    if kind == "grid":
        return GridMedium(_density(), sigma_a=0.5, sigma_s=4.0, g=0.3, majorant_res=(3, 2, 4))
    if kind == "rgbgrid":
        rng = np.random.default_rng(4)
        return RGBGridMedium(sigma_a_coeffs=_rgb_coeffs(rng, 0.8), sigma_s_coeffs=_rgb_coeffs(rng, 4.0),
                             Le_coeffs=_rgb_coeffs(rng, 2.0), Lescale=0.7, g=0.25, scale=1.3)
    if kind == "nanovdb":
        return _vdb_medium()
    if kind == "homogeneous":
        return HomogeneousMedium(sigma_a=0.5, sigma_s=4.0, g=0.3)
    assert kind == "cloud"
    return CloudMedium(sigma_a=0.1, sigma_s=6.0, g=0.6)


def _scene(kind="grid", w=W, h=H, sampler="independent", image=False, buckets=0, lights=None):
    from acceleratedvolrenderer_amd.scene import IndependentSampler, RGBFilm, Scene, SpectralFilm, ZSobolSampler
    film = SpectralFilm(w, h, nbuckets=buckets) if buckets else RGBFilm(w, h)
    smp = ZSobolSampler(pixelsamples=4) if sampler == "zsobol" else IndependentSampler(pixelsamples=4)
    return Scene(_camera(w, h), film, _medium(kind), _lights(image) if lights is None else lights, sampler=smp)


class State:
    """What a context holds: the grid layout, the scene, and what is set on top of the scene."""
    def __init__(self, scene, layout=0, bounds=None, order=None, overlap=True):
        self.scene, self.layout, self.bounds, self.order, self.overlap = scene, layout, bounds, order, overlap

    def npix(self):
        b = self.bounds or (0, 0, self.scene.film.width, self.scene.film.height)
        return (b[2] - b[0]) * (b[3] - b[1])

    def apply(self, ctx, old=None):
        """Bring ctx from state `old` (None: a fresh context) to this one, touching only what
        differs (the scene goes up as a whole: medium, lights, camera and film)."""
        ctx.set_pass_overlap(1 if self.overlap else 0)
        if old is None or old.scene is not self.scene or old.layout != self.layout:
            ctx.set_grid_layout(self.layout)
            ctx.set_scene(self.scene)
            old = State(self.scene, self.layout)
        if self.bounds != old.bounds:
            w, h = self.scene.film.width, self.scene.film.height
            ctx.film_pixel_bounds(*(self.bounds or (0, 0, w, h)))
            old = State(self.scene, self.layout, self.bounds)   # (new bounds drop the pixel order)
        if self.order is not old.order:
            ctx.set_pixel_order(self.order)


def _films(ctx, st, passes=1):
    """The film sums of `passes` calls of 1 spp each, in the persistent and the wavefront mode."""
    out = []
    for mode in (0, 1):
        ctx.set_kernel_mode(mode)
        ctx.film_clear()
        for s in range(passes):
            ctx.render(s, s + 1, 0, MAXDEPTH)
        out += list(ctx.film_read(st.npix()))
        nb = int(getattr(st.scene.film, "nbuckets", 0))
        if nb:
            out += list(ctx.film_read_spectral(st.npix(), nb))
    return out


def _check_against_fresh(ctx, st, name, passes=1):
    from acceleratedvolrenderer_amd import capi
    got = _films(ctx, st, passes)
    fresh = capi.Context(0)
    try:
        st.apply(fresh)
        want = _films(fresh, st, passes)
    finally:
        fresh.close()
    assert float(want[0].sum()) > 0, name
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (name, k)


def test_state_cycle_frees_everything_and_renders_as_a_fresh_context():
    from acceleratedvolrenderer_amd import capi
    before = live()
    ctx = capi.Context(0)
    try:
        assert live()[1] > before[1]
        grid, grid_big = _scene("grid"), _scene("grid", 20, 10)
        zs = _scene("grid", sampler="zsobol")
        rng = np.random.default_rng(8)
        steps = [
            # GridMedium in the linear, fat and bricked layouts
            ("linear", State(grid, 0)), ("fat", State(grid, 1)), ("bricked", State(grid, 2)),
            ("rgbgrid", State(_scene("rgbgrid"), 2)), ("nanovdb", State(_scene("nanovdb"), 1)),
            ("homogeneous", State(_scene("homogeneous"), 1)), ("cloud", State(_scene("cloud"), 1)),
            # the film twice at different sizes, pixel bounds, a spectral film with buckets
            ("film 20x10", State(grid_big, 1)), ("film 16x12", State(grid, 1)),
            ("bounds", State(grid, 1, bounds=(2, 1, 13, 9))),
            ("spectral", State(_scene("grid", buckets=4), 1)),
            # a pixel order, replaced, and dropped
            ("order", State(grid, 1, order=np.arange(W * H, dtype=np.int32)[::-1].copy())),
            ("order replaced", State(grid, 1, order=rng.permutation(W * H).astype(np.int32))),
            ("scanline", State(grid, 1)),
            # a light list with an image light, then one without
            ("image light", State(_scene("grid", image=True), 1)), ("no image light", State(grid, 1)),
        ]
        old = None
        for name, st in steps:
            st.apply(ctx, old)
            kind = getattr(st.scene.medium, "type_id", 0)   # the fat copy: grids and NanoVDB; bricks: grids
            assert ctx.grid_layout_active() == (st.layout if kind == 0 else int(kind == 3 and st.layout == 1)), name
            _check_against_fresh(ctx, st, name)
            old = st
        # pass overlap over three consecutive passes: both camera sets and both pass-table buffers
        st = State(zs, 1)
        st.apply(ctx, old)
        blocks = live()[1]
        _check_against_fresh(ctx, st, "overlap", passes=3)
        ctx.set_kernel_mode(0)
        for s in range(3):
            ctx.render(s, s + 1, 0, MAXDEPTH)
        assert ctx.pass_overlap_active() == 1
        assert live()[1] >= blocks + 9 + 2   # the other camera set (8 + heads) and a second pass table
        # ... and off again: the serial chain on the same buffers
        off = State(zs, 1, overlap=False)
        off.apply(ctx, st)
        _check_against_fresh(ctx, off, "overlap off", passes=3)
    finally:
        ctx.close()
    assert live() == before


def _graph_scene():
    from acceleratedvolrenderer_amd.scene import DistantLight
    return _scene("grid", lights=[DistantLight(from_=(-1.0, 1.0, -1.0), to=(0.0, 0.0, 0.0), scale=2.0)])


def test_scratch_entry_points_free_everything():
    """One call of every entry point that takes a scratch arena, at n <= 64."""
    from acceleratedvolrenderer_amd import capi, graph
    before = live()
    ctx = capi.Context(0)
    handles = []
    try:
        scene = _graph_scene()
        st = State(scene, 1)
        st.apply(ctx)
        f32 = np.float32
        md = graph.MediumData(scene)
        in_dir = np.array([0.3, -0.5, 0.81], f32)
        in_dir = (in_dir / f32(np.linalg.norm(in_dir))).astype(f32)
        smp = graph.GraphSampling(0, 0, 4, (64, 64)).struct()
        center = ((md.pmin + md.pmax) / 2).astype(f32)
        ty, o, t = ctx.graph_start_rays(center, md.max_dist_to_center, in_dir, 6)
        hit = np.flatnonzero(ty != 2)[:16]
        assert len(hit) > 0
        pts, counts = ctx.graph_walks(smp, o[hit], np.tile(in_dir, (len(hit), 1)), t[hit], np.arange(len(hit)), 2, 0, 3)
        assert counts.sum() > 0
        verts = np.concatenate([pts[w, :counts[w]] for w in range(len(counts))])[:40]
        light = ctx.graph_light(smp, verts, in_dir, f32(0.05), 1, 2, md.max_dist_to_center)
        assert np.all(np.isfinite(light))
        n = len(verts)
        assert n >= 8
        rp = np.arange(n + 1, dtype=np.int32)
        col = ((np.arange(n) + 1) % n).astype(np.int32)
        total, it = ctx.graph_propagate(rp, col, np.full(n, 0.5, f32), light, 3)
        assert total.shape == (n,) and 0 <= it <= 3
        ids = np.arange(min(n, 5), dtype=np.int32)
        ctx.graph_reinforce_rays(smp, ids, verts[:len(ids)], 0.05, 2, 0)
        idx = capi.GraphIndex(verts, np.abs(light) + f32(0.1), None, radius=0.08)
        handles.append(idx)
        ranges = ctx.graph_search_ranges(idx, 3)             # a knn with ranges
        assert ranges.shape == (n,) and np.all(ranges > 0)
        ctx.graph_knn(idx, 3)
        ctx.graph_connect(idx, verts[:7])
        ctx.graph_coverage(idx, verts[:7])
        ridx = capi.GraphIndex(verts, np.abs(light) + f32(0.1), ranges, radius=0.08)
        handles.append(ridx)
        # the graph render and the analysis with detail, against a fresh context's
        npix = st.npix()

        def graph_films(c):
            c.film_clear()
            c.graph_render(ridx, 0, 1, 0)
            films = list(c.film_read(npix))
            c.graph_analyze(ridx, 0, 1, 0, 2, detail=True)
            films += [np.asarray(a) for a in c.graph_analysis_read(npix)]
            films += [np.asarray(a) for a in c.graph_analyze_last_pass(npix, 1, 2)]
            return films
        got = graph_films(ctx)
        fresh = capi.Context(0)
        try:
            st.apply(fresh)
            want = graph_films(fresh)
        finally:
            fresh.close()
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
        # the uniform graph's and the voxel boundary's device calls
        uni = capi.GraphUniform.from_points_device(ctx, verts, f32(0.125))
        handles.append(uni)
        assert ctx.graph_uniform_count(verts, f32(0.125)) > 0
        ctx.graph_uniform_lookup(uni, verts[:9])
        ctx.graph_uniform_trace(uni, np.tile(center - in_dir, (4, 1)).astype(f32), np.tile(in_dir, (4, 1)))
        ctx.graph_render_uniform(uni, 0, 1, 0)
        xv, yv = np.array([[0.05, 0, 0]], f32), np.array([[0, 0.05, 0]], f32)
        ctx.graph_capture((center - in_dir)[None].astype(f32), in_dir[None], xv, yv, 2)
        coors = np.array([(x, y, z) for x in (1, 2, 3) for y in (1, 2, 3) for z in (1, 2, 3) if (x, y, z) != (2, 2, 2)],
                         np.int32)
        vox = capi.GraphVoxels(np.zeros(3, f32), np.full(3, 4, f32), 1.0, coors)   # a hollow 3^3 shell
        handles.append(vox)
        assert vox.single_layer(ctx) > 0
        vox.fill(ctx)
        g = capi.Graph(0.05)
        handles.append(g)
        g.add_walks_device(ctx, pts, counts, 3)
        # the light readbacks at n = 3
        u2, w3 = np.random.default_rng(2).random((3, 2), dtype=f32), np.tile(in_dir, (3, 1))
        lam = np.tile(np.array([450, 520, 610, 700], f32), (3, 1))
        ctx.light_probe(0, u2, w3, lam)
        ctx.light_probe_at(0, u2, verts[:3], lam)
        ctx.light_pick(u2[:, 0].copy())
        ctx.light_pick_at(u2[:, 0].copy(), verts[:3])
        ctx.transmittance(verts[:3], verts[3:6], lam)
        ctx.flip(np.full((H, W, 3), 0.5, f32), np.full((H, W, 3), 0.25, f32))
    finally:
        for h in handles:
            h.close()
        ctx.close()
    assert live() == before


def test_error_returns_keep_the_counters():
    """Entry points that fail after their scratch or a buffer exists give it back."""
    from acceleratedvolrenderer_amd import capi
    before = live()
    ctx = capi.Context(0)
    try:
        st = State(_graph_scene(), 1)
        st.apply(ctx)
        held = live()
        with pytest.raises(RuntimeError):
            ctx.set_pixel_order(np.zeros(W * H, np.int32))             # not a permutation
        with pytest.raises(RuntimeError):
            ctx.film_pixel_bounds(0, 0, W + 1, H)
        idx = capi.GraphIndex(np.array([[0.5, 0.5, 0.5]], np.float32), np.array([1.0], np.float32), None, radius=0.1)
        try:
            with pytest.raises(RuntimeError):
                ctx.graph_knn(idx, 3)                                  # k > n - 1
            ctx.graph_render(idx, 0, 1, 0)
            with pytest.raises(RuntimeError):
                ctx.graph_render(idx, 2, 1, 0)                         # a bad sample range, the index uploaded
        finally:
            idx.close()
        assert live()[0] >= held[0]
    finally:
        ctx.close()
    assert live() == before
