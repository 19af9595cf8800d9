"""The three GridMedium density layouts (linear, fat, bricked) on non-cubic grids: every layout
must return SampledGrid::Lookup (util/containers.h:804-835) bit for bit at caller-chosen points
(avr_density_fetch), on shapes with a dimension of 1 and dimensions 0, 1 and 7 mod 8, at voxel
centres, faces, brick borders, 0, 1 and just outside, and on a 1 x 8190 x 4096 slab whose fat
index passes 2^24 in its inner term (tests/test_grid_index.py has the arithmetic alone); on the
slab also Integrator::Tr and a render against the canonical oracle.

The reference is a vectorised numpy float32 restatement of SampledGrid::Lookup, itself compared
bit for bit with the oracle's (the CPU test below), so the GPU tests can afford 10^5 points."""
import itertools

import numpy as np
import pytest

SMALL = [(1, 1, 1), (1, 1, 64), (64, 1, 1), (2, 3, 5), (7, 8, 9), (8, 8, 8), (9, 16, 17), (15, 16, 17), (255, 3, 2)]
LAYOUTS = [("linear", 0), ("fat", 1), ("brick", 2)]
SLAB = (1, 8190, 4096)        # (nx, ny, nz): array shape (4096, 8190, 1), 134 MB
CONTROL = (8190, 4096, 1)     # the same values as a grid thin in z: the old index was right there


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()
    return torch


def np_grid_lookup(dens, p):
    """SampledGrid<float>::Lookup(p) in float32 for points p (n, 3): ps = p * res - .5, floor,
    eight taps (zero outside the grid), Lerp(t, a, b) = (1 - t) * a + t * b along x, y, then z."""
    nz, ny, nx = dens.shape
    one, half = np.float32(1), np.float32(.5)
    p = np.asarray(p, np.float32)
    ps = p * np.array([nx, ny, nz], np.float32) - half
    fl = np.floor(ps)
    d = ps - fl
    i = fl.astype(np.int64)

    def at(x, y, z):
        ok = (x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (z >= 0) & (z < nz)
        v = dens[np.clip(z, 0, nz - 1), np.clip(y, 0, ny - 1), np.clip(x, 0, nx - 1)]
        return np.where(ok, v, np.float32(0))

    def lerp(t, a, b):
        return (one - t) * a + t * b

    x, y, z = i[:, 0], i[:, 1], i[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    d00 = lerp(dx, at(x, y, z), at(x + 1, y, z))
    d10 = lerp(dx, at(x, y + 1, z), at(x + 1, y + 1, z))
    d01 = lerp(dx, at(x, y, z + 1), at(x + 1, y, z + 1))
    d11 = lerp(dx, at(x, y + 1, z + 1), at(x + 1, y + 1, z + 1))
    out = lerp(dz, lerp(dy, d00, d10), lerp(dy, d01, d11))
    assert out.dtype == np.float32
    return out


def _density(shape, seed):
    """Random densities in [0.25, 1.25): a wrong tap cannot give the right value by chance."""
    nx, ny, nz = shape
    return (np.float32(0.25) + np.random.default_rng(seed).random((nz, ny, nx), dtype=np.float32)).astype(np.float32)


def _axis_values(n):
    """Per axis: the centre (i + .5) / n and the face i / n of up to 64 cells (the first and the
    last 32 of a longer axis), and 0, 1, the floats just outside them, -1 and 2."""
    cells = list(range(n)) if n <= 64 else list(range(32)) + list(range(n - 32, n))
    faces = sorted(set(cells) | {c + 1 for c in cells})
    f = np.float32
    v = [f(c + .5) / f(n) for c in cells] + [f(c) / f(n) for c in faces]
    v += [f(0), f(1), np.nextafter(f(0), f(-1)), np.nextafter(f(1), f(2)), f(-1), f(2)]
    return np.array(v, np.float32)


def _points(shape, seed, n_uniform=40000, n_struct=60000):
    rng = np.random.default_rng(seed)
    uni = rng.uniform(-0.05, 1.05, (n_uniform, 3)).astype(np.float32)
    ax = [_axis_values(n) for n in shape]
    if len(ax[0]) * len(ax[1]) * len(ax[2]) <= n_struct:
        st = np.array(list(itertools.product(*ax)), np.float32)
    else:
        # every value of every axis at least once (cycled), in random combinations across axes
        st = np.stack([rng.permutation(np.resize(a, n_struct)) for a in ax], axis=1)
    return np.ascontiguousarray(np.concatenate([uni, st]), np.float32)


def test_numpy_reference_is_the_oracle_lookup():
    """The numpy restatement equals the oracle's SampledGrid::Lookup bit for bit on every small
    shape, at uniform and structured points (2000 or more per shape)."""
    from oracle import binding
    L = binding.lib()
    for k, shape in enumerate(SMALL + [(7, 9, 8), (1, 33, 17), (40, 1, 3)]):
        dens = _density(shape, 100 + k)
        p = _points(shape, 200 + k, n_uniform=1500, n_struct=1500)
        assert len(p) >= 2000
        got = np_grid_lookup(dens, p)
        want = np.array([L.oracle_grid_lookup(binding.fp(dens), *shape, float(q[0]), float(q[1]), float(q[2]))
                         for q in p], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), shape


_cases = {}


def _case(shape):
    """Density, points and reference values of a small shape: computed once, left unchanged."""
    if shape not in _cases:
        k = SMALL.index(shape)
        dens = _density(shape, 300 + k)
        pts = _points(shape, 400 + k)
        _cases[shape] = (dens, pts, np_grid_lookup(dens, pts))
    return _cases[shape]


def _context(gpu, dens, code, variant="scatter"):
    from acceleratedvolrenderer_amd import capi, scenes
    scene = scenes.s_uniform(n=1, width=4, height=4, variant=variant, density=dens)
    ctx = capi.Context(0)
    ctx.set_grid_layout(code)
    ctx.set_scene(scene)
    # a silent fall-back to the linear layout must not pass
    assert ctx.grid_layout_active() == code
    return ctx, scene


def _fetch(torch, ctx, pts):
    p4 = np.zeros((len(pts), 4), np.float32)
    p4[:, :3] = pts
    d = torch.from_numpy(p4).to("cuda:0")
    out = torch.empty(len(pts), dtype=torch.float32, device="cuda:0")
    ctx.density_fetch(d.data_ptr(), len(pts), out.data_ptr())
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("layout,code", LAYOUTS, ids=[l for l, _ in LAYOUTS])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_layouts_match_lookup_on_small_shapes_and_edges(gpu, shape, layout, code):
    dens, pts, want = _case(shape)
    ctx, _ = _context(gpu, dens, code)
    got = _fetch(gpu, ctx, pts)
    ctx.close()
    same = got.view(np.uint32) == want.view(np.uint32)
    print(f"{shape} {layout}: {int(same.sum())}/{len(same)} points bit-identical")
    assert same.all(), (shape, layout, pts[~same][:3], got[~same][:3], want[~same][:3])


@pytest.fixture(scope="module")
def slab():
    """The slab's densities (also the control's: the same buffer as a grid thin in z)."""
    return _density(SLAB, 7)


def _old_fat_index_differs(shape, p):
    """Per point: whether the earlier fat index (24-bit multiplies under the entry-count guard
    alone) differs from the true one, from the point and the shape alone."""
    nx, ny, nz = shape
    assert (nx + 1) * (ny + 1) * (nz + 1) < 2 ** 31
    ps = np.asarray(p, np.float32) * np.array([nx, ny, nz], np.float32) - np.float32(.5)
    u = np.floor(ps).astype(np.int64) + 1
    inside = np.all((u >= 0) & (u <= np.array([nx, ny, nz])), axis=1)
    m = 0xffffff
    t = (((u[:, 2] & m) * ((ny + 1) & m)) & 0xffffffff) + u[:, 1]
    old = ((((t & m) * ((nx + 1) & m)) & 0xffffffff) + u[:, 0]) & 0xffffffff
    true = (u[:, 2] * (ny + 1) + u[:, 1]) * (nx + 1) + u[:, 0]
    return inside & (old != true)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SLAB, CONTROL], ids=["slab", "control"])
def test_layouts_match_lookup_on_the_slab(gpu, slab, shape):
    """2 * 10^5 uniform points and 2 * 10^4 in the top three voxels of z, in every layout. On
    the slab half of the uniform points lie where the earlier fat index was truncated."""
    nx, ny, nz = shape
    dens = slab.reshape(nz, ny, nx)
    rng = np.random.default_rng(8)
    pts = rng.random((220000, 3)).astype(np.float32)
    pts[200000:, 2] = (1 - 3 * rng.random(20000) / nz).astype(np.float32)
    want = np_grid_lookup(dens, pts)
    hit = _old_fat_index_differs(shape, pts)
    print(f"{shape}: {int(hit.sum())} of {len(pts)} points in the band the earlier fat index truncated")
    assert (hit[:200000].mean() > 0.45 and hit[200000:].mean() > 0.99) if shape == SLAB else not hit.any()
    for layout, code in LAYOUTS:
        ctx, _ = _context(gpu, dens, code)
        got = _fetch(gpu, ctx, pts)
        ctx.close()
        same = got.view(np.uint32) == want.view(np.uint32)
        print(f"{shape} {layout}: {int(same.sum())}/{len(same)} points bit-identical")
        assert same.all(), (shape, layout, pts[~same][:3], got[~same][:3], want[~same][:3])


@pytest.mark.gpu
def test_transmittance_on_the_slab_matches_oracle(gpu, slab):
    """Integrator::Tr through the upper half of the slab (both ends at z > 0.5 in medium space,
    where the earlier fat index was truncated), in the default (fat) layout: bit-exact per query
    against the canonical oracle, as test_transmittance_matches_oracle_and_beer_lambert."""
    from oracle import binding
    nx, ny, nz = SLAB
    ctx, scene = _context(gpu, slab.reshape(nz, ny, nx), 1, variant="chromatic")
    rfm = scene.render_from_medium.astype(np.float64)

    def to_render(pm):
        h = np.concatenate([pm, np.ones((len(pm), 1))], axis=1) @ rfm.T
        return h[:, :3].astype(np.float32)

    rng = np.random.default_rng(9)
    q = 2000
    a, b = rng.random((q, 3)), rng.random((q, 3))
    a[:, 2] = 0.5 + 0.5 * a[:, 2]
    b[:, 2] = 0.5 + 0.5 * b[:, 2]
    p0, p1 = to_render(a), to_render(b)
    mfr = scene.medium_from_render.astype(np.float64)
    for p in (p0, p1):
        assert ((np.concatenate([p, np.ones((q, 1))], axis=1) @ mfr.T)[:, 2] > 0.5).all()
    lam = (360 + 470 * rng.random((q, 4))).astype(np.float32)
    dev = ctx.transmittance(p0, p1, lam)
    ctx.close()
    ora = binding.OracleRun(scene, max_depth=5, seed=0, libm="canonical").transmittance4(p0, p1, lam)
    same = np.mean(np.all(dev.view(np.uint32) == ora.view(np.uint32), axis=1))
    print(f"slab Tr bit-exact queries {same:.5f}; distinct values {len(np.unique(ora))}")
    assert len(np.unique(ora)) > q // 4       # not a degenerate all-0 / all-1 comparison
    assert same == 1.0


def _compare_samples(integ, ref, first, ns):
    """Per-sample replay as tests/test_gpu_parity.py: L, lambda, lambda pdfs and filter weight of
    the last pass against oracle_pixel_sample; the fraction of samples bit-identical in all four."""
    f = integ.scene.film
    npix = f.width * f.height
    _, _, L, lam, pdf = integ.ctx.last_pass_samples(npix, ns)
    wts = integ.ctx.last_pass_weights(npix, ns)
    exact = 0
    for s in range(ns):
        for pix in range(npix):
            Lo, lo, po, _, wo = ref.pixel_sample(pix % f.width, pix // f.width, first + s, with_weight=True)
            g = s * npix + pix
            exact += int(np.array_equal(L[g].view(np.uint32), Lo.view(np.uint32))
                         and np.array_equal(lam[g].view(np.uint32), lo.view(np.uint32))
                         and np.array_equal(np.asarray(pdf[g], np.float32).view(np.uint32),
                                            np.asarray(po, np.float32).view(np.uint32))
                         and np.float32(wts[g]).view(np.uint32) == np.float32(wo).view(np.uint32))
    return exact / (ns * npix)


@pytest.mark.gpu
def test_render_on_the_slab_is_identical_across_layouts_and_replays_the_oracle(gpu, slab):
    """A 16 x 16 film at 2 spp of the chromatic slab scene with the persistent kernel: films and
    per-sample records identical in the three layouts, and every sample the canonical oracle's.
    The camera looks along +y through the slab's upper part (medium z in 0.6 .. 1), so the render
    visits the band the earlier fat index truncated: the linear-layout wavefront lookup trace
    holds 1000 or more such points (computed from the points and the shape alone)."""
    from acceleratedvolrenderer_amd import VolPathIntegrator, scenes
    from acceleratedvolrenderer_amd.scene import OrthographicCamera, Scene
    from oracle import binding
    torch = gpu
    nx, ny, nz = SLAB
    W = H = 16
    spp = 2
    depth = 20
    base = scenes.s_uniform(n=1, width=W, height=H, variant="chromatic", density=slab.reshape(nz, ny, nx))
    cam = OrthographicCamera(pos=(0.5, -1.0, 0.8), look=(0.5, 0.0, 0.8), up=(0.0, 0.0, 1.0),
                             screenwindow=(-0.5, 0.5, -0.2, 0.2))
    scene = Scene(cam, base.film, base.medium, base.lights, sampler=base.sampler)
    out = []
    for layout, code in LAYOUTS:
        integ = VolPathIntegrator(scene, device=0, maxdepth=depth, spp=spp, kernel="persistent", grid_layout=layout)
        assert integ.ctx.grid_layout_active() == code
        rgb, w = integ.render()
        _, ns, L, lam, _ = integ.ctx.last_pass_samples(W * H, spp)
        out.append((rgb, w, L.view(np.uint32), lam.view(np.uint32)))
        if layout != "fat":
            integ.close()
        else:
            fat = integ
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b)
    canon = binding.OracleRun(scene, max_depth=depth, seed=0, libm="canonical")
    fat.render()                                       # the last pass compared is the fat layout's
    frac = _compare_samples(fat, canon, 0, spp)
    fat.close()
    print(f"slab render: bit-exact samples vs canonical oracle {frac:.5f}")
    # the lookups of the same paths, traced by the wavefront kernels in the linear layout
    tr = VolPathIntegrator(scene, device=0, maxdepth=depth, spp=spp, kernel="wavefront", grid_layout="linear")
    cap = 1 << 20
    pts = torch.zeros((cap, 4), dtype=torch.float32, device="cuda:0")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    tr.ctx.record_lookups(pts.data_ptr(), cap, cnt.data_ptr())
    rgb_t, w_t = tr.render()
    tr.ctx.record_lookups(0, 0, 0)
    n = int(cnt.item())
    assert 0 < n <= cap
    hit = int(_old_fat_index_differs(SLAB, pts[:n, :3].cpu().numpy()).sum())
    tr.close()
    print(f"slab render: {n} lookups, {hit} where the earlier fat index was truncated")
    assert np.array_equal(rgb_t, out[0][0]) and np.array_equal(w_t, out[0][1])
    assert hit >= 1000
    assert frac == 1.0
