"""NanoVDB trees with awkward shapes and the points at which the device's lookup is probed, shared
by tests/test_vdb_cases_reference.py (CPU: the conditions on the points, the oracle against a
float64 reference, the host-compiled csrc/avr_vdb.h against the oracle) and
tests/test_gpu_vdb_shapes.py (the device against the oracle) — TEST INFRASTRUCTURE, no device.

Trees (all valid: leaves and tiles disjoint, origins and sizes multiples of 8):
  thin-z, thin-y, thin-x  dense random values in [0.25, 1.25), 40 x 5 x 3 voxels along the long axis
                   and the two others, index_min all negative ((-3, -13, -37) for thin-z):
                   1 x 1 x 6 blocks and its permutations
  holes128         background 0.05; a 128^3 tile of 0.7 at (0, 0, 0); two 8^3 tiles of 0.3 and 0.9
                   side by side at (-128, -128, 0) and (-120, -128, 0) (their shared face makes the
                   apron classification's -2 branch); isolated random leaves at (-136, 0, 0) and
                   (-8, 120, 8); a leaf at (128, 0, 64) against the big tile's face and one at
                   (128, 128, 128) at its corner; background holes everywhere else
  background       test_vdb.py's two_tiles: background 0.25, tiles of 0.6 and 0.9, a tile of 0.0 (a
                   hole below the background), one leaf; index_min (8, -8, 0)
  single-leaf      3^3 random values at index_min (7, 7, 7): the corners of eight leaves
  mapped-holes128, mapped-thin-x   the same trees behind an index_to_world with a rotation, three
                   different scales (the world box is about unit size) and a translation
Trees without "mapped" have the identity map: world (medium-space) coordinates are index
coordinates exactly (worldToIndexF with the identity matrix and a zero vector is exact).
`temperature()` is mapped-holes128's temperature tree with a map of its own (half the voxel size,
another translation) and a negative index origin.

Points per tree: 10^5 float32 medium-space points.
  * uniform share, 40 %: a quarter uniform over the block extent enlarged by 4 voxels; three
    quarters uniform over the boxes of base voxels whose stencil can see more than one value: a
    leaf's voxels that differ from the background with the layer below them on each axis, and the
    one-voxel layers whose stencil crosses a face of a tile. Uniform points over the whole extent
    alone see a constant stencil almost everywhere (holes128: 272 x 264 x 136 voxels with four
    leaves; thin-z: 3 x 5 x 40 voxels in 8 x 8 x 48), and a probe of constants proves nothing.
  * structured share, 60 %: per axis the integers k at every face of every leaf and tile and at
    the extent's ends -10 ... +10 (the -1 extended block and the first voxels past the extent);
    for each k: k, the floats just below and above, k + 0.5, k + 0.37; and +-10^6. A third of the
    share combines the axes at random with every value of every axis used at least once; two
    thirds pick one of the boxes above and combine, at random, the values of each axis that lie
    within that box (same reason as above).
  * mapped trees: the index-space points go through the float64 index_to_world and are rounded to
    float32.
tests/test_vdb_cases_reference.py asserts the conditions that keep the GPU test from passing on
constants (`conditions`).

References: the oracle's tree (bit for bit), and for identity-map trees a float64 trilinear of
NanoVDBGrid.values semantics (`values` here, a vectorised restatement checked against it), with
tolerance F64_TOL_ULPS x 2^-23 x the tree's largest value: each of the three nested a + w (b - a)
is three float roundings of magnitudes at most the largest value v (values are non-negative, so
b - a, w (b - a) and the sum are all at most v): 3 x 2^-24 v per level; a level's input errors pass
through as a convex combination; 9 x 2^-24 v = 4.5 x 2^-23 v in all."""
import numpy as np

N_POINTS = 100000
N_UNIFORM = 40000
F64_TOL_ULPS = 4.5
IDENTITY = ("thin-z", "thin-y", "thin-x", "holes128", "background", "single-leaf")
MAPPED = ("mapped-holes128", "mapped-thin-x")
TREES = IDENTITY + MAPPED
MAJORANT_RES = (5, 8, 3)

_grids, _points, _temperature = {}, {}, []


def _random(rng, shape):
    """Random values in [0.25, 1.25): a wrong tap cannot give the right value by chance."""
    return (np.float32(0.25) + rng.random(shape, dtype=np.float32)).astype(np.float32)


def _map(voxel, translation):
    """index -> world: R_z(12) R_x(-8) diag(voxel x (1, 1.3, 0.8)), then the translation. The
    angles are small on purpose: pbrt's majorant maps a cell's min and max corners to index space
    and takes the box between them (media.cpp:585-613), which a large rotation turns inside out, so
    that a coarse majorant grid is all zero (R_z(35) R_x(-20) left no cell of (5, 8, 3) above 0)."""
    def rot(i, j, deg):
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        m = np.eye(3)
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    m = np.eye(4)
    m[:3, :3] = rot(0, 1, 12.0) @ rot(1, 2, -8.0) @ np.diag([voxel, 1.3 * voxel, 0.8 * voxel])
    m[:3, 3] = translation
    return m


def _thin(axis, index_to_world=None):
    from acceleratedvolrenderer_amd import NanoVDBGrid
    size = {"z": (3, 5, 40), "y": (5, 40, 3), "x": (40, 3, 5)}[axis]           # (nx, ny, nz)
    mn = {"z": (-3, -13, -37), "y": (-13, -37, -3), "x": (-37, -3, -13)}[axis]
    d = _random(np.random.default_rng(50 + "zyx".index(axis)), size[::-1])
    return NanoVDBGrid.from_dense(d, index_min=mn, index_to_world=index_to_world)


def _holes128(index_to_world=None):
    from acceleratedvolrenderer_amd import NanoVDBGrid
    rng = np.random.default_rng(60)
    leaf_origins = [(-136, 0, 0), (-8, 120, 8), (128, 0, 64), (128, 128, 128)]
    return NanoVDBGrid(leaf_origins, _random(rng, (len(leaf_origins), 8, 8, 8)), background=0.05,
                       tile_origins=[(0, 0, 0), (-128, -128, 0), (-120, -128, 0)], tile_sizes=[128, 8, 8],
                       tile_values=[0.7, 0.3, 0.9], index_to_world=index_to_world)


def grid(name):
    """The tree `name`: built once, left unchanged."""
    if name not in _grids:
        from acceleratedvolrenderer_amd import NanoVDBGrid
        if name.startswith("thin-"):
            g = _thin(name[-1])
        elif name == "holes128":
            g = _holes128()
        elif name == "background":
            e = np.full((24, 16, 16), 0.25, np.float32)
            e[0:8, 0:8, 0:8] = 0.6
            e[8:16, 0:8, 8:16] = 0.9
            e[16:24, 8:16, 0:8] = 0.0
            e[3, 12, 5] = 1.5
            g = NanoVDBGrid.from_dense(e, index_min=(8, -8, 0), background=0.25)
        elif name == "single-leaf":
            g = NanoVDBGrid.from_dense(_random(np.random.default_rng(61), (3, 3, 3)), index_min=(7, 7, 7))
        elif name == "mapped-holes128":
            g = _holes128(_map(1.0 / 272, (0.45, 0.1, 0.35)))
        elif name == "mapped-thin-x":
            g = _thin("x", _map(1.0 / 40, (-0.2, 0.6, 0.15)))
        else:
            raise ValueError(name)
        _grids[name] = g
    return _grids[name]


def temperature():
    """mapped-holes128's temperature tree: 224 x 224 x 112 voxels of half the density's voxel size from
    index (-40, -24, -16), 50 ... 4350 K (some below pbrt's 100 K cut), placed by its own translation
    inside the density's 128^3 tile."""
    if not _temperature:
        from acceleratedvolrenderer_amd import NanoVDBGrid
        nx, ny, nz = 224, 224, 112
        z, y, x = np.meshgrid(np.linspace(0, 1, nz, dtype=np.float32), np.linspace(0, 1, ny, dtype=np.float32),
                              np.linspace(0, 1, nx, dtype=np.float32), indexing="ij")
        t = (50 + 4000 * x * (1 - y) + 300 * z).astype(np.float32)
        d = grid("mapped-holes128")
        # density index (28, 20, 36) is the world position of temperature index (0, 0, 0)
        origin = d.index_to_world[:, :3] @ np.array([28.0, 20.0, 36.0]) + d.index_to_world[:, 3]
        _temperature.append(NanoVDBGrid.from_dense(t, index_min=(-40, -24, -16),
                                                   index_to_world=_map(0.5 / 272, origin)))
    return _temperature[0]


# ---------------------------------------------------------------------------
# the tree's boxes and extent

def boxes(g):
    """(origin, size) int64 arrays of every leaf (size 8) and tile, leaves first."""
    o = np.concatenate([g.leaf_origins, g.tile_origins]).astype(np.int64)
    s = np.concatenate([np.full(len(g.leaf_origins), 8), g.tile_sizes]).astype(np.int64)
    return o, s


def extent(g):
    """(lo, hi): the leaf-aligned box of all leaves and tiles, hi exclusive."""
    o, s = boxes(g)
    return o.min(axis=0), (o + s[:, None]).max(axis=0)


_lookup = {}


def _block_map(g):
    """Per 8^3 block of the extent: the index of the box (boxes order) that holds it, or -1."""
    if id(g) not in _lookup:
        lo, hi = extent(g)
        nb = (hi - lo) // 8
        bm = np.full(tuple(nb), -1, np.int64)
        o, s = boxes(g)
        for k in range(len(o)):
            b = (o[k] - lo) // 8
            n = s[k] // 8
            assert np.all(bm[b[0]:b[0] + n, b[1]:b[1] + n, b[2]:b[2] + n] == -1), "boxes overlap"
            bm[b[0]:b[0] + n, b[1]:b[1] + n, b[2]:b[2] + n] = k
        _lookup[id(g)] = (g, bm, lo, nb)
    return _lookup[id(g)][1:]


def sources(g, ijk):
    """Per integer coordinate ijk (n, 3): the index (boxes order) of the leaf or tile that holds
    it, or -1 for the background."""
    bm, lo, nb = _block_map(g)
    b = (np.asarray(ijk, np.int64) - lo) >> 3
    ok = np.all((b >= 0) & (b < nb), axis=1)
    c = np.clip(b, 0, nb - 1)
    return np.where(ok, bm[c[:, 0], c[:, 1], c[:, 2]], -1)


def values(g, ijk):
    """ReadAccessor::getValue at ijk (n, 3), float32: NanoVDBGrid.values, vectorised."""
    ijk = np.asarray(ijk, np.int64)
    src = sources(g, ijk)
    nl = len(g.leaf_origins)
    out = np.full(len(ijk), g.background, np.float32)
    t = src >= nl
    out[t] = g.tile_values[src[t] - nl]
    l = (src >= 0) & ~t
    q = ijk[l] & 7
    out[l] = g.leaf_values[src[l], q[:, 0], q[:, 1], q[:, 2]]
    return out


# ---------------------------------------------------------------------------
# points

def _interest_boxes(g):
    """float64 boxes [lo, hi) in index space of base voxels whose stencil sees more than one value:
    per leaf the voxels that differ from the background and the layer below them on each axis (the
    stencil of base voxel r reads r and r + 1); per tile and face f the layer [f - 1, f) whose
    stencil crosses the face."""
    out = []
    for o, v in zip(g.leaf_origins.astype(np.float64), g.leaf_values):
        idx = np.argwhere(v != g.background)
        out.append((o + idx.min(axis=0) - 1.0, o + idx.max(axis=0) + 1.0))
    for o, s in zip(g.tile_origins.astype(np.float64), g.tile_sizes.astype(np.float64)):
        for a in range(3):
            for f in (o[a], o[a] + s):
                lo, hi = o - 1.0, o + s
                lo[a], hi[a] = f - 1.0, f
                out.append((lo.copy(), hi.copy()))
    return out


def _axis_values(g, a):
    """The structured values of axis a, float32: see the module docstring."""
    o, s = boxes(g)
    lo, hi = extent(g)
    ks = set(o[:, a].tolist()) | set((o[:, a] + s).tolist())
    ks |= set(range(lo[a] - 10, lo[a] + 11)) | set(range(hi[a] - 10, hi[a] + 11))
    f = np.float32
    v = []
    for k in sorted(ks):
        v += [f(k), np.nextafter(f(k), f(-np.inf)), np.nextafter(f(k), f(np.inf)), f(k) + f(0.5), f(k) + f(0.37)]
    v += [f(1e6), f(-1e6)]
    return np.array(v, np.float32)


def index_points(name):
    """The tree's points in index space, float64 (n, 3); exactly float32 values for the structured
    share."""
    g = grid(name)
    rng = np.random.default_rng(1000 + TREES.index(name))
    lo, hi = extent(g)
    ib = _interest_boxes(g)
    n_whole = N_UNIFORM // 4
    whole = lo - 4.0 + rng.random((n_whole, 3)) * (hi - lo + 8.0)
    pick = rng.integers(0, len(ib), N_UNIFORM - n_whole)
    blo, bhi = np.array([b[0] for b in ib])[pick], np.array([b[1] for b in ib])[pick]
    near = blo + rng.random((len(pick), 3)) * (bhi - blo)
    ax = [_axis_values(g, a) for a in range(3)]
    n_struct = N_POINTS - N_UNIFORM
    n_any = n_struct // 3
    assert max(len(a) for a in ax) <= n_any
    # every value of every axis at least once (cycled), in random combinations across axes
    anyw = np.stack([rng.permutation(np.resize(a, n_any)) for a in ax], axis=1).astype(np.float64)
    # per box: the values of each axis within the box, combined at random
    per_box = (n_struct - n_any) // len(ib) + 1
    local = []
    for blo, bhi in ib:
        cols = []
        for a in range(3):
            inside = ax[a][(ax[a] >= blo[a]) & (ax[a] < bhi[a])]
            assert len(inside), (name, a, blo, bhi)
            cols.append(inside[rng.integers(0, len(inside), per_box)])
        local.append(np.stack(cols, axis=1))
    local = rng.permutation(np.concatenate(local))[:n_struct - n_any].astype(np.float64)
    return np.concatenate([whole, near, anyw, local])


def points(name):
    """The tree's float32 medium-space points (N_POINTS, 3): computed once, left unchanged."""
    if name not in _points:
        g = grid(name)
        q = index_points(name)
        if name in MAPPED:
            q = q @ g.index_to_world[:, :3].T + g.index_to_world[:, 3]
        p = np.ascontiguousarray(q, np.float32)
        assert p.shape == (N_POINTS, 3) and np.isfinite(p).all()
        p.setflags(write=False)
        _points[name] = p
    return _points[name]


def index_coordinates(g, p):
    """worldToIndexF of float32 points p as the tree's float map gives them, float32 (n, 3):
    row r = fmaf(dx, m0, fmaf(dy, m1, dz * m2)) with the fused steps evaluated in float64 and
    rounded to float32 (a double rounding can differ from the fused result in the last bit on rare
    points; used for the conditions' counts and, on identity maps, exact)."""
    inv = g.world_to_index.astype(np.float32)
    vec = g.index_to_world[:, 3].astype(np.float32)
    d = (np.asarray(p, np.float32) - vec).astype(np.float32)
    out = np.empty_like(d)
    for r in range(3):
        t = (d[:, 2] * inv[r, 2]).astype(np.float32)
        t = (d[:, 1].astype(np.float64) * np.float64(inv[r, 1]) + t).astype(np.float32)
        out[:, r] = (d[:, 0].astype(np.float64) * np.float64(inv[r, 0]) + t).astype(np.float32)
    return out


def _corners():
    return [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


def conditions(g, p):
    """Of points p: (share whose eight stencil taps are not all equal, taps' points per box
    (boxes order), points whose base voxel lies in the -1 extended block on some axis and in the
    extended range on all)."""
    x = index_coordinates(g, p)
    ijk = np.floor(x).astype(np.int64)
    o, _ = boxes(g)
    taps = np.stack([values(g, ijk + np.array(c)) for c in _corners()], axis=1)
    varied = float(np.mean(taps.max(axis=1) != taps.min(axis=1)))
    hit = np.zeros((len(p), len(o)), bool)
    for c in _corners():
        s = sources(g, ijk + np.array(c))
        ok = s >= 0
        hit[np.nonzero(ok)[0], s[ok]] = True
    lo, hi = extent(g)
    e = ((ijk - lo) >> 3) + 1
    inside = np.all((e >= 0) & (e <= (hi - lo) // 8), axis=1)
    minus1 = int(np.sum(inside & np.any(e == 0, axis=1)))
    return varied, hit.sum(axis=0), minus1


def trilinear64(g, p):
    """The float64 reference for an identity-map tree: ijk = floor(p), the trilinear of
    getValue(ijk + corner) evaluated in float64."""
    assert np.array_equal(g.index_to_world, np.eye(4)[:3])
    x = np.asarray(p, np.float32).astype(np.float64)
    fl = np.floor(x)
    w = x - fl
    ijk = fl.astype(np.int64)
    out = np.zeros(len(x))
    for c in _corners():
        wt = np.ones(len(x))
        for a in range(3):
            wt = wt * (w[:, a] if c[a] else 1.0 - w[:, a])
        out += wt * values(g, ijk + np.array(c)).astype(np.float64)
    return out


def f64_tolerance(g):
    vmax = max([float(g.background)] + [float(np.max(v)) for v in (g.leaf_values, g.tile_values) if v.size])
    return F64_TOL_ULPS * 2.0 ** -23 * vmax


_oracle = {}


def oracle_tree(name):
    """binding.VdbTree of the tree (`temperature` for the temperature tree), built once."""
    from oracle import binding
    if name not in _oracle:
        _oracle[name] = binding.VdbTree(temperature() if name == "temperature" else grid(name))
    return _oracle[name]


_want = {}


def oracle_values(name):
    """The oracle's sample_world at points(name): computed once, left unchanged."""
    if name not in _want:
        w = oracle_tree(name).sample_world(points(name))
        w.setflags(write=False)
        _want[name] = w
    return _want[name]


def temperature_points():
    """Medium-space float32 points for the temperature tree: mapped-holes128's points (most fall
    outside it: its background) and 50000 uniform over its own extent enlarged by 4 voxels."""
    if "temperature" not in _points:
        t = temperature()
        rng = np.random.default_rng(77)
        lo, hi = extent(t)
        q = lo - 4.0 + rng.random((50000, 3)) * (hi - lo + 8.0)
        q = q @ t.index_to_world[:, :3].T + t.index_to_world[:, 3]
        p = np.ascontiguousarray(np.concatenate([q.astype(np.float32), points("mapped-holes128")]), np.float32)
        p.setflags(write=False)
        _points["temperature"] = p
    return _points["temperature"]


def medium(name, with_temperature=False):
    """A NanoVDBMedium over the tree, with the sigma tables of tests/test_gpu_parity.py's
    _vdb_scene("temperature") when it has the temperature tree."""
    from acceleratedvolrenderer_amd.scene import NanoVDBMedium
    if with_temperature:
        return NanoVDBMedium(grid(name), temperature=temperature(), sigma_a=np.linspace(0.5, 1.5, 471).astype(np.float32),
                             sigma_s=2.0, g=0.3, Lescale=1.5, temperatureoffset=20.0, temperaturescale=1.1)
    return NanoVDBMedium(grid(name), sigma_a=0.5, sigma_s=2.0, g=0.3)


def scene(name, with_temperature=False, width=24, height=20):
    """media_cases.camera_for's orthographic camera over the medium's box, the default lights."""
    import media_cases as mc
    from acceleratedvolrenderer_amd.scene import RGBFilm, Scene
    med = medium(name, with_temperature)
    return Scene(mc.camera_for(med), RGBFilm(width, height), med, mc.default_lights())
