"""Index arithmetic of the GridMedium density layouts (csrc/avr_grid_index.h): the fat copy's
entry index (24-bit multiplies where every operand fits them, 64-bit otherwise), the bricked
copy's float offset and the linear index, compiled for the host with g++ and compared with exact
Python-int arithmetic on cubes, thin slabs and grids whose copies pass 2^31 entries: at the
corners of the index range, around every cell where the inner term or the whole index crosses a
multiple of 2^24 (2^31 and 2^32 among them) and at random cells.

The earlier fat index took the 24-bit multiplies whenever the copy had fewer than 2^31 entries;
its inner term (iz + 1)(ny + 1) + iy + 1 passes 2^24 on a 1 x 4096 x 4096 grid, where it read
wrong entries without a fault. That expression is kept here (old_fat) to show the test sees it."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = [(1, 1, 1), (1, 1, 64), (64, 1, 1), (2, 3, 5), (7, 8, 9), (8, 8, 8), (9, 16, 17), (15, 16, 17), (255, 3, 2)]
CUBES = [(1024,) * 3, (1290,) * 3]
SLABS = [(1, 4096, 4096), (1, 8190, 4096), (2, 4100, 4100), (8190, 4096, 1), (4096, 1, 8190), (8190, 1, 4096),
         (1, 4096, 8190), (4096, 8190, 1), (16777215, 1, 1)]
HUGE = [(1290, 1290, 1291), (1, 46340, 46340)]
SHAPES = SMALL + CUBES + SLABS + HUGE

SHIM = r"""
#define AVR_HD inline
#include <cstdint>
#include "%s"
typedef unsigned long long u64;
// the fat index as it was: 24-bit multiplies whenever the copy has fewer than 2^31 entries
static inline uint32_t m24(uint32_t a, uint32_t b) { return (a & 0xffffffu) * (b & 0xffffffu); }
static inline u64 old_fat_index(int nx, int ny, int nz, int ix, int iy, int iz) {
  const uint32_t ex = (uint32_t)nx + 1, ey = (uint32_t)ny + 1;
  if ((uint64_t)ex * ey * ((uint64_t)nz + 1) < (1ull << 31))
    return (u64)(m24(m24((uint32_t)(iz + 1), ey) + (uint32_t)(iy + 1), ex) + (uint32_t)(ix + 1));
  return (((u64)(iz + 1) * ey + (iy + 1)) * ex + (ix + 1));
}
extern "C" {
int fat_24bit(int nx, int ny, int nz) { return avr::fat_index_is_24bit(nx, ny, nz) ? 1 : 0; }
void fat(int nx, int ny, int nz, int n, const int *c, u64 *out) {
  for (int i = 0; i < n; ++i) out[i] = avr::fat_entry_index(nx, ny, nz, c[3 * i], c[3 * i + 1], c[3 * i + 2]); }
void old_fat(int nx, int ny, int nz, int n, const int *c, u64 *out) {
  for (int i = 0; i < n; ++i) out[i] = old_fat_index(nx, ny, nz, c[3 * i], c[3 * i + 1], c[3 * i + 2]); }
void linear(int nx, int ny, int nz, int n, const int *c, u64 *out) {
  for (int i = 0; i < n; ++i) out[i] = avr::grid_linear_index(nx, ny, nz, c[3 * i], c[3 * i + 1], c[3 * i + 2]); }
void brick(const int *nb, int n, const int *c, u64 *out) {
  for (int i = 0; i < n; ++i) out[i] = avr::brick_float_offset(nb, c[3 * i], c[3 * i + 1], c[3 * i + 2]); }
int brick_floats() { return avr::kBrickFloats; }
unsigned mul_u24(unsigned a, unsigned b) { return avr::mul_u24(a, b); }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("gridindex")
    src = d / "shim.cpp"
    src.write_text(SHIM % os.path.join(ROOT, "acceleratedvolrenderer_amd", "csrc", "avr_grid_index.h"))
    so = d / "shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    ip, up = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ulonglong)
    for name in ("fat", "old_fat", "linear"):
        getattr(L, name).argtypes = [ctypes.c_int] * 4 + [ip, up]
        getattr(L, name).restype = None
    L.brick.argtypes = [ip, ctypes.c_int, ip, up]
    L.brick.restype = None
    L.fat_24bit.argtypes = [ctypes.c_int] * 3
    L.mul_u24.argtypes = [ctypes.c_uint] * 2
    L.mul_u24.restype = ctypes.c_uint
    return L


def _run(fn, head, cells):
    c = np.ascontiguousarray(cells, np.int32)
    out = np.zeros(len(c), np.uint64)
    fn(*head, len(c), c.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
       out.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))
    return [int(v) for v in out]


def _crossings(limit):
    """Every multiple of 2^24 below `limit` (2^31 and 2^32 are among them), with its neighbours."""
    return [t + d for t in range(1 << 24, limit, 1 << 24) for d in (-1, 0, 1) if 0 <= t + d < limit]


def _cells(ext, rng):
    """Cells of an x-fastest index over extents ext = (ex, ey, ez), as 0-based coordinates: the
    eight corners, the cells where the inner term z * ey + y or the whole index crosses a
    multiple of 2^24 (the crossing and +-1), and 20 000 random ones."""
    ex, ey, ez = ext
    cells = list(itertools.product((0, ex - 1), (0, ey - 1), (0, ez - 1)))
    for t in _crossings(ey * ez):
        cells += [(x, t % ey, t // ey) for x in (0, ex // 2, ex - 1)]
    for e in _crossings(ex * ey * ez):
        cells.append((e % ex, (e // ex) % ey, e // (ex * ey)))
    r = np.stack([rng.integers(0, k, 20000) for k in ext], axis=1)
    return cells + [tuple(int(v) for v in row) for row in r]


def _flat(ext, c):
    return (c[2] * ext[1] + c[1]) * ext[0] + c[0]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fat_entry_index_is_exact(lib, shape):
    nx, ny, nz = shape
    ext = (nx + 1, ny + 1, nz + 1)
    cells = _cells(ext, np.random.default_rng(nx * 7 + ny * 3 + nz))
    want = [_flat(ext, c) for c in cells]
    got = _run(lib.fat, shape, [(x - 1, y - 1, z - 1) for x, y, z in cells])   # footprints -1 .. n - 1
    bad = [(c, g, w) for c, g, w in zip(cells, got, want) if g != w]
    assert not bad, (shape, len(bad), bad[:3])
    # the 24-bit path exactly where every operand provably fits it
    fits = ext[1] * ext[2] < 2 ** 24 and ext[0] < 2 ** 24 and ext[0] * ext[1] * ext[2] < 2 ** 31
    assert bool(lib.fat_24bit(*shape)) == fits


def test_fat_index_paths():
    """Which shapes take which path, from the bounds alone: the flagship cube keeps the 24-bit
    multiplies, every slab and every copy of 2^31 entries or more takes the plain path."""
    fits = lambda s: (s[1] + 1) * (s[2] + 1) < 2 ** 24 and s[0] + 1 < 2 ** 24 and (s[0] + 1) * (s[1] + 1) * (s[2] + 1) < 2 ** 31
    assert all(fits(s) for s in SMALL + [(1024,) * 3, (1289,) * 3, (8190, 4096, 1)])
    assert not any(fits(s) for s in [(1290,) * 3, (1, 4096, 4096), (1, 8190, 4096), (2, 4100, 4100), (16777215, 1, 1)] + HUGE)


def test_old_fat_index_was_wrong_on_the_slab_and_the_new_one_is_right(lib):
    """Failing first, both directions: on 1 x 4096 x 4096 the footprint iz = 4094, iy = 0 has the
    inner term 4095 * 4097 + 1 = 2^24, which the 24-bit multiply truncates to 0."""
    shape, cell = (1, 4096, 4096), (0, 0, 4094)
    true = ((cell[2] + 1) * 4097 + cell[1] + 1) * 2 + cell[0] + 1
    assert true == 2 ** 25 + 1
    old = _run(lib.old_fat, shape, [cell])[0]
    new = _run(lib.fat, shape, [cell])[0]
    assert old != true and old == 1       # the entry of footprint (0, -1, -1): inside the copy, no fault
    assert new == true
    # the band the issue names: every footprint with iz >= 4094 and iy >= 0 went astray, none below
    rng = np.random.default_rng(2)
    band = [(int(rng.integers(-1, 1)), int(rng.integers(0, 4096)), int(rng.integers(4094, 4096))) for _ in range(2000)]
    below = [(int(rng.integers(-1, 1)), int(rng.integers(-1, 4096)), int(rng.integers(-1, 4094))) for _ in range(2000)]
    flat = lambda c: ((c[2] + 1) * 4097 + c[1] + 1) * 2 + c[0] + 1
    assert all(o != flat(c) and o < flat(c) for o, c in zip(_run(lib.old_fat, shape, band), band))
    assert all(o == flat(c) for o, c in zip(_run(lib.old_fat, shape, below), below))
    assert all(n == flat(c) for n, c in zip(_run(lib.fat, shape, band + below), band + below))
    # and the old expression is the one the cubes were rendered with: right there
    cube = (1024,) * 3
    cc = [tuple(int(v) - 1 for v in rng.integers(0, 1025, 3)) for _ in range(2000)]
    assert _run(lib.old_fat, cube, cc) == _run(lib.fat, cube, cc)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_index_is_exact(lib, shape):
    cells = _cells(shape, np.random.default_rng(sum(shape)))
    want = [_flat(shape, c) for c in cells]
    got = _run(lib.linear, shape, cells)
    bad = [(c, g, w) for c, g, w in zip(cells, got, want) if g != w]
    assert not bad, (shape, len(bad), bad[:3])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_brick_float_offset_is_exact(lib, shape):
    """u = i + 1 in 0 .. n per axis; nb = ceil((n + 1) / 8) bricks per axis, as avr_medium_grid."""
    K = lib.brick_floats()
    assert K == 736
    nb = tuple((n + 8) // 8 for n in shape)
    rng = np.random.default_rng(sum(shape) + 1)
    ext = tuple(n + 1 for n in shape)
    cells = list(itertools.product(*((0, n) for n in shape)))
    # around every float offset where the whole offset or the brick index crosses a multiple of
    # 2^24: the footprint nearest the crossing, the last footprint of the brick before and the
    # first of the brick after
    nbricks = nb[0] * nb[1] * nb[2]
    bricks = set()
    for off in _crossings(nbricks * K):
        b, l = divmod(off, K)
        loc = tuple(min(7, v) for v in (l % 9, (l // 9) % 9, min(l, 728) // 81))
        for bb, lo in ((b, loc), (b, (0, 0, 0)), (b - 1, (7, 7, 7)), (b + 1, (0, 0, 0))):
            if 0 <= bb < nbricks:
                bricks.add((bb, lo))
    for b in _crossings(nbricks):
        bricks.update({(b, (0, 0, 0)), (b, (7, 7, 7))})
    for b, lo in bricks:
        bc = (b % nb[0], (b // nb[0]) % nb[1], b // (nb[0] * nb[1]))
        cells.append(tuple(min(n, 8 * k + v) for n, k, v in zip(shape, bc, lo)))
    r = np.stack([rng.integers(0, k, 20000) for k in ext], axis=1)
    cells += [tuple(int(v) for v in row) for row in r]
    want = [(((z >> 3) * nb[1] + (y >> 3)) * nb[0] + (x >> 3)) * K + ((z & 7) * 9 + (y & 7)) * 9 + (x & 7)
            for x, y, z in cells]
    c = np.ascontiguousarray(cells, np.int32)
    out = np.zeros(len(c), np.uint64)
    nba = np.asarray(nb, np.int32)
    lib.brick(nba.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(c), c.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
              out.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))
    bad = [(cc, int(g), w) for cc, g, w in zip(cells, out, want) if int(g) != w]
    assert not bad, (shape, len(bad), bad[:3])
    # the footprint's eight taps stay inside the brick's 729 values
    assert max(w % K for w in want) + 91 < 729


def test_host_24bit_multiply_truncates_like_the_device_instruction(lib):
    """The host wrapper keeps the low 24 bits of each operand and the low 32 of the product."""
    rng = np.random.default_rng(5)
    for a, b in [(0, 0), (1 << 24, 5), ((1 << 24) + 3, 7), (0xffffff, 0xffffff), (0xffffffff, 0xffffffff)] + \
            [tuple(int(v) for v in rng.integers(0, 2 ** 32, 2)) for _ in range(2000)]:
        assert lib.mul_u24(a, b) == ((a & 0xffffff) * (b & 0xffffff)) & 0xffffffff
