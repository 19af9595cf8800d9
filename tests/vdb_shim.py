"""csrc/avr_vdb.h compiled for the host behind a C shim, shared by tests/test_vdb.py and
tests/test_vdb_cases_reference.py — TEST INFRASTRUCTURE, no device.

`slots` builds the base block-slot layout as avr_capi.hip's upload_vdb does; `build` compiles the
shim (g++ -ffp-contract=off, the device build's float semantics); `sample` / `sample_apron` call it
for a vdb.NanoVDBGrid."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def slots(grid):
    """The device's block-slot layout (avr_capi.hip upload_vdb), built here for the
    host-compiled header test."""
    boxes = [(o, 8) for o in grid.leaf_origins] + list(zip(grid.tile_origins, grid.tile_sizes))
    lo = np.min([o for o, _ in boxes], axis=0)
    hi = np.max([o + s for o, s in boxes], axis=0)
    nb = (hi - lo) // 8
    slot = np.full((nb[2], nb[1], nb[0]), np.iinfo(np.int32).min, np.int32)
    for t, (o, s) in enumerate(zip(grid.tile_origins, grid.tile_sizes)):
        b = (o - lo) // 8
        slot[b[2]:b[2] + s // 8, b[1]:b[1] + s // 8, b[0]:b[0] + s // 8] = -(t + 1)
    for i, o in enumerate(grid.leaf_origins):
        b = (o - lo) // 8
        slot[b[2], b[1], b[0]] = i
    return slot, lo, nb


def build(d):
    """Compile the shim in directory `d` (a pathlib.Path) and load it."""
    src = d / "shim.cpp"
    src.write_text(
        "#define AVR_HD inline\n"
        f'#include "{ROOT}/acceleratedvolrenderer_amd/csrc/avr_vdb.h"\n'
        "using namespace avr::vdb;\n"
        'extern "C" void sample(const int *slot, const float *leaves, const float *tiles, const int *o, const int *nb,\n'
        "                       float bg, const float *inv, const float *vec, int n, const float *p, float *out) {\n"
        "  Grid g{slot, leaves, tiles, o[0], o[1], o[2], nb[0], nb[1], nb[2], bg};\n"
        "  for (int k = 0; k < 9; ++k) g.inv[k] = inv[k];\n"
        "  for (int k = 0; k < 3; ++k) g.vec[k] = vec[k];\n"
        "  for (int i = 0; i < n; ++i) out[i] = sample_world(g, p[3 * i], p[3 * i + 1], p[3 * i + 2]);\n"
        "}\n"
        # the apron layout the kernels sample, built on the host exactly as upload_vdb +
        # k_vdb_apron build it on the device
        'extern "C" long long sample_apron(const int *slot, const float *leaves, const float *tiles, int ntiles,\n'
        "                       const int *o, const int *nb, float bg, const float *inv, const float *vec, int n,\n"
        "                       const float *p, float *out, float *vals, int fat) {\n"
        "  Grid g{slot, leaves, tiles, o[0], o[1], o[2], nb[0], nb[1], nb[2], bg};\n"
        "  std::vector<int> aslot; std::vector<long long> list;\n"
        "  build_apron_slots(slot, nb[0], nb[1], nb[2], tiles, ntiles, bg, aslot, list);\n"
        "  std::vector<float> consts(tiles, tiles + ntiles); consts.push_back(bg);\n"
        "  std::vector<float> blocks(list.size() * kApronVals);\n"
        "  for (std::size_t i = 0; i < list.size(); ++i) {\n"
        "    const long long e = list[i];\n"
        "    const int ex = e % (nb[0] + 1), ey = (e / (nb[0] + 1)) % (nb[1] + 1), ez = e / ((nb[0] + 1) * (nb[1] + 1));\n"
        "    for (int k = 0; k < kApronVals; ++k) blocks[i * kApronVals + k] = apron_value(g, ex, ey, ez, k);\n"
        "  }\n"
        "  Apron a{aslot.data(), blocks.data(), consts.data(), o[0], o[1], o[2], nb[0], nb[1], nb[2], bg};\n"
        "  for (int k = 0; k < 9; ++k) a.inv[k] = inv[k];\n"
        "  for (int k = 0; k < 3; ++k) a.vec[k] = vec[k];\n"
        "  std::vector<float> fatv(fat ? list.size() * 512 * 8 : 0);\n"
        "  for (long long e = 0; e < (long long)fatv.size() / 8; ++e) apron_fat_entry(blocks.data(), e >> 9, (int)(e & 511), &fatv[8 * e]);\n"
        "  a.fat = fat ? fatv.data() : nullptr;\n"
        "  for (int i = 0; i < n; ++i) out[i] = sample_world(a, p[3 * i], p[3 * i + 1], p[3 * i + 2]);\n"
        "  // getValue over the extent +-10 voxels from the apron layout\n"
        "  long long q = 0;\n"
        "  for (int z = o[2] - 10; z < o[2] + 8 * nb[2] + 10; ++z)\n"
        "    for (int y = o[1] - 10; y < o[1] + 8 * nb[1] + 10; ++y)\n"
        "      for (int x = o[0] - 10; x < o[0] + 8 * nb[0] + 10; ++x) vals[q++] = get_value(a, x, y, z) - get_value(g, x, y, z);\n"
        "  return (long long)list.size();\n"
        "}\n")
    so = d / "shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.sample_apron.restype = ctypes.c_longlong
    return lib


_I = ctypes.POINTER(ctypes.c_int)
_F = ctypes.POINTER(ctypes.c_float)


def _arr(a, t):
    return np.ascontiguousarray(a).ctypes.data_as(t)


def _grid_args(g):
    slot, lo, nb = slots(g)
    keep = dict(slot=slot, lo=lo.astype(np.int32), nb=nb.astype(np.int32),
                inv=g.world_to_index.astype(np.float32).reshape(-1), vec=g.index_to_world[:, 3].astype(np.float32),
                tiles=g.tile_values if len(g.tile_values) else np.zeros(1, np.float32))
    return keep, nb


def sample(lib, g, p):
    """sample_world of the base layout (Grid) at float32 points p (n, 3)."""
    k, _ = _grid_args(g)
    p = np.ascontiguousarray(p, np.float32)
    out = np.zeros(len(p), np.float32)
    lib.sample(_arr(k["slot"], _I), _arr(g.leaf_values, _F), _arr(k["tiles"], _F), _arr(k["lo"], _I), _arr(k["nb"], _I),
               ctypes.c_float(float(g.background)), _arr(k["inv"], _F), _arr(k["vec"], _F), len(p), _arr(p, _F),
               _arr(out, _F))
    return out


def sample_apron(lib, g, p, fat):
    """(sample_world of the apron layout at p, the number of apron blocks, get_value(Apron) -
    get_value(Grid) over the extent +-10 voxels)."""
    k, nb = _grid_args(g)
    p = np.ascontiguousarray(p, np.float32)
    out = np.zeros(len(p), np.float32)
    vals = np.full(int(np.prod(8 * nb + 20)), np.nan, np.float32)
    nblk = lib.sample_apron(_arr(k["slot"], _I), _arr(g.leaf_values, _F), _arr(k["tiles"], _F), len(g.tile_values),
                            _arr(k["lo"], _I), _arr(k["nb"], _I), ctypes.c_float(float(g.background)), _arr(k["inv"], _F),
                            _arr(k["vec"], _F), len(p), _arr(p, _F), _arr(out, _F), _arr(vals, _F), int(fat))
    return out, int(nblk), vals
