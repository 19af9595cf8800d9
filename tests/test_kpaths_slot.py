"""The k_paths kernel table (csrc/avr_kpaths_slot.h over csrc/avr_kpaths_list.h): the list's 168
instantiations fill 168 distinct slots of the 192, the 24 left are RGBGridMedium's gray slots and
resolve to the non-gray entry beside them, and every render configuration selects the
instantiation whose template arguments are its own. Checked on the host: a stand-alone program
expands the list as avr_context_create does and prints the table; the expected names are written
out here independently."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acceleratedvolrenderer_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "avr_kpaths_list.h"
#include "avr_kpaths_slot.h"
int main() {
    using namespace avr::kp;
    const char *names[kNumSlots] = {};
    int hits[kNumSlots] = {};
#define ENTRY(em, gr, zs, med, im, fa) \
    ++hits[slot_of(em, gr, zs, med, im, fa)]; names[slot_of(em, gr, zs, med, im, fa)] = AVR_KP_NAME(em, gr, zs, med, im, fa);
    AVR_KP_ALL(ENTRY)
    for (int k = 0; k < kNumSlots; ++k) std::printf("F|%d|%d|%s\n", k, hits[k], names[k] ? names[k] : "");
    alias_rgb_gray(names);
    for (int k = 0; k < kNumSlots; ++k) std::printf("A|%d|%s\n", k, names[k] ? names[k] : "");
    for (int fast = 0; fast < 2; ++fast) for (int image = 0; image < 2; ++image) for (int type = 0; type < 5; ++type)
    for (int smp = 0; smp < 3; ++smp) for (int em = 0; em < 2; ++em) for (int gray = 0; gray < 2; ++gray)
        std::printf("S|%d|%d|%d|%d|%d|%d|%d\n", fast, image, type, smp, em, gray,
                    select(fast, image, type, smp ? 1 : 0, smp == 2, em, gray));
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("kpslot")
    src = d / "slots.cpp"
    src.write_text(PROGRAM)
    exe = d / "slots"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])
    rows = [l.split("|") for l in subprocess.check_output([str(exe)], text=True).splitlines()]
    filled = {int(r[1]): (int(r[2]), r[3]) for r in rows if r[0] == "F"}
    aliased = {int(r[1]): r[2] for r in rows if r[0] == "A"}
    select = {tuple(int(x) for x in r[1:7]): int(r[7]) for r in rows if r[0] == "S"}
    return filled, aliased, select


def _b(x):
    return "true" if x else "false"


def test_list_fills_168_distinct_slots(table):
    filled, _, _ = table
    assert len(filled) == 192
    assert sum(1 for h, _ in filled.values() if h == 1) == 168
    assert sum(1 for h, _ in filled.values() if h == 0) == 24
    assert len({n for h, n in filled.values() if h}) == 168   # 168 different instantiations


def test_empty_slots_are_rgb_gray_and_alias_their_neighbour(table):
    filled, aliased, _ = table
    empty = sorted(k for k, (h, _) in filled.items() if h == 0)
    # slot = ((((fast*2 + image)*4 + medium)*3 + sampler)*2 + emissive)*2 + gray, medium 2 = RGB grid
    expect = sorted(((((f * 2 + i) * 4 + 2) * 3 + s) * 2 + e) * 2 + 1
                    for f, i, s, e in itertools.product(range(2), range(2), range(3), range(2)))
    assert empty == expect
    for k in empty:
        assert aliased[k] == filled[k - 1][1] != ""
        assert aliased[k].split(", ")[1] == "false" and aliased[k].split(", ")[3] == "4"   # non-gray, RGB grid
    for k in set(filled) - set(empty):
        assert aliased[k] == filled[k][1]


def test_every_configuration_selects_its_instantiation(table):
    _, aliased, select = table
    assert len(select) == 2 * 2 * 5 * 3 * 2 * 2
    for (fast, image, mtype, smp, em, gray), slot in select.items():
        # medium types 0 grid, 1 homogeneous, 2 cloud, 3 NanoVDB, 4 RGB grid -> the kernels' medium
        # kinds 0, 1, 1, 3, 4; samplers independent, ZSobol 32-bit, ZSobol 64-bit -> 0, 2, 3;
        # an RGB grid is never gray
        med = {0: 0, 1: 1, 2: 1, 3: 3, 4: 4}[mtype]
        want = "k_paths<%s, %s, %d, %d, %s, %s>" % (_b(em), _b(gray and mtype != 4), (0, 2, 3)[smp], med,
                                                     _b(image), _b(fast))
        assert aliased[slot] == want, (fast, image, mtype, smp, em, gray)
