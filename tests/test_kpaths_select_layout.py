"""avr::kp::select's density-layout argument (csrc/avr_kpaths_slot.h): the parked instantiations
(gray GridMedium, no emission, no image light) read the fat layout alone, so a render whose
GridMedium has no fat copy (grid_layout linear or brick) must launch the general instantiation
beside them, the kImage one; every other configuration selects the same slot with and without
a fat copy, and the default argument is the fat layout. Checked on the host, as
tests/test_kpaths_slot.py checks the table: a stand-alone program prints select() for every
configuration."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acceleratedvolrenderer_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "avr_kpaths_slot.h"
int main() {
    using namespace avr::kp;
    for (int fast = 0; fast < 2; ++fast) for (int image = 0; image < 2; ++image) for (int type = 0; type < 5; ++type)
    for (int smp = 0; smp < 3; ++smp) for (int em = 0; em < 2; ++em) for (int gray = 0; gray < 2; ++gray)
        std::printf("%d %d %d %d %d %d %d %d %d %d\n", fast, image, type, smp, em, gray,
                    select(fast, image, type, smp ? 1 : 0, smp == 2, em, gray),
                    select(fast, image, type, smp ? 1 : 0, smp == 2, em, gray, true),
                    select(fast, image, type, smp ? 1 : 0, smp == 2, em, gray, false),
                    int(parked(em, gray, medium_arg(type), image)));
    return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("kpselect")
    src = d / "select.cpp"
    src.write_text(PROGRAM)
    exe = d / "select"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])
    return [tuple(int(x) for x in l.split()) for l in subprocess.check_output([str(exe)], text=True).splitlines()]


def test_a_parked_medium_without_a_fat_copy_runs_the_image_instantiation(rows):
    assert len(rows) == 2 * 2 * 5 * 3 * 2 * 2
    by_cfg = {r[:6]: r[6:] for r in rows}
    n_parked = 0
    for (fast, image, mtype, smp, em, gray), (default, fat, nofat, parked) in by_cfg.items():
        # parked: gray GridMedium (type 0), no emission, no image light
        assert parked == int(mtype == 0 and gray and not em and not image)
        assert default == fat                       # the default argument is the fat layout
        if parked:
            n_parked += 1
            # the same configuration's slot with image lights: the general instantiation
            assert nofat == by_cfg[(fast, 1, mtype, smp, em, gray)][1]
            assert nofat != fat
        else:
            assert nofat == fat
    assert n_parked == 2 * 3                        # replay and fast, three samplers
