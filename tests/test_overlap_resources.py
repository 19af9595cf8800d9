"""Pass overlap: a block of the next pass's camera stage runs on every CU beside four
blocks of k_paths' headline instantiation, which is launched with kOverlapLdsPad bytes of dynamic
LDS so that a fifth block of its own does not fit.

That holds only while the compiler-reported resources add up: four k_paths waves and one wave
of the side kernel within a SIMD's 512 VGPRs (allocated in blocks of 8), four padded k_paths
blocks and one camera block within a CU's 160 KiB of LDS, and five padded k_paths blocks beyond
it. k_film is checked with the camera stage: its block has to fit the same slot for it to follow
there. The kernels are cross-compiled for gfx950 with the build's own flags and the figures read
from the -Rpass-analysis=kernel-resource-usage remarks, as tests/test_kpaths_resources.py does.
No GPU needed."""
import os
import re
import subprocess

import pytest

from acceleratedvolrenderer_amd import build as avr_build

LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD = 512
KERNELS = {
    "k_paths": ("k_pathsILb0ELb1ELi3ELi0ELb0ELb0E", "template __global__ void k_paths<false, true, 3, 0, false, false>(Params);"),
    "camera": ("k_paths_cameraILi3ELb0E", "template __global__ void k_paths_camera<3, false>(Params);"),
    "film": ("k_filmILb0ELb0E", "template __global__ void k_film<false, false>(Params);"),
}


def _remarks(tmp, name, body, flags):
    src = tmp / f"{name}.hip"
    src.write_text(body)
    cmd = ([avr_build.HIPCC] + avr_build.FLAGS + flags +
           ["-I" + avr_build.CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
            "-c", str(src), "-o", str(tmp / f"{name}.o")])
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _usage(log, mangled):
    blocks = [b for b in log.split("Function Name: ")[1:] if b.split()[0].startswith("_ZN3avr") and mangled in b.split()[0]]
    assert len(blocks) == 1, (mangled, len(blocks))
    out = {}
    for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
        out[key] = int(re.search(pat, blocks[0]).group(1))
    out["vgpr8"] = (out["vgpr"] + 7) // 8 * 8
    return out


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(avr_build.HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("overlap_resources")
    # k_paths as its build unit compiles it; the camera stage and k_film as the C-ABI unit does
    kp = _remarks(tmp, "kpaths", '#define AVR_KPATHS_TU\n#include "avr_kernels.hip"\n'
                  f"namespace avr {{ {KERNELS['k_paths'][1]} }}\n", avr_build.kp_unit_flags(0))
    side = _remarks(tmp, "side", '#include "avr_kernels.hip"\n'
                    f"namespace avr {{ {KERNELS['camera'][1]} {KERNELS['film'][1]} }}\n", [])
    out = {"k_paths": _usage(kp, KERNELS["k_paths"][0]), "camera": _usage(side, KERNELS["camera"][0]),
           "film": _usage(side, KERNELS["film"][0])}
    with open(os.path.join(avr_build.CSRC, "avr_capi.hip")) as f:
        out["pad"] = int(re.search(r"constexpr int kOverlapLdsPad = (\d+);", f.read()).group(1))
    print(out)
    return out


def test_a_side_block_fits_beside_four_k_paths_blocks(usage):
    kp, cam, film, pad = usage["k_paths"], usage["camera"], usage["film"], usage["pad"]
    assert kp["agpr"] == cam["agpr"] == film["agpr"] == 0
    assert 4 * kp["vgpr8"] + max(cam["vgpr8"], film["vgpr8"]) <= VGPRS_PER_SIMD
    assert 4 * (kp["lds"] + pad) + cam["lds"] <= LDS_PER_CU


def test_the_pad_keeps_a_fifth_k_paths_block_out(usage):
    assert 5 * (usage["k_paths"]["lds"] + usage["pad"]) > LDS_PER_CU
