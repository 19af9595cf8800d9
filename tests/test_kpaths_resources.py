"""Compiler-reported resources of k_paths' headline instantiation (gray GridMedium, 64-bit
ZSobol index, replay: the kernel bench.py's flagship line spends its time in).

It runs at 5 waves/SIMD only while it fits 96 VGPRs without scratch and five 256-lane blocks
fit a CU's 160 KiB of LDS (at most 32 KiB each). The instantiation is cross-compiled alone for
gfx950 with the build's own flags and the figures are read from the
-Rpass-analysis=kernel-resource-usage remarks (what tools/kres.py tabulates). No GPU needed."""
import os
import re
import subprocess

import pytest

from acceleratedvolrenderer_amd import build as avr_build

HEADLINE = "false, true, 3, 0, false, false"


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(avr_build.HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("kpaths_resources")
    src = tmp / "headline.hip"
    src.write_text('#define AVR_KPATHS_TU\n#include "avr_kernels.hip"\n'
                   f"namespace avr {{ template __global__ void k_paths<{HEADLINE}>(Params); }}\n")
    cmd = ([avr_build.HIPCC] + avr_build.FLAGS + avr_build.kp_unit_flags(0) +
           ["-I" + avr_build.CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
            "-c", str(src), "-o", str(tmp / "headline.o")])
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    log = r.stderr
    assert len(re.findall(r"Function Name: (\S+)", log)) == 1
    assert "k_pathsILb0ELb1ELi3ELi0ELb0ELb0E" in log
    out = {}
    for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
        out[key] = int(re.search(pat, log).group(1))
    print(f"k_paths<{HEADLINE}>: {out}")
    return out


def test_headline_kernel_fits_five_waves(usage):
    assert usage["vgpr"] <= 96 and usage["agpr"] == 0
    assert usage["scratch"] == 0
    assert usage["lds"] <= 32768          # five 256-lane blocks per CU
    assert usage["occ"] == 5
