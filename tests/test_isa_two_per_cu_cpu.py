"""The forms of gemm_tile_kernel that tune("tile_pair") launches (csrc/shim_decoder.hip: launch_tile_shape), cross-compiled for gfx950 without a GPU.
Two workgroups of eight waves on one CU are four waves per SIMD: a SIMD's 512 vector registers, handed out in granules of 8, leave a wave 128.  A form
above that, or one that spills, would fit the LDS budget (at most 72 KB of 160 KB) and still run alone on its CU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

EPIS = ("EPI_STORE", "EPI_QKV", "EPI_RESID", "EPI_GELU")
# (BM, BN, WM, WN, BK, S): the 128 x 128 tile with two buffers, the 128 x 64 tile with three, and the 64 x 64 tile with four that the rest of a layer takes
FORMS = ((128, 128, 2, 4, 64, 2), (128, 64, 4, 2, 64, 3), (64, 64, 2, 4, 64, 4))
VGPR_PER_SIMD, GRANULE, WAVES_PER_SIMD = 512, 8, 4


def _lds_bytes(bm, bn, bk, s):
    return s * (bm + bn) * bk * 2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_two_per_cu_forms_fit_twice_on_a_cu(tmp_path):
    lines = ["#include <hip/hip_runtime.h>", "#include <algorithm>", "#include <cmath>", f'#include "{ROOT}/tts.cpp_amd/csrc/gemm_tile_kernels.h"']
    want = []
    for bm, bn, wm, wn, bk, s in FORMS:
        assert wm * wn == 8 and 2 * _lds_bytes(bm, bn, bk, s) <= 160 * 1024 and _lds_bytes(bm, bn, bk, s) <= 72 * 1024
        for epi in EPIS + (("EPI_CROSS",) if (bm, bn) == (64, 64) else ()):
            lines.append(f"template __global__ void gemm_tile_kernel<{bm}, {bn}, {wm}, {wn}, {bk}, {s}, {epi}>(GemmArgs, TileMap);")
            want.append(f"gemm_tile_kernelILi{bm}ELi{bn}ELi{wm}ELi{wn}ELi{bk}ELi{s}E")
    src = tmp_path / "two_per_cu.hip"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "two_per_cu.s"), str(src)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    seen = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", p.stderr, re.S):
        seen[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4))
    checked = 0
    for name, (vgpr, agpr, scratch) in seen.items():
        if not any(w in name for w in want):
            continue
        regs = -(-(vgpr + agpr) // GRANULE) * GRANULE
        print(f"{name}: {vgpr} VGPRs + {agpr} AGPRs -> {regs} allocated, scratch {scratch}")
        assert scratch == 0, f"{name} spills ({scratch} bytes per lane)"
        assert regs * WAVES_PER_SIMD <= VGPR_PER_SIMD, f"{name}: {regs} registers per wave, two workgroups of eight waves need <= {VGPR_PER_SIMD // WAVES_PER_SIMD}"
        checked += 1
    assert checked == 2 * len(EPIS) + len(EPIS) + 1, sorted(seen)
