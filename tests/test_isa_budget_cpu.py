"""The register budget that lets a self-attention wave sit beside a codec wave, checked without a GPU: hipcc cross-compiles the
instantiations for gfx950 and -Rpass-analysis=kernel-resource-usage says what each one takes.

A SIMD of gfx950 holds 512 vector registers per lane, handed out in granules of 8.  The codec's fused residual units run two waves per SIMD (one
workgroup of 8 waves per CU: launch_bounds(512, 2)), so a unit of V registers leaves 512 - 2 V to anybody else.  attn_rows_kernel<U> runs one wave per
SIMD and workgroup (16 heads x 16 lanes = 4 waves, no LDS) and needs 80 / 48 / 32 registers at U = 8 / 4 / 2 keys in flight per lane:
  96-channel unit  <= 232  ->  48 left: U = 4 fits
  192-channel unit    240  ->  32 left: U = 2 fits (at <= 232 U = 4 would)
The bars are those boundaries, not what the compiler happens to give today."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SIMD_VGPRS, GRANULE = 512, 8

ATTN_TU = """
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include "{root}/tts.cpp_amd/csrc/gemm_tile_kernels.h"
template __global__ void attn_rows_kernel<2>(AttnArgs);
template __global__ void attn_rows_kernel<4>(AttnArgs);
template __global__ void attn_rows_kernel<8>(AttnArgs);
"""
UNIT_TU = """
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <type_traits>
#include "{root}/tts.cpp_amd/csrc/dac_kernels.h"
#include "{root}/tts.cpp_amd/csrc/dac_b3_kernels.h"
template __global__ void resunit_t7_kernel<3, 3, SplitH2, true, 2, 2>(ResUnitArgs);   // 96 channels, as launch_resunit_t7 instantiates it
template __global__ void resunit_t7_kernel<6, 4, SplitH2, true, 2, 1>(ResUnitArgs);   // 192 channels
"""


def _usage(tmp_path, name, src):
    """-> {demangled-ish function name: (VGPRs, AGPRs, scratch bytes per lane)} from the compiler's remarks"""
    cu = tmp_path / f"{name}.hip"
    cu.write_text(src.format(root=ROOT))
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, str(cu)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    out = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        fn = blk.split()[0]
        get = lambda what: int(re.search(what + r": (\d+)", blk).group(1))   # noqa: E731
        out[fn] = (get(r"VGPRs"), get(r"AGPRs"), get(r"ScratchSize \[bytes/lane\]"))
    return out


def _one(usage, mangled_part):
    hits = [v for k, v in usage.items() if mangled_part in k]
    assert len(hits) == 1, (mangled_part, sorted(usage))
    return hits[0]


def _granules(n):
    return -(-n // GRANULE) * GRANULE


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_attention_rows_kernel_register_budget(tmp_path):
    usage = _usage(tmp_path, "attn_budget", ATTN_TU)
    for u, bar in ((2, 32), (4, 48)):
        v, a, scratch = _one(usage, f"attn_rows_kernelILi{u}E")
        print(f"attn_rows_kernel<{u}>: {v} VGPRs + {a} AGPRs, scratch {scratch}")
        assert _granules(v + a) <= bar and scratch == 0, (u, v, a, scratch)
    v, a, scratch = _one(usage, "attn_rows_kernelILi8E")
    print(f"attn_rows_kernel<8>: {v} VGPRs + {a} AGPRs, scratch {scratch}")
    assert scratch == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fused_units_leave_room_for_an_attention_wave(tmp_path):
    usage = _usage(tmp_path, "unit_budget", UNIT_TU)
    v96, a96, s96 = _one(usage, "resunit_t7_kernelILi3ELi3E")
    v192, a192, s192 = _one(usage, "resunit_t7_kernelILi6ELi4E")
    print(f"96-channel unit: {v96} + {a96}, scratch {s96}; 192-channel unit: {v192} + {a192}, scratch {s192}")
    assert s96 == 0 and s192 == 0
    # 96 channels: two waves of the unit and one wave of attn_rows_kernel<4> (48 registers) per SIMD
    assert SIMD_VGPRS - 2 * _granules(v96 + a96) >= 48, (v96, a96)
    # 192 channels: the unit stays as it is (a cap at 232 registers was measured and buys the default U = 2 nothing), so what must hold
    # is that two of its waves leave the 32 registers of attn_rows_kernel<2>
    assert SIMD_VGPRS - 2 * _granules(v192 + a192) >= 32, (v192, a192)
