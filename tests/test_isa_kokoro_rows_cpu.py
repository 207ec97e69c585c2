"""The lock-step Kokoro recurrence keeps everything in registers, checked without a GPU in the way of tests/test_isa_budget_cpu.py: hipcc cross-compiles
kk_lstm_rows_kernel<CP> for gfx950 at every instantiated CP and -Rpass-analysis=kernel-resource-usage says what each takes.

A thread holds CP recurrent weights for the whole launch plus, per live sequence, a poll in flight, an input term and an accumulator.  The grid is
hid / 16 workgroups of 4 waves per direction with one wave per SIMD, so a wave may use the SIMD's 512 registers per lane; what must hold is that nothing
goes to scratch (a spill would put memory traffic between two granule hand-offs, the time the kernel exists to fill).

VGPRs at the time of writing (AGPRs 0, scratch 0 everywhere): CP 4: 99, CP 8: 103, CP 16: 111, CP 32: 127, CP 64: 165, CP 128: 229
(kk_lstm_split_kernel<CP>, one sequence: 40 at CP 4, 95 at CP 64, 164 at CP 128)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SIMD_VGPRS = 512
CPS = (4, 8, 16, 32, 64, 128)

TU = """
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include "{root}/tts.cpp_amd/csrc/kokoro_kernels.h"
""" + "".join(f"template __global__ void kk_lstm_rows_kernel<{cp}>(LstmRowsArgs);\n" for cp in CPS)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{function name: (VGPRs, AGPRs, scratch bytes per lane)} from the compiler's remarks, one compilation for all cases"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    cu = tmp_path_factory.mktemp("isa") / "kokoro_rows.hip"
    cu.write_text(TU.format(root=ROOT))
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, str(cu)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    out = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        get = lambda what: int(re.search(what + r": (\d+)", blk).group(1))   # noqa: E731
        out[blk.split()[0]] = (get(r"VGPRs"), get(r"AGPRs"), get(r"ScratchSize \[bytes/lane\]"))
    return out


@pytest.mark.parametrize("cp", CPS)
def test_lock_step_recurrence_stays_in_registers(usage, cp):
    hits = [v for k, v in usage.items() if f"kk_lstm_rows_kernelILi{cp}E" in k]
    assert len(hits) == 1, (cp, sorted(usage))
    v, a, scratch = hits[0]
    print(f"kk_lstm_rows_kernel<{cp}>: {v} VGPRs + {a} AGPRs, scratch {scratch}")
    assert scratch == 0, (cp, scratch)
    assert v + a <= SIMD_VGPRS, (cp, v, a)
    assert v >= cp, (cp, v)   # the recurrent weights do live in registers
