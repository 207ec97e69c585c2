"""The producers of an Orpheus forward of 65 .. 256 rows (csrc/llama_kernels.h), cross-compiled for gfx950 without a GPU: rms_fold_rows_q8t_kernel and
silu_mul_q8t_kernel write Q8_0 codes and transposed block scales for qgemm_tile_kernel.  The rms form holds a 3072-wide row and eight slabs of it in
registers (the loads of a round trip are straight-line): a spill to scratch would serialise exactly those loads.  Resource usage only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("rms_fold_rows_q8t_kernel", "silu_mul_q8t_kernel", "rms_fold_rows_kernel")   # the last: the form contexts of at most 64 slots keep launching


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_q8t_producers_compile_without_scratch(tmp_path):
    src = tmp_path / "orpheus_q8t.hip"
    src.write_text(f'#include <hip/hip_runtime.h>\n#include <algorithm>\n#include <cmath>\n#include "{ROOT}/tts.cpp_amd/csrc/llama_kernels.h"\n'
                   "// the kernels are static: taking their addresses keeps them in this unit\n"
                   "const void *keep[] = {(const void *) rms_fold_rows_q8t_kernel, (const void *) silu_mul_q8t_kernel, (const void *) rms_fold_rows_kernel};\n")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-Wno-unused-function", "-o", str(tmp_path / "orpheus_q8t.s"), str(src)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    seen = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", p.stderr, re.S):
        seen[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4))
    for k in KERNELS:
        names = [n for n in seen if re.search(rf"\d+{k}", n) or n == k]   # the mangled name carries the length and the plain name
        assert len(names) == 1, (k, sorted(seen))
        vgpr, agpr, scratch = seen[names[0]]
        print(f"{k}: {vgpr} VGPRs + {agpr} AGPRs, scratch {scratch}")
        assert scratch == 0, f"{k} spills ({scratch} bytes per lane)"
