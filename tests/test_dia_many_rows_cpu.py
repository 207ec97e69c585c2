"""Without a GPU: the two producers of Dia's tiled route (csrc/dia_rows_kernels.h, a unit of their own: shim_dia_rows.hip) cross-compiled for gfx950, and the public header.

rms_fold_rows_f16_kernel holds a row of up to 2048 values, its weight and 32 slab values of one round trip in registers, and silu_mul_f16_kernel eight
values per lane: a spill to scratch would serialise exactly the loads they issue straight-line.  Bounds ("Dia with up to 128 lock-step utterances"):
silu_mul_f16_kernel 64 VGPRs (compiled: 39); the rms form 84 (compiled: 80) — 48 values plus the eight 64-bit addresses of the clamped columns; a launch
has one workgroup of four waves per row, at most 256, so occupancy is not what the count buys."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BOUNDS = {"rms_fold_rows_f16_kernel": 84, "silu_mul_f16_kernel": 64}      # compiled: 80 and 39


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tiled_route_producers_fit_their_registers_without_scratch(tmp_path):
    src = tmp_path / "dia_rows.hip"
    src.write_text(f'#include <hip/hip_runtime.h>\n#include <algorithm>\n#include <cmath>\n#include "{ROOT}/tts.cpp_amd/csrc/dia_rows_kernels.h"\n'
                   "// the kernels are static: taking their addresses keeps them in this unit\n"
                   "const void *keep[] = {(const void *) rms_fold_rows_f16_kernel, (const void *) silu_mul_f16_kernel};\n")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-Wno-unused-function", "-o", str(tmp_path / "dia_rows.s"), str(src)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    seen = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", p.stderr, re.S):
        seen[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4))
    for k, bound in BOUNDS.items():
        names = [n for n in seen if k in n]
        assert len(names) == 1, (k, sorted(seen))
        vgpr, agpr, scratch = seen[names[0]]
        print(f"{k}: {vgpr} VGPRs + {agpr} AGPRs, scratch {scratch}")
        assert scratch == 0, f"{k} spills ({scratch} bytes per lane)"
        assert agpr == 0 and vgpr <= bound, f"{k}: {vgpr} VGPRs + {agpr} AGPRs, bound {bound}"


def test_header_names_the_cap_and_the_key():
    text = open(os.path.join(ROOT, "include", "tts_hip.h")).read()
    at = text.index("uint32_t max_utterances;")
    desc = text[at:text.index("uint32_t kv_type;", at)]
    assert "128" in desc and "tts_hip_dia_create" in desc
    tune = text[text.index("Tuning and fallback switches by name"):text.index("int tts_hip_tune(")]
    assert "dia_tile_min_rows" in tune and "17" in tune
