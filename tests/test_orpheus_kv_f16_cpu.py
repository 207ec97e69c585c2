"""The fp16 K/V cache of the Orpheus decoder (TTS_HIP_FLAG_KV_F16), checked without a GPU: the flag's value and documentation, and a gfx950 cross-compile
of the six _Float16 instantiations of the cache's writers and readers (one body per kernel, the element type KV a template parameter) whose resource usage
is read the way test_isa_budget_cpu.py reads it.

The register condition is derived, not measured: an fp16 reader keeps the same rows in flight as its fp32 counterpart in half the registers and adds
nothing that lives as long, so it may not need more vector registers; neither form may spill, and the fp16 form's LDS may not be larger.  Every reader,
fp32 or fp16, stays within 128 VGPRs + AGPRs: a workgroup of 256 threads is one wave per SIMD, a SIMD has 512 registers per lane, and the kernels'
request depths were chosen for four workgroups per CU (512 / 4)."""
import os
import re
import shutil
import subprocess

import pytest

from tts_cpp_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "tts_hip.h")

TU = """
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include "{root}/tts.cpp_amd/csrc/gemv_kernels.h"
#define ATTN_ARGS(KV) const float *, int, const uint32_t *, const KV *, const KV *, int, int, float, float *
#define GQA(SPLIT, KV) template __global__ void attn_gqa_kernel<128, SPLIT, KV>(ATTN_ARGS(KV), const uint32_t *, const uint32_t *, const uint32_t *, int64_t, QPre, int8_t *, float *);
#define WAVE(KV) template __global__ void attn_gqa_wave_kernel<128, 4, false, KV>(ATTN_ARGS(KV), int, const uint32_t *, const uint32_t *, int64_t, QPre);
GQA(false, float) GQA(true, float) WAVE(float)
GQA(false, _Float16) GQA(true, _Float16) WAVE(_Float16)
template __global__ void gemv_q4_qkv_rope_kernel<4, 0, 2, _Float16>(QGemmArgs, const uint8_t *, RopeEpi<_Float16>, RmsSrc);
template __global__ void gemv_q4_qkv_rope_kernel<4, 2, 2, _Float16>(QGemmArgs, const uint8_t *, RopeEpi<_Float16>, RmsSrc);
template __global__ void llama_rope_kv_kernel<_Float16>(float *, const uint32_t *, const float *, float, int, int, int, _Float16 *, _Float16 *, const uint32_t *, int64_t, int, int64_t);
"""


def test_flag_value_is_the_same_in_the_header_and_in_python():
    text = open(HEADER).read()
    m = re.search(r"#define\s+TTS_HIP_FLAG_KV_F16\s+(\d+)u", text)
    assert m and int(m.group(1)) == hip.FLAG_KV_F16 == 64
    taken = {int(v) for v in re.findall(r"#define\s+TTS_HIP_FLAG_\w+\s+(\d+)u", text)}
    assert taken == {1, 2, 4, 8, 16, 32, 64}          # the next free bit after TTS_HIP_FLAG_DAC_F32, no bit twice
    assert "TTS_HIP_FLAG_KV_F16" in re.search(r"typedef struct tts_hip_orpheus_desc \{.*?\} tts_hip_orpheus_desc;", text, re.S).group(0)


def test_header_names_the_layout_the_rounding_and_the_range():
    text = open(HEADER).read()
    doc = " ".join(re.search(r"#define\s+TTS_HIP_FLAG_KV_F16.*?\*/", text, re.S).group(0).split())
    for needle in ("[slot][layer][position][kv width]", "fp16", "nearest-even", "appended", "65504", "inf", "arithmetic stays fp32", "half the cache memory",
                   "tts_hip_dia_create", "refuse"):
        assert needle in doc, needle


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{mangled kernel name: (VGPRs, AGPRs, scratch bytes per lane, LDS bytes)} from the compiler's remarks"""
    tmp = tmp_path_factory.mktemp("kv_f16_isa")
    cu = tmp / "kv_f16.hip"
    cu.write_text(TU.format(root=ROOT))
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, str(cu)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    out = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        get = lambda what: int(re.search(what + r": (\d+)", blk).group(1))   # noqa: E731
        out[blk.split()[0]] = (get(r"VGPRs"), get(r"AGPRs"), get(r"ScratchSize \[bytes/lane\]"), get(r"LDS Size \[bytes/block\]"))
    return out


def _one(usage, mangled_part):
    hits = [v for k, v in usage.items() if mangled_part in k]
    assert len(hits) == 1, (mangled_part, sorted(usage))
    return hits[0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("f32,f16", [("15attn_gqa_kernelILi128ELb0EfE", "15attn_gqa_kernelILi128ELb0EDF16_E"),
                                     ("15attn_gqa_kernelILi128ELb1EfE", "15attn_gqa_kernelILi128ELb1EDF16_E"),
                                     ("20attn_gqa_wave_kernelILi128ELi4ELb0EfE", "20attn_gqa_wave_kernelILi128ELi4ELb0EDF16_E")],
                         ids=["unsplit", "split", "wave"])
def test_f16_readers_fit_in_the_budget_of_their_fp32_counterparts(usage, f32, f16):
    (v32, a32, s32, l32), (v16, a16, s16, l16) = _one(usage, f32), _one(usage, f16)
    print(f"{f32}: {v32} VGPRs + {a32} AGPRs, scratch {s32}, LDS {l32};  {f16}: {v16} + {a16}, scratch {s16}, LDS {l16}")
    assert s16 == 0 and s32 == 0
    assert v16 + a16 <= v32 + a32
    assert l16 <= l32
    assert v32 + a32 <= 128, f32      # four workgroups of 256 threads per CU
    assert v16 + a16 <= 128, f16


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_f16_writers_compile_for_gfx950_without_scratch(usage):
    for part in ("23gemv_q4_qkv_rope_kernelILi4ELi0ELi2EDF16_E", "23gemv_q4_qkv_rope_kernelILi4ELi2ELi2EDF16_E", "20llama_rope_kv_kernelIDF16_E"):
        v, a, scratch, _ = _one(usage, part)
        print(f"{part}: {v} VGPRs + {a} AGPRs, scratch {scratch}")
        assert scratch == 0, part
