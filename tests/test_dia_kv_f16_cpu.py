"""The fp16 self and cross K/V caches of a Dia context (tts_hip_dia_desc::kv_type), checked without a GPU: the field and its documentation, what the
libraries and the Python layer expose, and a gfx950 cross-compile of the cross-attention kernel's two instantiations, attn_gqa_wave_kernel<128, U, EXT, KV>
at KV = _Float16 next to KV = float (U = KVRow<KV>::EXT_SLOTS: 4 and 3).

The register condition is derived, not measured: the fp16 instantiation keeps a pass in flight in 8 registers where the fp32 one needs 16, and
adds nothing that lives as long; with 4 slots against 3 it holds 32 row registers against 48 — so it may not need more vector registers
than the fp32 instantiation of the same compile, neither may spill, and the static LDS (partials of four waves, the folded query) is the same.  Both stay
within 128 VGPRs + AGPRs, the line of four 256-thread workgroups per CU (512 registers per lane and SIMD / 4) that their slot counts were chosen for."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

from tts_cpp_amd import gguf, hip, runner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "tts_hip.h")

TU = """
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include "{root}/tts.cpp_amd/csrc/gemv_kernels.h"
#include "{root}/tts.cpp_amd/csrc/dia_kernels.h"
#define ATTN_ARGS(KV) const float *, int, const uint32_t *, const KV *, const KV *, int, int, float, float *
#define EXT(KV) template __global__ void attn_gqa_wave_kernel<128, KVRow<KV>::EXT_SLOTS, true, KV>(ATTN_ARGS(KV), int, const uint32_t *, const uint32_t *, int64_t, QPre);
EXT(float) EXT(_Float16)
template __global__ void dia_stream_clear_kernel<_Float16>(_Float16 *, _Float16 *, uint64_t, int, int64_t, int);
"""


def _desc():
    return re.search(r"typedef struct tts_hip_dia_desc \{.*?\} tts_hip_dia_desc;", open(HEADER).read(), re.S).group(0)


def test_header_declares_kv_type_last_in_the_dia_desc():
    body = _desc()
    fields = re.findall(r"^\s*(?:uint32_t|float)\s+(\w+);", body, re.M)
    assert fields[-1] == "kv_type" and fields[-2] == "max_utterances"      # appended: every earlier field keeps its offset
    text = open(HEADER).read()
    assert re.search(r"TTS_HIP_F32\s*=\s*0,", text) and re.search(r"TTS_HIP_F16\s*=\s*1,", text)      # a zeroed desc stays fp32


def test_header_documents_rounding_range_and_the_calls():
    doc = " ".join(re.search(r"uint32_t kv_type;\s*/\*.*?\*/", _desc(), re.S).group(0).split())
    for needle in ("TTS_HIP_F32", "TTS_HIP_F16", "[layer][row slot][max_gen][kv width]", "[layer][row slot][max_ctx][heads * head_dim]", "nearest-even", "65504", "inf",
                   "6.1e-5", "arithmetic stays fp32", "half the cache memory", "encoder's own K/V scratch stays fp32", "tts_hip_dia_encode", "tts_hip_dia_step",
                   "tts_hip_dia_generate", "gen_*", "stream_*", "refused", "tts_hip_dia_create"):
        assert needle in doc, needle
    flag = " ".join(re.search(r"#define\s+TTS_HIP_FLAG_KV_F16.*?\*/", open(HEADER).read(), re.S).group(0).split())
    assert "tts_hip_dia_desc::kv_type" in flag          # the flag stays refused on Dia and says where to go instead


def test_python_layer_takes_kv_type():
    names = [n for n, _ in hip.DiaDesc._fields_]
    assert names[-1] == "kv_type" and names[-2] == "max_utterances"
    p = inspect.signature(hip.DiaEngine.__init__).parameters
    assert "kv_type" in p and p["kv_type"].default == gguf.F32 == 0 and gguf.F16 == 1
    assert "di_kv_elem" in hip.DiaEngine.debug_read.__doc__


def test_libraries_export_what_the_option_uses():
    """the create call and the debug item travel through existing symbols; the runner's element size through tts_c_runner_kv_element_bytes"""
    L = hip.load_lib()
    for name in ("tts_hip_dia_create", "tts_hip_debug_read", "tts_hip_tune"):
        assert hasattr(L, name), name
    R = runner.load_lib()
    assert hasattr(R, "tts_c_runner_kv_element_bytes")
    src = open(os.path.join(ROOT, "tts.cpp_amd", "host", "dia_runner.h")).read()
    assert re.search(r"kv_element_bytes\(\) const override", src)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{mangled kernel name: (VGPRs, AGPRs, scratch bytes per lane, LDS bytes)} from the compiler's remarks"""
    tmp = tmp_path_factory.mktemp("dia_kv_f16_isa")
    cu = tmp / "dia_kv_f16.hip"
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
def test_ext_f16_kernel_fits_in_the_budget_of_the_fp32_ext_kernel(usage):
    v32, a32, s32, l32 = _one(usage, "20attn_gqa_wave_kernelILi128ELi3ELb1EfE")
    v16, a16, s16, l16 = _one(usage, "20attn_gqa_wave_kernelILi128ELi4ELb1EDF16_E")
    print(f"fp32 EXT <128, 3>: {v32} VGPRs + {a32} AGPRs, scratch {s32}, LDS {l32};  fp16 EXT <128, 4>: {v16} + {a16}, scratch {s16}, LDS {l16}")
    assert s16 == 0 and s32 == 0
    assert l16 == l32
    assert v16 + a16 <= v32 + a32
    assert v32 + a32 <= 128      # four workgroups of 256 threads per CU
    assert v16 + a16 <= 128


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_clear_kernel_compiles_for_gfx950_without_scratch(usage):
    v, a, scratch, lds = _one(usage, "23dia_stream_clear_kernelIDF16_E")
    assert scratch == 0 and lds == 0
