"""The opt-in e4m3 K/V cache of the Orpheus decoder (tts_hip_orpheus_desc::kv_type = TTS_HIP_KV_F8_E4M3), checked without a GPU: the constant, the
descriptor's layout and documentation, the numpy rounding reference the GPU tests use (tests/e4m3_reference.py) against torch.float8_e4m3fn, and a gfx950
cross-compile of the six kv_f8 instantiations of the cache's writers and readers whose resource usage is read the way test_orpheus_kv_f16_cpu.py reads it.

The register condition is derived, not measured: an e4m3 reader keeps the same rows in flight as its fp32 counterpart in a quarter of the registers, and
the widened values live no longer than the fp16 form's, so it may not need more vector registers than the fp32 form, and never more than 128 (four
workgroups of 256 threads per CU); no form may spill, and the e4m3 form's LDS may not be larger."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from e4m3_reference import e4m3_finite_codes, e4m3_round
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
GQA(false, kv_f8) GQA(true, kv_f8) WAVE(kv_f8)
template __global__ void gemv_q4_qkv_rope_kernel<4, 0, 2, kv_f8>(QGemmArgs, const uint8_t *, RopeEpi<kv_f8>, RmsSrc);
template __global__ void gemv_q4_qkv_rope_kernel<4, 2, 2, kv_f8>(QGemmArgs, const uint8_t *, RopeEpi<kv_f8>, RmsSrc);
template __global__ void llama_rope_kv_kernel<kv_f8>(float *, const uint32_t *, const float *, float, int, int, int, kv_f8 *, kv_f8 *, const uint32_t *, int64_t, int, int64_t);
"""


# ---- 1. constants and layout ------------------------------------------------------------------------------------------------------------
def _desc_text():
    return re.search(r"typedef struct tts_hip_orpheus_desc \{.*?\} tts_hip_orpheus_desc;", open(HEADER).read(), re.S).group(0)


def test_constant_is_the_same_in_the_header_and_in_python():
    text = open(HEADER).read()
    m = re.search(r"#define\s+TTS_HIP_KV_F8_E4M3\s+(\d+)u", text)
    assert m and int(m.group(1)) == hip.KV_F8_E4M3 == 256
    enum = re.search(r"enum tts_hip_type \{.*?\};", text, re.S).group(0)
    assert "F8" not in enum                                            # not a ggml tensor type id
    taken = {int(v) for v in re.findall(r"#define\s+TTS_HIP_FLAG_\w+\s+(\d+)u", text)}
    assert taken == {1, 2, 4, 8, 16, 32, 64}                           # no new flag bit: the cache type is a field of the descriptor


def test_kv_type_is_the_last_field_of_the_descriptor():
    fields = re.findall(r"^\s*(?:uint32_t|float)\s+(\w+);", _desc_text(), re.M)
    assert fields[-2:] == ["max_seqs", "kv_type"], fields
    names = [n for n, _ in hip.OrpheusDesc._fields_]
    assert names == fields                                             # the binding declares the header's fields in the header's order
    assert hip.OrpheusDesc.kv_type.offset == C.sizeof(hip.OrpheusDesc) - 4 and hip.OrpheusDesc.max_seqs.offset == C.sizeof(hip.OrpheusDesc) - 8
    assert C.sizeof(hip.OrpheusDesc) == 4 * len(fields)


def test_header_names_the_layout_the_rounding_and_the_range():
    doc = re.search(r"uint32_t\s+kv_type;.*?\*/", _desc_text(), re.S).group(0)
    doc = " ".join(re.sub(r"\n\s*\*(?!/)", "\n", doc).split())         # without the comment's leading asterisks
    for needle in ("[slot][layer][position][kv width]", "one byte per element", "e4m3fn", "nearest-even", "appended", "448", "subnormals below 2^-6",
                   "zero below 2^-10", "arithmetic stays fp32", "widened exactly", "a quarter of the fp32 cache memory", "Fixed at create", "decode",
                   "captured step", "step_batch / generate_batch", "gen_*", "stream_*", "65 .. 256-row forwards", "Dia and Parler contexts have no fp8 cache",
                   "TTS_HIP_F16", "TTS_HIP_KV_F8_E4M3", "TTS_HIP_FLAG_KV_F16", "refused", "size before this field"):
        assert needle in doc, needle


# ---- 2. the rounding reference ----------------------------------------------------------------------------------------------------------
def _torch_e4m3(x):
    """torch's conversion of the values the hardware conversion sees: the kernels clamp to +-448 in plain arithmetic first"""
    import torch
    return torch.from_numpy(np.clip(np.asarray(x, dtype=np.float32), -448.0, 448.0)).to(torch.float8_e4m3fn).to(torch.float32).numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def test_reference_equals_torch_on_normal_draws():
    rng = np.random.default_rng(0xE4A3)
    scales = np.float32([1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0, 300.0])
    x = (rng.standard_normal((len(scales), 1_000_000 // len(scales) + 1), dtype=np.float32) * scales[:, None]).ravel()
    assert x.size >= 1_000_000 and (np.abs(x) > 448).any() and (np.abs(x) < 2.0 ** -10).any()
    assert _same_bits(e4m3_round(x), _torch_e4m3(x))


def test_reference_at_the_edges_of_the_format():
    pts = np.float32([448.0, 464.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 0.0])
    pts = np.concatenate([pts, -pts])
    got = e4m3_round(pts)
    assert _same_bits(got, _torch_e4m3(pts))
    # 464 saturates; 2^-9 is the smallest subnormal; 2^-10 is the tie between 0 and 2^-9 (to even: 0); 3 * 2^-10 the tie between 2^-9 and 2^-8 (to even: 2^-8)
    assert got[:6].tolist() == [448.0, 448.0, 2.0 ** -9, 0.0, 2.0 ** -8, 0.0] and got[6:].tolist() == [-448.0, -448.0, -2.0 ** -9, -0.0, -2.0 ** -8, -0.0]
    assert e4m3_round(np.float32([1e9, -np.inf, 449.0])).tolist() == [448.0, -448.0, 448.0]
    assert np.signbit(got[9]) and np.signbit(got[11])


def test_the_finite_codes_are_the_fixed_points():
    import torch
    codes = e4m3_finite_codes()
    assert codes.size == 254 and np.unique(codes).size == 253          # +0 and -0 compare equal
    raw = np.array([c for c in range(256) if c & 127 != 127], dtype=np.uint8)
    assert _same_bits(codes, torch.from_numpy(raw).view(torch.float8_e4m3fn).to(torch.float32).numpy())
    assert _same_bits(e4m3_round(codes), codes)
    assert np.abs(codes).max() == 448.0 and np.abs(codes[codes != 0]).min() == 2.0 ** -9


# ---- 3. the gfx950 cross-compile --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{mangled kernel name: (VGPRs, AGPRs, scratch bytes per lane, LDS bytes)} from the compiler's remarks"""
    tmp = tmp_path_factory.mktemp("kv_f8_isa")
    cu = tmp / "kv_f8.hip"
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
@pytest.mark.parametrize("stem", ["15attn_gqa_kernelILi128ELb0E", "15attn_gqa_kernelILi128ELb1E", "20attn_gqa_wave_kernelILi128ELi4ELb0E"], ids=["unsplit", "split", "wave"])
def test_f8_readers_fit_in_the_budget_of_their_fp32_counterparts(usage, stem):
    (v32, a32, s32, l32), (v16, a16, s16, l16), (v8, a8, s8, l8) = _one(usage, stem + "fE"), _one(usage, stem + "DF16_E"), _one(usage, stem + "5kv_f8E")
    print(f"{stem}: fp32 {v32} VGPRs + {a32} AGPRs, scratch {s32}, LDS {l32};  fp16 {v16} + {a16}, scratch {s16}, LDS {l16};  e4m3 {v8} + {a8}, scratch {s8}, LDS {l8}")
    assert s8 == 0 and s32 == 0
    assert v8 + a8 <= v32 + a32
    assert v8 + a8 <= 128
    assert l8 <= l32


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_f8_writers_compile_for_gfx950_without_scratch(usage):
    for part in ("23gemv_q4_qkv_rope_kernelILi4ELi0ELi2E5kv_f8E", "23gemv_q4_qkv_rope_kernelILi4ELi2ELi2E5kv_f8E", "20llama_rope_kv_kernelI5kv_f8E"):
        v, a, scratch, _ = _one(usage, part)
        print(f"{part}: {v} VGPRs + {a} AGPRs, scratch {scratch}")
        assert scratch == 0, part
