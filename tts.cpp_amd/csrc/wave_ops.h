// wave_ops.h — vector typedefs, cross-lane reductions (DPP / permlane, no LDS crossbar) and ggml's GELU: shared by every kernel header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef int int2v __attribute__((ext_vector_type(2)));

#define LN_EPS 1e-5f  // model.cpp:414 "parler always uses default eps"

// Cross-lane reductions without the LDS crossbar.  __shfl_xor compiles to ds_bpermute_b32 + s_waitcnt lgkmcnt(0): six dependent LDS round
// trips per wave_sum, which is most of a LayerNorm's time at batch 1 (profiles/r03/b1_chain.txt).  The xor butterfly 32, 16, 8, 4, 2, 1 is
// reproduced bit for bit: v_permlane32_swap / v_permlane16_swap of (v, v) leave lane i's value in one result and lane (i ^ 32) / (i ^ 16)'s in the
// other (fp add and max commute); inside a row of 16 lanes the value has period 8 after the xor-8 step, period 4 after the xor-4 step ..., so
// rotating the row by 8, 4, 2, 1 (DPP row_ror) pairs every lane with the same partner value the xor would (profiles/wave_sum_check.hip).
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_sum(float v) {   // == v += __shfl_xor(v, 8); ... 4; 2; 1 for aligned groups of 16 lanes
    v += dpp_f<0x128>(v); v += dpp_f<0x124>(v); v += dpp_f<0x122>(v); v += dpp_f<0x121>(v);
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_f<0x128>(v)); v = fmaxf(v, dpp_f<0x124>(v)); v = fmaxf(v, dpp_f<0x122>(v)); v = fmaxf(v, dpp_f<0x121>(v));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    v = __builtin_bit_cast(float, (unsigned) a[0]) + __builtin_bit_cast(float, (unsigned) a[1]);
    const unsigned w = __builtin_bit_cast(unsigned, v);
    const auto b = __builtin_amdgcn_permlane16_swap(w, w, false, false);
    v = __builtin_bit_cast(float, (unsigned) b[0]) + __builtin_bit_cast(float, (unsigned) b[1]);
    return row16_sum(v);
}
__device__ __forceinline__ float wave_max(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    v = fmaxf(__builtin_bit_cast(float, (unsigned) a[0]), __builtin_bit_cast(float, (unsigned) a[1]));
    const unsigned w = __builtin_bit_cast(unsigned, v);
    const auto b = __builtin_amdgcn_permlane16_swap(w, w, false, false);
    v = fmaxf(__builtin_bit_cast(float, (unsigned) b[0]), __builtin_bit_cast(float, (unsigned) b[1]));
    return row16_max(v);
}

// max over aligned groups of 32 lanes (a Q8_0 block held one value per lane): the xor-16 step as v_permlane16_swap, the rest inside the rows by DPP.
// A maximum does not depend on the order of the comparisons: the same value as the five-step __shfl_xor butterfly (five ds_bpermute round trips).
__device__ __forceinline__ float lanes32_max(float v) {
    const unsigned w = __builtin_bit_cast(unsigned, v);
    const auto b = __builtin_amdgcn_permlane16_swap(w, w, false, false);
    v = fmaxf(__builtin_bit_cast(float, (unsigned) b[0]), __builtin_bit_cast(float, (unsigned) b[1]));
    return row16_max(v);
}

// One-byte cache element: OCP e4m3fn (1 sign, 4 exponent, 3 mantissa bits, bias 7: largest finite 448, subnormals below 2^-6 in steps of 2^-9, no inf).
// The writers convert with `(KV) y`, as they do for _Float16: clamped to +-448 here (what v_cvt_pk_fp8_f32 does above 448 depends on a mode bit the
// kernels do not own), then rounded to nearest-even by the hardware conversion.  Readers widen exactly (KVRow<kv_f8>, kv_f8_widen4).
// Shared by the Llama decoder's cache (llama_kernels.h) and Parler's (parler_kernels.h: element code KV_E4M3).
struct kv_f8 {
    uint8_t b;
    kv_f8() = default;
    explicit __device__ __forceinline__ kv_f8(float x) {
        const float c = fminf(fmaxf(x, -448.0f), 448.0f);
        b = (uint8_t) __builtin_amdgcn_cvt_pk_fp8_f32(c, c, 0, false);
    }
};
static_assert(sizeof(kv_f8) == 1, "a cache row of kv_f8 is one byte per element");
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // 16 bytes of an e4m3 row: 16 elements, element e in byte e (the 16-byte-lane readers: dia_f8_kernels.h, attn_rows_f8_kernel)
// four consecutive elements of a row as one word (element e in byte e): the same clamp and conversion, two v_cvt_pk_fp8_f32
__device__ __forceinline__ uint32_t kv_f8_pack4(float4v v) {
    float c[4];
#pragma unroll
    for (int e = 0; e < 4; e++) c[e] = fminf(fmaxf(v[e], -448.0f), 448.0f);
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], 0, false);
    return (uint32_t) __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], lo, true);
}
// and back, exactly (every finite e4m3 number is an fp32 number): two v_cvt_pk_f32_fp8, bytes 0-1 and bytes 2-3
__device__ __forceinline__ float4v kv_f8_widen4(uint32_t w) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int) w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int) w, true);
    return (float4v){lo[0], lo[1], hi[0], hi[1]};
}

// ggml_gelu.  mode 1 restates ggml's CPU path, which evaluates GELU through a table indexed by the
// fp16 bits of x and holding fp16 results (upstream ggml_vec_gelu_f32 / GGML_GELU_FP16): a table is
// memoisation, so rounding x to fp16, evaluating in fp32 and rounding the result to fp16 is the
// same function.
__device__ __forceinline__ float gelu_tanh_f32(float x) {
    const float A = 0.044715f, S = 0.79788456080286535587989211986876f;
    return 0.5f * x * (1.0f + tanhf(S * x * (1.0f + A * x * x)));
}
__device__ __forceinline__ float gelu_apply(float x, int mode) {
    if (mode == 0) return gelu_tanh_f32(x);
    if (x <= -10.0f) return 0.0f;
    if (x >= 10.0f) return x;
    const float xr = (float) (_Float16) x;
    return (float) (_Float16) gelu_tanh_f32(xr);
}

