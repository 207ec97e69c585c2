// dia_rows_kernels.h — the row producers of Dia's tiled route (decoder steps of more than 16 rows on gemm_tile_kernel, which reads fp16 rows; shim_llama.hip:
// dia_forward_tiled).  They live in a unit of their own (shim_dia_rows.hip) so that the code object of shim_llama.hip holds the kernels it always held: a
// context of at most 64 slots, which never launches these, runs device code that adding them has not moved.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_ops.h"

// Each writes the fp16 rows its GEMM reads and nothing else: no fp32 row plus a conversion pass.  The stored value is the round-to-nearest-even of the
// fp32 value rms_fold_rows_kernel / silu_mul_kernel hand to their GEMM (the rounding ggml_mul_mat applies to the activations of an F16 matrix).

// rms_fold_rows_kernel for an fp16 consumer: one workgroup (4 waves) per row, the row (H <= 2048, the host checks) in registers, element tid + k * 256 in
// v[k].  The pending K-slice slabs (parts, n_parts <= 8, slab_stride floats apart) are folded into x in slab order, four per round trip (rms_fold_rows_kernel
// takes all eight in one: 32 more live values; here eight slabs are two dependent trips, up to four slabs one); the normalised row leaves as fp16 only.  Loads are straight-line with clamped indices (a chunk beyond the row re-reads the row's last element, a slab beyond
// n_parts the last slab; neither is used); only arithmetic and stores sit under `i < H`.  The sum of squares, its reduction and the scale are those of
// rms_fold_rows_kernel, statement for statement.
static __global__ __launch_bounds__(256) void rms_fold_rows_f16_kernel(float *x, int H, const float *w, _Float16 *y, int R, float eps, const float *parts, int n_parts,
                                                                       int64_t slab_stride) {
    constexpr int NK = 8, PQ = 4;   // values of the row per thread; slabs per round trip: 32 values in flight beside the row and its weight
    __shared__ float red[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r >= R) return;
    float *xr = x + (int64_t) r * H;
    float v[NK], wv[NK];
    unsigned at[NK];   // clamped column of v[k]: every load is a uniform base plus this 32-bit offset
#pragma unroll
    for (int k = 0; k < NK; k++) {
        at[k] = (unsigned) min(tid + k * 256, H - 1);
        v[k] = xr[at[k]]; wv[k] = w[at[k]];
    }
    if (parts) {
        for (int p = 0; p < n_parts; p += PQ) {
            float t[PQ][NK];
#pragma unroll
            for (int q = 0; q < PQ; q++) {
                const float *slab = parts + min(p + q, n_parts - 1) * slab_stride + (int64_t) r * H;
#pragma unroll
                for (int k = 0; k < NK; k++) t[q][k] = slab[at[k]];
            }
#pragma unroll
            for (int q = 0; q < PQ; q++)
#pragma unroll
                for (int k = 0; k < NK; k++)
                    if (p + q < n_parts && tid + k * 256 < H) v[k] += t[q][k];
        }
#pragma unroll
        for (int k = 0; k < NK; k++) {
            const int i = tid + k * 256;
            if (i < H) xr[i] = v[k];
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < NK; k++)
        if (tid + k * 256 < H) s += v[k] * v[k];
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    const float scale = 1.0f / sqrtf(s / (float) H + eps);
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int i = tid + k * 256;
        if (i < H) y[(int64_t) r * H + i] = (_Float16) (v[k] * scale * wv[k]);
    }
}

// gu [R][2F] fp32 (gate | up, the plain output of the gate|up tile: no slabs) -> g [R][F] fp16 = silu(gate) * up, silu_mul_kernel's expression.
// grid (ceil(F / 2048), R); a lane holds 8 consecutive values: four 16-byte loads, one 16-byte store.  F % 8 == 0 (the host checks).
static __global__ __launch_bounds__(256) void silu_mul_f16_kernel(const float *gu, int F, int R, _Float16 *g) {
    const int r = blockIdx.y, c = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (r >= R || c >= F) return;
    const float *gr = gu + (int64_t) r * 2 * F + c;
    const float4 x0 = *(const float4 *) gr, x1 = *(const float4 *) (gr + 4), u0 = *(const float4 *) (gr + F), u1 = *(const float4 *) (gr + F + 4);
    const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w}, u[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    h8 h;
#pragma unroll
    for (int e = 0; e < 8; e++) h[e] = (_Float16) ((x[e] / (1.0f + expf(-x[e]))) * u[e]);
    *(h8 *) (g + (int64_t) r * F + c) = h;
}
