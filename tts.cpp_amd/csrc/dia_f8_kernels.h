// dia_f8_kernels.h — Dia's cross-attention over a one-byte e4m3 cache (kv_f8, wave_ops.h; tts_hip_tune "kv_f8" on a Dia context), and the
// pad-sum's column vector over it.  A unit of their own (shim_dia_f8.hip), as dia_cross_kernels.h is: the code objects of the other units hold the kernels
// they always held.
//
// Why not attn_gqa_wave_kernel's EXT mapping over kv_f8: there a lane owns dims 4 sub .. + 3 and 64 + 4 sub .. + 3 of a key, which over e4m3 is four 4-byte
// loads per key and lane — 32 load instructions per lane for a 128-key slice, a wave instruction moving 256 bytes.  A head row of one key in e4m3 is 128 bytes,
// exactly eight 16-byte pieces, so here
//   * eight lanes share a key: lane sub8 = lane & 7 holds dims 16 sub8 .. + 15, K is one 16-byte non-temporal load and V another; a wave instruction covers
//     8 keys (1 KB), a workgroup of 256 threads 32 keys per pass: 8 load instructions per lane for a 128-key slice;
//   * key j: slice (j / 32) % nz, group j % 32 (group = wave * 8 + (lane >> 3)), pass j / (32 nz).  The host launches the slice form only where four
//     passes cover the context (max_ctx <= 32 nz 4: 1024 keys at nz = 8), and all four are requested before anything else, beside the query's slabs and the
//     limits: 4 x (4 + 4) = 32 registers in flight, no rolling slot, no request behind a consume;
//   * a piece is widened by v_cvt_pk_f32_fp8 (exact) where it is consumed; the score is a 16-term dot summed over the 8 lanes (DPP: xor 1, xor 2, then the
//     mirror of the 8 lanes, which pairs the two quads); online softmax per group in fp32, 16 accumulators per lane;
//   * the wave's eight groups (lanes sub8 + 8 g hold the same dims) merge by xor 8 (DPP), 16 and 32 (permlane swaps) under one common max, the four waves
//     through LDS with one barrier; partials in attn_gqa_combine_kernel's format, so the combine and the PRO_ATTN8 fold follow unchanged;
//   * the query: slabs folded through LDS as attn_cross_bounded_body does, then attn_q_finish's NEOX rotation IN LDS (pair i, i + 64 sits in lanes sub8 and
//     sub8 ^ 4 of this mapping: threads 0 .. 63 rotate the pair in place) before the lanes pick up their 16 values.
// Limits: lim = clamp(kend[r]); BOUNDED: live = min(klive[row_seq[r]], lim) and the lim - live pad keys enter once, in slice 0, as a fifth partial
// (m = 0, l = lim - live, o = Vsum), exactly as in attn_cross_bounded_body (its precondition holds here too); otherwise live = lim.  Requests clamp to key
// live - 1, consume masks at live, a workgroup leaves the pass loop at the first pass that starts at or beyond live; a parked row (kend = 1) reads one key.
// ROWS (a launch that splits no keys): grid (head, row), nz = 1, ceil(live / 32) passes in rounds of four, shaped as attn_cross_bounded_rows_kernel's loop
// is (straight-line rounds, one exit, a straight-line tail); the workgroup divides by the total and writes `out` itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dia_cross_kernels.h"   // PadVec, dia_cross_padsum_kernel; llama_kernels.h: QPre, ATTN_PART

// the pad-sum's 16 bytes per lane over e4m3: 16 columns in one load, widened exactly; dia_cross_padsum_kernel<kv_f8> keeps the stretches, the request order
// and the sum order of the other two types (A is a multiple of 128, so of 16)
template <> struct PadVec<kv_f8> {
    static constexpr int N = 16;
    typedef u32x4 vec;
    static __device__ __forceinline__ float at(const vec &v, int e) {   // e is a constant where the kernel's loops are unrolled
        const auto p = (e & 2) ? __builtin_amdgcn_cvt_pk_f32_fp8((int) v[e >> 2], true) : __builtin_amdgcn_cvt_pk_f32_fp8((int) v[e >> 2], false);
        return p[e & 1];
    }
};

// sum over aligned groups of 8 lanes, the same bits in all eight: xor 1 and xor 2 inside the quads (quad_perm), then the mirror of the 8 lanes, which hands
// every lane the other quad's sum (fp add commutes)
__device__ __forceinline__ float lanes8_sum(float v) {
    v += dpp_f<0xB1>(v); v += dpp_f<0x4E>(v); v += dpp_f<0x141>(v);
    return v;
}

template <bool ROWS, bool BOUNDED>
__device__ __forceinline__ void attn_cross_f8_body(const float *qkv, int ld, const kv_f8 *kcache, const kv_f8 *vcache, int NH, float scale, float *dst, int n_ctx,
                                                   const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, const QPre &qp) {
    constexpr int HD = 128, NP = 4;   // four passes in flight
    __shared__ float s_m[4], s_l[4];
    __shared__ __attribute__((aligned(16))) float s_acc[4][HD];
    __shared__ __attribute__((aligned(16))) float s_q[HD];
    __shared__ float s_pad[HD];
    const int h = blockIdx.x, r = blockIdx.y, z = ROWS ? 0 : blockIdx.z, nz = ROWS ? 1 : gridDim.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 3, sub8 = lane & 7, gi = wave * 8 + g;
    const int kvH = NH * HD;   // one K/V head per query head; bytes per key row of the cache
    const int seq = (int) row_seq[r];
    const int lim = max(1, min((int) kend[r], n_ctx));
    int live = lim;
    if constexpr (BOUNDED) live = max(1, min((int) klive[seq], lim));
    const int P = lim - live;
    const char *kp = (const char *) (kcache + (int64_t) seq * seq_stride + h * HD) + sub8 * 16;
    const char *vp = (const char *) (vcache + (int64_t) seq * seq_stride + h * HD) + sub8 * 16;
    auto key_of = [&](int p) { return 32 * (nz * p + z) + gi; };
    u32x4 kr[NP], vr[NP];
    auto request_one = [&](int u, int pass) __attribute__((always_inline)) {
        const uint32_t off = (uint32_t) min(key_of(pass), live - 1) * (uint32_t) kvH;   // the host checks that a sequence's rows fit 32-bit byte offsets
        kr[u] = __builtin_nontemporal_load((const u32x4 *) (kp + off));
        vr[u] = __builtin_nontemporal_load((const u32x4 *) (vp + off));
    };
    // the small inputs first (vmcnt retires in issue order): the query's slabs, the rope position, the pad row
    float tq[4];   // threads 0-127 hold slabs 0-3 of query element tid, threads 128-255 slabs 4-7 of element tid - 128
    uint32_t rp = 0;
    const float *qe = qkv + (int64_t) r * ld + h * HD + (tid & (HD - 1));
#pragma unroll
    for (int p = 0; p < 4; p++) tq[p] = qe[(int64_t) min((tid >> 7) * 4 + p, qp.n_parts - 1) * qp.part_stride];
    if (qp.rope_pos) rp = qp.rope_pos[r];
    float pv = 0.0f;
    if constexpr (BOUNDED) pv = vsum[(int64_t) seq * kvH + h * HD + (tid & (HD - 1))];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < NP; u++) request_one(u, u);
    __builtin_amdgcn_sched_barrier(0);
    // attn_q_finish's arithmetic: slabs in slab order (the upper half of the workgroup continues the lower half's sum), then ggml_rope NEOX with the iterated
    // theta on the pair (i, i + 64), in place in LDS
    if (tid < HD) {
        float x = tq[0];
#pragma unroll
        for (int p = 1; p < 4; p++)
            if (p < qp.n_parts) x += tq[p];
        s_q[tid] = x;
        if constexpr (BOUNDED) s_pad[tid] = pv;
    }
    __syncthreads();
    if (tid >= HD) {
        float x = s_q[tid - HD];
#pragma unroll
        for (int p = 0; p < 4; p++)
            if (4 + p < qp.n_parts) x += tq[p];   // (the host sends at most 8 slabs here)
        s_q[tid - HD] = x;
    }
    __syncthreads();
    if (qp.rope_pos && tid < HD / 2) {   // only this thread touches elements tid and tid + 64 between the two barriers
        float theta = (float) rp;
        for (int j = 0; j < tid; j++) theta *= qp.theta_scale;
        const float cs = cosf(theta), sn = sinf(theta);
        const float x0 = s_q[tid], x1 = s_q[tid + HD / 2];
        s_q[tid] = x0 * cs - x1 * sn; s_q[tid + HD / 2] = x0 * sn + x1 * cs;
    }
    __syncthreads();
    float q[16];
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const float4 t = *(const float4 *) (s_q + sub8 * 16 + w * 4);
        q[4 * w] = t.x; q[4 * w + 1] = t.y; q[4 * w + 2] = t.z; q[4 * w + 3] = t.w;
    }
    float m = -INFINITY, l = 0.0f, acc[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;
    auto consume = [&](int u, int pass) __attribute__((always_inline)) {
        if (key_of(pass) < live) {
            float dw[4];
#pragma unroll
            for (int w = 0; w < 4; w++) {   // a word's four elements: bytes 0-1, bytes 2-3
                const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int) kr[u][w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int) kr[u][w], true);
                dw[w] = lo[0] * q[4 * w] + lo[1] * q[4 * w + 1] + hi[0] * q[4 * w + 2] + hi[1] * q[4 * w + 3];
            }
            const float d = lanes8_sum((dw[0] + dw[1]) + (dw[2] + dw[3])) * scale;
            const float mn = fmaxf(m, d);
            const float f = expf(m - mn);   // 0 on the group's first key (m = -inf)
            const float pr = expf(d - mn);
            l = l * f + pr;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int) vr[u][w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int) vr[u][w], true);
                acc[4 * w] = acc[4 * w] * f + pr * lo[0]; acc[4 * w + 1] = acc[4 * w + 1] * f + pr * lo[1];
                acc[4 * w + 2] = acc[4 * w + 2] * f + pr * hi[0]; acc[4 * w + 3] = acc[4 * w + 3] * f + pr * hi[1];
            }
            m = mn;
        }
    };
    if constexpr (ROWS) {
        // ceil(live / 32) passes in rounds of NP: slot u of a round holds pass p0 + u and is requested again for pass p0 + u + NP the moment it has been consumed
        int p0 = 0;
        for (; 32 * (p0 + NP) < live; p0 += NP) {   // a whole round with at least one pass behind it
#pragma unroll
            for (int u = 0; u < NP; u++) {
                consume(u, p0 + u);
                __builtin_amdgcn_sched_barrier(0);   // the slot's registers are free only now
                request_one(u, p0 + u + NP);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int u = 0; u < NP; u++) {   // the last round: its passes are all requested, 32 (p0 + NP) >= live
            consume(u, p0 + u);
            __builtin_amdgcn_sched_barrier(0);
            if (32 * (p0 + u + 1) >= live) break;   // workgroup-uniform: no key of the next pass is below `live`
        }
    } else {
#pragma unroll
        for (int p = 0; p < NP; p++) {   // the host checks: at most 32 nz NP keys
            consume(p, p);
            __builtin_amdgcn_sched_barrier(0);
            if (32 * nz * (p + 1) >= live) break;   // workgroup-uniform: no key of pass p + 1 or later, in any slice, is below `live`
        }
    }
    // the wave's eight groups (lanes sub8 + 8 g hold the same dims): common max, rescale, add
    auto x16 = [](float v) { const unsigned w = __builtin_bit_cast(unsigned, v); const auto b = __builtin_amdgcn_permlane16_swap(w, w, false, false);
                             return make_float2(__builtin_bit_cast(float, (unsigned) b[0]), __builtin_bit_cast(float, (unsigned) b[1])); };
    auto x32 = [](float v) { const unsigned w = __builtin_bit_cast(unsigned, v); const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
                             return make_float2(__builtin_bit_cast(float, (unsigned) b[0]), __builtin_bit_cast(float, (unsigned) b[1])); };
    float mw = fmaxf(m, dpp_f<0x128>(m));
    { float2 t = x16(mw); mw = fmaxf(t.x, t.y); t = x32(mw); mw = fmaxf(t.x, t.y); }
    const float fg = m == -INFINITY ? 0.0f : expf(m - mw);
    auto groups_sum = [&](float v) __attribute__((always_inline)) {
        v += dpp_f<0x128>(v);
        float2 t = x16(v); v = t.x + t.y;
        t = x32(v); return t.x + t.y;
    };
    l = groups_sum(l * fg);
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = groups_sum(acc[e] * fg);
    if (g == 0) {
#pragma unroll
        for (int w = 0; w < 4; w++) *(float4 *) (&s_acc[wave][sub8 * 16 + w * 4]) = make_float4(acc[4 * w], acc[4 * w + 1], acc[4 * w + 2], acc[4 * w + 3]);
        if (sub8 == 0) { s_m[wave] = mw; s_l[wave] = l; }
    }
    __syncthreads();
    if (tid < HD) {
        const bool pad = BOUNDED && z == 0 && P > 0;   // the pad keys' partial: max 0, sum P, out Vsum — once per (head, row), behind the waves'
        float M = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
        if (pad) M = fmaxf(M, 0.0f);
        float o = 0.0f, L = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const float f = s_m[w] == -INFINITY ? 0.0f : expf(s_m[w] - M);
            o += f * s_acc[w][tid];
            L += f * s_l[w];
        }
        if (pad) {
            const float f = expf(0.0f - M);
            o += f * s_pad[tid];
            L += f * (float) P;
        }
        if constexpr (ROWS) {
            dst[((int64_t) r * NH + h) * HD + tid] = o / L;   // live >= 1: never 0 (a parked row: o is its one V row, L is 1)
        } else {
            float *pz = dst + (((int64_t) r * NH + h) * nz + z) * ATTN_PART;
            pz[2 + tid] = o;
            if (tid == 0) { pz[0] = M; pz[1] = L; }
        }
    }
}

// grid (head, row, slice); `part`: the slices' partials for attn_gqa_combine_kernel.  klive / vsum are read only with BOUNDED
template <bool BOUNDED>
__global__ __launch_bounds__(256) void attn_cross_f8_kernel(const float *qkv, int ld, const kv_f8 *kcache, const kv_f8 *vcache, int NH, float scale, float *part, int n_ctx,
                                                           const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, QPre qp) {
    attn_cross_f8_body<false, BOUNDED>(qkv, ld, kcache, vcache, NH, scale, part, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
}

// grid (head, row); `out`: the attended rows [rows][NH 128], fp32
template <bool BOUNDED>
__global__ __launch_bounds__(256) void attn_cross_f8_rows_kernel(const float *qkv, int ld, const kv_f8 *kcache, const kv_f8 *vcache, int NH, float scale, float *out, int n_ctx,
                                                                const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, QPre qp) {
    attn_cross_f8_body<true, BOUNDED>(qkv, ld, kcache, vcache, NH, scale, out, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
}
