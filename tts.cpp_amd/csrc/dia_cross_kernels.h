// dia_cross_kernels.h — Dia's cross-attention over the sentence's keys only (tune("dia_cross_bounded"), shim_llama.hip: dia_forward; DESIGN.md, "Dia
// cross-attention that reads only the sentence's keys").  A unit of their own (shim_dia_cross.hip), as dia_rows_kernels.h is: the code object of
// shim_llama.hip holds the kernels it always held, and a context that leaves the key at 0 runs device code these have not moved.
//
// The cross cache of a row slot holds K for the n positions of its sentence and zero rows behind them, V for all S positions (build_dia_cross_kv_store),
// and the softmax runs over all S (tests/test_gpu_dia_kv_f16.py pins it).  A zero K row scores exactly 0 for every query, so with P = S - n
//     sum_j e^(s_j - m) V_j = sum_{j < n} e^(s_j - m) V_j + e^(0 - m) Vsum,   sum_j e^(s_j - m) = sum_{j < n} e^(s_j - m) + P e^(0 - m),
//     Vsum = sum_{j = n .. S - 1} V_j,
// and Vsum depends on neither the query nor the step: dia_cross_padsum_kernel writes it once per encoder pass, attn_cross_bounded_kernel reads n K/V rows
// and that one fp32 row instead of S K/V rows.  The same softmax . V in another association: results agree with the whole-context kernel to rounding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "llama_kernels.h"   // KVRow<KV>, QPre, ATTN_PART, the lane reductions

#define PADSUM_STRETCHES 4   // contiguous stretches of pad positions per workgroup, one per wave; part of the sum's order (tests restate it)

// 16 bytes of a cache row per lane: 4 fp32 or 8 fp16 columns (16 e4m3 ones: dia_f8_kernels.h), non-temporal (up to 2 S A L elements per encoder pass, read
// once); at(v, e): column e widened exactly
template <typename KV> struct PadVec;
template <> struct PadVec<float> {
    static constexpr int N = 4;
    typedef float4v vec;
    static __device__ __forceinline__ float at(const vec &v, int e) { return v[e]; }
};
template <> struct PadVec<_Float16> {
    static constexpr int N = 8;
    typedef half8 vec;
    static __device__ __forceinline__ float at(const vec &v, int e) { return (float) v[e]; }
};

// Vsum[layer][row][A] (fp32) = sum over j = n .. S - 1 of the cache's V row j widened exactly (an fp16 cache sums its rounded rows), for the two row slots
// row0, row0 + 1 of one utterance and every layer; klive[row] = n.  grid (ceil(A / (64 lanes x 16 bytes)), 2, L), 256 threads.
// Lanes run across the columns — a wave instruction reads 1 KB of one row — and the four waves of a workgroup own the PADSUM_STRETCHES contiguous
// stretches of ceil(P / 4) positions each: a wave adds its rows in ascending position into one accumulator per column (eight rows requested at a
// time, added in request order), waves 1 .. 3 leave theirs in LDS, wave 0 adds them in stretch order.  Every column's sum is therefore one fixed
// expression of (n, S): the bits depend on neither the timing nor the grid.  n = S leaves zeros.
template <typename KV>
__global__ __launch_bounds__(256) void dia_cross_padsum_kernel(const KV *vcache, int64_t layer_stride, int row0, int S, int A, int n, float *vsum, int RS, uint32_t *klive) {
    constexpr int N = PadVec<KV>::N, NB = 8;
    typedef typename PadVec<KV>::vec vec;
    __shared__ float s_part[PADSUM_STRETCHES - 1][64 * N];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = blockIdx.z, row = row0 + blockIdx.y, col = (blockIdx.x * 64 + lane) * N;
    const bool on = col < A;   // A is a multiple of 128: a lane's columns are all inside or all outside
    const int P = S - n, len = (P + PADSUM_STRETCHES - 1) / PADSUM_STRETCHES;
    const int j0 = min(S, n + wave * len), j1 = min(S, j0 + len);
    const KV *base = vcache + (int64_t) l * layer_stride + (int64_t) row * S * A + (on ? col : 0);
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; e++) acc[e] = 0.0f;
    for (int j = j0; j < j1; j += NB) {
        vec v[NB];
#pragma unroll
        for (int u = 0; u < NB; u++) v[u] = __builtin_nontemporal_load((const vec *) (base + (int64_t) min(j + u, j1 - 1) * A));   // a row beyond the stretch re-reads its last row; not used
#pragma unroll
        for (int u = 0; u < NB; u++)
            if (j + u < j1) {
#pragma unroll
                for (int e = 0; e < N; e++) acc[e] += PadVec<KV>::at(v[u], e);
            }
    }
    if (wave) {
#pragma unroll
        for (int e = 0; e < N; e++) s_part[wave - 1][lane * N + e] = acc[e];
    }
    __syncthreads();
    if (wave == 0 && on) {
        float *dst = vsum + ((int64_t) l * RS + row) * A + col;
#pragma unroll
        for (int e = 0; e < N; e++) {
            float t = acc[e];
#pragma unroll
            for (int s = 0; s < PADSUM_STRETCHES - 1; s++) t += s_part[s][lane * N + e];
            dst[e] = t;
        }
    }
    if (blockIdx.x == 0 && l == 0 && tid == 0) klive[row] = (uint32_t) n;
}

// attn_gqa_wave_kernel's EXT form (llama_kernels.h) with the keys of a row ending at its sentence: the same key -> (slice, 16-lane group, pass) mapping
// (key j: slice (j / 16) % nz, group j % 16, pass j / (16 nz)), the same eight straight-line passes through U = KVRow<KV>::EXT_SLOTS rolling register slots,
// the same slab fold and NEOX rotation of the query under the first rows in flight, non-temporal K / V loads, and partials in attn_gqa_combine_kernel's
// format.  grid (head, row, slice), 256 threads.  What differs:
//   * live = min(klive[row_seq[r]], kend[r]) keys are read and P = kend[r] - live pad keys are not: requests clamp to key live - 1 and consume masks at
//     live.  Slices interleave by 16 keys, so a short sentence keeps all nz slices busy for fewer passes; once a pass starts at or beyond `live` the
//     workgroup leaves the pass loop (a uniform branch: the rows still in flight behind it are repeats of one cached row and are dropped).  A parked row
//     (kend = 1) has P = 0 and reads its one key; a sentence as long as the context has P = 0 and issues the requests of the EXT form.
//   * the pad keys enter once per (head, row), in slice 0, as a fifth partial (m = 0, l = P, o = Vsum[row_seq[r]][h 128 + tid]) behind the four waves' in
//     the workgroup's merge: the same max, rescale and add.  Its 128 floats are requested with q and the limits, ahead of the K / V rows, and parked in
//     LDS while the query is folded: no round trip of their own, no register through the passes.
// Precondition (the host's callers keep it: kend is max_ctx for a live row, 1 for a parked one): kend[r] = n_ctx wherever kend[r] > klive[row_seq[r]] — Vsum
// always runs to the last position of the context, so a row that ended between its sentence and the context's end would take pad rows it does not own.
// klive >= 1 (the encoder pass refuses an empty sentence; the max(1, ..) below only keeps a request in bounds).
// klive is indexed by row slot, so the limits are two dependent scalar loads (row_seq[r], then klive) ahead of the first row request, one more than the
// EXT form's.
//
// attn_cross_bounded_rows_kernel (ROWS; launch_attn_gqa's launch of more than 256 (head, row) pairs, where no keys are split): the finished-row form.  grid
// (head, row), one slice (z = 0, nz = 1: key j is group j % 16, pass j / 16), the same requests, consume, wave merge and five-partial workgroup merge; what differs:
//   * the pass count is ceil(live / 16), a runtime value up to n_ctx / 16, not eight: rounds of U passes, straight-line inside a round so that every slot
//     index is a compile-time constant (the slots stay registers), around them a loop whose carried state is the U slots, the running max / sum / row and the
//     round's first pass.  Pass p's slot is requested again for pass p + U the moment p is consumed, clamped to key live - 1 whatever p + U is (a request
//     behind the sentence re-reads one cached row and is dropped).  The loop runs the whole rounds that have a pass behind them and has one exit; the last
//     round — every pass of it is in flight by then, nothing more is requested — is a straight-line tail with the slice form's uniform exit after each pass.
//     (One loop with that exit inside its rounds compiles to exits that join the round's end before they leave, and the waits at the head of a round then
//     cover every request in flight: vmcnt(0) where 4 (U - 1) may stay outstanding.  As written the waits are vmcnt(4 (U - 1) + 3 ..) throughout.)
//   * the workgroup divides by the total (live >= 1: never 0) and writes out[r][h 128 + tid], fp32, itself: no partial buffer, no combine launch.
// Against attn_gqa_kernel<128, false, KV>, the launch it replaces: K and V of a pass are requested together and consumed by an online softmax — no LDS score
// buffer, no second key pass, three barriers in all — and `live` keys plus one fp32 row are read instead of kend[r].
template <int U, typename KV, bool ROWS>
__device__ __forceinline__ void attn_cross_bounded_body(const float *qkv, int ld, const KV *kcache, const KV *vcache, int NH, float scale, float *dst, int n_ctx,
                                                        const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum,
                                                        const QPre &qp) {
    constexpr int HD = 128;
    static_assert(U >= 1 && U <= 8, "eight passes through U register slots");
    typedef KVRow<KV> Row;
    __shared__ float s_m[4], s_l[4];
    __shared__ __attribute__((aligned(16))) float s_acc[4][HD];
    __shared__ __attribute__((aligned(16))) float s_q[HD];
    __shared__ float s_pad[HD];
    const int h = blockIdx.x, r = blockIdx.y, z = ROWS ? 0 : blockIdx.z, nz = ROWS ? 1 : gridDim.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, sub = lane & 15, gi = wave * 4 + g;
    const int kvH = NH * HD;   // one K/V head per query head
    const int seq = (int) row_seq[r];
    const int lim = max(1, min((int) kend[r], n_ctx));
    const int live = max(1, min((int) klive[seq], lim));
    const int P = lim - live;
    kcache += (int64_t) seq * seq_stride; vcache += (int64_t) seq * seq_stride;
    const char *kp = (const char *) (kcache + h * HD), *vp = (const char *) (vcache + h * HD);
    auto key_of = [&](int p) { return 16 * (nz * p + z) + gi; };
    constexpr uint32_t ESZ = sizeof(KV), HALF = 64 * sizeof(KV);
    typename Row::vec4 ka[U], kb[U], va[U], vb[U];
    auto request_one = [&](int u, int pass) __attribute__((always_inline)) {
        const uint32_t off = ((uint32_t) min(key_of(pass), live - 1) * (uint32_t) kvH + (uint32_t) sub * 4u) * ESZ;
        ka[u] = Row::load_nt(kp + off); kb[u] = Row::load_nt(kp + off + HALF);
        va[u] = Row::load_nt(vp + off); vb[u] = Row::load_nt(vp + off + HALF);
    };
    // the small inputs first (vmcnt retires in issue order): the query's slabs, the rope position, the pad row
    float4 q0, q1;
    float tq[4];   // threads 0-127 hold slabs 0-3 of query element tid, threads 128-255 slabs 4-7 of element tid - 128
    uint32_t rp = 0;
    const float *qe = qkv + (int64_t) r * ld + h * HD + (tid & (HD - 1));
#pragma unroll
    for (int p = 0; p < 4; p++) tq[p] = qe[(int64_t) min((tid >> 7) * 4 + p, qp.n_parts - 1) * qp.part_stride];
    if (qp.rope_pos) rp = qp.rope_pos[r];
    const float pv = vsum[(int64_t) seq * kvH + h * HD + (tid & (HD - 1))];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; u++) request_one(u, u);
    __builtin_amdgcn_sched_barrier(0);
    // attn_q_finish's arithmetic: slabs in slab order (the upper half of the workgroup continues the lower half's sum), then ggml_rope NEOX with the
    // iterated theta (pair i, i + 64: both in this lane)
    if (tid < HD) {
        float x = tq[0];
#pragma unroll
        for (int p = 1; p < 4; p++)
            if (p < qp.n_parts) x += tq[p];
        s_q[tid] = x;
        s_pad[tid] = pv;
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
    q0 = *(const float4 *) (s_q + sub * 4); q1 = *(const float4 *) (s_q + 64 + sub * 4);
    if (qp.rope_pos) {
        float theta = (float) rp;
        for (int j = 0; j < sub * 4; j++) theta *= qp.theta_scale;
        float *a = (float *) &q0, *b = (float *) &q1;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float cs = cosf(theta), sn = sinf(theta);
            const float x0 = a[e], x1 = b[e];
            a[e] = x0 * cs - x1 * sn; b[e] = x0 * sn + x1 * cs;
            theta *= qp.theta_scale;
        }
    }
    float m = -INFINITY, l = 0.0f;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
    auto consume = [&](int u, int pass) __attribute__((always_inline)) {
        if (key_of(pass) < live) {
            // fp32: references to the slot's registers, not copies (attn_gqa_wave_kernel's consume says why)
            decltype(auto) k0 = Row::widen(ka[u]); decltype(auto) k1 = Row::widen(kb[u]); decltype(auto) v0 = Row::widen(va[u]); decltype(auto) v1 = Row::widen(vb[u]);
            float d = (k0.x * q0.x + k0.y * q0.y + k0.z * q0.z + k0.w * q0.w) + (k1.x * q1.x + k1.y * q1.y + k1.z * q1.z + k1.w * q1.w);
            d = row16_sum(d) * scale;
            const float mn = fmaxf(m, d);
            const float f = expf(m - mn);   // 0 on the group's first key (m = -inf)
            const float pr = expf(d - mn);
            l = l * f + pr;
            a0.x = a0.x * f + pr * v0.x; a0.y = a0.y * f + pr * v0.y; a0.z = a0.z * f + pr * v0.z; a0.w = a0.w * f + pr * v0.w;
            a1.x = a1.x * f + pr * v1.x; a1.y = a1.y * f + pr * v1.y; a1.z = a1.z * f + pr * v1.z; a1.w = a1.w * f + pr * v1.w;
            m = mn;
        }
    };
    if constexpr (ROWS) {
        // ceil(live / 16) passes in rounds of U: slot u of a round holds pass p0 + u and is requested again for pass p0 + u + U the moment it has been consumed
        int p0 = 0;
        for (; 16 * (p0 + U) < live; p0 += U) {   // a whole round with at least one pass behind it
#pragma unroll
            for (int u = 0; u < U; u++) {
                consume(u, p0 + u);
                __builtin_amdgcn_sched_barrier(0);   // the slot's registers are free only now
                request_one(u, p0 + u + U);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {   // the last round: its passes are all requested, 16 (p0 + U) >= live
            consume(u, p0 + u);
            __builtin_amdgcn_sched_barrier(0);
            if (16 * (p0 + u + 1) >= live) break;   // workgroup-uniform: no key of the next pass is below `live`
        }
    } else {
        // eight passes (the host checks: at most 16 nz 8 keys), U register slots: a slot is requested again for pass p + U the moment pass p has been consumed
#pragma unroll
        for (int p = 0; p < 8; p++) {
            consume(p % U, p);
            __builtin_amdgcn_sched_barrier(0);   // the slot's registers are free only now
            if (p + U < 8) request_one(p % U, p + U);
            __builtin_amdgcn_sched_barrier(0);
            if (16 * nz * (p + 1) >= live) break;   // workgroup-uniform: no key of pass p + 1 or later, in any slice, is below `live`
        }
    }
    // the wave's four groups (lanes sub, 16 + sub, 32 + sub, 48 + sub hold the same dims): common max, rescale, add
    auto x16 = [](float v) { const unsigned w = __builtin_bit_cast(unsigned, v); const auto b = __builtin_amdgcn_permlane16_swap(w, w, false, false);
                             return make_float2(__builtin_bit_cast(float, (unsigned) b[0]), __builtin_bit_cast(float, (unsigned) b[1])); };
    auto x32 = [](float v) { const unsigned w = __builtin_bit_cast(unsigned, v); const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
                             return make_float2(__builtin_bit_cast(float, (unsigned) b[0]), __builtin_bit_cast(float, (unsigned) b[1])); };
    float mw;
    { float2 t = x16(m); mw = fmaxf(t.x, t.y); t = x32(mw); mw = fmaxf(t.x, t.y); }
    const float fg = m == -INFINITY ? 0.0f : expf(m - mw);
    float vals[9] = {l * fg, a0.x * fg, a0.y * fg, a0.z * fg, a0.w * fg, a1.x * fg, a1.y * fg, a1.z * fg, a1.w * fg};
#pragma unroll
    for (int i = 0; i < 9; i++) {
        float2 t = x16(vals[i]); float v = t.x + t.y;
        t = x32(v); vals[i] = t.x + t.y;
    }
    if (g == 0) {
        *(float4 *) (&s_acc[wave][sub * 4]) = make_float4(vals[1], vals[2], vals[3], vals[4]);
        *(float4 *) (&s_acc[wave][64 + sub * 4]) = make_float4(vals[5], vals[6], vals[7], vals[8]);
        if (sub == 0) { s_m[wave] = mw; s_l[wave] = vals[0]; }
    }
    __syncthreads();
    if (tid < HD) {
        const bool pad = z == 0 && P > 0;   // the pad keys' partial: max 0, sum P, out Vsum — once per (head, row), behind the waves'
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
            dst[((int64_t) r * NH + h) * HD + tid] = o / L;   // (a parked row: o is its one V row, L is 1)
        } else {
            float *pz = dst + (((int64_t) r * NH + h) * nz + z) * ATTN_PART;
            pz[2 + tid] = o;
            if (tid == 0) { pz[0] = M; pz[1] = L; }
        }
    }
}

// grid (head, row, slice); `part`: the slices' partials for attn_gqa_combine_kernel
template <int U, typename KV>
__global__ __launch_bounds__(256) void attn_cross_bounded_kernel(const float *qkv, int ld, const KV *kcache, const KV *vcache, int NH, float scale, float *part, int n_ctx,
                                                                const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum,
                                                                QPre qp) {
    attn_cross_bounded_body<U, KV, false>(qkv, ld, kcache, vcache, NH, scale, part, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
}

// grid (head, row); `out`: the attended rows [rows][NH 128], fp32
template <int U, typename KV>
__global__ __launch_bounds__(256) void attn_cross_bounded_rows_kernel(const float *qkv, int ld, const KV *kcache, const KV *vcache, int NH, float scale, float *out, int n_ctx,
                                                                     const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive,
                                                                     const float *vsum, QPre qp) {
    attn_cross_bounded_body<U, KV, true>(qkv, ld, kcache, vcache, NH, scale, out, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
}
