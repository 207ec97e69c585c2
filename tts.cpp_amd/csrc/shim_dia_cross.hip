// shim_dia_cross.hip — the pad-sum writer and the bounded cross-attention reader of a Dia context as a translation unit of their own
// (dia_cross_kernels.h says why).  Built without packed fp32 arithmetic (build.py: -target-feature -packed-fp32-ops) for the registers: the reader compiles
// to 101 (fp32 cache) / 85 (fp16) VGPRs, with v_pk_* operand pairs to 110 / 94 (the EXT form: 112 / 98); its finished-row form (attn_cross_bounded_rows_kernel) to 100 / 84.  The sums' order does not depend on it.  The `static` kernels of the headers it includes ride along unused, as in every unit.
#include "shim_dia_cross.h"

#include "dia_cross_kernels.h"

template <typename KV>
static void padsum(hipStream_t stream, const void *cv, int L, int RS, int S, int A, int slot, int n, float *vsum, uint32_t *klive) {
    const int cols = 64 * PadVec<KV>::N;
    hipLaunchKernelGGL(dia_cross_padsum_kernel<KV>, dim3((A + cols - 1) / cols, 2, L), dim3(256), 0, stream, (const KV *) cv, (int64_t) RS * S * A, 2 * slot, S, A, n, vsum, RS, klive);
}

bool dia_cross_padsum(hipStream_t stream, int kv_esz, const void *cv, int L, int RS, int S, int A, int slot, int n, float *vsum, uint32_t *klive) {
    if (kv_esz == 2) padsum<_Float16>(stream, cv, L, RS, S, A, slot, n, vsum, klive);
    else padsum<float>(stream, cv, L, RS, S, A, slot, n, vsum, klive);
    return hipGetLastError() == hipSuccess;
}

// nz >= 1: the slice form, partials into dst; nz = 0: the finished-row form, rows into dst
template <typename KV>
static void bounded(hipStream_t stream, const float *q, int ld, const void *kc, const void *vc, int NH, int rows, int nz, float scale, float *dst, int n_ctx, const uint32_t *kend,
                    const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, const QPre &qp) {
    constexpr int U = KVRow<KV>::EXT_SLOTS;
    if (nz)
        hipLaunchKernelGGL((attn_cross_bounded_kernel<U, KV>), dim3(NH, rows, nz), dim3(256), 0, stream, q, ld, (const KV *) kc, (const KV *) vc, NH, scale, dst, n_ctx, kend, row_seq,
                           seq_stride, klive, vsum, qp);
    else
        hipLaunchKernelGGL((attn_cross_bounded_rows_kernel<U, KV>), dim3(NH, rows), dim3(256), 0, stream, q, ld, (const KV *) kc, (const KV *) vc, NH, scale, dst, n_ctx, kend, row_seq,
                           seq_stride, klive, vsum, qp);
}

static bool bounded_any(hipStream_t stream, int kv_esz, const float *q, int ld, const void *kc, const void *vc, int NH, int rows, int nz, float scale, float *dst, int n_ctx,
                        const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, int n_parts, int64_t part_stride,
                        const uint32_t *rope_pos, float theta_scale) {
    QPre qp;
    qp.n_parts = n_parts; qp.part_stride = part_stride; qp.rope_pos = rope_pos; qp.theta_scale = theta_scale;
    if (kv_esz == 2) bounded<_Float16>(stream, q, ld, kc, vc, NH, rows, nz, scale, dst, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
    else bounded<float>(stream, q, ld, kc, vc, NH, rows, nz, scale, dst, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
    return hipGetLastError() == hipSuccess;
}

bool dia_cross_bounded(hipStream_t stream, int kv_esz, const float *q, int ld, const void *kc, const void *vc, int NH, int rows, int nz, float scale, float *part, int n_ctx,
                       const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, int n_parts, int64_t part_stride,
                       const uint32_t *rope_pos, float theta_scale) {
    return bounded_any(stream, kv_esz, q, ld, kc, vc, NH, rows, nz, scale, part, n_ctx, kend, row_seq, seq_stride, klive, vsum, n_parts, part_stride, rope_pos, theta_scale);
}

bool dia_cross_bounded_rows(hipStream_t stream, int kv_esz, const float *q, int ld, const void *kc, const void *vc, int NH, int rows, float scale, float *out, int n_ctx,
                            const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, int n_parts, int64_t part_stride,
                            const uint32_t *rope_pos, float theta_scale) {
    return bounded_any(stream, kv_esz, q, ld, kc, vc, NH, rows, 0, scale, out, n_ctx, kend, row_seq, seq_stride, klive, vsum, n_parts, part_stride, rope_pos, theta_scale);
}
