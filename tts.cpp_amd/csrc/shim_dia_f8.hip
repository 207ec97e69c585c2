// shim_dia_f8.hip — the e4m3 cross-attention reader and pad-sum writer of a Dia context as a translation unit of their own (dia_f8_kernels.h says why).
// Built without packed fp32 arithmetic, as shim_dia_cross.hip is (build.py: -target-feature -packed-fp32-ops), for the registers; the sums' order does not
// depend on it.  The `static` kernels of the headers it includes ride along unused, as in every unit.
#include "shim_dia_f8.h"

#include "dia_f8_kernels.h"

bool dia_f8_padsum(hipStream_t stream, const void *cv, int L, int RS, int S, int A, int slot, int n, float *vsum, uint32_t *klive) {
    const int cols = 64 * PadVec<kv_f8>::N;
    hipLaunchKernelGGL(dia_cross_padsum_kernel<kv_f8>, dim3((A + cols - 1) / cols, 2, L), dim3(256), 0, stream, (const kv_f8 *) cv, (int64_t) RS * S * A, 2 * slot, S, A, n, vsum, RS, klive);
    return hipGetLastError() == hipSuccess;
}

template <bool BOUNDED>
static void cross(hipStream_t stream, const float *q, int ld, const kv_f8 *kc, const kv_f8 *vc, int NH, int rows, int nz, float scale, float *dst, int n_ctx, const uint32_t *kend,
                  const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, const QPre &qp) {
    if (nz)
        hipLaunchKernelGGL(attn_cross_f8_kernel<BOUNDED>, dim3(NH, rows, nz), dim3(256), 0, stream, q, ld, kc, vc, NH, scale, dst, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
    else
        hipLaunchKernelGGL(attn_cross_f8_rows_kernel<BOUNDED>, dim3(NH, rows), dim3(256), 0, stream, q, ld, kc, vc, NH, scale, dst, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
}

bool dia_f8_cross(hipStream_t stream, const float *q, int ld, const void *kc, const void *vc, int NH, int rows, int nz, float scale, float *dst, int n_ctx, const uint32_t *kend,
                  const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, int n_parts, int64_t part_stride, const uint32_t *rope_pos,
                  float theta_scale) {
    QPre qp;
    qp.n_parts = n_parts; qp.part_stride = part_stride; qp.rope_pos = rope_pos; qp.theta_scale = theta_scale;
    if (nz && n_ctx > 32 * nz * 4) return false;   // the slice form holds four passes
    if (vsum && klive) cross<true>(stream, q, ld, (const kv_f8 *) kc, (const kv_f8 *) vc, NH, rows, nz, scale, dst, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
    else cross<false>(stream, q, ld, (const kv_f8 *) kc, (const kv_f8 *) vc, NH, rows, nz, scale, dst, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
    return hipGetLastError() == hipSuccess;
}
