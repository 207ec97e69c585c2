// shim_dia_cross.hip — the pad-sum writer and the bounded cross-attention reader of a Dia context as a translation unit of their own
// (dia_cross_kernels.h says why).  Built without packed fp32 arithmetic (build.py: -target-feature -packed-fp32-ops) for the registers: the reader compiles
// to 101 (fp32 cache) / 85 (fp16) VGPRs, with v_pk_* operand pairs to 110 / 94 (the EXT form: 112 / 98).  The sums' order does not depend on it.  The `static` kernels of the headers it includes ride along unused, as in every unit.
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

bool dia_cross_bounded(hipStream_t stream, int kv_esz, const float *q, int ld, const void *kc, const void *vc, int NH, int rows, int nz, float scale, float *part, int n_ctx,
                       const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, int n_parts, int64_t part_stride,
                       const uint32_t *rope_pos, float theta_scale) {
    QPre qp;
    qp.n_parts = n_parts; qp.part_stride = part_stride; qp.rope_pos = rope_pos; qp.theta_scale = theta_scale;
    const dim3 grid(NH, rows, nz);
    if (kv_esz == 2)
        hipLaunchKernelGGL((attn_cross_bounded_kernel<KVRow<_Float16>::EXT_SLOTS, _Float16>), grid, dim3(256), 0, stream, q, ld, (const _Float16 *) kc, (const _Float16 *) vc, NH, scale,
                           part, n_ctx, kend, row_seq, seq_stride, klive, vsum, qp);
    else
        hipLaunchKernelGGL((attn_cross_bounded_kernel<KVRow<float>::EXT_SLOTS, float>), grid, dim3(256), 0, stream, q, ld, (const float *) kc, (const float *) vc, NH, scale, part, n_ctx,
                           kend, row_seq, seq_stride, klive, vsum, qp);
    return hipGetLastError() == hipSuccess;
}
