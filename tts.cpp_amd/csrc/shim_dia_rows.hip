// shim_dia_rows.hip — the two row producers of Dia's tiled route as a translation unit of their own (dia_rows_kernels.h says why).
#include "shim_dia_rows.h"

#include "dia_rows_kernels.h"

bool dia_rows_rms_fold_f16(hipStream_t stream, float *x, int H, const float *w, _Float16 *y, int R, float eps, const float *parts, int n_parts, int64_t slab_stride) {
    hipLaunchKernelGGL(rms_fold_rows_f16_kernel, dim3(R), dim3(256), 0, stream, x, H, w, y, R, eps, parts, n_parts, slab_stride);
    return hipGetLastError() == hipSuccess;
}

bool dia_rows_silu_mul_f16(hipStream_t stream, const float *gu, int F, int R, _Float16 *g) {
    hipLaunchKernelGGL(silu_mul_f16_kernel, dim3((F + 2047) / 2048, R), dim3(256), 0, stream, gu, F, R, g);
    return hipGetLastError() == hipSuccess;
}
