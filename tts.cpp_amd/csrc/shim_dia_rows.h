// shim_dia_rows.h — launchers of shim_dia_rows.hip (the kernels of dia_rows_kernels.h), called by dia_forward_tiled.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// rms norm of R rows of x (H <= 2048) with n_parts pending slabs folded in first, stored as fp16 rows in y; false: the launch failed
bool dia_rows_rms_fold_f16(hipStream_t stream, float *x, int H, const float *w, _Float16 *y, int R, float eps, const float *parts, int n_parts, int64_t slab_stride);
// gu [R][2F] fp32 -> g [R][F] fp16 = silu(gate) * up (F % 8 == 0)
bool dia_rows_silu_mul_f16(hipStream_t stream, const float *gu, int F, int R, _Float16 *g);
