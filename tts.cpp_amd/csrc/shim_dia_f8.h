// shim_dia_f8.h — launchers of shim_dia_f8.hip (the kernels of dia_f8_kernels.h over a one-byte e4m3 cache), called by dia_encode_into and launch_attn_gqa.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// dia_cross_padsum (shim_dia_cross.h) over e4m3 V rows: dia_cross_padsum_kernel<kv_f8>; false: the launch failed
bool dia_f8_padsum(hipStream_t stream, const void *cv, int L, int RS, int S, int A, int slot, int n, float *vsum, uint32_t *klive);
// Dia's cross-attention over an e4m3 cache, 16 bytes per lane and key (attn_cross_f8_kernel / attn_cross_f8_rows_kernel).  nz >= 1: grid (NH, rows, nz), at
// most 32 nz 4 keys (the caller checks), partials into dst for attn_gqa_combine_kernel; nz = 0: grid (NH, rows), any number of keys up to n_ctx, the attended
// rows into dst [rows][NH 128].  vsum / klive of this layer's row slots: the bounded form (the sentence's keys plus the pad rows' V sum); vsum = NULL: all
// kend[r] keys.  The query arrives as n_parts <= 8 slabs part_stride floats apart and is rotated at rope_pos[r] (QPre)
bool dia_f8_cross(hipStream_t stream, const float *q, int ld, const void *kc, const void *vc, int NH, int rows, int nz, float scale, float *dst, int n_ctx, const uint32_t *kend,
                  const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, int n_parts, int64_t part_stride, const uint32_t *rope_pos,
                  float theta_scale);
