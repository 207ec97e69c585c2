// shim_dia_cross.h — launchers of shim_dia_cross.hip (the kernels of dia_cross_kernels.h), called by dia_encode_into and launch_attn_gqa (both of its branches).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Vsum[l][2 slot + b][A] = the sum of V rows n .. S - 1 of the slot's two row slots in every layer's cross cache ([L][RS][S][A] of kv_esz bytes per
// element), klive[2 slot + b] = n; false: the launch failed
bool dia_cross_padsum(hipStream_t stream, int kv_esz, const void *cv, int L, int RS, int S, int A, int slot, int n, float *vsum, uint32_t *klive);
// the bounded sibling of attn_gqa_wave_kernel<128, EXT_SLOTS, true, KV>: grid (NH, rows, nz), partials into `part`; vsum / klive of this layer's row slots.
// The query arrives as n_parts slabs part_stride floats apart and is rotated at rope_pos[r] (QPre)
bool dia_cross_bounded(hipStream_t stream, int kv_esz, const float *q, int ld, const void *kc, const void *vc, int NH, int rows, int nz, float scale, float *part, int n_ctx,
                       const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, int n_parts, int64_t part_stride,
                       const uint32_t *rope_pos, float theta_scale);
// the finished-row form for a launch that splits no keys (attn_cross_bounded_rows_kernel): grid (NH, rows), the attended rows into out [rows][NH 128] (fp32), any
// number of keys up to n_ctx, no partials and no combine launch behind it
bool dia_cross_bounded_rows(hipStream_t stream, int kv_esz, const float *q, int ld, const void *kc, const void *vc, int NH, int rows, float scale, float *out, int n_ctx,
                            const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, const uint32_t *klive, const float *vsum, int n_parts, int64_t part_stride,
                            const uint32_t *rope_pos, float theta_scale);
