// shim_decoder.h — launchers of shim_decoder.hip that shim_llama.hip reuses (their argument records come from parler_kernels.h).
#pragma once
#include "shim_internal.h"
#include "parler_kernels.h"

enum { DIA_STREAM_SLABS = 8 };   // slab budget of the Dia step buffers (di_qkv, di_q, di_gu, di_parts)
int stream_slices(const tts_hip_ctx *c, const W &w, int R, int max_slabs);
bool stream_fold_ok(const tts_hip_ctx *c, const W &w, int R, int max_slabs);
int run_qgemm(tts_hip_ctx *c, int kclass, const W &w, GemmArgs a, int pro, int epi);
int qstream_slab_rows(int R);
int qstream_slices(const tts_hip_ctx *c, const W &w, int R, int max_slabs);
int launch_qstream(tts_hip_ctx *c, int kclass, const W &w, int R, float *out, int ldo, int64_t slab_stride, int ks);
int run_gemm(tts_hip_ctx *c, int kclass, const W &w, GemmArgs a, int pro, int epi);
// one fp16 matrix on gemm_tile_kernel whatever tile_min_rows says (the caller has checked F16, K % 128, N % 16): a.A fp16 rows, all of them in one launch.
// EPI_RESID onto a.out with N == H may split K: the slabs go to parts ([8][RMAX][H]) and *pending becomes their count, for the caller's next folding norm
int run_gemm_tile_f16(tts_hip_ctx *c, int kclass, const W &w, GemmArgs a, int epi, float *parts, int *pending);
enum { DIA_MAX_UTTERANCES = 128 };   // RMAX = 256 rows of one Dia forward, two guidance rows per utterance
// an Orpheus forward of 65 .. 256 rows on qgemm_tile_kernel: shape / k slices of a GEMM, and its launch on the codes in c->aq / c->adT
void choose_llama_qtile(const tts_hip_ctx *c, int R, int N, int K, bool residual, int max_slabs, int *shape_out, int *ks_out);
int run_qtile_rows(tts_hip_ctx *c, int kclass, const W &w, int R, float *out, int ldo, int epi, int shape, int ks, int64_t slab_stride);
