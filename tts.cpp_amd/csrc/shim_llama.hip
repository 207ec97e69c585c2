// shim_llama.hip — the Orpheus (Llama-3) decoder step and Dia, on the row-streaming GEMV kernels.
#include "shim_session.h"

#include "gemv_stream_kernels.h"
#include "t5_kernels.h"
#include "llama_kernels.h"
#include "dia_kernels.h"
#include "gemv_kernels.h"
#include "shim_decoder.h"
#include "shim_dia_rows.h"

// Orpheus decoder (src/models/orpheus/model.cpp:186-325)
// ------------------------------------------------------------------------------------------------
extern "C" tts_hip_ctx *tts_hip_orpheus_create(int device, const tts_hip_orpheus_desc *ld_in) {
    // a desc of the size before kv_type was appended (callers built against that header) reads as kv_type = 0; every other size is refused
    constexpr size_t size_before_kv_type = offsetof(tts_hip_orpheus_desc, kv_type);
    if (!ld_in || (ld_in->struct_size != sizeof(tts_hip_orpheus_desc) && ld_in->struct_size != size_before_kv_type)) {
        set_err("tts_hip_orpheus_create: bad desc (struct_size mismatch)");
        return nullptr;
    }
    tts_hip_orpheus_desc full{};
    memcpy(&full, ld_in, ld_in->struct_size);
    full.struct_size = sizeof(full);
    const tts_hip_orpheus_desc *ld = &full;
    if (ld->kv_type != 0 && ld->kv_type != TTS_HIP_F16 && ld->kv_type != TTS_HIP_KV_F8_E4M3) {
        set_err("tts_hip_orpheus_create: kv_type %u is none of 0 (the flags decide), TTS_HIP_F16 (1) and TTS_HIP_KV_F8_E4M3 (256)", ld->kv_type);
        return nullptr;
    }
    if (ld->kv_type == TTS_HIP_KV_F8_E4M3 && (ld->flags & TTS_HIP_FLAG_KV_F16)) {
        set_err("tts_hip_orpheus_create: kv_type TTS_HIP_KV_F8_E4M3 together with TTS_HIP_FLAG_KV_F16: one cache element type per context");
        return nullptr;
    }
    tts_hip_desc d{};
    d.struct_size = sizeof(d);
    d.hidden_size = ld->hidden_size; d.n_layers = ld->n_layers; d.n_attn_heads = ld->n_attn_heads; d.max_ctx_length = ld->n_ctx;
    d.max_seqs = 1;
    d.flags = (ld->flags & (TTS_HIP_FLAG_VALU_GEMM | TTS_HIP_FLAG_DEQUANT_Q)) | TTS_HIP_FLAG_NO_PARLER | TTS_HIP_FLAG_NO_DAC;
    tts_hip_ctx *c = tts_hip_create(device, &d);
    if (!c) return nullptr;
    c->has_llama = true;
    c->lm = *ld;
    if ((ld->flags & TTS_HIP_FLAG_KV_F16) || ld->kv_type == TTS_HIP_F16) c->l_kv_esz = 2;
    if (ld->kv_type == TTS_HIP_KV_F8_E4M3) c->l_kv_esz = 1;
    if (c->lm.max_seqs == 0) c->lm.max_seqs = 1;
    // up to 64 slots: the streaming kernels carry every step.  65 .. 256 (= RMAX, the rows of one forward): the steps of more than 64 rows run on the
    // LDS-tiled integer GEMM (llama_forward); such a context plans the transposed scale tables into its arena
    if (c->lm.max_seqs > LLAMA_MAX_SEQS) { set_err("tts_hip_orpheus_create: max_seqs %u > %d", c->lm.max_seqs, (int) LLAMA_MAX_SEQS); tts_hip_destroy(c); return nullptr; }
    // measured on MI355X at the orpheus-3b Q4_0 shapes (profiles/r02/first_call_orpheus_*.log): 3.84 ms/step through the
    // lock-step workgroups, 2.98 with the streaming 1-4 row kernels, 2.84 reading the Q4_0 codes themselves, 2.80 with the
    // step captured in one hipGraph -> all three are the default here; TTS_HIP_GEMV_ROWS / _Q4_NATIVE / _LLAMA_GRAPH=0 turn them off
    if (!getenv("TTS_HIP_GEMV_ROWS")) c->gemv_rows = true;
    if (!getenv("TTS_HIP_Q4_NATIVE")) c->q4_native = true;
    if (!getenv("TTS_HIP_LLAMA_GRAPH")) c->llama_graph = true;
    if (c->lm.rope_base == 0.0f) c->lm.rope_base = 500000.0f;
    // lock-step utterances (5 .. 64 rows per step): the rows are quantised once (quant_rows_q8_kernel), not by every 16-feature workgroup again — at 8 rows
    // of width 3072 a workgroup read 98 KB of fp32 rows beside its 49 KB of weights (4.11 -> 3.35 ms per step, profiles/r06/orpheus_batch_call2.txt)
    if (c->lm.max_seqs > 4) c->q_fuse_max = 4;
    return c;
}

// The one dispatch on a K/V cache's element size (4: fp32; 2: fp16 — Orpheus TTS_HIP_FLAG_KV_F16, Dia tts_hip_dia_desc::kv_type): f(kc, vc) runs with the two
// pointers typed float * or _Float16 *, and the writers and readers it launches are the instantiations for that type (kv_of<decltype(kc)>).
template <typename P> using kv_of = std::remove_pointer_t<P>;
template <typename F>
static int with_kv(int kv_esz, void *kc, void *vc, F &&f) {
    return kv_esz == 2 ? f((_Float16 *) kc, (_Float16 *) vc) : f((float *) kc, (float *) vc);
}
// The Llama forward's dispatch: the same, plus 1: e4m3 (tts_hip_orpheus_desc::kv_type = TTS_HIP_KV_F8_E4M3).  Dia's call sites stay on with_kv: no Dia writer
// and no EXT reader is built for kv_f8.
template <typename F>
static int with_kv_llama(int kv_esz, void *kc, void *vc, F &&f) {
    return kv_esz == 1 ? f((kv_f8 *) kc, (kv_f8 *) vc) : with_kv(kv_esz, kc, vc, f);
}

// attn_gqa_kernel<128, false, KV> with more than 48 KB of scores: the attribute once per instantiation and device
template <typename KV>
static int attn_gqa_allow_lds(tts_hip_ctx *c, size_t lds) {
    static std::atomic<uint64_t> attr{0};
    if (lds > 48 * 1024 && attr_needed(attr, c->device))
        HIPCHK(hipFuncSetAttribute((const void *) attn_gqa_kernel<128, false, KV>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 8192));
    return 0;
}

// attention of the Llama / Dia steps: one workgroup per (head, row), or — few rows, many keys — the keys split over `nz` workgroups
// plus a combine launch (attn_gqa_kernel<128, true, KV>).  max_keys bounds the LDS score buffer.  seq_stride counts cache elements.
template <typename KV>
static int launch_attn_gqa(tts_hip_ctx *c, int NHq, int rows, int max_keys, const float *qkv, int ld, const uint32_t *pos, const KV *kc, const KV *vc, int NKV,
                           float scale, float *out, const uint32_t *kbeg, const uint32_t *kend, const uint32_t *row_seq, int64_t seq_stride, bool fixed_split, bool q_out = false,
                           QPre qp = QPre{}, int *deferred = nullptr, int n_ctx_keys = 0) {
    int nz = 1;
    if (deferred) *deferred = 0;
    if (c->attn_split_max > 1 && NHq * rows <= 256) {
        // a graph captured once replays for every position: the split count must not depend on the position then
        nz = fixed_split ? c->attn_split_max : std::min(c->attn_split_max, std::max(1, max_keys / 128));
        while (nz > 1 && (size_t) rows * NHq * nz > c->attn_part_cap) nz--;
    }
    if (nz <= 1) {
        hipLaunchKernelGGL((attn_gqa_kernel<128, false, KV>), dim3(NHq, rows), dim3(256), (size_t) (128 + max_keys) * 4, c->stream, qkv, ld, pos, kc, vc, NHq, NKV, scale, out, kbeg, kend,
                           row_seq, seq_stride, qp, q_out ? c->aq : (int8_t *) nullptr, q_out ? c->ad : (float *) nullptr);
        HIPCHK(hipGetLastError());
        if (q_out) c->aq_src = out;
        return 0;
    }
    const int chunk = (max_keys + nz - 1) / nz;
    const bool off32 = (uint64_t) std::max(n_ctx_keys, 1) * (uint64_t) NKV * 128 * sizeof(KV) < (1ull << 32);   // attn_gqa_wave_kernel addresses a sequence's rows with 32-bit byte offsets
    if (c->attn_wave && off32 && !kbeg && !kend && !row_seq && qp.n_parts == 1 && !qp.rope_pos && n_ctx_keys > 0) {
        // the captured one-row step (Orpheus): every key row requested at kernel start, online softmax per 16-lane group, one barrier (attn_gqa_wave_kernel)
        hipLaunchKernelGGL((attn_gqa_wave_kernel<128, 4, false, KV>), dim3(NHq, rows, nz), dim3(256), 0, c->stream, qkv, ld, pos, kc, vc, NHq, NKV, scale, c->attn_part, n_ctx_keys);
    } else {
        bool ext = false;
        if constexpr (KVRow<KV>::EXT_SLOTS > 0) {   // (kv_f8, the Llama decoder's alone, has no EXT form: nothing of it is built)
            ext = c->attn_wave && off32 && !kbeg && kend && n_ctx_keys > 0 && max_keys <= 16 * nz * 8 && qp.n_parts <= 8;
            // Dia's cross-attention (keys end at kend[r], per-row sequences, the query as slabs to fold and rotate): the same form, 8 passes through KVRow<KV>::EXT_SLOTS
            // rolling register slots (the parked rows of a loop step, kend[r] = 1, request that one key only)
            if (ext) {
                hipLaunchKernelGGL((attn_gqa_wave_kernel<128, KVRow<KV>::EXT_SLOTS, true, KV>), dim3(NHq, rows, nz), dim3(256), 0, c->stream, qkv, ld, pos, kc, vc, NHq, NKV, scale,
                                   c->attn_part, n_ctx_keys, kend, row_seq, seq_stride, qp);
            }
        }
        if (!ext) {
            hipLaunchKernelGGL((attn_gqa_kernel<128, true, KV>), dim3(nz, rows, NHq), dim3(256), (size_t) (128 + chunk + 1) * 4, c->stream, qkv, ld, pos, kc, vc, NHq, NKV, scale,
                               c->attn_part, kbeg, kend, row_seq, seq_stride, qp, (int8_t *) nullptr, (float *) nullptr);
        }
    }
    HIPCHK(hipGetLastError());
    if (deferred && c->attn_fold && nz == ATTN_FOLD_NZ && !c->prof && !c->debug) {
        *deferred = nz;   // the caller's next projection merges the slices in its staging prologue (gemv_stream_kernel<.., PRO_ATTN8, ..>); `out` is not written
        return 0;
    }
    hipLaunchKernelGGL(attn_gqa_combine_kernel, dim3(NHq, rows), dim3(128), 0, c->stream, (const float *) c->attn_part, nz, NHq, out, q_out ? c->aq : (int8_t *) nullptr, q_out ? c->ad : (float *) nullptr);
    if (q_out) c->aq_src = out;
    HIPCHK(hipGetLastError());
    return 0;
}

static int llama_gemm(tts_hip_ctx *c, const W &w, const float *A, int lda, float *out, int ldo, int n, int epi, int ksplit = 1) {
    for (int r0 = 0; r0 < n; r0 += c->RMAX) {
        GemmArgs g{};
        g.R = std::min(c->RMAX, n - r0); g.H = c->H;
        g.A = A + (size_t) r0 * lda; g.lda = lda;
        g.out = out + (size_t) r0 * ldo; g.ldo = ldo;
        if (ksplit > 1) {  // slabs [ksplit][RMAX][ldo], folded into the residual stream by the next rms_fold_rows_kernel
            g.kchunk = (int) w.K / ksplit;
            g.slab_stride = (int64_t) c->RMAX * ldo;
        }
        CHK(run_gemm(c, TTS_HIP_K_GEMM_OTHER, w, g, PRO_F32, epi));
    }
    return 0;
}

// one call of orpheus_runner::decode: n rows (<= RMAX) at pos0..; leaves the final-normed last row's logits in l_logits
// ids == nullptr: one row whose token id and position are already in l_ids[0] / l_pos[0] (the device-resident greedy loop)
// attn_positions != 0: size the attention scratch for that many cached positions instead of pos0 + n (a captured step is replayed
// at every position)
// row_seq != NULL (lock-step utterances, tts_hip_orpheus_step_batch / _generate_batch): row r belongs to cache slot row_seq[r] (device array); ids / positions /
// slots are already in l_ids / l_pos / l_seq (ids == NULL, any n), attn_positions bounds the keys of any row; logits_row: where the last row's logits go
// (l_logits + logits_row * Vpad), or -1: the logits of EVERY row r to l_logits + r * Vpad.  The one-sequence kernels that append to "the" cache
// (gemv_q4_qkv_rope_kernel) stay out of it.
static int llama_forward(tts_hip_ctx *c, const uint32_t *ids, int n, uint32_t pos0, int attn_positions = 0, const uint32_t *row_seq = nullptr, int logits_row = 0) {
    const int H = c->H, F = c->F, NH = c->NH, NKV = (int) c->lm.n_kv_heads, HD = (int) c->lm.head_dim;
    const int QKV = (NH + 2 * NKV) * HD, NCTX = (int) c->lm.n_ctx;
    if (n < 1 || n > c->RMAX) return set_err("tts_hip_orpheus_decode: %d tokens per call outside 1..%d", n, c->RMAX);
    // (lock-step rows carry their own positions, checked by llama_stage_rows: more rows than cached positions is fine there)
    if (!row_seq && pos0 + (uint32_t) n > (uint32_t) NCTX) return set_err("tts_hip_orpheus_decode: positions up to %u exceed the %d cached positions", pos0 + n, NCTX);
    auto f32 = [&](size_t off) { return (const float *) (c->arena + off); };
    if (ids) {
        std::vector<uint32_t> hp((size_t) n);
        for (int i = 0; i < n; i++) {
            if (ids[i] >= (uint32_t) c->l_V) return set_err("tts_hip_orpheus_decode: token id %u >= vocabulary %d", ids[i], c->l_V);
            hp[(size_t) i] = pos0 + (uint32_t) i;
        }
        HIPCHK(hipMemcpyAsync(c->l_ids, ids, (size_t) n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->l_pos, hp.data(), (size_t) n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));  // hp is a local
    } else if (n != 1 && !row_seq) {
        return set_err("llama_forward: device-resident inputs carry one row");
    }
    const int64_t seq_stride = (int64_t) c->L * NCTX * c->l_kvH;   // the cache is [slot][layer][position][kv width]: slot 0 is the one-sequence context's cache
    hipLaunchKernelGGL(t5_embed_kernel, dim3(n), dim3(256), 0, c->stream, f32(c->l_embd), (const uint32_t *) c->l_ids, H, c->l_x);
    HIPCHK(hipGetLastError());
    const float theta_scale = powf(c->lm.rope_base, -2.0f / (float) HD);
    c->l_pending = 0;
    // the streaming integer GEMV of 1..4 rows takes its Q8_0 activation blocks from the producing kernel where there is one
    enum { QS_QKV = 1, QS_O = 2, QS_GU = 4, QS_DOWN = 8, QS_HEAD = 16 };   // bits of tune("q_stream")
    auto slices = [&](const W &w, int bit, int rows, int max_slabs) { return (c->q_stream & bit) ? qstream_slices(c, w, rows, max_slabs) : 0; };
    auto q_for = [&](const W &w, int rows, int bit) {
        if (slices(w, bit, rows, std::min(16, 8 * c->RMAX / qstream_slab_rows(rows)))) return true;   // 5 .. 16 rows: the weight-streaming integer GEMM takes the producer's blocks as well
        return c->gemv_rows && rows <= 4 && w.type == TTS_HIP_Q8I && !(c->d.flags & (TTS_HIP_FLAG_VALU_GEMM | TTS_HIP_FLAG_DEQUANT_Q)) && w.K % 32 == 0;
    };
    // 5 .. 16 rows on a quantised matrix: qgemv_stream_kernel — K slices as fp32 slabs the consumer folds.  Returns the slab count (0: the shape does not
    // qualify, the caller takes the MFMA workgroups), < 0 on error.  A: the fp32 rows whose Q8_0 blocks the producer left in aq / ad (quantised here otherwise).
    const int srows = qstream_slab_rows(n), smax = std::min(16, c->RMAX / srows), pmax = std::min(16, 8 * c->RMAX / srows);   // rows per slab of the streaming integer GEMM; slabs l_qkv / l_gu and l_parts hold
    auto qstream = [&](const W &w, int bit, const float *A, int K, float *out, int ldo, int64_t slab_stride, int max_slabs) -> int {
        const int ks = slices(w, bit, n, max_slabs);
        if (!ks) return 0;
        if (c->aq_src != A) {
            hipLaunchKernelGGL(quant_rows_q8_kernel, dim3((K / 32 + 7) / 8, n), dim3(256), 0, c->stream, A, K, K, c->aq, c->ad, n);
            if (hipGetLastError() != hipSuccess) { set_err("quant_rows_q8_kernel launch failed"); return -1; }
        }
        c->aq_src = nullptr;
        if (launch_qstream(c, TTS_HIP_K_GEMM_OTHER, w, n, out, ldo, slab_stride, ks) != 0) return -1;
        return ks;
    };
    // 65 .. 256 rows of a context of more than 64 slots on a quantised matrix: one qgemm_tile_kernel launch over all rows (65 is where qgemv_stream_kernel
    // ends).  Its operands are Q8_0 codes [n][K] in aq and TRANSPOSED block scales in adT, written by the producer: rms_fold_rows_q8t_kernel (qkv, gate | up,
    // the head), silu_mul_q8t_kernel (down), quant_rows_q8t_kernel on the attention's rows (o).  tune("qtile_min_rows") = 0: the 16-feature kernel as before.
    auto tiled = [&](const W &w) {
        return c->adT && w.stoff && H <= 4096 && n > LLAMA_STREAM_ROWS && c->qtile_min_rows > 0 && n >= c->qtile_min_rows && !(c->d.flags & (TTS_HIP_FLAG_VALU_GEMM | TTS_HIP_FLAG_DEQUANT_Q));
    };
    // o / down projection: K slices as slabs in l_parts ([8][RMAX][H]) that the next rms norm folds, or the residual add in the epilogue
    auto tile_resid = [&](const W &w) {
        int shape, ks;
        choose_llama_qtile(c, n, (int) w.N, (int) w.K, true, 8, &shape, &ks);
        if (ks > 1) {
            CHK(run_qtile_rows(c, TTS_HIP_K_GEMM_OTHER, w, n, c->l_parts, H, EPI_STORE, shape, ks, (int64_t) c->RMAX * H));
            c->l_pending = ks; c->l_pstride = (int64_t) c->RMAX * H;
            return 0;
        }
        return run_qtile_rows(c, TTS_HIP_K_GEMM_OTHER, w, n, c->l_x, H, EPI_RESID, shape, 1, 0);
    };
    auto tile_store = [&](int kclass, const W &w, float *out, int ldo) {
        int shape, ks;
        choose_llama_qtile(c, n, (int) w.N, (int) w.K, false, 1, &shape, &ks);
        return run_qtile_rows(c, kclass, w, n, out, ldo, EPI_STORE, shape, 1, 0);
    };
    auto rms = [&](size_t w_off, int rows, float *x, float *y, const W *next, int bit = 0) {
        if (next && rows == n && tiled(*next)) {
            // y (l_xn) is not written on this path: the consumer reads the codes, and no debug_read item reads l_xn
            hipLaunchKernelGGL(rms_fold_rows_q8t_kernel, dim3(rows), dim3(256), 0, c->stream, x, H, f32(w_off), rows, 1e-5f,
                               c->l_pending ? (const float *) c->l_parts : (const float *) nullptr, c->l_pending, c->l_pstride ? c->l_pstride : (int64_t) c->RMAX * H,
                               c->aq, c->adT, c->ldr);
            c->l_pending = 0; c->l_pstride = 0;
            c->aq_src = nullptr;
            return hipGetLastError() == hipSuccess ? 0 : set_err("rms_fold_rows_q8t_kernel launch failed");
        }
        const bool q = next && q_for(*next, rows, bit);
        hipLaunchKernelGGL(rms_fold_rows_kernel, dim3(rows), dim3(256), 0, c->stream, x, H, f32(w_off), y, rows, 1e-5f,
                           c->l_pending ? (const float *) c->l_parts : (const float *) nullptr, c->l_pending, c->l_pstride ? c->l_pstride : (int64_t) c->RMAX * H,
                           q ? c->aq : (int8_t *) nullptr, q ? c->ad : (float *) nullptr);
        c->l_pending = 0; c->l_pstride = 0;
        c->aq_src = q ? y : nullptr;
        return hipGetLastError() == hipSuccess ? 0 : set_err("rms_fold_rows_kernel launch failed");
    };
    for (int l = 0; l < c->L; l++) {
        const auto &y = c->l_layers[l];
        // this layer of slot 0: fp32 rows, fp16 rows under TTS_HIP_FLAG_KV_F16 or e4m3 bytes under kv_type = TTS_HIP_KV_F8_E4M3 (with_kv_llama: the cache's writer and
        // readers below are launched for that type)
        const size_t layer_off = (size_t) l * NCTX * c->l_kvH * (size_t) c->l_kv_esz;
        const size_t qkv_lds = (size_t) n * H + (size_t) n * (H / 32) * 4;
        const bool qkv_fused = !row_seq && n <= 4 && c->q4_rope && c->q4_lds && y.qkv.q4 && q_for(y.qkv, n, QS_QKV) && HD == 128 && H % 512 == 0 && qkv_lds <= 64 * 1024 && !c->prof;
        // the rms norm inside the consuming projection's staging (stage_rms_q8): no slabs may be pending, the row is held in registers
        const bool rms_fused = c->q4_rms && !c->l_pending && H <= 4096;
        CHK(with_kv_llama(c->l_kv_esz, (char *) c->l_kc + layer_off, (char *) c->l_vc + layer_off, [&](auto *kc, auto *vc) -> int {
            typedef kv_of<decltype(kc)> KV;
            const RopeEpi<KV> re{(const uint32_t *) c->l_pos, f32(c->l_ropef), theta_scale, NH, NKV, kc, vc};
            if (qkv_fused && rms_fused) {
                QGemmArgs qa{};
                qa.g.W = c->arena + y.qkv.off; qa.g.K = H; qa.g.N = QKV; qa.g.R = n; qa.g.out = c->l_qkv; qa.g.ldo = QKV;
                qa.wd = (const _Float16 *) (c->arena + y.qkv.soff);
                RmsSrc rs{c->l_x, f32(y.in_norm), 1e-5f};
                hipLaunchKernelGGL((gemv_q4_qkv_rope_kernel<4, 2, 2, KV>), dim3((QKV / 2 + 3) / 4), dim3(256), qkv_lds + 16, c->stream, qa, y.qkv.q4, re, rs);
                HIPCHK(hipGetLastError());
                c->aq_src = nullptr;
            } else if (qkv_fused) {
                CHK(rms(y.in_norm, n, c->l_x, c->l_xn, &y.qkv, QS_QKV));
                // the projection, the rope of q and k and the cache append in one launch (gemv_q4_qkv_rope_kernel)
                QGemmArgs qa{};
                qa.g.W = c->arena + y.qkv.off; qa.g.K = H; qa.g.N = QKV; qa.g.R = n; qa.g.out = c->l_qkv; qa.g.ldo = QKV;
                qa.wd = (const _Float16 *) (c->arena + y.qkv.soff); qa.aq = c->aq; qa.ad = c->ad;
                hipLaunchKernelGGL((gemv_q4_qkv_rope_kernel<4, 0, 2, KV>), dim3((QKV / 2 + 3) / 4), dim3(256), qkv_lds, c->stream, qa, y.qkv.q4, re, RmsSrc{});
                HIPCHK(hipGetLastError());
                c->aq_src = nullptr;
            } else {
                CHK(rms(y.in_norm, n, c->l_x, c->l_xn, &y.qkv, QS_QKV));
                const int sl = qstream(y.qkv, QS_QKV, c->l_xn, H, c->l_qkv, QKV, (int64_t) srows * QKV, smax);   // slabs of srows rows inside l_qkv ([RMAX][QKV])
                if (sl < 0) return -1;
                if (!sl) {
                    if (tiled(y.qkv)) CHK(tile_store(TTS_HIP_K_GEMM_OTHER, y.qkv, c->l_qkv, QKV));
                    else CHK(llama_gemm(c, y.qkv, c->l_xn, H, c->l_qkv, QKV, n, EPI_STORE));
                }
                hipLaunchKernelGGL(llama_rope_kv_kernel<KV>, dim3(n, NH + NKV), dim3(64), 0, c->stream, c->l_qkv, (const uint32_t *) c->l_pos, f32(c->l_ropef), theta_scale, NH, NKV, HD, kc, vc,
                                   row_seq, row_seq ? seq_stride : (int64_t) 0, std::max(sl, 1), (int64_t) srows * QKV);
                HIPCHK(hipGetLastError());
            }
            // tts_hip_profile: the attention launches of the step as TTS_HIP_K_ATTN_SELF (bytes: K and V rows up to the bound on the rows' keys)
            const int max_keys = (int) (attn_positions ? (uint32_t) attn_positions : pos0 + n);
            CHK(prof_begin(c, TTS_HIP_K_ATTN_SELF, 2.0 * n * max_keys * c->l_kvH * c->l_kv_esz, 0.0));
            CHK(launch_attn_gqa<KV>(c, NH, n, max_keys, (const float *) c->l_qkv, QKV, (const uint32_t *) c->l_pos, kc, vc, NKV, 1.0f / sqrtf((float) HD), c->l_att, nullptr, nullptr,
                                    row_seq, row_seq ? seq_stride : (int64_t) 0, attn_positions != 0 && !row_seq, q_for(y.o, n, QS_O), QPre{}, nullptr, NCTX));
            return prof_end(c);
        }));
        {
            const int sl = qstream(y.o, QS_O, c->l_att, NH * HD, c->l_parts, H, (int64_t) srows * H, pmax);   // slabs of srows rows inside l_parts ([8][RMAX][H]), folded into the residual stream by the next rms norm
            if (sl < 0) return -1;
            if (sl) { c->l_pending = sl; c->l_pstride = (int64_t) srows * H; }
            else if (tiled(y.o)) {
                CHK(qtile_quant_rows(c, c->l_att, NH * HD, NH * HD, n));   // the attention's rows -> codes and transposed scales, a launch of its own
                CHK(tile_resid(y.o));
            }
            else CHK(llama_gemm(c, y.o, c->l_att, NH * HD, c->l_x, H, n, EPI_RESID));
        }
        const size_t gu_lds = (size_t) n * H + (size_t) n * (H / 32) * 4, dn_lds = (size_t) n * F + (size_t) n * (F / 32) * 4;
        const bool gu_fused = n <= 4 && c->q4_silu && c->q4_lds && y.gu.q4 && y.down.q4 && q_for(y.gu, n, QS_GU) && q_for(y.down, n, QS_DOWN) && H % 512 == 0 && F % 512 == 0 &&
                              gu_lds <= 64 * 1024 && dn_lds <= 64 * 1024 && (int) y.gu.N == 2 * F && !c->prof;
        if (!(gu_fused && rms_fused)) CHK(rms(y.post_norm, n, c->l_x, c->l_xn, &y.gu, QS_GU));
        if (gu_fused) {
            // gate | up with silu * up in the epilogue, then the down projection quantising that product while it stages it: two launches
            // instead of three (gemv_q4_gateup_silu_kernel, gemv_q4_rows_lds_kernel<.., QSRC 1>)
            const int gu_grid = std::min((F / 2 + 3) / 4, 512);   // 256 / 384 / 512 / 1024 workgroups: 1.24 / 1.17 / 1.14 / 1.25 ms per step (profiles/r05/orpheus_gu_grid_call12.txt)   // two resident workgroups per CU; a wave walks its items (gemv_q4_gateup_silu_kernel)
            QGemmArgs qa{};
            qa.g.W = c->arena + y.gu.off; qa.g.K = H; qa.g.N = 2 * F; qa.g.R = n;
            qa.wd = (const _Float16 *) (c->arena + y.gu.soff); qa.aq = c->aq; qa.ad = c->ad;
            if (rms_fused) {
                RmsSrc rs{c->l_x, f32(y.post_norm), 1e-5f};
                hipLaunchKernelGGL((gemv_q4_gateup_silu_kernel<4, 2>), dim3(gu_grid), dim3(256), gu_lds + 16, c->stream, qa, y.gu.q4, F, c->l_g, rs);
            } else {
                hipLaunchKernelGGL(gemv_q4_gateup_silu_kernel<4>, dim3(gu_grid), dim3(256), gu_lds, c->stream, qa, y.gu.q4, F, c->l_g);
            }
            HIPCHK(hipGetLastError());
            c->aq_src = nullptr;
            QGemmArgs qd{};
            qd.g.W = c->arena + y.down.off; qd.g.K = F; qd.g.N = H; qd.g.R = n; qd.g.A = c->l_g; qd.g.lda = F; qd.g.out = c->l_x; qd.g.ldo = H;
            qd.wd = (const _Float16 *) (c->arena + y.down.soff);
            static std::atomic<uint64_t> attr{0};
            if (attr_needed(attr, c->device)) {
                HIPCHK(hipFuncSetAttribute((const void *) gemv_q4_rows_lds_kernel<4, 2, 1, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                HIPCHK(hipFuncSetAttribute((const void *) gemv_q4_rows_lds_kernel<4, 2, 1, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            }
            if (F > 4096) hipLaunchKernelGGL((gemv_q4_rows_lds_kernel<4, 2, 1, 4>), dim3((H + 7) / 8), dim3(256), dn_lds, c->stream, qd, y.down.q4, (int) EPI_RESID);
            else hipLaunchKernelGGL((gemv_q4_rows_lds_kernel<4, 2, 1, 2>), dim3((H + 7) / 8), dim3(256), dn_lds, c->stream, qd, y.down.q4, (int) EPI_RESID);
            HIPCHK(hipGetLastError());
            continue;
        }
        const int slg = qstream(y.gu, QS_GU, c->l_xn, H, c->l_gu, 2 * F, (int64_t) srows * 2 * F, smax);   // slabs of srows rows inside l_gu; silu_mul_kernel folds them
        if (slg < 0) return -1;
        if (!slg) {
            if (tiled(y.gu)) CHK(tile_store(TTS_HIP_K_GEMM_OTHER, y.gu, c->l_gu, 2 * F));
            else CHK(llama_gemm(c, y.gu, c->l_xn, H, c->l_gu, 2 * F, n, EPI_STORE));
        }
        if (tiled(y.down) && F % 32 == 0) {
            hipLaunchKernelGGL(silu_mul_q8t_kernel, dim3((F + 1023) / 1024, n), dim3(256), 0, c->stream, (const float *) c->l_gu, F, c->aq, c->adT, c->ldr);
            HIPCHK(hipGetLastError());
            c->aq_src = nullptr;
            CHK(tile_resid(y.down));
            continue;
        }
        const bool down_stream = slices(y.down, QS_DOWN, n, pmax) != 0;
        const int ks = ((c->gemv_rows && n <= 4) || down_stream) ? 1 : c->l_ksplit;   // the streaming kernels walk all of K themselves
        const bool qd = ks == 1 && q_for(y.down, n, QS_DOWN);
        hipLaunchKernelGGL(silu_mul_kernel, dim3((unsigned) (((size_t) n * F + 255) / 256)), dim3(256), 0, c->stream, (const float *) c->l_gu, F, n, c->l_g,
                           qd ? c->aq : (int8_t *) nullptr, qd ? c->ad : (float *) nullptr, std::max(slg, 1), (int64_t) srows * 2 * F);
        HIPCHK(hipGetLastError());
        c->aq_src = qd ? c->l_g : nullptr;
        if (down_stream) {
            const int sl = qstream(y.down, QS_DOWN, c->l_g, F, c->l_parts, H, (int64_t) srows * H, pmax);
            if (sl <= 0) return sl < 0 ? -1 : set_err("llama_forward: the down projection lost its streaming form");
            c->l_pending = sl; c->l_pstride = (int64_t) srows * H;
        } else if (ks > 1) {
            CHK(llama_gemm(c, y.down, c->l_g, F, c->l_parts, H, n, EPI_STORE, ks));
            c->l_pending = ks;
        } else {
            CHK(llama_gemm(c, y.down, c->l_g, F, c->l_x, H, n, EPI_RESID));
        }
    }
    // lm_head on the last token only (:287-290) — or, for lock-step utterances, on every row (each row is an utterance's last token)
    const bool head_stream = logits_row < 0 && slices(c->l_head, QS_HEAD, n, 1) != 0;
    const bool head_tiled = logits_row < 0 && tiled(c->l_head);   // every row's logits: N = Vpad is no multiple of the tile width, the last tile's stores stop at Vpad
    CHK(rms(c->l_out_norm, n, c->l_x, c->l_xn, (head_stream || head_tiled) ? &c->l_head : nullptr, QS_HEAD));
    if (head_tiled) return tile_store(TTS_HIP_K_GEMM_HEADS, c->l_head, c->l_logits, c->l_Vpad);
    if (head_stream) {   // lock-step utterances, 5 .. 16 of them: the head streams once, whole K per wave (no slabs)
        const int sl = qstream(c->l_head, QS_HEAD, c->l_xn, H, c->l_logits, c->l_Vpad, 0, 1);
        if (sl < 0) return -1;
        if (sl) return 0;
    }
    GemmArgs g{};
    g.H = H; g.lda = H; g.ldo = c->l_Vpad;
    if (logits_row < 0) { g.R = n; g.A = c->l_xn; g.out = c->l_logits; }
    else { g.R = 1; g.A = c->l_xn + (size_t) (n - 1) * H; g.out = c->l_logits + (size_t) logits_row * c->l_Vpad; }
    CHK(run_gemm(c, TTS_HIP_K_GEMM_HEADS, c->l_head, g, PRO_F32, EPI_STORE));
    return 0;
}

// between a tts_hip_orpheus_gen_launch and its gen_wait the steps may still be running on the stream: nothing else touches the context
static int llama_gen_idle(const tts_hip_ctx *c, const char *what) {
    if (c->ls.mode == tts_hip_ctx::LlamaStream::SESSION) return set_err("%s: a continuous session is open on this context (tts_hip_orpheus_stream_end first)", what);
    if (c->lg.active && c->lg.pending) return set_err("%s: the steps of a tts_hip_orpheus_gen_launch are under way (tts_hip_orpheus_gen_wait first)", what);
    return 0;
}

extern "C" int tts_hip_orpheus_decode(tts_hip_ctx *c, const uint32_t *ids, uint32_t n, uint32_t pos0, float *logits_out, uint32_t *token_out) {
    if (!c || !c->has_llama) return set_err("tts_hip_orpheus_decode: not an Orpheus context (tts_hip_orpheus_create)");
    if (!c->finalized || !c->weights_present) return set_err("tts_hip_orpheus_decode: context not finalized");
    if (!ids || n == 0) return set_err("tts_hip_orpheus_decode: no tokens");
    CHK(llama_gen_idle(c, "tts_hip_orpheus_decode"));
    HIPCHK(hipSetDevice(c->device));
    uint32_t done = 0;
    while (done < n) {   // a long prompt goes through in pieces of RMAX rows (same cache semantics as one call)
        const uint32_t m = std::min<uint32_t>((uint32_t) c->RMAX, n - done);
        CHK(llama_forward(c, ids + done, (int) m, pos0 + done));
        done += m;
    }
    if (token_out) {
        // l_tok: [0] the token, [1..] stage-1 indices, then stage-1 maxima
        uint32_t *pi = c->l_tok + 1;
        float *pv = (float *) (c->l_tok + 1 + ARGMAX_PARTS);
        hipLaunchKernelGGL(argmax_parts_kernel, dim3(ARGMAX_PARTS), dim3(256), 0, c->stream, (const float *) c->l_logits, c->l_V, pv, pi);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(argmax_fold_kernel, dim3(1), dim3(64), 0, c->stream, (const float *) pv, (const uint32_t *) pi, c->l_tok, (uint32_t *) nullptr,
                           (uint32_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(token_out, c->l_tok, 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (logits_out) HIPCHK(hipMemcpyAsync(logits_out, c->l_logits, (size_t) c->l_V * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// sampler::max or sampler::sample of l_logits -> l_tok[0]; captured: the history slot and the uniform come from device counters and the
// token is fed back; eager: hist_slot (may be NULL) receives the token, feed says whether it goes back as the next input
static int llama_select(tts_hip_ctx *c, const tts_hip_sampling *sp, bool captured, uint32_t *hist_slot, bool feed) {
    uint32_t *pi = c->l_tok + 1, *hist = c->l_tok + 1 + 2 * ARGMAX_PARTS, *hist_idx = hist + LLAMA_GREEDY_CHUNK;
    float *pv = (float *) (c->l_tok + 1 + ARGMAX_PARTS);
    if (!sp) {
        hipLaunchKernelGGL(argmax_parts_kernel, dim3(ARGMAX_PARTS), dim3(256), 0, c->stream, (const float *) c->l_logits, c->l_V, pv, pi);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(argmax_fold_kernel, dim3(1), dim3(64), 0, c->stream, (const float *) pv, (const uint32_t *) pi, c->l_tok, captured ? hist : hist_slot,
                           captured ? hist_idx : (uint32_t *) nullptr, (captured || feed) ? c->l_ids : (uint32_t *) nullptr, (captured || feed) ? c->l_pos : (uint32_t *) nullptr);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const double *pen = sp->repetition_penalty != 1.0f ? c->d_pen : nullptr;
    int32_t *last = (int32_t *) c->l_smp;
    uint32_t *repc = c->l_smp + 1, *call = c->l_smp + 2;
    hipLaunchKernelGGL(topk_parts_kernel, dim3(TOPK_PARTS), dim3(512), 0, c->stream, (const float *) c->l_logits, c->l_V, (int) sp->top_k, pen, c->pen_len, (const int32_t *) last,
                       (const uint32_t *) repc, c->l_cand);
    HIPCHK(hipGetLastError());
    float *total = nullptr;
    if (sp->top_p < 1.0f) {   // nucleus sampling: the softmax total over the whole vocabulary, accumulated in index order like the reference's
        total = (float *) (c->l_cand + (size_t) TOPK_PARTS * TOPK_MAXK);
        hipLaunchKernelGGL(softmax_total_kernel, dim3(1), dim3(1024), 0, c->stream, (const float *) c->l_logits, c->l_V, (const unsigned long long *) c->l_cand, sp->temperature, pen,
                           c->pen_len, (const int32_t *) last, (const uint32_t *) repc, total);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(topk_sample_kernel, dim3(1), dim3(1024), 0, c->stream, (const unsigned long long *) c->l_cand, (int) sp->top_k, sp->temperature, (const float *) c->d_uniforms,
                       call, pen, last, repc, c->l_tok, captured ? hist : hist_slot, captured ? hist_idx : (uint32_t *) nullptr,
                       (captured || feed) ? c->l_ids : (uint32_t *) nullptr, (captured || feed) ? c->l_pos : (uint32_t *) nullptr, sp->top_p, (const float *) total);
    HIPCHK(hipGetLastError());
    return 0;
}

// what the two-stage device sampler covers (topk_parts_kernel / topk_sample_kernel, llama_kernels.h); anything else: sample on the host
// from tts_hip_orpheus_decode's logits
static int check_llama_sampling(const tts_hip_ctx *c, const tts_hip_sampling *sp, const char *what) {
    if (!sp) return set_err("%s: null sampling parameters", what);
    if (!(sp->temperature > 0.0f)) return set_err("%s: temperature must be > 0", what);
    if (!(sp->repetition_penalty > 0.0f)) return set_err("%s: repetition_penalty must be > 0 (1 = off)", what);
    if (!(sp->top_p > 0.0f)) return set_err("%s: top_p must be > 0", what);
    if (sp->top_k == 0 || sp->top_k > TOPK_MAXK || (int) sp->top_k >= c->l_V)
        return set_err("%s: the device sampler takes top_k in 1..%d (got %u): sample on the host", what, TOPK_MAXK, sp->top_k);
    if (c->l_V > TOPK_PARTS * TOPK_SLICE) return set_err("%s: vocabulary %d > %d", what, c->l_V, TOPK_PARTS * TOPK_SLICE);
    return 0;
}

// generate_from_batch (:378-392) with sampler::max (sp == NULL) or sampler::sample (sp, uniforms[max_new]), one sequence, in pieces:
// begin = the prompt and the first selection, launch = up to n_steps replays of the captured step, wait = look at their ids.
// An utterance ends once its last id is the stopping token, max_new ids exist or the cache is full.
static void llama_gen_emit(tts_hip_ctx *c, uint32_t tok) {
    auto &g = c->lg;
    g.toks.push_back(tok);
    g.cur = tok;
    if (tok == g.stop_id || g.toks.size() >= g.max_new || g.pos >= c->lm.n_ctx) g.done = true;
}

static int llama_gen_begin_one(tts_hip_ctx *c, const char *what, const uint32_t *prompt, uint32_t n_prompt, uint32_t max_new, uint32_t stop_id, const tts_hip_sampling *sp,
                               const float *uniforms) {
    auto &g = c->lg;
    g.active = false;
    if (!prompt || n_prompt == 0) return set_err("%s: null argument", what);
    HIPCHK(hipSetDevice(c->device));
    g.sampled = sp != nullptr; g.max_new = max_new; g.stop_id = stop_id; g.pending = 0;
    if (sp) g.sp = *sp;
    g.pos = n_prompt; g.cur = 0; g.toks.clear(); g.handed = 0; g.done = false;
    if (max_new == 0) { g.done = true; g.active = true; return 0; }
    if (sp) {
        CHK(check_llama_sampling(c, sp, what));
        if (!uniforms) return set_err("%s: null uniforms", what);
        CHK(stage_uniforms(c, uniforms, (size_t) max_new));   // one sampler call per token, at most max_new tokens
        CHK(stage_penalty(c, sp->repetition_penalty, (int) max_new));
        const uint32_t init[3] = {0xFFFFFFFFu, 0u, 0u};   // sampler::reset (sampler.cpp:71-80): last token -1, count 0; call index 0
        HIPCHK(hipMemcpyAsync(c->l_smp, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const void *pen = sp->repetition_penalty != 1.0f ? (const void *) c->d_pen : nullptr;
        if (c->l_smp_baked.uni != c->d_uniforms || c->l_smp_baked.pen != pen || c->l_smp_baked.k != sp->top_k || c->l_smp_baked.temp != sp->temperature || c->l_smp_baked.top_p != sp->top_p) {
            auto it = c->graphs.find(9000002);
            if (it != c->graphs.end()) { (void) hipGraphExecDestroy(it->second); c->graphs.erase(it); }
            c->l_smp_baked.uni = c->d_uniforms; c->l_smp_baked.pen = pen; c->l_smp_baked.k = sp->top_k; c->l_smp_baked.temp = sp->temperature; c->l_smp_baked.top_p = sp->top_p;
        }
    }
    uint32_t tok = 0;
    {   // the prompt (pieces of RMAX rows), then the first selection
        uint32_t done = 0;
        while (done < n_prompt) {
            const uint32_t m = std::min<uint32_t>((uint32_t) c->RMAX, n_prompt - done);
            CHK(llama_forward(c, prompt + done, (int) m, done));
            done += m;
        }
        CHK(llama_select(c, sp, false, nullptr, false));
        HIPCHK(hipMemcpyAsync(&tok, c->l_tok, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    llama_gen_emit(c, tok);
    g.active = true;
    return 0;
}

// The token never leaves the device between two steps (the selection writes it back as the next input and bumps the position).  The
// history the captured step writes holds LLAMA_GREEDY_CHUNK ids: after that many replays it is copied to pinned host memory and its
// counter reset, all on the stream, so a launch of any size returns at once.  Steps run past the stopping token are discarded by
// gen_wait (their cache rows are never read: the next generation starts at position 0; the sampler draws they consume belong to no token).
static int llama_gen_launch_one(tts_hip_ctx *c, const char *what, uint32_t n_steps) {
    auto &g = c->lg;
    if (g.pending) return set_err("%s: the steps of the last gen_launch have not been looked at (gen_wait)", what);
    if (g.done || n_steps == 0) return 0;
    const tts_hip_sampling *sp = g.sampled ? &g.sp : nullptr;
    const uint32_t pos = g.pos;
    const uint32_t steps = std::min<uint32_t>(std::min<uint32_t>(n_steps, g.max_new - (uint32_t) g.toks.size()), c->lm.n_ctx - pos);
    if (steps > c->h_hist_cap) CHK(grow_pinned(&c->h_hist, &c->h_hist_cap, std::max<size_t>(steps, 64)));
    uint32_t *hist = c->l_tok + 1 + 2 * ARGMAX_PARTS, *hist_idx = hist + LLAMA_GREEDY_CHUNK;
    HIPCHK(hipMemcpyAsync(c->l_ids, &g.cur, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->l_pos, &g.pos, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const bool graph = c->llama_graph && !c->prof;
    hipGraphExec_t exec = nullptr;
    if (graph) {
        // one captured step (forward + selection + feedback); the history slot is a device counter
        const int key = sp ? 9000002 : 9000001;
        auto it = c->graphs.find(key);
        if (it == c->graphs.end()) {
            // one eager pass first: per-kernel attributes are set outside the capture (it rewrites the cache row of `pos`
            // with the values the first replay writes again, nothing else)
            CHK(llama_forward(c, nullptr, 1, pos, (int) c->lm.n_ctx));
            HIPCHK(hipStreamSynchronize(c->stream));
            CHK(capture_graph(c, key, [&] {
                const int rc = llama_forward(c, nullptr, 1, 0, (int) c->lm.n_ctx);
                return rc ? rc : llama_select(c, sp, true, nullptr, true);
            }, &exec));
        } else {
            exec = it->second;
        }
    }
    for (uint32_t s0 = 0; s0 < steps; s0 += LLAMA_GREEDY_CHUNK) {
        const uint32_t chunk = std::min<uint32_t>(LLAMA_GREEDY_CHUNK, steps - s0);
        if (graph) {
            HIPCHK(hipMemsetAsync(hist_idx, 0, 4, c->stream));
            for (uint32_t s = 0; s < chunk; s++) HIPCHK(hipGraphLaunch(exec, c->stream));
        } else {
            for (uint32_t s = 0; s < chunk; s++) {
                CHK(llama_forward(c, nullptr, 1, pos + s0 + s));
                CHK(llama_select(c, sp, false, hist + s, true));
            }
        }
        HIPCHK(hipMemcpyAsync(c->h_hist + s0, hist, (size_t) chunk * 4, hipMemcpyDeviceToHost, c->stream));
    }
    g.pending = steps;
    return 0;
}

static int llama_gen_wait_one(tts_hip_ctx *c) {
    auto &g = c->lg;
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint32_t steps = g.pending;
    g.pending = 0;
    if (steps == 0) return 0;
    g.pos += steps;
    for (uint32_t s = 0; s < steps && !g.done; s++) {
        // only the launch's last id meets the end of the cache: the ids before it were fed back inside the launch
        g.toks.push_back(c->h_hist[s]);
        g.cur = c->h_hist[s];
        if (c->h_hist[s] == g.stop_id || g.toks.size() >= g.max_new || (s + 1 == steps && g.pos >= c->lm.n_ctx)) g.done = true;
    }
    return 0;
}

// the ids no gen_wait has handed out yet -> tokens_out [max_new]
static void llama_gen_hand_one(tts_hip_ctx *c, uint32_t *tokens_out, uint32_t *n_out, uint8_t *done) {
    auto &g = c->lg;
    for (size_t i = g.handed; i < g.toks.size(); i++) tokens_out[i] = g.toks[i];
    g.handed = n_out[0] = (uint32_t) g.toks.size();
    if (done) done[0] = g.done;
}

static int llama_gen_ready(tts_hip_ctx *c, const char *what, bool may_be_running = false) {
    if (!c || !c->has_llama) return set_err("%s: not an Orpheus context (tts_hip_orpheus_create)", what);
    if (!c->finalized || !c->weights_present) return set_err("%s: context not finalized", what);
    return may_be_running ? 0 : llama_gen_idle(c, what);
}

// a one-sequence generation takes the context: a fixed batch that was under way is dropped
static void llama_batch_drop(tts_hip_ctx *c) {
    if (c->ls.mode == tts_hip_ctx::LlamaStream::BATCH) c->ls.mode = tts_hip_ctx::LlamaStream::NONE;
}

static int orpheus_generate(tts_hip_ctx *c, const char *what, const uint32_t *prompt, uint32_t n_prompt, uint32_t max_new, uint32_t stop_id, const tts_hip_sampling *sp,
                            const float *uniforms, uint32_t *tokens_out, uint32_t *n_out) {
    CHK(llama_gen_ready(c, what));
    if (!prompt || n_prompt == 0 || !tokens_out || !n_out) return set_err("%s: null argument", what);
    *n_out = 0;
    llama_batch_drop(c);
    CHK(llama_gen_begin_one(c, what, prompt, n_prompt, max_new, stop_id, sp, uniforms));
    // the host looks at LLAMA_GREEDY_CHUNK steps at once, so at most CHUNK-1 steps run past the stopping token
    int rc = 0;
    while (rc == 0 && !c->lg.done) {
        rc = llama_gen_launch_one(c, what, LLAMA_GREEDY_CHUNK);
        if (rc == 0) rc = llama_gen_wait_one(c);
    }
    if (rc == 0 && max_new) llama_gen_hand_one(c, tokens_out, n_out, nullptr);
    c->lg.active = false;
    return rc;
}

extern "C" int tts_hip_orpheus_generate_greedy(tts_hip_ctx *c, const uint32_t *prompt, uint32_t n_prompt, uint32_t max_new, uint32_t stop_id,
                                               uint32_t *tokens_out, uint32_t *n_out) {
    return orpheus_generate(c, "tts_hip_orpheus_generate_greedy", prompt, n_prompt, max_new, stop_id, nullptr, nullptr, tokens_out, n_out);
}

extern "C" int tts_hip_orpheus_generate_sampled(tts_hip_ctx *c, const uint32_t *prompt, uint32_t n_prompt, uint32_t max_new, uint32_t stop_id,
                                                const tts_hip_sampling *sampling, const float *uniforms, uint32_t *tokens_out, uint32_t *n_out) {
    if (!sampling) return set_err("tts_hip_orpheus_generate_sampled: null sampling parameters");
    return orpheus_generate(c, "tts_hip_orpheus_generate_sampled", prompt, n_prompt, max_new, stop_id, sampling, uniforms, tokens_out, n_out);
}

extern "C" int tts_hip_orpheus_sample_logits(tts_hip_ctx *c, const float *logits, const tts_hip_sampling *sp, float uniform, int32_t *last_id, uint32_t *rep_count,
                                             uint32_t *token_out) {
    if (!c || !c->has_llama) return set_err("tts_hip_orpheus_sample_logits: not an Orpheus context (tts_hip_orpheus_create)");
    if (!c->finalized) return set_err("tts_hip_orpheus_sample_logits: context not finalized");
    if (!logits || !token_out) return set_err("tts_hip_orpheus_sample_logits: null argument");
    CHK(llama_gen_idle(c, "tts_hip_orpheus_sample_logits"));
    CHK(check_llama_sampling(c, sp, "tts_hip_orpheus_sample_logits"));
    HIPCHK(hipSetDevice(c->device));
    const bool rep = sp->repetition_penalty != 1.0f;
    if (rep && (!last_id || !rep_count)) return set_err("tts_hip_orpheus_sample_logits: repetition penalty needs last_id and rep_count");
    CHK(stage_uniforms(c, &uniform, 1));
    if (rep) CHK(stage_penalty(c, sp->repetition_penalty, (int) std::min<uint32_t>(*rep_count + 2, 1u << 20)));
    const uint32_t init[3] = {rep ? (uint32_t) *last_id : 0xFFFFFFFFu, rep ? *rep_count : 0u, 0u};
    HIPCHK(hipMemcpyAsync(c->l_smp, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->l_logits, logits, (size_t) c->l_V * 4, hipMemcpyHostToDevice, c->stream));
    CHK(llama_select(c, sp, false, nullptr, false));
    uint32_t back[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(token_out, c->l_tok, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(back, c->l_smp, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (rep) { *last_id = (int32_t) back[0]; *rep_count = back[1]; }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Lock-step utterances ("within a GPU, B utterances batched in lock-step"; the reference's only concurrency is N independent
// workers, each with its own model copy, examples/server/server.cpp:225-321).  The cache holds lm.max_seqs slots; a step carries one row per
// live utterance, every row with its own slot and position.
// ------------------------------------------------------------------------------------------------
static int llama_stage_rows(tts_hip_ctx *c, const char *what, uint32_t n, const uint32_t *slots, const uint32_t *ids, const uint32_t *pos, uint32_t *max_pos) {
    if (n == 0 || (int) n > c->RMAX) return set_err("%s: %u rows outside 1..%d", what, n, c->RMAX);
    *max_pos = 0;
    for (uint32_t r = 0; r < n; r++) {
        if (slots[r] >= c->lm.max_seqs) return set_err("%s: cache slot %u >= max_seqs %u", what, slots[r], c->lm.max_seqs);
        if (ids[r] >= (uint32_t) c->l_V) return set_err("%s: token id %u >= vocabulary %d", what, ids[r], c->l_V);
        if (pos[r] >= c->lm.n_ctx) return set_err("%s: position %u outside the %u cached positions", what, pos[r], c->lm.n_ctx);
        *max_pos = std::max(*max_pos, pos[r]);
    }
    HIPCHK(hipMemcpyAsync(c->l_ids, ids, (size_t) n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->l_pos, pos, (size_t) n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->l_seq, slots, (size_t) n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// The selection of `rows` logits rows (first at `logits`) for slots row_slot[r] (NULL: slot0 + r) -> l_btok[r], every row with its slot's sampler
// (samp[], tables pen[][pen_len]; samp NULL: sampler::max for all): the arg-max pair when a row is greedy, the top-k kernels when one is sampled,
// the total when a sampled one has top_p < 1 — the caller knows which of its rows are.
static int llama_select_slots(tts_hip_ctx *c, bool any_max, bool any_sample, bool any_nucleus, int rows, const float *logits, const uint32_t *row_slot, int slot0,
                              const uint32_t *slot_state, const llama_slot_sampler *samp, const double *pen, int pen_len, uint32_t *smp, const float *uni, int64_t uni_stride,
                              unsigned long long *cand, float *total) {
    if (!any_sample) samp = nullptr;   // every row is sampler::max: the arg-max pair need not read the records
    if (any_max) {
        hipLaunchKernelGGL(argmax_slots_parts_kernel, dim3(ARGMAX_PARTS, rows), dim3(256), 0, c->stream, logits, c->l_V, c->l_Vpad, c->l_bpv, c->l_bpi, samp, row_slot, slot0, slot_state);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(argmax_slots_fold_kernel, dim3(rows), dim3(64), 0, c->stream, (const float *) c->l_bpv, (const uint32_t *) c->l_bpi, c->l_btok, samp, row_slot, slot0, slot_state);
        HIPCHK(hipGetLastError());
    }
    if (!any_sample) return 0;
    hipLaunchKernelGGL(topk_parts_rows_kernel, dim3(TOPK_PARTS, rows), dim3(512), 0, c->stream, logits, c->l_V, c->l_Vpad, samp, pen, pen_len, (const uint32_t *) smp, cand, row_slot, slot0,
                       slot_state);
    HIPCHK(hipGetLastError());
    if (any_nucleus) {
        hipLaunchKernelGGL(softmax_total_rows_kernel, dim3(1, rows), dim3(1024), 0, c->stream, logits, c->l_V, c->l_Vpad, (const unsigned long long *) cand, samp, pen, pen_len,
                           (const uint32_t *) smp, total, row_slot, slot0, slot_state);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(topk_sample_rows_kernel, dim3(1, rows), dim3(1024), 0, c->stream, (const unsigned long long *) cand, samp, uni, uni_stride, pen, pen_len, smp, c->l_btok,
                       (const float *) total, row_slot, slot0, slot_state);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int tts_hip_orpheus_step_batch(tts_hip_ctx *c, uint32_t n, const uint32_t *slots, const uint32_t *ids, const uint32_t *pos, float *logits_out, uint32_t *tokens_out) {
    if (!c || !c->has_llama) return set_err("tts_hip_orpheus_step_batch: not an Orpheus context (tts_hip_orpheus_create)");
    if (!c->finalized || !c->weights_present) return set_err("tts_hip_orpheus_step_batch: context not finalized");
    if (!slots || !ids || !pos) return set_err("tts_hip_orpheus_step_batch: null argument");
    CHK(llama_gen_idle(c, "tts_hip_orpheus_step_batch"));
    if (n > c->lm.max_seqs) return set_err("tts_hip_orpheus_step_batch: %u rows > max_seqs %u (one row per utterance)", n, c->lm.max_seqs);
    HIPCHK(hipSetDevice(c->device));
    uint32_t max_pos = 0;
    CHK(llama_stage_rows(c, "tts_hip_orpheus_step_batch", n, slots, ids, pos, &max_pos));
    CHK(llama_forward(c, nullptr, (int) n, 0, (int) max_pos + 1, c->l_seq, -1));
    if (tokens_out) {   // sampler::max of every row: no records
        CHK(llama_select_slots(c, true, false, false, (int) n, c->l_logits, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr));
        HIPCHK(hipMemcpyAsync(tokens_out, c->l_btok, (size_t) n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (logits_out) HIPCHK(hipMemcpy2DAsync(logits_out, (size_t) c->l_V * 4, c->l_logits, (size_t) c->l_Vpad * 4, (size_t) c->l_V * 4, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// the prompt of one utterance into its cache slot (pieces of RMAX rows); the last row's logits land in l_logits row `slot`
static int llama_prefill_slot(tts_hip_ctx *c, const char *what, uint32_t slot, const uint32_t *prompt, uint32_t n_prompt) {
    std::vector<uint32_t> sl, ps;
    uint32_t done = 0;
    while (done < n_prompt) {
        const uint32_t m = std::min<uint32_t>((uint32_t) c->RMAX, n_prompt - done);
        sl.assign(m, slot);
        ps.resize(m);
        for (uint32_t i = 0; i < m; i++) ps[i] = done + i;
        uint32_t max_pos = 0;
        CHK(llama_stage_rows(c, what, m, sl.data(), prompt + done, ps.data(), &max_pos));
        CHK(llama_forward(c, nullptr, (int) m, 0, (int) max_pos + 1, c->l_seq, (int) slot));
        done += m;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The lock-step loop (tts_hip_ctx::LlamaStream): generate_from_batch (orpheus/model.cpp:378-392) for the utterances in the cache slots, every one
// with exactly the tokens its own one-sequence generation gets (sampler::max, or sampler::sample with its own uniforms and repetition state).
// The state of a slot — ids so far, finished flag, latest id and position, sampler record and state, penalty table, uniforms — lives on the
// device, so a run of k steps is k x (forward, row-batched selection, llama_advance_rows_kernel) enqueued back to back: no copy and no
// synchronise inside the run.  Rows that finish inside a run idle as padding until its end.  The fixed batch (tts_hip_orpheus_gen_* at
// n_utt > 1, tts_hip_orpheus_generate_batch) admits slots 0 .. n-1 at begin; the continuous session (tts_hip_orpheus_stream_*) admits and
// refills slots while the others generate.
// ------------------------------------------------------------------------------------------------
typedef tts_hip_ctx::LlamaStream LS;

static int llama_stream_ready(tts_hip_ctx *c, const char *what, bool need_session = true) {
    if (!c || !c->has_llama) return set_err("%s: not an Orpheus context (tts_hip_orpheus_create)", what);
    if (!c->finalized || !c->weights_present) return set_err("%s: context not finalized", what);
    if (need_session && c->ls.mode != LS::SESSION) return set_err("%s: no session (tts_hip_orpheus_stream_begin)", what);
    return 0;
}

static const char *const LLAMA_WAIT = "tts_hip_orpheus_stream_wait", *const LLAMA_RUN = "tts_hip_orpheus_stream_run";   // as SlotLedger's texts name them

// one slot's record and table, as the rows kernels read them: sp NULL is sampler::max; the table is stage_penalty's for sp's penalty, len entries
// (all 0.0 where the penalty is 1)
static void llama_slot_sampler_host(const tts_hip_sampling *sp, int len, llama_slot_sampler *rec, double *table) {
    *rec = sp ? llama_slot_sampler{LLAMA_SLOT_SAMPLE, sp->top_k, sp->temperature, sp->top_p} : llama_slot_sampler{LLAMA_SLOT_MAX, 0u, 1.0f, 1.0f};
    if (sp && sp->repetition_penalty != 1.0f) penalty_table(table, sp->repetition_penalty, len);
    else std::fill(table, table + len, 0.0);
}

static void llama_loop_free(tts_hip_ctx *c) {
    auto &g = c->ls;
    free_dev(g.state); free_dev(g.tokens); free_dev(g.smp); free_dev(g.uni); free_dev(g.cand); free_dev(g.total); free_dev(g.samp); free_dev(g.pen);
    free_dev(g.d_handed); free_dev(g.look);
    if (g.h_state) (void) hipHostFree(g.h_state);
    if (g.h_look) (void) hipHostFree(g.h_look);
    g = LS{};
}

// Enter the loop.  The buffers stay on the context from one loop to the next while (n_slots, max_new) fits and grow when it does not (tts_hip_destroy
// frees them); whatever an earlier loop left in them is overwritten slot by slot by the admissions.  sp: what every admission of a loop that is
// not mixed selects with (NULL: sampler::max).
static int llama_loop_begin(tts_hip_ctx *c, const char *what, LS::Mode mode, uint32_t n_slots, uint32_t max_new, uint32_t stop_id, const tts_hip_sampling *sp, bool mixed) {
    auto &g = c->ls;
    const size_t S = n_slots, M = std::max<uint32_t>(max_new, 1);
    if (S > g.cap_slots || M > g.cap_new) {
        const size_t CS = std::max(S, g.cap_slots), CM = std::max(M, g.cap_new);
        (void) hipStreamSynchronize(c->stream);
        llama_loop_free(c);
        int rc = dmalloc(&g.state, CS * LLAMA_SLOT_STATE);
        if (rc == 0) rc = dmalloc(&g.tokens, CS * CM);
        if (rc == 0) rc = dmalloc(&g.smp, CS * 3);
        if (rc == 0) rc = dmalloc(&g.uni, CS * CM);
        if (rc == 0) rc = dmalloc(&g.total, CS);
        if (rc == 0 && hipMalloc((void **) &g.cand, CS * TOPK_PARTS * TOPK_MAXK * 8) != hipSuccess) rc = set_err("%s: out of device memory", what);
        if (rc == 0) rc = dmalloc((llama_slot_sampler **) &g.samp, CS);
        if (rc == 0) rc = dmalloc(&g.pen, CS * CM);
        if (rc == 0 && hipHostMalloc((void **) &g.h_state, CS * LLAMA_SLOT_STATE * 4) != hipSuccess) rc = set_err("%s: out of pinned memory", what);
        if (rc == 0) rc = dmalloc(&g.d_handed, CS);
        if (rc == 0) rc = dmalloc(&g.look, CS * (LLAMA_SLOT_STATE + CM));
        if (rc == 0 && hipHostMalloc((void **) &g.h_look, CS * (LLAMA_SLOT_STATE + CM) * 4) != hipSuccess) rc = set_err("%s: out of pinned memory", what);
        if (rc != 0) { llama_loop_free(c); return rc; }
        g.cap_slots = CS; g.cap_new = CM;
    }
    g.sampled = sp != nullptr; g.mixed = mixed; g.n_slots = n_slots; g.max_new = max_new; g.stop_id = stop_id;
    if (sp) g.sp = *sp;
    g.slot.assign(S, LS::FREE);
    g.count.assign(S, 0); g.cur.assign(S, 0); g.pos.assign(S, 0); g.handed.assign(S, 0);
    g.slot_sampled.assign(S, 0); g.slot_nucleus.assign(S, 0);
    g.rows.clear();
    g.in_flight = 0; g.unread = 0;
    g.mode = mode;
    return 0;
}

// One utterance into slot s (the arguments have been checked): everything the slot's predecessor left is overwritten — state, sampler state,
// record, table and the uniforms a sampled utterance draws from ([max_new]) — then the prompt goes into the slot's cache, its last row's logits
// land in l_logits row s, and the first selection and advance follow.
static int llama_loop_admit(tts_hip_ctx *c, const char *what, uint32_t s, const uint32_t *prompt, uint32_t n_prompt, const tts_hip_sampling *sp, const float *uniforms) {
    auto &g = c->ls;
    uint32_t *h = g.h_state + (size_t) s * LLAMA_SLOT_STATE;
    g.count[s] = 0; g.cur[s] = 0; g.pos[s] = n_prompt - 1; g.handed[s] = 0;
    if (g.max_new == 0) { g.slot[s] = LS::ENDED; return 0; }
    // count 0, not finished, no id yet, position of the prompt's last row; sampler::reset and the utterance's own draws
    const uint32_t init[LLAMA_SLOT_STATE] = {0u, 0u, 0u, n_prompt - 1};
    const uint32_t reset[3] = {0xFFFFFFFFu, 0u, 0u};
    // max_new entries, read at index min(count, max_new - 1).  The clamp never binds: a count goes up by at most one per selection, so the i-th
    // selection of an utterance (i = 1 .. max_new) reads a count of at most i - 1 <= max_new - 1.
    llama_slot_sampler rec;
    std::vector<double> table(g.max_new);
    llama_slot_sampler_host(sp, (int) g.max_new, &rec, table.data());
    HIPCHK(hipMemcpyAsync(g.state + (size_t) s * LLAMA_SLOT_STATE, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g.smp + (size_t) s * 3, reset, sizeof(reset), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(g.d_handed + s, 0, 4, c->stream));   // the look-ins start at the occupant's first id
    HIPCHK(hipMemcpyAsync((llama_slot_sampler *) g.samp + s, &rec, sizeof(rec), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g.pen + (size_t) s * g.max_new, table.data(), table.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (sp) HIPCHK(hipMemcpyAsync(g.uni + (size_t) s * g.max_new, uniforms, (size_t) g.max_new * 4, hipMemcpyHostToDevice, c->stream));
    g.slot_sampled[s] = sp != nullptr; g.slot_nucleus[s] = sp && sp->top_p < 1.0f;
    HIPCHK(hipStreamSynchronize(c->stream));   // init / reset / rec / table are locals
    CHK(llama_prefill_slot(c, what, s, prompt, n_prompt));
    CHK(llama_select_slots(c, !sp, sp != nullptr, g.slot_nucleus[s] != 0, 1, c->l_logits + (size_t) s * c->l_Vpad, nullptr, (int) s, g.state, (const llama_slot_sampler *) g.samp, g.pen,
                           (int) g.max_new, g.smp, g.uni, (int64_t) g.max_new, g.cand, g.total));
    hipLaunchKernelGGL(llama_advance_rows_kernel, dim3(1), dim3(64), 0, c->stream, 1, (const uint32_t *) nullptr, (int) s, (const uint32_t *) c->l_btok, g.state, g.tokens, g.max_new,
                       g.stop_id, c->lm.n_ctx, (uint32_t *) nullptr, (uint32_t *) nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, g.state + (size_t) s * LLAMA_SLOT_STATE, LLAMA_SLOT_STATE * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    g.count[s] = h[0]; g.cur[s] = h[2]; g.pos[s] = h[3];
    g.slot[s] = h[1] ? LS::ENDED : LS::LIVE;
    return 0;
}

static void llama_loop_live_rows(tts_hip_ctx *c) {
    auto &g = c->ls;
    g.rows.clear();
    for (uint32_t s = 0; s < g.n_slots; s++) if (g.slot[s] == LS::LIVE) g.rows.push_back(s);
}

// The enqueue half of a run: the live rows staged once, then up to n_steps x (forward, selection, advance), no copy and no synchronise behind them.
// The run is over once no row can still be live: a row with `count` ids at position `pos` ends after min(max_new - count, n_ctx - pos) steps at
// the latest.  With no live row nothing is launched.
static int llama_loop_launch(tts_hip_ctx *c, const char *what, uint32_t n_steps) {
    auto &g = c->ls;
    const uint32_t n = (uint32_t) g.rows.size();
    if (n == 0 || n_steps == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    std::vector<uint32_t> ids(n), ps(n);
    uint32_t left = 0;
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t s = g.rows[r];
        ids[r] = g.cur[s]; ps[r] = g.pos[s];
        left = std::max(left, std::min(g.max_new - g.count[s], c->lm.n_ctx - g.pos[s]));
    }
    uint32_t max_pos = 0;
    CHK(llama_stage_rows(c, what, n, g.rows.data(), ids.data(), ps.data(), &max_pos));   // the live rows, once per run
    bool any_max = false, any_sample = false, any_nucleus = false;   // which selection kernels this run's rows need
    for (uint32_t s : g.rows) { any_max |= !g.slot_sampled[s]; any_sample |= g.slot_sampled[s] != 0; any_nucleus |= g.slot_nucleus[s] != 0; }
    const uint32_t steps = std::min(n_steps, left);
    for (uint32_t i = 0; i < steps; i++) {
        // the longest row as long as nobody finishes, an upper bound once someone has (a finished row's position stands still)
        const uint32_t keys = std::min(max_pos + i + 1, c->lm.n_ctx);
        int rc = llama_forward(c, nullptr, (int) n, 0, (int) keys, c->l_seq, -1);
        if (rc == 0) rc = llama_select_slots(c, any_max, any_sample, any_nucleus, (int) n, c->l_logits, c->l_seq, 0, g.state, (const llama_slot_sampler *) g.samp, g.pen, (int) g.max_new,
                                             g.smp, g.uni, (int64_t) g.max_new, g.cand, g.total);
        if (rc == 0) {
            hipLaunchKernelGGL(llama_advance_rows_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, (int) n, (const uint32_t *) c->l_seq, 0, (const uint32_t *) c->l_btok, g.state,
                               g.tokens, g.max_new, g.stop_id, c->lm.n_ctx, c->l_ids, c->l_pos);
            if (hipGetLastError() != hipSuccess) rc = set_err("%s: llama_advance_rows_kernel did not launch", what);
        }
        g.in_flight = i + 1; g.unread += 1;   // also when the step was enqueued in part: the look-in that follows waits for it
        if (rc != 0) return rc;
    }
    return 0;
}

// The look-in half: one llama_loop_lookin_kernel launch (none when nothing is taken), one copy into pinned memory, one synchronise, whatever the slot count.  The slots' state
// becomes the host's; slots that finished are ENDED afterwards and have left the rows of the next run.  tokens_out != NULL ([n_slots][max_new])
// takes each occupant's ids that no earlier look-in took, at their places; n_out / done (may be NULL): ids so far / no longer live.
static int llama_loop_look(tts_hip_ctx *c, uint32_t *tokens_out, uint32_t *n_out, uint8_t *done) {
    auto &g = c->ls;
    HIPCHK(hipSetDevice(c->device));
    const int take = tokens_out ? 1 : 0;
    // an occupant's un-taken ids: one per step enqueued since the last look-in that took ids, plus the one its admission selected
    const uint32_t cap = take ? std::min(g.unread + 1, g.max_new) : 0u;
    const size_t stride = LLAMA_SLOT_STATE + (size_t) cap;
    if (take) {
        hipLaunchKernelGGL(llama_loop_lookin_kernel, dim3(g.n_slots), dim3(64), 0, c->stream, (int) g.n_slots, take, cap, g.max_new, (const uint32_t *) g.state,
                           (const uint32_t *) g.tokens, g.d_handed, g.look);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(g.h_look, g.look, (size_t) g.n_slots * stride * 4, hipMemcpyDeviceToHost, c->stream));
    } else {
        // nothing to gather: a block of headers alone is the state array itself, copied as a run has always copied it
        HIPCHK(hipMemcpyAsync(g.h_look, g.state, (size_t) g.n_slots * LLAMA_SLOT_STATE * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    g.in_flight = 0;
    for (uint32_t s = 0; s < g.n_slots; s++) {
        const uint32_t *h = g.h_look + (size_t) s * stride;
        if (g.slot[s] == LS::LIVE) {
            g.count[s] = h[0]; g.cur[s] = h[2]; g.pos[s] = h[3];
            if (h[1]) g.slot[s] = LS::ENDED;
        }
        const bool occupied = g.slot[s] != LS::FREE && g.max_new != 0;   // a free slot's block holds what its last occupant left
        if (take && occupied) {
            const uint32_t from = g.handed[s], to = std::min(g.count[s], g.max_new);
            const uint32_t ids = to > from ? std::min(to - from, cap) : 0u;   // as the kernel counts them
            if (ids) memcpy(tokens_out + (size_t) s * g.max_new + from, h + LLAMA_SLOT_STATE, (size_t) ids * 4);
            g.handed[s] = from + ids;
        }
        if (n_out) n_out[s] = occupied ? g.count[s] : 0u;
        if (done) done[s] = g.slot[s] != LS::LIVE;
    }
    if (take) g.unread = 0;
    llama_loop_live_rows(c);
    return 0;
}

// A run: launch, then a look-in that takes nothing.  With no live row nothing is launched and nothing is looked at.
static int llama_loop_run(tts_hip_ctx *c, const char *what, uint32_t n_steps) {
    const int rc = llama_loop_launch(c, what, n_steps);
    if (c->ls.in_flight) {
        const int rl = llama_loop_look(c, nullptr, nullptr, nullptr);
        return rc ? rc : rl;
    }
    llama_loop_live_rows(c);
    return rc;
}

// ---- the fixed batch: slots 0 .. n_utt-1, all admitted at begin; every utterance takes sp (NULL: sampler::max) and its row of uniforms [n_utt][max_new] ----
static int llama_gen_begin_rows(tts_hip_ctx *c, const char *what, uint32_t n_utt, const uint32_t *prompts, const uint32_t *n_prompt, uint32_t max_new, uint32_t stop_id,
                                const tts_hip_sampling *sp, const float *uniforms) {
    auto &g = c->ls;
    if (!prompts || !n_prompt) return set_err("%s: null argument", what);
    if (n_utt == 0 || n_utt > c->lm.max_seqs) return set_err("%s: %u utterances outside 1..max_seqs = %u", what, n_utt, c->lm.max_seqs);
    HIPCHK(hipSetDevice(c->device));
    for (uint32_t u = 0; u < n_utt; u++) if (n_prompt[u] == 0 || n_prompt[u] >= c->lm.n_ctx) return set_err("%s: utterance %u: prompt of %u ids", what, u, n_prompt[u]);
    if (max_new != 0 && sp) {
        CHK(check_llama_sampling(c, sp, what));
        if (!uniforms) return set_err("%s: null uniforms", what);
    }
    CHK(llama_loop_begin(c, what, LS::BATCH, n_utt, max_new, stop_id, sp, false));
    size_t off = 0;
    for (uint32_t u = 0; u < n_utt; u++) {
        if (llama_loop_admit(c, what, u, prompts + off, n_prompt[u], sp, sp ? uniforms + (size_t) u * max_new : nullptr) != 0) { g.mode = LS::NONE; return -1; }
        off += n_prompt[u];
    }
    llama_loop_live_rows(c);
    return 0;
}

// each utterance's ids since the last wait, from the device token buffer -> tokens_out [n_utt][max_new]
static int llama_gen_wait_rows(tts_hip_ctx *c, uint32_t *tokens_out, uint32_t *n_out, uint8_t *done) {
    auto &g = c->ls;
    for (uint32_t u = 0; u < g.n_slots; u++) {
        const size_t at = (size_t) u * g.max_new + g.handed[u];
        if (g.count[u] > g.handed[u]) HIPCHK(hipMemcpyAsync(tokens_out + at, g.tokens + at, (size_t) (g.count[u] - g.handed[u]) * 4, hipMemcpyDeviceToHost, c->stream));
        g.handed[u] = n_out[u] = g.count[u];
        if (done) done[u] = g.slot[u] != LS::LIVE;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int tts_hip_orpheus_generate_batch(tts_hip_ctx *c, uint32_t n_utt, const uint32_t *prompts, const uint32_t *n_prompt, uint32_t max_new, uint32_t stop_id,
                                              const tts_hip_sampling *sp, const float *uniforms, uint32_t *tokens_out, uint32_t *n_out) {
    const char *what = "tts_hip_orpheus_generate_batch";
    CHK(llama_gen_ready(c, what));
    if (!prompts || !n_prompt || !tokens_out || !n_out) return set_err("%s: null argument", what);
    for (uint32_t u = 0; u < n_utt && u < c->lm.max_seqs; u++) n_out[u] = 0;
    c->lg.active = false;
    llama_batch_drop(c);
    CHK(llama_gen_begin_rows(c, what, n_utt, prompts, n_prompt, max_new, stop_id, sp, uniforms));
    int rc = 0;
    while (rc == 0 && !c->ls.rows.empty()) rc = llama_loop_run(c, what, c->l_batch_run);
    if (rc == 0 && max_new) rc = llama_gen_wait_rows(c, tokens_out, n_out, nullptr);
    c->ls.mode = LS::NONE;
    return rc;
}

extern "C" int tts_hip_orpheus_gen_begin(tts_hip_ctx *c, uint32_t n_utt, const uint32_t *prompts, const uint32_t *n_prompt, uint32_t max_new, uint32_t stop_id,
                                         const tts_hip_sampling *sp, const float *uniforms) {
    const char *what = "tts_hip_orpheus_gen_begin";
    CHK(llama_gen_ready(c, what));
    c->lg.active = false;
    llama_batch_drop(c);
    if (!prompts || !n_prompt) return set_err("%s: null argument", what);
    if (n_utt == 1) return llama_gen_begin_one(c, what, prompts, n_prompt[0], max_new, stop_id, sp, uniforms);
    return llama_gen_begin_rows(c, what, n_utt, prompts, n_prompt, max_new, stop_id, sp, uniforms);
}

// blocking for a batch (the run ends with its look-in), asynchronous for one sequence
extern "C" int tts_hip_orpheus_gen_launch(tts_hip_ctx *c, uint32_t n_steps) {
    const char *what = "tts_hip_orpheus_gen_launch";
    CHK(llama_gen_ready(c, what));
    if (c->ls.mode == LS::BATCH) return llama_loop_run(c, what, n_steps);
    if (!c->lg.active) return set_err("%s: no generation (tts_hip_orpheus_gen_begin)", what);
    HIPCHK(hipSetDevice(c->device));
    return llama_gen_launch_one(c, what, n_steps);
}

extern "C" int tts_hip_orpheus_gen_wait(tts_hip_ctx *c, uint32_t *tokens_out, uint32_t *n_out, uint8_t *done) {
    const char *what = "tts_hip_orpheus_gen_wait";
    CHK(llama_gen_ready(c, what, true));
    const bool batch = c->ls.mode == LS::BATCH;
    if (!batch && !c->lg.active) return set_err("%s: no generation (tts_hip_orpheus_gen_begin)", what);
    if (!tokens_out || !n_out) return set_err("%s: null argument", what);
    HIPCHK(hipSetDevice(c->device));
    if (batch) return llama_gen_wait_rows(c, tokens_out, n_out, done);
    CHK(llama_gen_wait_one(c));
    llama_gen_hand_one(c, tokens_out, n_out, done);
    return 0;
}

// ---- the continuous session ----
// mixed: every admission brings its utterances' samplers (sp is NULL); otherwise every admission takes sp
static int llama_stream_begin(tts_hip_ctx *c, const char *what, uint32_t n_slots, uint32_t max_new, uint32_t stop_id, const tts_hip_sampling *sp, bool mixed) {
    CHK(llama_stream_ready(c, what, false));
    CHK(llama_gen_idle(c, what));   // an open session or the window between a gen_launch and its gen_wait
    if ((c->lg.active && !c->lg.done) || (c->ls.mode == LS::BATCH && !c->ls.rows.empty())) return set_err("%s: a tts_hip_orpheus_gen_* generation is under way", what);
    if (n_slots == 0 || n_slots > c->lm.max_seqs) return set_err("%s: %u slots outside 1..max_seqs = %u", what, n_slots, c->lm.max_seqs);
    if (sp) CHK(check_llama_sampling(c, sp, what));
    HIPCHK(hipSetDevice(c->device));
    c->lg.active = false;
    c->ls.mode = LS::NONE;
    return llama_loop_begin(c, what, LS::SESSION, n_slots, max_new, stop_id, sp, mixed);
}

extern "C" int tts_hip_orpheus_stream_begin(tts_hip_ctx *c, uint32_t n_slots, uint32_t max_new, uint32_t stop_id, const tts_hip_sampling *sp) {
    return llama_stream_begin(c, "tts_hip_orpheus_stream_begin", n_slots, max_new, stop_id, sp, false);
}
extern "C" int tts_hip_orpheus_stream_begin_mixed(tts_hip_ctx *c, uint32_t n_slots, uint32_t max_new, uint32_t stop_id) {
    return llama_stream_begin(c, "tts_hip_orpheus_stream_begin_mixed", n_slots, max_new, stop_id, nullptr, true);
}

// sampling (mixed session only): utterance i's sampler, NULL = sampler::max
static int llama_stream_admit(tts_hip_ctx *c, const char *what, bool mixed, uint32_t n, const uint32_t *slots, const uint32_t *prompts, const uint32_t *n_prompt,
                              const tts_hip_sampling *const *sampling, const float *uniforms) {
    CHK(llama_stream_ready(c, what));
    auto &g = c->ls;
    if (mixed != g.mixed)
        return set_err(g.mixed ? "%s: the session carries a sampler per slot (tts_hip_orpheus_stream_admit_mixed)" : "%s: the session has one sampler (tts_hip_orpheus_stream_admit)", what);
    CHK(g.idle(what, LLAMA_WAIT));
    if (n == 0) return 0;
    if (!slots || !prompts || !n_prompt) return set_err("%s: null argument", what);
    if (g.sampled && !uniforms) return set_err("%s: a sampled session needs the utterances' uniforms [n][max_new]", what);
    if (mixed) {
        if (!sampling) return set_err("%s: null argument", what);
        for (uint32_t i = 0; i < n; i++) {
            if (!sampling[i]) continue;
            CHK(check_llama_sampling(c, sampling[i], what));
            if (!uniforms) return set_err("%s: a sampled utterance needs the uniforms [n][max_new]", what);
        }
    }
    CHK(g.check_list(what, n, slots, LS::ADMIT));
    size_t off = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (n_prompt[i] == 0 || n_prompt[i] >= c->lm.n_ctx) return set_err("%s: utterance %u: a prompt of %u ids does not fit %u cached positions", what, i, n_prompt[i], c->lm.n_ctx);
        for (uint32_t j = 0; j < n_prompt[i]; j++)
            if (prompts[off + j] >= (uint32_t) c->l_V) return set_err("%s: token id %u >= vocabulary %d", what, prompts[off + j], c->l_V);
        off += n_prompt[i];
    }
    HIPCHK(hipSetDevice(c->device));
    off = 0;
    for (uint32_t i = 0; i < n; i++) {
        const tts_hip_sampling *sp = sampling ? sampling[i] : (g.sampled ? &g.sp : nullptr);   // the one sampler of a session that is not mixed, in every slot's record
        CHK(llama_loop_admit(c, what, slots[i], prompts + off, n_prompt[i], sp, sp ? uniforms + (size_t) i * g.max_new : nullptr));
        off += n_prompt[i];
    }
    llama_loop_live_rows(c);
    return 0;
}

extern "C" int tts_hip_orpheus_stream_admit(tts_hip_ctx *c, uint32_t n, const uint32_t *slots, const uint32_t *prompts, const uint32_t *n_prompt, const float *uniforms) {
    return llama_stream_admit(c, "tts_hip_orpheus_stream_admit", false, n, slots, prompts, n_prompt, nullptr, uniforms);
}
extern "C" int tts_hip_orpheus_stream_admit_mixed(tts_hip_ctx *c, uint32_t n, const uint32_t *slots, const uint32_t *prompts, const uint32_t *n_prompt,
                                                  const tts_hip_sampling *const *sampling, const float *uniforms) {
    return llama_stream_admit(c, "tts_hip_orpheus_stream_admit_mixed", true, n, slots, prompts, n_prompt, sampling, uniforms);
}

extern "C" int tts_hip_orpheus_stream_launch(tts_hip_ctx *c, uint32_t n_steps) {
    const char *what = "tts_hip_orpheus_stream_launch";
    CHK(llama_stream_ready(c, what));
    CHK(c->ls.idle(what, LLAMA_WAIT));
    return llama_loop_launch(c, what, n_steps);
}

// a look-in, then the slots it or an earlier one saw finished and no call has reported yet
extern "C" int tts_hip_orpheus_stream_wait(tts_hip_ctx *c, uint32_t *tokens_out, uint32_t *n_out, uint8_t *done, uint32_t *n_finished, uint32_t *finished_slots,
                                           uint32_t *finished_counts) {
    const char *what = "tts_hip_orpheus_stream_wait";
    CHK(llama_stream_ready(c, what));
    if (!n_finished || !finished_slots || !finished_counts) return set_err("%s: null argument", what);
    *n_finished = 0;
    CHK(llama_loop_look(c, tokens_out, n_out, done));
    c->ls.report(c->ls.count, n_finished, finished_slots, finished_counts);
    return 0;
}

// launch + a wait that takes nothing + the report
extern "C" int tts_hip_orpheus_stream_run(tts_hip_ctx *c, uint32_t n_steps, uint32_t *n_finished, uint32_t *finished_slots, uint32_t *finished_counts) {
    const char *what = "tts_hip_orpheus_stream_run";
    CHK(llama_stream_ready(c, what));
    if (!n_finished || !finished_slots || !finished_counts) return set_err("%s: null argument", what);
    *n_finished = 0;
    CHK(c->ls.idle(what, LLAMA_WAIT));
    CHK(llama_loop_run(c, what, n_steps));
    c->ls.report(c->ls.count, n_finished, finished_slots, finished_counts);
    return 0;
}

// Live slots leave the session without a report.  The rows of a run are staged from the host's state, so nothing is launched: the slot is gone from
// the next run's rows, and what it left on the device is rewritten by the next admission.
extern "C" int tts_hip_orpheus_stream_drop(tts_hip_ctx *c, uint32_t n, const uint32_t *slots) {
    const char *what = "tts_hip_orpheus_stream_drop";
    CHK(llama_stream_ready(c, what));
    auto &g = c->ls;
    CHK(g.idle(what, LLAMA_WAIT));
    if (n == 0) return 0;
    if (!slots) return set_err("%s: null argument", what);
    CHK(g.check_list(what, n, slots, LS::DROP));
    for (uint32_t i = 0; i < n; i++) g.slot[slots[i]] = LS::FREE;
    llama_loop_live_rows(c);
    return 0;
}

extern "C" int tts_hip_orpheus_stream_collect(tts_hip_ctx *c, uint32_t slot, uint32_t count, uint32_t *tokens_out) {
    const char *what = "tts_hip_orpheus_stream_collect";
    CHK(llama_stream_ready(c, what));
    auto &g = c->ls;
    CHK(g.idle(what, LLAMA_WAIT));
    CHK(g.check_collect(what, slot, count, g.count, LLAMA_RUN, "produced", "ids"));
    if (count == 0) return 0;
    if (!tokens_out) return set_err("%s: null argument", what);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(tokens_out, g.tokens + (size_t) slot * g.max_new, (size_t) count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// leaves the loop; its buffers stay for the next one
extern "C" int tts_hip_orpheus_stream_end(tts_hip_ctx *c) {
    if (!c || !c->has_llama) return set_err("tts_hip_orpheus_stream_end: not an Orpheus context (tts_hip_orpheus_create)");
    if (c->ls.mode != LS::SESSION) return 0;
    (void) hipSetDevice(c->device);
    (void) hipStreamSynchronize(c->stream);   // also the steps of a launch nobody waited for
    c->ls.in_flight = 0;
    c->ls.mode = LS::NONE;
    return 0;
}

// the selection of the rows kernels on n_rows rows of caller-supplied logits; row r selects with at(r) (NULL: sampler::max)
template <typename At>
static int llama_sample_rows(tts_hip_ctx *c, const char *what, uint32_t n_rows, const float *logits, At at, const float *uniforms, int32_t *last_id, uint32_t *rep_count,
                             uint32_t *tokens_out) {
    CHK(llama_gen_idle(c, what));
    if (n_rows == 0 || n_rows > c->lm.max_seqs) return set_err("%s: %u rows outside 1..max_seqs = %u", what, n_rows, c->lm.max_seqs);
    bool any_max = false, any_sample = false, any_nucleus = false;
    uint32_t mx = 0;
    auto rep = [&](uint32_t r) { return at(r) && at(r)->repetition_penalty != 1.0f; };
    for (uint32_t r = 0; r < n_rows; r++) {
        const tts_hip_sampling *sp = at(r);
        if (!sp) { any_max = true; continue; }
        CHK(check_llama_sampling(c, sp, what));
        if (!uniforms) return set_err("%s: null uniforms", what);
        if (rep(r) && (!last_id || !rep_count)) return set_err("%s: repetition penalty needs last_id and rep_count", what);
        any_sample = true; any_nucleus |= sp->top_p < 1.0f;
        if (rep(r)) mx = std::max(mx, rep_count[r]);
    }
    HIPCHK(hipSetDevice(c->device));
    const int len = (int) std::min<uint32_t>(mx + 2, 1u << 20) + 1;   // what stage_penalty builds for the one-row call
    std::vector<llama_slot_sampler> rec(n_rows);
    std::vector<double> table((size_t) n_rows * len);
    std::vector<uint32_t> init((size_t) 3 * n_rows);
    for (uint32_t r = 0; r < n_rows; r++) {
        llama_slot_sampler_host(at(r), len, &rec[r], table.data() + (size_t) r * len);
        init[3 * r] = rep(r) ? (uint32_t) last_id[r] : 0xFFFFFFFFu; init[3 * r + 1] = rep(r) ? rep_count[r] : 0u; init[3 * r + 2] = 0u;
    }
    uint32_t *smp = nullptr;
    float *uni = nullptr, *total = nullptr;
    unsigned long long *cand = nullptr;
    llama_slot_sampler *samp = nullptr;
    double *pen = nullptr;
    auto drop = [&](int rc) { free_dev(smp); free_dev(uni); free_dev(total); free_dev(cand); free_dev(samp); free_dev(pen); return rc; };
    int rc = dmalloc(&smp, (size_t) 3 * n_rows);
    if (rc == 0) rc = dmalloc(&uni, (size_t) n_rows);
    if (rc == 0) rc = dmalloc(&total, (size_t) n_rows);
    if (rc == 0) rc = dmalloc(&samp, (size_t) n_rows);
    if (rc == 0) rc = dmalloc(&pen, table.size());
    if (rc == 0 && hipMalloc((void **) &cand, (size_t) n_rows * TOPK_PARTS * TOPK_MAXK * 8) != hipSuccess) rc = set_err("%s: out of device memory", what);
    if (rc != 0) return drop(rc);
    if (hipMemcpy(smp, init.data(), init.size() * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(samp, rec.data(), rec.size() * sizeof(rec[0]), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(pen, table.data(), table.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
        (uniforms && hipMemcpy(uni, uniforms, (size_t) n_rows * 4, hipMemcpyHostToDevice) != hipSuccess))
        return drop(set_err("%s: copy failed", what));
    if (hipMemcpy2DAsync(c->l_logits, (size_t) c->l_Vpad * 4, logits, (size_t) c->l_V * 4, (size_t) c->l_V * 4, n_rows, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return drop(set_err("%s: copy failed", what));
    if (llama_select_slots(c, any_max, any_sample, any_nucleus, (int) n_rows, c->l_logits, nullptr, 0, nullptr, samp, pen, len, smp, uni, 1, cand, total) != 0) return drop(-1);
    std::vector<uint32_t> back((size_t) 3 * n_rows);
    bool ok = hipMemcpyAsync(tokens_out, c->l_btok, (size_t) n_rows * 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(back.data(), smp, back.size() * 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    ok = hipStreamSynchronize(c->stream) == hipSuccess && ok;
    if (!ok) return drop(set_err("%s: copy failed", what));
    for (uint32_t r = 0; r < n_rows; r++) if (rep(r)) { last_id[r] = (int32_t) back[3 * r]; rep_count[r] = back[3 * r + 1]; }
    return drop(0);
}

// one setting for all rows: the per-row entry with sp repeated
extern "C" int tts_hip_orpheus_sample_logits_rows(tts_hip_ctx *c, uint32_t n_rows, const float *logits, const tts_hip_sampling *sp, const float *uniforms, int32_t *last_id,
                                                  uint32_t *rep_count, uint32_t *tokens_out) {
    const char *what = "tts_hip_orpheus_sample_logits_rows";
    CHK(llama_stream_ready(c, what, false));
    if (!logits || !tokens_out) return set_err("%s: null argument", what);
    return llama_sample_rows(c, what, n_rows, logits, [&](uint32_t) { return sp; }, uniforms, last_id, rep_count, tokens_out);
}

extern "C" int tts_hip_orpheus_sample_logits_rows_mixed(tts_hip_ctx *c, uint32_t n_rows, const float *logits, const tts_hip_sampling *const *sampling, const float *uniforms,
                                                        int32_t *last_id, uint32_t *rep_count, uint32_t *tokens_out) {
    const char *what = "tts_hip_orpheus_sample_logits_rows_mixed";
    CHK(llama_stream_ready(c, what, false));
    if (!logits || !tokens_out || !sampling) return set_err("%s: null argument", what);
    return llama_sample_rows(c, what, n_rows, logits, [&](uint32_t r) { return sampling[r]; }, uniforms, last_id, rep_count, tokens_out);
}

// ------------------------------------------------------------------------------------------------
// Dia (src/models/dia/model.cpp:383-659)
// ------------------------------------------------------------------------------------------------

extern "C" tts_hip_ctx *tts_hip_dia_create(int device, const tts_hip_dia_desc *dd) {
    if (!dd || dd->struct_size != sizeof(tts_hip_dia_desc)) { set_err("tts_hip_dia_create: bad desc (struct_size mismatch)"); return nullptr; }
    if (refuse_kv_f16(dd->flags, "tts_hip_dia_create")) return nullptr;
    if (dd->kv_type != TTS_HIP_F32 && dd->kv_type != TTS_HIP_F16) {
        set_err("tts_hip_dia_create: kv_type %u is neither TTS_HIP_F32 (0) nor TTS_HIP_F16 (1)", dd->kv_type);
        return nullptr;
    }
    // two guidance rows per utterance, RMAX = 256 rows per forward
    if (dd->max_utterances > (uint32_t) DIA_MAX_UTTERANCES) {
        set_err("tts_hip_dia_create: max_utterances %u > %d (one decoder forward carries %d rows, two per utterance)", dd->max_utterances, (int) DIA_MAX_UTTERANCES, 2 * (int) DIA_MAX_UTTERANCES);
        return nullptr;
    }
    tts_hip_desc d{};
    d.struct_size = sizeof(d);
    d.hidden_size = dd->dec_hidden_size; d.n_layers = dd->dec_layers; d.n_attn_heads = dd->dec_attn_heads; d.max_ctx_length = dd->max_gen;
    d.max_seqs = 1;
    // TTS_HIP_FLAG_NO_GRAPH reaches dia_loop_launch: the loop's steps then run eagerly instead of as replays of one captured graph
    d.flags = (dd->flags & (TTS_HIP_FLAG_VALU_GEMM | TTS_HIP_FLAG_DEQUANT_Q | TTS_HIP_FLAG_NO_GRAPH)) | TTS_HIP_FLAG_NO_PARLER | TTS_HIP_FLAG_NO_DAC;
    tts_hip_ctx *c = tts_hip_create(device, &d);
    if (!c) return nullptr;
    c->has_dia = true;
    c->dia = *dd;
    if (dd->kv_type == TTS_HIP_F16) c->di_kv_esz = 2;
    if (c->dia.cfg_scale == 0.0f) c->dia.cfg_scale = 3.0f;
    // up to 64 slots: every step launches what it always launched.  65 .. 128: the steps of more than 16 rows run fp16 matrices on gemm_tile_kernel
    // (dia_forward_tiled); tune("dia_tile_min_rows") moves either default
    c->dia_tile_min_rows = dd->max_utterances > 64 ? 17 : 0;
    return c;
}

// rows in pieces of RMAX (the activation-quantisation scratch holds RMAX rows); ksplit > 1 only with n <= RMAX
static int dia_gemm(tts_hip_ctx *c, const W &w, const float *A, int lda, float *out, int ldo, int n, int epi, int ksplit = 1) {
    if (ksplit > 1 && n > c->RMAX) return set_err("dia_gemm: split-K needs all rows in one piece");
    for (int r0 = 0; r0 < n; r0 += c->RMAX) {
        GemmArgs g{};
        g.R = std::min(c->RMAX, n - r0); g.H = c->H;
        g.A = A + (size_t) r0 * lda; g.lda = lda;
        g.out = out + (size_t) r0 * ldo; g.ldo = ldo;
        if (ksplit > 1) {
            g.kchunk = (int) w.K / ksplit;
            g.slab_stride = (int64_t) c->RMAX * ldo;
        }
        CHK(run_gemm(c, TTS_HIP_K_GEMM_OTHER, w, g, PRO_F32, epi));
    }
    return 0;
}

// the encoder's GEMMs (2 x max_ctx rows): fp16 matrices take gemm_tile_kernel with all rows in one launch — the activations are rounded
// to fp16 once (what ggml_mul_mat does with them for an F16 weight), every matrix leaves HBM once instead of once per RMAX rows
static int dia_gemm_rows(tts_hip_ctx *c, const W &w, const float *A, int lda, float *out, int ldo, int n, int epi) {
    if (w.type != TTS_HIP_F16 || c->tile_min_rows <= 0 || n < c->tile_min_rows || w.K % 128 || w.N % 16 || (c->d.flags & TTS_HIP_FLAG_VALU_GEMM) || c->prof)
        return dia_gemm(c, w, A, lda, out, ldo, n, epi);
    const int64_t n8 = (int64_t) n * (int64_t) (w.K / 8);
    hipLaunchKernelGGL(rows_to_f16_kernel, dim3((unsigned) ((n8 + 255) / 256)), dim3(256), 0, c->stream, A, lda, (int) w.K, n8, c->di_e16);
    HIPCHK(hipGetLastError());
    GemmArgs g{};
    g.R = n; g.H = c->H;
    g.A = c->di_e16; g.lda = (int) w.K;
    g.out = out; g.ldo = ldo;
    return run_gemm(c, TTS_HIP_K_GEMM_OTHER, w, g, PRO_F16, epi);
}

// <= 16 rows through gemv_stream_kernel: `out` receives *slabs K-slice slabs 16 * ldo floats apart (the consumer folds them);
// *slabs = 0: the shape does not qualify and nothing was launched
// pro: PRO_F32 (A = fp32 rows), PRO_ATTN8 (A unused: the eight key slices in c->attn_part are merged while the rows are staged) or PRO_SILU (A = the
// gate | up rows [n][2 K] as in_parts slabs in_stride floats apart: silu(gate) * up while staged); the last two need stream_fold_ok()
static int dia_gemm_stream(tts_hip_ctx *c, const W &w, const float *A, int lda, float *out, int ldo, int n, int max_slabs, int64_t slab_stride, int *slabs,
                           int pro = PRO_F32, int in_parts = 1, int64_t in_stride = 0) {
    const int ks = stream_slices(c, w, n, max_slabs);
    *slabs = ks;
    if (!ks) return pro == PRO_F32 ? 0 : set_err("dia_gemm_stream: a folding prologue was promised to a shape the streaming kernel does not take");
    GemmArgs g{};
    g.R = n; g.H = c->H;
    g.A = A; g.lda = lda;
    g.out = out; g.ldo = ldo;
    g.stream = 1;
    g.kchunk = ks > 1 ? (int) w.K / ks : 0;
    g.slab_stride = slab_stride;
    if (pro == PRO_ATTN8) g.att_part = c->attn_part;
    if (pro == PRO_SILU) { g.n_parts = std::max(in_parts, 1); g.parts_stride = in_stride; }
    return run_gemm(c, TTS_HIP_K_GEMM_OTHER, w, g, pro, EPI_STORE);
}

static int dia_rms(tts_hip_ctx *c, size_t w_off, int rows, int H, float *x, float *y, bool fold) {
    const int pend = fold ? c->di_pending : 0;
    c->di_pending_max = std::max(c->di_pending_max, pend);
    hipLaunchKernelGGL(rms_fold_rows_kernel, dim3(rows), dim3(256), 0, c->stream, x, H, (const float *) (c->arena + w_off), y, rows, 1e-5f,
                       pend ? (const float *) c->di_parts : (const float *) nullptr, pend, (int64_t) c->RMAX * H, (int8_t *) nullptr, (float *) nullptr);
    if (fold) c->di_pending = 0;
    return hipGetLastError() == hipSuccess ? 0 : set_err("rms_fold_rows_kernel launch failed");
}

typedef tts_hip_ctx::DiaLoop DL;
static int dia_loop_end(tts_hip_ctx *c);
static int dia_encode_into(tts_hip_ctx *c, uint32_t slot, const uint32_t *tokens, uint32_t sentence_len, float *enc_out);

// between tts_hip_dia_stream_begin and _end the loop state, the cross extents and the slots belong to the session
static int dia_no_session(const tts_hip_ctx *c, const char *what) {
    return c->dl.mode == DL::SESSION ? set_err("%s: a continuous session is open on this context (tts_hip_dia_stream_end)", what) : 0;
}

extern "C" int tts_hip_dia_encode_slot(tts_hip_ctx *c, uint32_t slot, const uint32_t *tokens, uint32_t sentence_len, float *enc_out) {
    if (!c || !c->has_dia) return set_err("tts_hip_dia_encode: not a Dia context (tts_hip_dia_create)");
    CHK(dia_no_session(c, "tts_hip_dia_encode"));
    if (slot >= (uint32_t) c->di_U) return set_err("tts_hip_dia_encode_slot: slot %u outside the %d utterance slots of this context (max_utterances)", slot, c->di_U);
    if (!c->finalized || !c->weights_present) return set_err("tts_hip_dia_encode: context not finalized");
    if (!tokens) return set_err("tts_hip_dia_encode: null argument");
    const int S = (int) c->dia.max_ctx;
    if (sentence_len == 0 || sentence_len > (uint32_t) S) return set_err("tts_hip_dia_encode: sentence length %u outside 1..%d", sentence_len, S);
    for (int t = 0; t < S; t++)
        if (tokens[t] >= (uint32_t) c->di_evocab) return set_err("tts_hip_dia_encode: token %u >= encoder vocabulary %d", tokens[t], c->di_evocab);
    CHK(dia_loop_end(c));   // an unfinished tts_hip_dia_gen_* loop is waited for and dropped
    return dia_encode_into(c, slot, tokens, sentence_len, enc_out);
}

// the encoder pass and the cross K/V fill of one slot; the arguments have been checked (tts_hip_dia_encode_slot, tts_hip_dia_stream_admit)
static int dia_encode_into(tts_hip_ctx *c, uint32_t slot, const uint32_t *tokens, uint32_t sentence_len, float *enc_out) {
    const int S = (int) c->dia.max_ctx, EH = c->di_EH, EF = c->di_EF, A = c->di_A, HD = (int) c->dia.head_dim, ENH = (int) c->dia.enc_attn_heads;
    const int NH = c->NH, n = 2 * S;
    std::vector<uint32_t> tok((size_t) n, 0u), epos((size_t) n), eseq((size_t) n), kbeg((size_t) n), kend((size_t) n);
    for (int t = 0; t < S; t++) tok[(size_t) t] = tokens[t];
    for (int t = 0; t < n; t++) {   // set_inputs :712-721: real positions see real positions, pad positions see pad positions
        const uint32_t p = (uint32_t) (t % S);
        epos[(size_t) t] = p; eseq[(size_t) t] = (uint32_t) (t / S);
        kbeg[(size_t) t] = p < sentence_len ? 0u : sentence_len;
        kend[(size_t) t] = p < sentence_len ? sentence_len : (uint32_t) S;
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t nb = (size_t) n * 4;
    HIPCHK(hipMemcpyAsync(c->di_tok, tok.data(), nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->di_epos, epos.data(), nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->di_eseq, eseq.data(), nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->di_kbeg, kbeg.data(), nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->di_kend, kend.data(), nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // the vectors are locals
    auto f32 = [&](size_t off) { return (const float *) (c->arena + off); };
    const float theta_scale = powf(10000.0f, -2.0f / (float) HD);   // ggml_rope(..., head_size, 2): default base
    const size_t attn_lds = (size_t) (128 + S) * 4;
    CHK(attn_gqa_allow_lds<float>(c, attn_lds));   // the encoder's own K/V scratch is fp32
    hipLaunchKernelGGL(t5_embed_kernel, dim3(n), dim3(256), 0, c->stream, f32(c->di_enc_embd), (const uint32_t *) c->di_tok, EH, c->di_ex);
    HIPCHK(hipGetLastError());
    for (const auto &y : c->di_enc) {
        CHK(dia_rms(c, y.sa_norm, n, EH, c->di_ex, c->di_exn, false));
        CHK(dia_gemm_rows(c, y.qkv, c->di_exn, EH, c->di_eqkv, 3 * A, n, EPI_STORE));
        hipLaunchKernelGGL(llama_rope_kv_kernel<float>, dim3(n, 2 * ENH), dim3(64), 0, c->stream, c->di_eqkv, (const uint32_t *) c->di_epos, (const float *) nullptr, theta_scale,
                           ENH, ENH, HD, c->di_ek, c->di_ev, (const uint32_t *) c->di_eseq, (int64_t) S * A);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((attn_gqa_kernel<128, false, float>), dim3(ENH, n), dim3(256), attn_lds, c->stream, (const float *) c->di_eqkv, 3 * A, (const uint32_t *) c->di_epos,
                           (const float *) c->di_ek, (const float *) c->di_ev, ENH, ENH, 1.0f, c->di_eatt, (const uint32_t *) c->di_kbeg, (const uint32_t *) c->di_kend,
                           (const uint32_t *) c->di_eseq, (int64_t) S * A);
        HIPCHK(hipGetLastError());
        CHK(dia_gemm_rows(c, y.o, c->di_eatt, A, c->di_ex, EH, n, EPI_RESID));
        CHK(dia_rms(c, y.mlp_norm, n, EH, c->di_ex, c->di_exn, false));
        CHK(dia_gemm_rows(c, y.gu, c->di_exn, EH, c->di_egu, 2 * EF, n, EPI_STORE));
        hipLaunchKernelGGL(silu_mul_kernel, dim3((unsigned) (((size_t) n * EF + 255) / 256)), dim3(256), 0, c->stream, (const float *) c->di_egu, EF, n, c->di_eg, (int8_t *) nullptr, (float *) nullptr);
        HIPCHK(hipGetLastError());
        CHK(dia_gemm_rows(c, y.out, c->di_eg, EF, c->di_ex, EH, n, EPI_RESID));
    }
    CHK(dia_rms(c, c->di_enc_norm, n, EH, c->di_ex, c->di_exn, false));
    // cross K/V of every decoder layer (build_dia_cross_kv_store :505-541): V for all positions, K (rope'd with the encoder
    // positions) only for the sentence; the other K rows are zero as in the freshly cleared cache
    for (int l = 0; l < c->L; l++) {
        const auto &y = c->di_dec[(size_t) l];
        const size_t esz = (size_t) c->di_kv_esz, slot_off = ((size_t) l * c->di_U + slot) * n * A * esz;   // rows 2*slot, 2*slot+1
        char *ck = (char *) c->di_ck + slot_off, *cv = (char *) c->di_cv + slot_off;
        CHK(dia_gemm_rows(c, y.ckv, c->di_exn, EH, c->di_ckv, 2 * A, n, EPI_STORE));
        CHK(with_kv(c->di_kv_esz, ck, cv, [&](auto *k, auto *v) -> int {   // an fp16 cache: the same rotation, K and V rounded once as they are stored
            hipLaunchKernelGGL(llama_rope_kv_kernel<kv_of<decltype(k)>>, dim3(n, NH), dim3(64), 0, c->stream, c->di_ckv, (const uint32_t *) c->di_epos,
                               (const float *) nullptr, theta_scale, 0, NH, HD, k, v, (const uint32_t *) c->di_eseq, (int64_t) S * A);
            HIPCHK(hipGetLastError());
            return 0;
        }));
        if ((int) sentence_len < S)
            for (int b = 0; b < 2; b++)
                HIPCHK(hipMemsetAsync(ck + ((size_t) b * S + sentence_len) * A * esz, 0, (size_t) (S - (int) sentence_len) * A * esz, c->stream));
    }
    if (enc_out) HIPCHK(hipMemcpyAsync(enc_out, c->di_exn, (size_t) n * EH * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->di_slot_encoded[slot] = 1;
    return 0;
}

extern "C" int tts_hip_dia_encode(tts_hip_ctx *c, const uint32_t *tokens, uint32_t sentence_len, float *enc_out) {
    return tts_hip_dia_encode_slot(c, 0, tokens, sentence_len, enc_out);
}

// tts_hip_set_debug on an eager step: the query buffer an attention launch was handed (self: the rotated [R][ld] rows; cross: the raw slabs the kernel
// folds and rotates itself), the rows it left in di_att, and the extents it read, copied to the host table tts_hip_debug_read serves
// ("di_attn:<layer>:<self|cross>:<q|out|meta>").  meta: n_parts, part_stride, ld, R, then pos[R], kend[R], row_seq[R].
static int dia_attn_snapshot(tts_hip_ctx *c, int layer, bool cross, const float *q, int ld, int n_parts, int64_t part_stride, int R, int A, const uint32_t *kend) {
    HIPCHK(hipStreamSynchronize(c->stream));
    auto &s = c->dia_attn_dbg[layer * 2 + (cross ? 1 : 0)];
    s.q.resize((size_t) (n_parts - 1) * (size_t) part_stride + (size_t) R * ld);
    s.out.resize((size_t) R * A);
    std::vector<uint32_t> u((size_t) 3 * R);
    HIPCHK(hipMemcpy(s.q.data(), q, s.q.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(s.out.data(), c->di_att, s.out.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(u.data(), c->di_pos, (size_t) R * 4, hipMemcpyDeviceToHost));
    if (kend) HIPCHK(hipMemcpy(u.data() + R, kend, (size_t) R * 4, hipMemcpyDeviceToHost));
    else for (int r = 0; r < R; r++) u[(size_t) R + r] = u[(size_t) r] + 1;   // causal over the row's cache
    HIPCHK(hipMemcpy(u.data() + 2 * R, c->di_seq, (size_t) R * 4, hipMemcpyDeviceToHost));
    s.meta.assign({(float) n_parts, (float) part_stride, (float) ld, (float) R});
    for (uint32_t v : u) s.meta.push_back((float) v);
    return 0;
}

// ---- the tiled route: a decoder step of more than 16 rows with every matrix on gemm_tile_kernel -----------------------------------------------
// Whether a step of R rows takes it: fp16 matrices of tile shapes throughout, no TTS_HIP_FLAG_VALU_GEMM, and tune("dia_tile_min_rows") non-zero and at
// most R (0 on contexts of at most 64 slots, so those launch what they always launched; 17 on larger ones).  The rms producer holds a row of at most
// 2048 values in registers (Dia-1.6B's width; run_tile splits K up to that width too).
static bool dia_step_tiled(const tts_hip_ctx *c, int R) {
    if (R <= 16 || c->dia_tile_min_rows <= 0 || R < c->dia_tile_min_rows || (c->d.flags & TTS_HIP_FLAG_VALU_GEMM) || !c->di_h16 || c->H > 2048) return false;
    auto ok = [](const W &w) { return w.type == TTS_HIP_F16 && w.K % 128 == 0 && w.N % 16 == 0; };
    for (const auto &y : c->di_dec)
        for (const W *w : {&y.sqkv, &y.so, &y.cq, &y.co, &y.gu, &y.out})
            if (!ok(*w)) return false;
    return ok(c->di_heads);
}

// rms norm of the R rows of di_x, the pending slabs of di_parts folded in first, as the fp16 rows the next tiled GEMM reads (di_h16)
static int dia_rms_f16(tts_hip_ctx *c, size_t w_off, int R, int H) {
    const int pend = c->di_pending;
    c->di_pending_max = std::max(c->di_pending_max, pend);
    CHK(prof_begin(c, TTS_HIP_K_LN, (double) R * H * (6 + 4 * pend), 0));
    const float *w = (const float *) (c->arena + w_off), *parts = pend ? (const float *) c->di_parts : (const float *) nullptr;
    if (!dia_rows_rms_fold_f16(c->stream, c->di_x, H, w, c->di_h16, R, 1e-5f, parts, pend, (int64_t) c->RMAX * H)) return set_err("rms_fold_rows_f16_kernel launch failed");   // H <= 2048 (dia_step_tiled)
    c->di_pending = 0;
    return prof_end(c);
}

// one matrix over the fp16 rows in di_h16, all R rows in one launch; resid: onto di_x, K slices as slabs in di_parts where the cost model (or tile_ks) splits
static int dia_gemm_tile(tts_hip_ctx *c, int kclass, const W &w, float *out, int ldo, int R, bool resid) {
    GemmArgs g{};
    g.R = R; g.H = c->H;
    g.A = c->di_h16; g.lda = (int) w.K;
    g.out = out; g.ldo = ldo;
    return run_gemm_tile_f16(c, kclass, w, g, resid ? EPI_RESID : EPI_STORE, resid ? c->di_parts : (float *) nullptr, &c->di_pending);
}

// the attended rows (di_att, fp32) rounded to fp16 for the out projections
static int dia_att_f16(tts_hip_ctx *c, int R, int A) {
    const int64_t n8 = (int64_t) R * (A / 8);
    CHK(prof_begin(c, TTS_HIP_K_LN, (double) R * A * 6, 0));
    hipLaunchKernelGGL(rows_to_f16_kernel, dim3((unsigned) ((n8 + 255) / 256)), dim3(256), 0, c->stream, (const float *) c->di_att, A, A, n8, c->di_h16);
    HIPCHK(hipGetLastError());
    return prof_end(c);
}

// The layers, the final norm and the heads of dia_forward for a step dia_step_tiled() accepts (di_x holds the embedded rows).  Per layer: rms -> fp16,
// sqkv, rope + cache append, self attention, rows -> fp16, so (+ residual), rms -> fp16, cq, cross attention (the query arrives as one part and is
// rotated inside the kernel, as on the streaming route), rows -> fp16, co, rms -> fp16, gate|up, silu * up -> fp16, out.  so / co / out add into di_x
// in their epilogue or leave K-slice slabs in di_parts for the next rms (di_pending), the contract dia_rms has with the streaming route.  Both attention
// launches are launch_attn_gqa's, with nothing deferred.  Profiling classes: the GEMMs under their Parler names (qkv, attn_out, cross_q, cross_out,
// fc1 = gate|up, fc2 = out, heads), attn_self, attn_cross, and the row producers (rms, rows -> fp16, silu, rope) under "ln".
static int dia_forward_tiled(tts_hip_ctx *c, int U, int self_keys, bool fixed_split, bool snap) {
    const int S = (int) c->dia.max_ctx, G = (int) c->dia.max_gen, DH = c->H, DF = c->di_DF, A = c->di_A, kvH = c->di_kvH, HD = (int) c->dia.head_dim;
    const int NH = c->NH, NKV = (int) c->dia.dec_kv_heads, NO = c->NO, V = c->di_V, QKV = A + 2 * kvH;
    const int R = 2 * U, RS = 2 * c->di_U, kv_esz = c->di_kv_esz;
    const float theta_scale = powf(10000.0f, -2.0f / (float) HD);
    const uint32_t *nul = nullptr;
    const double kvb = (double) kv_esz;
    for (int l = 0; l < c->L; l++) {
        const auto &y = c->di_dec[(size_t) l];
        const size_t self_off = (size_t) l * RS * G * kvH * (size_t) kv_esz, cross_off = (size_t) l * RS * S * A * (size_t) kv_esz;
        char *kc = (char *) c->di_k + self_off, *vc = (char *) c->di_v + self_off, *ck = (char *) c->di_ck + cross_off, *cv = (char *) c->di_cv + cross_off;
        CHK(dia_rms_f16(c, y.sa_norm, R, DH));
        CHK(dia_gemm_tile(c, TTS_HIP_K_GEMM_QKV, y.sqkv, c->di_qkv, QKV, R, false));
        CHK(with_kv(kv_esz, kc, vc, [&](auto *k, auto *v) -> int {
            typedef kv_of<decltype(k)> KV;
            CHK(prof_begin(c, TTS_HIP_K_LN, (double) R * QKV * 8, 0));
            hipLaunchKernelGGL(llama_rope_kv_kernel<KV>, dim3(R, NH + NKV), dim3(64), 0, c->stream, c->di_qkv, (const uint32_t *) c->di_pos, (const float *) nullptr, theta_scale, NH,
                               NKV, HD, k, v, (const uint32_t *) c->di_seq, (int64_t) G * kvH, 1, (int64_t) 0);
            HIPCHK(hipGetLastError());
            CHK(prof_end(c));
            CHK(prof_begin(c, TTS_HIP_K_ATTN_SELF, (double) R * self_keys * 2 * kvH * kvb, 0));
            CHK(launch_attn_gqa<KV>(c, NH, R, self_keys, (const float *) c->di_qkv, QKV, (const uint32_t *) c->di_pos, k, v, NKV, 1.0f, c->di_att, nul, nul,
                                    (const uint32_t *) c->di_seq, (int64_t) G * kvH, fixed_split, false, QPre{}, nullptr, 0));
            return prof_end(c);
        }));
        if (snap) CHK(dia_attn_snapshot(c, l, false, c->di_qkv, QKV, 1, 0, R, A, nullptr));
        CHK(dia_att_f16(c, R, A));
        CHK(dia_gemm_tile(c, TTS_HIP_K_GEMM_ATTN_OUT, y.so, c->di_x, DH, R, true));
        CHK(dia_rms_f16(c, y.ca_norm, R, DH));
        CHK(dia_gemm_tile(c, TTS_HIP_K_GEMM_CROSS_Q, y.cq, c->di_q, A, R, false));
        QPre qp;   // one part; the rope of the cross-attention query happens as the attention workgroups load it
        qp.n_parts = 1; qp.part_stride = 0; qp.rope_pos = c->di_pos; qp.theta_scale = theta_scale;
        CHK(with_kv(kv_esz, ck, cv, [&](auto *k, auto *v) -> int {
            CHK(prof_begin(c, TTS_HIP_K_ATTN_CROSS, (double) R * S * 2 * A * kvb, 0));
            CHK(launch_attn_gqa<kv_of<decltype(k)>>(c, NH, R, S, (const float *) c->di_q, A, (const uint32_t *) c->di_pos, k, v, NH, 1.0f, c->di_att, nul,
                                                    (const uint32_t *) c->di_cend, (const uint32_t *) c->di_seq, (int64_t) S * A, false, false, qp, nullptr, S));
            return prof_end(c);
        }));
        if (snap) CHK(dia_attn_snapshot(c, l, true, c->di_q, A, 1, 0, R, A, c->di_cend));
        CHK(dia_att_f16(c, R, A));
        CHK(dia_gemm_tile(c, TTS_HIP_K_GEMM_CROSS_OUT, y.co, c->di_x, DH, R, true));
        CHK(dia_rms_f16(c, y.mlp_norm, R, DH));
        CHK(dia_gemm_tile(c, TTS_HIP_K_GEMM_FC1, y.gu, c->di_gu, 2 * DF, R, false));
        CHK(prof_begin(c, TTS_HIP_K_LN, (double) R * DF * 10, 0));
        if (!dia_rows_silu_mul_f16(c->stream, (const float *) c->di_gu, DF, R, c->di_h16)) return set_err("silu_mul_f16_kernel launch failed");
        CHK(prof_end(c));
        CHK(dia_gemm_tile(c, TTS_HIP_K_GEMM_FC2, y.out, c->di_x, DH, R, true));
    }
    CHK(dia_rms_f16(c, c->di_dec_norm, R, DH));
    CHK(dia_gemm_tile(c, TTS_HIP_K_GEMM_HEADS, c->di_heads, c->di_logits, c->di_Vpad, R, false));
    hipLaunchKernelGGL(dia_cfg_kernel, dim3((NO * V + 255) / 256, U), dim3(256), 0, c->stream, (const float *) c->di_logits, c->di_Vpad, NO * V, c->dia.cfg_scale, c->di_guided);
    HIPCHK(hipGetLastError());
    return 0;
}

// the decoder step for the U utterances whose input ids / positions / cache rows are in di_ids / di_pos / di_seq; leaves the guided
// logits in di_guided.  self_keys sizes the self-attention scratch; fixed_split: a captured step is replayed at every position, so the
// key-split count must not depend on it (the kernels read the true extent from di_pos)
static int dia_forward(tts_hip_ctx *c, int U, int self_keys, bool fixed_split, bool snap = false) {
    const int S = (int) c->dia.max_ctx, G = (int) c->dia.max_gen, DH = c->H, DF = c->di_DF, A = c->di_A, kvH = c->di_kvH, HD = (int) c->dia.head_dim;
    const int NH = c->NH, NKV = (int) c->dia.dec_kv_heads, NO = c->NO, V = c->di_V, QKV = A + 2 * kvH;
    const int R = 2 * U, RS = 2 * c->di_U, kv_esz = c->di_kv_esz;
    auto f32 = [&](size_t off) { return (const float *) (c->arena + off); };
    const float theta_scale = powf(10000.0f, -2.0f / (float) HD);
    const size_t attn_lds = (size_t) (128 + std::max(S, G)) * 4;
    CHK(kv_esz == 2 ? attn_gqa_allow_lds<_Float16>(c, attn_lds) : attn_gqa_allow_lds<float>(c, attn_lds));
    DiaEmbedArgs ea{};
    for (int i = 0; i < NO; i++) ea.table[i] = f32(c->di_embd[i]);
    ea.ids = c->di_ids; ea.n_out = NO; ea.H = DH; ea.x = c->di_x;
    hipLaunchKernelGGL(dia_embed_kernel, dim3((DH + 255) / 256, U), dim3(256), 0, c->stream, ea);
    HIPCHK(hipGetLastError());
    c->di_pending = 0;
    c->di_pending_max = 0;
    c->di_tiled = 0;
    if (dia_step_tiled(c, R)) {   // more than 16 rows, fp16 matrices, tune("dia_tile_min_rows") reached: every GEMM on gemm_tile_kernel
        const uint64_t before = c->tile_launches;
        CHK(dia_forward_tiled(c, U, self_keys, fixed_split, snap));
        c->di_tiled = (int) (c->tile_launches - before);
        return 0;
    }
    const uint32_t *nul = nullptr;
    for (int l = 0; l < c->L; l++) {
        const auto &y = c->di_dec[(size_t) l];
        const size_t self_off = (size_t) l * RS * G * kvH * (size_t) kv_esz, cross_off = (size_t) l * RS * S * A * (size_t) kv_esz;
        char *kc = (char *) c->di_k + self_off, *vc = (char *) c->di_v + self_off, *ck = (char *) c->di_ck + cross_off, *cv = (char *) c->di_cv + cross_off;   // fp32 or fp16 rows (with_kv)
        // every projection: gemv_stream_kernel slabs folded by its consumer when the step has <= 16 rows and fp16 matrices
        // (sl = slabs written, 0 = shape does not qualify -> gemm16_kernel as before)
        int sl = 0;
        const int64_t st16 = 16;   // slab stride in rows
        CHK(dia_rms(c, y.sa_norm, R, DH, c->di_x, c->di_xn, true));
        CHK(dia_gemm_stream(c, y.sqkv, c->di_xn, DH, c->di_qkv, QKV, R, DIA_STREAM_SLABS, st16 * QKV, &sl));
        if (!sl) CHK(dia_gemm(c, y.sqkv, c->di_xn, DH, c->di_qkv, QKV, R, EPI_STORE));
        int slices = 0;   // key slices the attention left unmerged for the projection's staging prologue (0: di_att holds the rows)
        CHK(with_kv(kv_esz, kc, vc, [&](auto *k, auto *v) -> int {   // an fp16 cache: the same slab fold and rotation, K and V rounded once as they are appended
            typedef kv_of<decltype(k)> KV;
            hipLaunchKernelGGL(llama_rope_kv_kernel<KV>, dim3(R, NH + NKV), dim3(64), 0, c->stream, c->di_qkv, (const uint32_t *) c->di_pos, (const float *) nullptr, theta_scale, NH,
                               NKV, HD, k, v, (const uint32_t *) c->di_seq, (int64_t) G * kvH, std::max(sl, 1), st16 * QKV);
            HIPCHK(hipGetLastError());
            return launch_attn_gqa<KV>(c, NH, R, self_keys, (const float *) c->di_qkv, QKV, (const uint32_t *) c->di_pos, k, v, NKV, 1.0f,
                                       c->di_att, nul, nul, (const uint32_t *) c->di_seq, (int64_t) G * kvH, fixed_split, false, QPre{},
                                       A % 128 == 0 && stream_fold_ok(c, y.so, R, DIA_STREAM_SLABS) ? &slices : nullptr, 0);
        }));
        if (snap) CHK(dia_attn_snapshot(c, l, false, c->di_qkv, QKV, 1, 0, R, A, nullptr));
        CHK(dia_gemm_stream(c, y.so, c->di_att, A, c->di_parts, DH, R, DIA_STREAM_SLABS, (int64_t) c->RMAX * DH, &sl, slices ? PRO_ATTN8 : PRO_F32));
        if (sl) c->di_pending = sl;
        else CHK(dia_gemm(c, y.so, c->di_att, A, c->di_x, DH, R, EPI_RESID));
        CHK(dia_rms(c, y.ca_norm, R, DH, c->di_x, c->di_xn, true));
        CHK(dia_gemm_stream(c, y.cq, c->di_xn, DH, c->di_q, A, R, DIA_STREAM_SLABS, st16 * A, &sl));
        if (!sl) CHK(dia_gemm(c, y.cq, c->di_xn, DH, c->di_q, A, R, EPI_STORE));
        QPre qp;   // slab fold + rope of the cross-attention query happen as the attention workgroups load it
        qp.n_parts = std::max(sl, 1); qp.part_stride = st16 * A; qp.rope_pos = c->di_pos; qp.theta_scale = theta_scale;
        slices = 0;
        CHK(with_kv(kv_esz, ck, cv, [&](auto *k, auto *v) -> int {
            return launch_attn_gqa<kv_of<decltype(k)>>(c, NH, R, S, (const float *) c->di_q, A, (const uint32_t *) c->di_pos, k, v, NH, 1.0f, c->di_att, nul,
                                                                       (const uint32_t *) c->di_cend, (const uint32_t *) c->di_seq, (int64_t) S * A, false, false, qp,
                                                                       A % 128 == 0 && stream_fold_ok(c, y.co, R, DIA_STREAM_SLABS) ? &slices : nullptr, S);
        }));
        if (snap) CHK(dia_attn_snapshot(c, l, true, c->di_q, A, qp.n_parts, qp.part_stride, R, A, c->di_cend));
        CHK(dia_gemm_stream(c, y.co, c->di_att, A, c->di_parts, DH, R, DIA_STREAM_SLABS, (int64_t) c->RMAX * DH, &sl, slices ? PRO_ATTN8 : PRO_F32));
        if (sl) c->di_pending = sl;
        else CHK(dia_gemm(c, y.co, c->di_att, A, c->di_x, DH, R, EPI_RESID));
        CHK(dia_rms(c, y.mlp_norm, R, DH, c->di_x, c->di_xn, true));
        CHK(dia_gemm_stream(c, y.gu, c->di_xn, DH, c->di_gu, 2 * DF, R, DIA_STREAM_SLABS, st16 * 2 * DF, &sl));
        if (!sl) CHK(dia_gemm(c, y.gu, c->di_xn, DH, c->di_gu, 2 * DF, R, EPI_STORE));
        if (c->attn_fold && !c->prof && !c->debug && std::max(sl, 1) <= 8 && stream_fold_ok(c, y.out, R, DIA_STREAM_SLABS)) {
            // silu(gate) * up while the down projection stages its rows: no launch of its own, di_g is not written
            CHK(dia_gemm_stream(c, y.out, c->di_gu, 2 * DF, c->di_parts, DH, R, DIA_STREAM_SLABS, (int64_t) c->RMAX * DH, &sl, PRO_SILU, std::max(sl, 1), st16 * 2 * DF));
        } else {
            hipLaunchKernelGGL(silu_mul_kernel, dim3((unsigned) (((size_t) R * DF + 255) / 256)), dim3(256), 0, c->stream, (const float *) c->di_gu, DF, R, c->di_g, (int8_t *) nullptr,
                               (float *) nullptr, std::max(sl, 1), st16 * 2 * DF);
            HIPCHK(hipGetLastError());
            CHK(dia_gemm_stream(c, y.out, c->di_g, DF, c->di_parts, DH, R, DIA_STREAM_SLABS, (int64_t) c->RMAX * DH, &sl));
        }
        if (sl) {
            c->di_pending = sl;
        } else if (c->di_ksplit > 1) {
            CHK(dia_gemm(c, y.out, c->di_g, DF, c->di_parts, DH, R, EPI_STORE, c->di_ksplit));
            c->di_pending = c->di_ksplit;
        } else {
            CHK(dia_gemm(c, y.out, c->di_g, DF, c->di_x, DH, R, EPI_RESID));
        }
    }
    CHK(dia_rms(c, c->di_dec_norm, R, DH, c->di_x, c->di_xn, true));
    GemmArgs g{};
    g.R = R; g.H = DH; g.A = c->di_xn; g.lda = DH; g.out = c->di_logits; g.ldo = c->di_Vpad;
    CHK(run_gemm(c, TTS_HIP_K_GEMM_HEADS, c->di_heads, g, PRO_F32, EPI_STORE));
    hipLaunchKernelGGL(dia_cfg_kernel, dim3((NO * V + 255) / 256, U), dim3(256), 0, c->stream, (const float *) c->di_logits, c->di_Vpad, NO * V, c->dia.cfg_scale, c->di_guided);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int tts_hip_dia_step_batch(tts_hip_ctx *c, uint32_t n_utt, const uint32_t *slots, const uint32_t *ids, const uint32_t *pos, float *logits_out,
                                      float *raw_out) {
    if (!c || !c->has_dia) return set_err("tts_hip_dia_step: not a Dia context (tts_hip_dia_create)");
    if (!c->finalized || !c->weights_present) return set_err("tts_hip_dia_step: context not finalized");
    if (!ids || !pos || !logits_out) return set_err("tts_hip_dia_step: null argument");
    CHK(dia_no_session(c, "tts_hip_dia_step"));
    if (n_utt == 0 || n_utt > (uint32_t) c->di_U) return set_err("tts_hip_dia_step_batch: %u utterances outside 1..%d (max_utterances)", n_utt, c->di_U);
    const int G = (int) c->dia.max_gen, NO = c->NO, V = c->di_V;
    const int U = (int) n_utt, R = 2 * U, RS = 2 * c->di_U;   // rows of this step, row slots of the caches
    uint32_t max_pos = 0;
    uint32_t *h_ids = c->h_di, *h_pos = c->h_di + (size_t) c->di_U * 16, *h_seq = h_pos + RS;
    for (int u = 0; u < U; u++) {
        const uint32_t slot = slots ? slots[u] : (uint32_t) u;
        if (slot >= (uint32_t) c->di_U) return set_err("tts_hip_dia_step_batch: slot %u outside the %d utterance slots", slot, c->di_U);
        if (!c->di_slot_encoded[slot]) return set_err("tts_hip_dia_step: tts_hip_dia_encode has not run%s", c->di_U > 1 ? " for this slot" : "");
        if (pos[u] >= (uint32_t) G) return set_err("tts_hip_dia_step: position %u outside the %d cached positions", pos[u], G);
        for (int i = 0; i < NO; i++) {
            if (ids[u * NO + i] >= (uint32_t) V) return set_err("tts_hip_dia_step: id %u >= output vocabulary %d", ids[u * NO + i], V);
            h_ids[u * NO + i] = ids[u * NO + i];
        }
        h_pos[2 * u] = h_pos[2 * u + 1] = pos[u];
        h_seq[2 * u] = 2 * slot; h_seq[2 * u + 1] = 2 * slot + 1;
        max_pos = std::max(max_pos, pos[u]);
    }
    CHK(dia_loop_end(c));   // an unfinished tts_hip_dia_gen_* loop is waited for and dropped
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->di_ids, h_ids, (size_t) U * NO * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->di_pos, h_pos, (size_t) R * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->di_seq, h_seq, (size_t) R * 4, hipMemcpyHostToDevice, c->stream));
    if (c->debug) c->dia_attn_dbg.clear();
    CHK(dia_forward(c, U, (int) max_pos + 1, false, c->debug));   // debug: the attention launches' inputs and outputs go to dia_attn_dbg (never under a capture: this step is eager)
    HIPCHK(hipMemcpyAsync(logits_out, c->di_guided, (size_t) U * NO * V * 4, hipMemcpyDeviceToHost, c->stream));
    if (raw_out)
        for (int b = 0; b < R; b++)
            HIPCHK(hipMemcpyAsync(raw_out + (size_t) b * NO * V, c->di_logits + (size_t) b * c->di_Vpad, (size_t) NO * V * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- the device loop (include/tts_hip.h; kernels in dia_kernels.h) ------------------------------------------------------------------------
// One loop under tts_hip_dia_gen_* / tts_hip_dia_generate (DiaLoop::BATCH) and tts_hip_dia_stream_* (DiaLoop::SESSION): every replay steps
// all 2 * n rows through the same dia_forward, so what a live slot computes does not depend on who else is live.  Budget, uniforms and the
// parked flag are device memory: an admission changes values, never the captured launches.  The modes differ in how slots become live
// (all at begin / by admission), in how many replays a launch may enqueue, and in what a look-in reports.
#define DIA_LOOP_CHUNK 16
static const int DIA_GRAPH_KEY = 9100001;   // + 1 for the session's graph, + 2 for the mixed session's
// which captured step and which DiaBaked entry a loop uses: 0 BATCH, 1 SESSION, 2 mixed SESSION
static int dia_graph_slot(const DL &g) { return g.mixed ? 2 : g.mode == DL::SESSION ? 1 : 0; }

// leaving the loop, whichever mode: steps in flight are waited for and dropped (encode / step / a new loop overwrite what they read), and
// the cross extent of every row is the whole text context again, as the other entry points expect (parking moved it to one key)
static int dia_loop_end(tts_hip_ctx *c) {
    if (c->dl.mode == DL::NONE) return 0;
    HIPCHK(hipSetDevice(c->device));
    const std::vector<uint32_t> cend((size_t) 2 * c->di_U, c->dia.max_ctx);
    HIPCHK(hipMemcpyAsync(c->di_cend, cend.data(), cend.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->dl = DL{};
    return 0;
}

static int dia_stream_ready(tts_hip_ctx *c, const char *what, bool need_session = true) {
    if (!c || !c->has_dia) return set_err("%s: not a Dia context (tts_hip_dia_create)", what);
    if (!c->finalized || !c->weights_present) return set_err("%s: context not finalized", what);
    if (need_session && c->dl.mode != DL::SESSION) return set_err("%s: no session (tts_hip_dia_stream_begin)", what);
    return 0;
}

// a session's launch must be followed by a wait (SlotLedger::idle): admit, collect, drop and a second launch find the state they read or write still moving
static const char *const DIA_WAIT = "tts_hip_dia_stream_wait", *const DIA_RUN = "tts_hip_dia_stream_run";

static DiaLoopArgs dia_loop_args(tts_hip_ctx *c) {
    const auto &g = c->dl;
    DiaLoopArgs la{};
    la.n_utt = (int) g.n; la.n_out = c->NO;
    la.bos = g.codes.bos; la.eos = g.codes.eos; la.pad = g.codes.pad; la.max_delay = g.codes.max_delay; la.max_gen = g.max_gen;
    for (int i = 0; i < 16; i++) la.delay_pattern[i] = g.codes.delay_pattern[i];
    la.ids = c->di_ids; la.pos = c->di_pos;
    la.delay = (int32_t *) c->di_loop; la.done = c->di_loop + c->di_U; la.call = c->di_loop + 2 * c->di_U;
    la.tok = c->di_stok; la.hist = c->di_hist;
    la.budget = c->di_sbud; la.steps = c->di_sbud + c->di_U; la.cend = c->di_cend;
    return la;
}

// pre-step, forward, guidance, sampler (parked slots sit out), post-step: what one replay of the captured graph runs
static int dia_loop_step(tts_hip_ctx *c, const DiaLoopArgs &la, bool captured) {
    const auto &g = c->dl;
    const int U = (int) g.n, NO = c->NO, V = c->di_V;
    hipLaunchKernelGGL(dia_loop_prestep_kernel, dim3((U + 63) / 64), dim3(64), 0, c->stream, la);
    HIPCHK(hipGetLastError());
    CHK(dia_forward(c, U, (int) c->dia.max_gen, captured));
    if (g.mixed) {   // one launch whatever the slots hold: every row reads its slot's record, greedy rows leave after sampler::max
        SampleArgs sa{};
        sa.logits = c->di_guided; sa.V = V; sa.n_out = NO; sa.R = U;
        sa.uniforms = c->d_uniforms; sa.row_step = la.call; sa.out = c->di_stok; sa.idle = la.done;
        sa.last_ids = c->d_last; sa.rep_counts = c->d_repc;
        sa.rows = (const SampleRow *) c->di_srec;
        hipLaunchKernelGGL(sample_kernel, dim3(NO, U), dim3(256), 0, c->stream, sa);
    } else if (g.sampled) {
        SampleArgs sa{};
        sa.logits = c->di_guided; sa.V = V; sa.n_out = NO; sa.R = U;
        sa.top_k = g.sp.top_k; sa.top_p = g.sp.top_p; sa.temperature = g.sp.temperature;
        sa.uniforms = c->d_uniforms; sa.row_step = la.call; sa.out = c->di_stok; sa.idle = la.done;
        if (g.rep) { sa.pen_table = c->d_pen; sa.pen_len = c->pen_len; sa.last_ids = c->d_last; sa.rep_counts = c->d_repc; }
        hipLaunchKernelGGL(sample_kernel, dim3(NO, U), dim3(256), 0, c->stream, sa);
    } else {
        hipLaunchKernelGGL(argmax_kernel, dim3(U * NO), dim3(256), 0, c->stream, (const float *) c->di_guided, V, c->di_stok);
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(dia_loop_poststep_kernel, dim3((U + 63) / 64), dim3(64), 0, c->stream, la);
    HIPCHK(hipGetLastError());
    return 0;
}

// what both begin calls ask of their arguments; `rows` names the n of the caller ("utterances", "slots")
static int dia_loop_check(tts_hip_ctx *c, const char *what, const char *rows, uint32_t n, uint32_t max_gen, const tts_hip_dia_codes *codes, const tts_hip_sampling *sp) {
    CHK(dia_stream_ready(c, what, false));
    if (!codes) return set_err("%s: null argument", what);
    CHK(dia_no_session(c, what));
    const int G = (int) c->dia.max_gen, V = c->di_V;
    if (n == 0 || n > (uint32_t) c->di_U) return set_err("%s: %u %s outside 1..%d (max_utterances)", what, n, rows, c->di_U);
    if (max_gen == 0 || max_gen > (uint32_t) G) return set_err("%s: max_gen %u outside 1..%d cached positions", what, max_gen, G);
    if (codes->max_delay >= max_gen) return set_err("%s: max_gen %u must exceed max_delay %u", what, max_gen, codes->max_delay);
    if (codes->bos >= (uint32_t) V || codes->eos >= (uint32_t) V || codes->pad >= (uint32_t) V) return set_err("%s: special ids outside the vocabulary %d", what, V);
    if (sp) {
        if (V > SMP_VMAX) return set_err("%s: output vocabulary %d > %d", what, V, SMP_VMAX);
        if (!(sp->temperature > 0.0f) || !(sp->top_p > 0.0f) || !(sp->repetition_penalty > 0.0f)) return set_err("%s: temperature, top_p, repetition_penalty must be > 0", what);
    }
    return 0;
}

// The loop over slots 0..n-1 from its first step; the arguments have been checked.  BATCH: every slot live, over the whole text context, with
// the budget max_gen and the caller's uniforms [call][utt][head] (what an admission of all n slots leaves, without the encoder passes).
// SESSION: every slot parked over one cross key until an admission; the admissions fill the slots' uniform columns.
// mixed (SESSION with sp NULL): every slot carries its own sampler record and penalty table [max_gen], sampler::max until an admission
// writes them; the uniforms block and the sampler state exist whatever the occupants turn out to be.
static int dia_loop_begin(tts_hip_ctx *c, DL::Mode mode, uint32_t n, uint32_t max_gen, const tts_hip_dia_codes *codes, const tts_hip_sampling *sp, const float *uniforms,
                          bool mixed = false) {
    const int S = (int) c->dia.max_ctx, NO = c->NO, U = (int) n, DU = c->di_U;
    const bool live = mode == DL::BATCH, rep = sp && sp->repetition_penalty != 1.0f;
    CHK(dia_loop_end(c));   // an unfinished tts_hip_dia_gen_* loop is waited for and dropped
    HIPCHK(hipSetDevice(c->device));
    if (sp || mixed) {
        const std::vector<float> zero(uniforms ? 0 : (size_t) max_gen * U * NO, 0.0f);   // sizes d_uniforms
        CHK(stage_uniforms(c, uniforms ? uniforms : zero.data(), (size_t) max_gen * U * NO));
        if (sp) CHK(stage_penalty(c, sp->repetition_penalty, (int) max_gen));
    }
    if (mixed) {
        if (!c->di_srec) {
            HIPCHK(hipMalloc(&c->di_srec, (size_t) DU * sizeof(SampleRow)));
            HIPCHK(hipMalloc(&c->di_srec_in, (size_t) DU * sizeof(SampleRow)));
        }
        CHK(grow_bufs(&c->di_spen_cap, (size_t) DU * max_gen, nullptr, &c->di_spen, &c->di_spen_in));   // nothing is in flight (dia_loop_end), and no captured launch holds these
        c->di_spen_len = (int) max_gen;
        HIPCHK(hipMemsetAsync(c->di_srec, 0, (size_t) DU * sizeof(SampleRow), c->stream));   // SAMPLE_ROW_MAX, no table
    }
    // ids BOS (the embedding reads them), position 0, countdown -1, sampler call 1, nothing handed out, budget max_gen; sampler::reset (sampler.cpp:71-80)
    {
        std::vector<uint32_t> ids((size_t) U * NO, codes->bos), loop((size_t) 4 * DU, 0u), seq((size_t) 2 * U), cend((size_t) 2 * U, live ? (uint32_t) S : 1u), bud((size_t) 2 * DU, 0u);
        for (int u = 0; u < U; u++) {
            loop[(size_t) u] = 0xFFFFFFFFu; loop[(size_t) DU + u] = live ? 0u : 1u; loop[(size_t) 2 * DU + u] = 1u;
            seq[(size_t) 2 * u] = 2 * u; seq[(size_t) 2 * u + 1] = 2 * u + 1;
            bud[(size_t) u] = max_gen;
        }
        HIPCHK(hipMemcpyAsync(c->di_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(c->di_pos, 0, (size_t) 2 * U * 4, c->stream));
        HIPCHK(hipMemcpyAsync(c->di_seq, seq.data(), seq.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->di_cend, cend.data(), cend.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->di_loop, loop.data(), loop.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->di_sbud, bud.data(), bud.size() * 4, hipMemcpyHostToDevice, c->stream));
        if (rep || mixed) {
            HIPCHK(hipMemsetAsync(c->d_last, 0xFF, (size_t) U * NO * 4, c->stream));
            HIPCHK(hipMemsetAsync(c->d_repc, 0, (size_t) U * NO * 4, c->stream));
        }
        // a slot no encoder pass has filled (SESSION; BATCH refuses it) holds whatever its cross K/V held: the one position its parked rows attend over becomes zero
        // the kernel's mask holds 64 slots: one launch per group of 64, on the caches from that group's first row on (the layer stride stays 2 * DU rows)
        for (int u0 = 0; u0 < U; u0 += 64) {
            const int m = std::min(64, U - u0);
            uint64_t clear = 0;
            for (int u = 0; u < m; u++) if (!c->di_slot_encoded[(size_t) (u0 + u)]) clear |= 1ull << u;
            if (!clear) continue;
            CHK(with_kv(c->di_kv_esz, c->di_ck, c->di_cv, [&](auto *ck, auto *cv) -> int {
                const size_t first = (size_t) 2 * u0 * S * c->di_A;
                hipLaunchKernelGGL(dia_stream_clear_kernel<kv_of<decltype(ck)>>, dim3((c->di_A + 255) / 256, 2 * m, c->L), dim3(256), 0, c->stream, ck + first, cv + first, clear, 2 * DU,
                                   (int64_t) S, c->di_A);
                HIPCHK(hipGetLastError());
                return 0;
            }));
        }
        HIPCHK(hipStreamSynchronize(c->stream));   // the vectors are locals
    }
    // everything the captured launches hold by value: a change drops this mode's graph
    tts_hip_ctx::DiaBaked now;
    now.sampled = mixed ? 2 : sp ? 1 : 0; now.n = n; now.max_gen = max_gen; now.codes = *codes;
    if (sp) { now.uni = c->d_uniforms; now.pen = rep ? (const void *) c->d_pen : nullptr; now.sp = *sp; }
    if (mixed) { now.uni = c->d_uniforms; now.pen = c->di_srec; }   // the settings themselves are the records' contents
    DL next;
    next.mode = mode; next.mixed = mixed;
    const int gs = dia_graph_slot(next);
    auto &bk = c->di_baked[gs];
    const bool same = bk.sampled == now.sampled && bk.n == n && bk.max_gen == max_gen && memcmp(&bk.codes, codes, sizeof(*codes)) == 0 &&
                      (!(sp || mixed) || (bk.uni == now.uni && bk.pen == now.pen && memcmp(&bk.sp, &now.sp, sizeof(now.sp)) == 0));
    if (!same) {
        auto it = c->graphs.find(DIA_GRAPH_KEY + gs);
        if (it != c->graphs.end()) { (void) hipGraphExecDestroy(it->second); c->graphs.erase(it); }
        bk = now;
    }
    auto &g = c->dl;
    g.mode = mode; g.sampled = sp != nullptr; g.rep = rep; g.mixed = mixed;
    g.n = n; g.max_gen = max_gen; g.codes = *codes; g.sp = now.sp;
    g.slot.assign((size_t) U, live ? DL::LIVE : DL::FREE);
    g.steps.assign((size_t) U, 0u);
    g.budget.assign((size_t) U, max_gen);
    g.handed.assign((size_t) U, 0u);
    return 0;
}

// enqueues min(n_steps, what the mode allows) replays; no copy, no synchronise after the graph exists
static int dia_loop_launch(tts_hip_ctx *c, uint32_t n_steps) {
    auto &g = c->dl;
    uint32_t allowed = 0;
    if (g.mode == DL::BATCH) {
        // at most max_gen sampler calls, then one pre-step that ends the countdown: never more than max_gen + 1 pre-steps
        if (!g.all_done && g.launched < g.max_gen + 1) allowed = g.max_gen + 1 - g.launched;
    } else {
        // a live slot parks in the pre-step at position budget - 1 at the latest: no replay beyond the last one any live slot can need
        for (uint32_t s = 0; s < g.n; s++)
            if (g.slot[s] == DL::LIVE) allowed = std::max(allowed, g.budget[s] - std::min(g.steps[s], g.budget[s] - 1));
    }
    const uint32_t k = std::min(n_steps, allowed);
    if (k == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    const bool use_graph = !(c->d.flags & TTS_HIP_FLAG_NO_GRAPH) && !c->prof;
    const int key = DIA_GRAPH_KEY + dia_graph_slot(g);
    const DiaLoopArgs la = dia_loop_args(c);
    for (uint32_t i = 0; i < k; i++) {
        auto it = c->graphs.find(key);
        if (use_graph && it != c->graphs.end()) {
            HIPCHK(hipGraphLaunch(it->second, c->stream));
        } else {
            CHK(dia_loop_step(c, la, false));
            if (use_graph) {
                // that step ran eagerly (per-kernel attributes are set outside a capture); the capture for the next ones follows
                HIPCHK(hipStreamSynchronize(c->stream));
                hipGraphExec_t exec = nullptr;
                CHK(capture_graph(c, key, [&] { return dia_loop_step(c, la, true); }, &exec));
            }
        }
        g.launched++; g.in_flight++; g.unread++;
    }
    return 0;
}

// the look-in: one launch, one copy, one synchronise.  tokens_out != NULL takes the rows no earlier look-in took.
static int dia_loop_look(tts_hip_ctx *c, uint32_t *tokens_out, uint32_t *steps_done, uint8_t *done) {
    auto &g = c->dl;
    const int U = (int) g.n, NO = c->NO;
    HIPCHK(hipSetDevice(c->device));
    DiaLookArgs a{};
    a.n_utt = U; a.n_out = NO; a.max_gen = g.max_gen;
    a.take = tokens_out ? 1 : 0;
    // a slot's un-taken rows were all recorded by steps enqueued since the last look-in that took rows (an admission starts at row 0), and
    // di_look holds max_generation_size >= max_gen rows per slot
    a.cap = a.take ? std::min(g.unread, g.max_gen) : 0u;
    a.pos = c->di_pos; a.done = c->di_loop + c->di_U; a.steps = c->di_sbud + c->di_U; a.hist = c->di_hist; a.handed = c->di_loop + 3 * c->di_U; a.block = c->di_look;
    const size_t slot = 2 + (size_t) a.cap * NO;
    hipLaunchKernelGGL(dia_loop_lookin_kernel, dim3(U), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_di_look, c->di_look, (size_t) U * slot * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    g.in_flight = 0;
    g.all_done = true;
    for (int u = 0; u < U; u++) {
        const uint32_t *s = c->h_di_look + (size_t) u * slot;
        const uint32_t from = g.handed[(size_t) u], to = s[0];
        const uint32_t rows = a.take && to > from ? std::min(to - from, a.cap) : 0u;
        if (rows) memcpy(tokens_out + ((size_t) u * g.max_gen + from) * NO, s + 2, (size_t) rows * NO * 4);
        g.handed[(size_t) u] = from + rows;
        if (steps_done) steps_done[u] = to;
        if (done) done[u] = s[1] != 0;
        if (g.slot[(size_t) u] != DL::LIVE) continue;
        g.steps[(size_t) u] = to;
        if (s[1]) g.slot[(size_t) u] = DL::ENDED;
        else g.all_done = false;
    }
    if (a.take) g.unread = 0;
    return 0;
}

// ---- the fixed batch ----
static int dia_gen_begin(tts_hip_ctx *c, const char *what, uint32_t n_utt, uint32_t max_gen, const tts_hip_dia_codes *codes, const tts_hip_sampling *sp,
                         const float *uniforms) {
    CHK(dia_loop_check(c, what, "utterances", n_utt, max_gen, codes, sp));
    for (uint32_t u = 0; u < n_utt; u++)
        if (!c->di_slot_encoded[u]) return set_err("%s: slot %u has not been encoded (tts_hip_dia_encode_slot)", what, u);
    if (sp && !uniforms) return set_err("%s: null uniforms", what);
    return dia_loop_begin(c, DL::BATCH, n_utt, max_gen, codes, sp, uniforms);
}

static int dia_gen_ready(tts_hip_ctx *c, const char *what) {
    if (!c || !c->has_dia) return set_err("%s: not a Dia context (tts_hip_dia_create)", what);
    CHK(dia_no_session(c, what));
    return c->dl.mode == DL::BATCH ? 0 : set_err("%s: no generation (tts_hip_dia_gen_begin)", what);
}

extern "C" int tts_hip_dia_gen_begin(tts_hip_ctx *c, uint32_t n_utt, uint32_t max_gen, const tts_hip_dia_codes *codes, const tts_hip_sampling *sp, const float *uniforms) {
    return dia_gen_begin(c, "tts_hip_dia_gen_begin", n_utt, max_gen, codes, sp, uniforms);
}

extern "C" int tts_hip_dia_gen_launch(tts_hip_ctx *c, uint32_t n_steps) {
    CHK(dia_gen_ready(c, "tts_hip_dia_gen_launch"));
    return dia_loop_launch(c, n_steps);
}

extern "C" int tts_hip_dia_gen_wait(tts_hip_ctx *c, uint32_t *tokens_out, uint32_t *steps_done, uint8_t *done, uint32_t *ran) {
    CHK(dia_gen_ready(c, "tts_hip_dia_gen_wait"));
    CHK(dia_loop_look(c, tokens_out, steps_done, done));
    if (ran) *ran = c->dl.launched;
    return 0;
}

// begin + (launch 16, wait) until every utterance is done or the max_gen + 1 pre-steps are spent
extern "C" int tts_hip_dia_generate(tts_hip_ctx *c, uint32_t n_utt, uint32_t max_gen, const tts_hip_dia_codes *codes, const tts_hip_sampling *sp, const float *uniforms,
                                    uint32_t *tokens_out, uint32_t *steps_out) {
    if (!c || !c->has_dia) return set_err("tts_hip_dia_generate: not a Dia context (tts_hip_dia_create)");
    if (!c->finalized || !c->weights_present) return set_err("tts_hip_dia_generate: context not finalized");
    if (!codes || !tokens_out || !steps_out) return set_err("tts_hip_dia_generate: null argument");
    CHK(dia_gen_begin(c, "tts_hip_dia_generate", n_utt, max_gen, codes, sp, uniforms));
    int rc = 0;
    while (rc == 0 && !c->dl.all_done && c->dl.launched < max_gen + 1) {
        rc = dia_loop_launch(c, DIA_LOOP_CHUNK);
        if (rc == 0) rc = dia_loop_look(c, tokens_out, steps_out, nullptr);
    }
    (void) dia_loop_end(c);
    return rc;
}

// ---- the continuous session ----
extern "C" int tts_hip_dia_stream_begin(tts_hip_ctx *c, uint32_t n_slots, uint32_t max_gen, const tts_hip_dia_codes *codes, const tts_hip_sampling *sp) {
    CHK(dia_loop_check(c, "tts_hip_dia_stream_begin", "slots", n_slots, max_gen, codes, sp));
    return dia_loop_begin(c, DL::SESSION, n_slots, max_gen, codes, sp, nullptr);
}

// one sampler's limits, as dia_loop_check asks them of a session's
static bool dia_sampling_ok(const tts_hip_sampling *sp) { return sp->temperature > 0.0f && sp->top_p > 0.0f && sp->repetition_penalty > 0.0f; }

// both admissions.  mixed: sampling [n] (NULL, or an entry NULL: sampler::max) and the slot's record, table and sampler state rewritten
static int dia_stream_admit(tts_hip_ctx *c, const char *what, bool mixed, uint32_t n, const uint32_t *slots, const uint32_t *tokens, const uint32_t *sentence_len,
                            const uint32_t *budget, const tts_hip_sampling *const *sampling, const float *uniforms) {
    CHK(dia_stream_ready(c, what));
    auto &g = c->dl;
    if (mixed != g.mixed)
        return set_err(mixed ? "%s: the session was opened by tts_hip_dia_stream_begin (tts_hip_dia_stream_admit)"
                             : "%s: the session was opened by tts_hip_dia_stream_begin_mixed (tts_hip_dia_stream_admit_mixed)", what);
    CHK(g.idle(what, DIA_WAIT));
    if (n == 0) return 0;
    if (!slots || !tokens || !sentence_len) return set_err("%s: null argument", what);
    if (g.sampled && !uniforms) return set_err("%s: a sampled session needs the utterances' uniforms [n][max_gen][n_output_heads]", what);
    const int S = (int) c->dia.max_ctx, NO = c->NO;
    CHK(g.check_list(what, n, slots, DL::ADMIT));
    for (uint32_t i = 0; i < n; i++) {
        if (sentence_len[i] == 0 || sentence_len[i] > (uint32_t) S) return set_err("%s: utterance %u: sentence length %u outside 1..%d", what, i, sentence_len[i], S);
        if (budget && (budget[i] <= g.codes.max_delay || budget[i] > g.max_gen))
            return set_err("%s: utterance %u: budget %u outside max_delay %u < budget <= max_gen %u", what, i, budget[i], g.codes.max_delay, g.max_gen);
        for (int t = 0; t < S; t++)
            if (tokens[(size_t) i * S + t] >= (uint32_t) c->di_evocab) return set_err("%s: token %u >= encoder vocabulary %d", what, tokens[(size_t) i * S + t], c->di_evocab);
        const tts_hip_sampling *sp = mixed && sampling ? sampling[i] : nullptr;
        if (!sp) continue;
        if (!dia_sampling_ok(sp)) return set_err("%s: utterance %u: temperature, top_p, repetition_penalty must be > 0", what, i);
        if (!uniforms) return set_err("%s: utterance %u is sampled: it needs uniforms [n][max_gen][n_output_heads]", what, i);
    }
    // a mixed session: per utterance its record and its penalty table, for the staging copies
    const int len = c->di_spen_len;
    bool any_sampled = g.sampled, any_rep = false;
    std::vector<SampleRow> recs;
    std::vector<double> tabs;
    if (mixed) build_sample_rows(n, sampling, len, [&](uint32_t i) { return c->di_spen + (size_t) slots[i] * len; }, recs, tabs, &any_sampled, &any_rep);
    HIPCHK(hipSetDevice(c->device));
    const size_t per = (size_t) g.max_gen * NO;
    if (any_sampled && n * per > c->di_suni_cap) {
        HIPCHK(hipStreamSynchronize(c->stream));
        CHK(grow_dev(&c->di_suni, &c->di_suni_cap, n * per));
    }
    // the encoder and the cross K/V of each slot (stream order: the running slots' steps of the last run are behind us), then one launch for all
    for (uint32_t i = 0; i < n; i++) {
        CHK(dia_encode_into(c, slots[i], tokens + (size_t) i * S, sentence_len[i], nullptr));
        c->di_slot_encoded[slots[i]] = 1;
    }
    std::vector<uint32_t> adm((size_t) 2 * n);
    for (uint32_t i = 0; i < n; i++) { adm[i] = slots[i]; adm[(size_t) n + i] = budget ? budget[i] : g.max_gen; }
    HIPCHK(hipMemcpyAsync(c->di_sadm, adm.data(), adm.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (any_sampled) HIPCHK(hipMemcpyAsync(c->di_suni, uniforms, n * per * 4, hipMemcpyHostToDevice, c->stream));
    if (mixed) {
        HIPCHK(hipMemcpyAsync(c->di_srec_in, recs.data(), recs.size() * sizeof(SampleRow), hipMemcpyHostToDevice, c->stream));
        if (any_rep) HIPCHK(hipMemcpyAsync(c->di_spen_in, tabs.data(), tabs.size() * 8, hipMemcpyHostToDevice, c->stream));
    }
    DiaAdmitArgs a{};
    a.n = (int) n; a.n_slots = (int) g.n; a.n_out = NO;
    a.bos = g.codes.bos; a.max_gen = g.max_gen; a.max_ctx = (uint32_t) S;
    a.slots = c->di_sadm; a.budgets = c->di_sadm + n;
    a.uni_in = any_sampled ? c->di_suni : nullptr; a.uni = c->d_uniforms;
    a.last = g.rep || mixed ? c->d_last : nullptr; a.repc = c->d_repc;
    if (mixed) { a.rec_in = (const SampleRow *) c->di_srec_in; a.rec = (SampleRow *) c->di_srec; a.pen_in = c->di_spen_in; a.pen = c->di_spen; a.pen_len = len; }
    a.ids = c->di_ids; a.pos = c->di_pos; a.cend = c->di_cend;
    a.delay = (int32_t *) c->di_loop; a.done = c->di_loop + c->di_U; a.call = c->di_loop + 2 * c->di_U; a.handed = c->di_loop + 3 * c->di_U;
    a.budget = c->di_sbud; a.steps = c->di_sbud + c->di_U;
    const unsigned bx = any_sampled || any_rep ? (unsigned) std::min<size_t>((per + 255) / 256, 64) : 1u;
    hipLaunchKernelGGL(dia_stream_admit_kernel, dim3(bx, n), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));   // adm, recs and tabs are locals, uniforms the caller's
    for (uint32_t i = 0; i < n; i++) { g.slot[slots[i]] = DL::LIVE; g.steps[slots[i]] = 0; g.budget[slots[i]] = adm[(size_t) n + i]; g.handed[slots[i]] = 0; }
    return 0;
}

extern "C" int tts_hip_dia_stream_admit(tts_hip_ctx *c, uint32_t n, const uint32_t *slots, const uint32_t *tokens, const uint32_t *sentence_len, const uint32_t *budget,
                                        const float *uniforms) {
    return dia_stream_admit(c, "tts_hip_dia_stream_admit", false, n, slots, tokens, sentence_len, budget, nullptr, uniforms);
}

extern "C" int tts_hip_dia_stream_begin_mixed(tts_hip_ctx *c, uint32_t n_slots, uint32_t max_gen, const tts_hip_dia_codes *codes) {
    const char *what = "tts_hip_dia_stream_begin_mixed";
    CHK(dia_loop_check(c, what, "slots", n_slots, max_gen, codes, nullptr));
    if (c->di_V > SMP_VMAX) return set_err("%s: output vocabulary %d > %d", what, c->di_V, SMP_VMAX);   // every row goes through sample_kernel
    return dia_loop_begin(c, DL::SESSION, n_slots, max_gen, codes, nullptr, nullptr, true);
}

extern "C" int tts_hip_dia_stream_admit_mixed(tts_hip_ctx *c, uint32_t n, const uint32_t *slots, const uint32_t *tokens, const uint32_t *sentence_len,
                                              const uint32_t *budget, const tts_hip_sampling *const *sampling, const float *uniforms) {
    return dia_stream_admit(c, "tts_hip_dia_stream_admit_mixed", true, n, slots, tokens, sentence_len, budget, sampling, uniforms);
}

extern "C" int tts_hip_dia_stream_launch(tts_hip_ctx *c, uint32_t n_steps) {
    const char *what = "tts_hip_dia_stream_launch";
    CHK(dia_stream_ready(c, what));
    CHK(c->dl.idle(what, DIA_WAIT));
    return dia_loop_launch(c, n_steps);
}

extern "C" int tts_hip_dia_stream_wait(tts_hip_ctx *c, uint32_t *tokens_out, uint32_t *steps_done, uint8_t *done, uint32_t *n_finished, uint32_t *finished_slots,
                                       uint32_t *finished_steps) {
    const char *what = "tts_hip_dia_stream_wait";
    CHK(dia_stream_ready(c, what));
    if (!n_finished || !finished_slots || !finished_steps) return set_err("%s: null argument", what);
    *n_finished = 0;
    CHK(dia_loop_look(c, tokens_out, steps_done, done));
    c->dl.report(c->dl.steps, n_finished, finished_slots, finished_steps);
    return 0;
}

// launch + a wait that takes no rows; with no live slot nothing is launched and nothing is looked at
extern "C" int tts_hip_dia_stream_run(tts_hip_ctx *c, uint32_t n_steps, uint32_t *n_finished, uint32_t *finished_slots, uint32_t *finished_steps) {
    const char *what = "tts_hip_dia_stream_run";
    CHK(dia_stream_ready(c, what));
    if (!n_finished || !finished_slots || !finished_steps) return set_err("%s: null argument", what);
    *n_finished = 0;
    CHK(c->dl.idle(what, DIA_WAIT));
    CHK(dia_loop_launch(c, n_steps));
    if (c->dl.in_flight) CHK(dia_loop_look(c, nullptr, nullptr, nullptr));
    c->dl.report(c->dl.steps, n_finished, finished_slots, finished_steps);
    return 0;
}

extern "C" int tts_hip_dia_stream_drop(tts_hip_ctx *c, uint32_t n, const uint32_t *slots) {
    const char *what = "tts_hip_dia_stream_drop";
    CHK(dia_stream_ready(c, what));
    CHK(c->dl.idle(what, DIA_WAIT));
    auto &g = c->dl;
    if (n == 0) return 0;
    if (!slots) return set_err("%s: null argument", what);
    CHK(g.check_list(what, n, slots, DL::DROP));
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->di_sadm, slots, (size_t) n * 4, hipMemcpyHostToDevice, c->stream));   // n <= n_slots <= max_utterances
    DiaDropArgs a{};
    a.n = (int) n; a.slots = c->di_sadm;
    a.pos = c->di_pos; a.done = c->di_loop + c->di_U; a.call = c->di_loop + 2 * c->di_U; a.steps = c->di_sbud + c->di_U; a.cend = c->di_cend;
    hipLaunchKernelGGL(dia_stream_drop_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));   // slots is the caller's
    for (uint32_t i = 0; i < n; i++) g.slot[slots[i]] = DL::FREE;
    return 0;
}

extern "C" int tts_hip_dia_stream_collect(tts_hip_ctx *c, uint32_t slot, uint32_t steps, uint32_t *tokens_out) {
    const char *what = "tts_hip_dia_stream_collect";
    CHK(dia_stream_ready(c, what));
    CHK(c->dl.idle(what, DIA_WAIT));
    auto &g = c->dl;
    CHK(g.check_collect(what, slot, steps, g.steps, DIA_RUN, "made", "steps"));
    if (steps == 0) return 0;
    if (!tokens_out) return set_err("%s: null argument", what);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(tokens_out, c->di_hist + (size_t) slot * g.max_gen * c->NO, (size_t) steps * c->NO * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int tts_hip_dia_stream_end(tts_hip_ctx *c) {
    if (!c || !c->has_dia) return set_err("tts_hip_dia_stream_end: not a Dia context (tts_hip_dia_create)");
    return c->dl.mode == DL::SESSION ? dia_loop_end(c) : 0;
}

extern "C" int tts_hip_dia_step(tts_hip_ctx *c, const uint32_t *ids, uint32_t pos, float *logits_out, float *raw_out) {
    return tts_hip_dia_step_batch(c, 1, nullptr, ids, &pos, logits_out, raw_out);
}

// ------------------------------------------------------------------------------------------------
