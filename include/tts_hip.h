/*
 * tts_hip.h — C ABI of the MI355X (gfx950) compute shim underneath TTS.cpp's
 * tts_generation_runner API.  Plain pointers and sizes only; no C++/torch types.
 *
 * What this replaces in the reference (file:line under /root/reference):
 *   - the ggml graph build + backend-sched execution inside
 *       parler_tts_runner::decode            src/models/parler/model.cpp:648-693
 *       parler_tts_runner::build_parler_graph                      :520-614
 *       parler_tts_model::prep_cross_key_values                    :110-173
 *       parler_kv_cache_init / parler_build_kv_store               :339-385, :420-439
 *       dac_runner::run / build_dac_graph    src/decoder/dac_model.cpp:146-212
 *   - the weight buffer owned by tts_model (tts_model::set_tensor, src/tts_model.cpp:157-164)
 *   - runner_context's device/backend state (src/tts_model.h:16-44)
 * The host C++ runner (tts.cpp_amd/host) keeps tokenisation, the AR loop, sampling and the
 * delay pattern exactly where the reference has them and calls into this ABI once per
 * decode step and once per codec decode.
 *
 * Conventions: every int-returning call returns 0 on success, non-zero on failure and
 * leaves a message retrievable by tts_hip_last_error().  The reference has no error codes
 * (TTS_ABORT -> abort(), src/util.cpp:14-22); the C++ wrapper aborts on non-zero to match.
 * A context is single-threaded from the caller's point of view (one HIP stream + one device
 * per context), mirroring "one runner per worker thread" (examples/server/server.cpp:316-321).
 */
#ifndef TTS_HIP_H
#define TTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ggml tensor type ids as they appear in GGUF tensor infos (examples/quantize/README.md:48-55) */
enum tts_hip_type {
    TTS_HIP_F32  = 0,
    TTS_HIP_F16  = 1,
    TTS_HIP_Q4_0 = 2,
    TTS_HIP_Q5_0 = 6,
    TTS_HIP_Q8_0 = 8,
};

#define TTS_HIP_MAX_DAC_BLOCKS 8

/* Hyper-parameters that the reference reads from GGUF KV pairs
 * (parler_tts_model::prep_constants model.cpp:51-108, dac_model::prep_constants/prep_layers
 * dac_model.cpp:15-55).  Shapes that the reference takes from tensor shapes (FFN width,
 * prompt vocab, DAC channel counts) are inferred from the uploaded tensors at finalize. */
typedef struct tts_hip_desc {
    uint32_t struct_size;         /* sizeof(tts_hip_desc), ABI guard */
    /* Parler decoder */
    uint32_t hidden_size;         /* parler-tts.decoder.hidden_size          (1024) */
    uint32_t n_layers;            /* parler-tts.decoder.num_hidden_layers    (24)   */
    uint32_t n_attn_heads;        /* parler-tts.decoder.attention.head_count (16)   */
    uint32_t n_output_heads;      /* parler-tts.decoder.output_heads         (9)    */
    uint32_t output_vocab_size;   /* parler-tts.decoder.out_vocab_size       (1088) */
    uint32_t max_ctx_length;      /* parler-tts.decoder.context_length       (4096) */
    uint32_t n_encode_length;     /* parler-tts.decoder.encode_length (voice prompt tokens) */
    uint32_t use_cross_attn;      /* generation_configuration.use_cross_attn (common.h:59) */
    /* DAC */
    uint32_t dac_n_blocks;        /* 4 (dac_model.h:33) */
    uint32_t dac_stride[TTS_HIP_MAX_DAC_BLOCKS];   /* dac.dac_layer_stride_i  */
    uint32_t dac_padding[TTS_HIP_MAX_DAC_BLOCKS];  /* dac.dac_layer_padding_i */
    uint32_t dac_max_frames;      /* parler-tts.decoder.max_generation (2580) */
    /* engine knobs (extensions; the reference is max_seqs=1, kv F32) */
    uint32_t max_seqs;            /* utterances decoded in lock-step on this device */
    uint32_t kv_type;             /* TTS_HIP_F32 (reference, model.h:138-139) or TTS_HIP_F16 */
    uint32_t gelu_mode;           /* 1 = ggml CPU's fp16-table GELU semantics, 0 = fp32 tanh GELU */
    uint32_t flags;               /* TTS_HIP_FLAG_* */
    uint32_t kv_positions;        /* positions kept per sequence in the self-attention cache; 0 = max_ctx_length
                                     (reference, model.cpp:368-369).  Generation stops at position
                                     max_generation (check_stopping, model.cpp:720-722), so max_generation suffices. */
} tts_hip_desc;

#define TTS_HIP_FLAG_NO_GRAPH   1u  /* launch kernels eagerly instead of replaying a captured hipGraph */
#define TTS_HIP_FLAG_VALU_GEMM  2u  /* use the scalar-FMA reference GEMV kernels instead of MFMA (debug/parity) */
#define TTS_HIP_FLAG_NO_DAC     4u  /* context carries no audio codec */
#define TTS_HIP_FLAG_NO_PARLER  8u  /* context carries only the audio codec */
#define TTS_HIP_FLAG_DAC_F32    32u /* F16 codec tensors: compute with fp32 activations (exact-fp32 MFMA) instead of ggml's
                                       fp16 im2col x fp16 kernel semantics */
#define TTS_HIP_FLAG_DEQUANT_Q  16u /* decode Q4_0/Q5_0/Q8_0 matrices to fp32 at upload (fp32 activations) instead of
                                       the integer path with Q8_0-quantised activations (ggml's CPU semantics) */
#define TTS_HIP_FLAG_KV_F16     64u /* tts_hip_orpheus_create only (extension; the reference keeps fp32 K/V, orpheus/model.cpp:176-181):
                                       the K/V cache is [slot][layer][position][kv width] in fp16 — half the cache memory and half
                                       the bytes every attention launch reads.  Rotated K and V are rounded once, to nearest-even,
                                       when they are appended (a plain fp32 -> fp16 conversion, as in Parler's fp16 cache,
                                       tts_hip_desc::kv_type): a magnitude above 65504 becomes inf, one below 6.1e-5 keeps
                                       fewer bits (fp16 subnormals).  All arithmetic stays fp32: query, scores, softmax and the
                                       P.V sums run on the cache rows widened exactly.  Fixed at create for every path of the
                                       context (decode, the captured step, step_batch / generate_batch, gen_*, stream_*).
                                       tts_hip_create, tts_hip_t5_create, tts_hip_snac_create and tts_hip_dia_create refuse it
                                       with an error that names the flag and the call; a Dia context selects its fp16 caches
                                       through tts_hip_dia_desc::kv_type. */
/* A value of tts_hip_orpheus_desc::kv_type (see there): the one-byte OCP e4m3fn K/V cache.  Not a ggml tensor type id, so not in enum tts_hip_type. */
#define TTS_HIP_KV_F8_E4M3 256u

typedef struct tts_hip_ctx tts_hip_ctx;

/* ---- lifecycle ------------------------------------------------------------------------- */
int          tts_hip_device_count(void);
tts_hip_ctx *tts_hip_create(int device, const tts_hip_desc *desc);  /* NULL on failure */
void         tts_hip_destroy(tts_hip_ctx *ctx);
const char  *tts_hip_last_error(void);
const char  *tts_hip_version(void);

/* ---- weights -----------------------------------------------------------------------------
 * One call per GGUF tensor, with the tensor's GGUF name, e.g.
 * "decoder.layers.3.self_attn.q_proj.weight", "audio_encoder.decoder_block.2.residual_unit.0.res.initial.weight"
 * (== runner->assign_weight(name, tensor), src/models/loaders.cpp:79-88, parler/model.cpp:500-508).
 * ne[] is the GGUF order (ne[0] fastest).  host_data may be NULL: the tensor is then only
 * declared (its bytes arrive later through the arena, see tts_hip_arena_*). Unknown names are
 * ignored with return value 0 and a warning, like the reference (model.cpp:506). */
int tts_hip_upload(tts_hip_ctx *ctx, const char *name, int type, int n_dims, const int64_t *ne,
                   const void *host_data);

/* Lays the weight arena out (fusing q/k/v and the lm heads into single matrices), moves the
 * uploaded tensors into it, allocates KV cache + workspaces, and — when weights are present —
 * runs prep_cross_key_values (model.cpp:110-173).  `external_arena` may be NULL (the shim
 * allocates) or a device pointer of at least tts_hip_arena_bytes() bytes owned by the caller
 * (e.g. a torch uint8 tensor that is then broadcast with RCCL). */
size_t tts_hip_arena_bytes(tts_hip_ctx *ctx); /* valid after all uploads, before or after finalize */
int    tts_hip_finalize(tts_hip_ctx *ctx, void *external_arena);
void  *tts_hip_arena_ptr(tts_hip_ctx *ctx);
/* After the arena of a declare-only context was filled by a collective: mark weights present.
 * (cross K/V live inside the arena, so they arrive with the broadcast.) */
int    tts_hip_arena_filled(tts_hip_ctx *ctx);

/* The one collective of the path: RCCL broadcast of the finished weight arena (weights + precomputed cross
 * K/V) from ctxs[root] to every other context, so that a host serving G devices parses and uploads the GGUF once — where the
 * reference's server re-parses the file for every worker (examples/server/server.cpp:316-321).  All n contexts belong to this
 * process, one per DISTINCT device, each finalized with its own arena of the same tts_hip_arena_bytes(); the non-root contexts
 * were filled declare-only (tts_hip_upload with host_data == NULL) and are marked ready here (tts_hip_arena_filled).
 * Single process: ncclCommInitAll over the contexts' devices, ncclGroupStart, one ncclBroadcast(uint8, arena bytes) per context on
 * its own stream, ncclGroupEnd, stream syncs, communicators destroyed.  n == 1 is a no-op that only validates.  librccl.so is
 * opened on first use (it is not a load-time dependency of this library). */
int    tts_hip_broadcast_weights(tts_hip_ctx **ctxs, int n, int root);
/* One-process-per-GPU form of the same broadcast: rank 0 obtains a 128-byte id (tts_hip_comm_unique_id) and hands it to the other
 * ranks by whatever the launcher offers (bench.py: torch.distributed); every rank then calls tts_hip_broadcast_weights_rank. */
int    tts_hip_comm_unique_id(void *id128);
int    tts_hip_broadcast_weights_rank(tts_hip_ctx *ctx, const void *id128, int rank, int world, int root);
/* update_conditional_prompt (model.cpp:510-518): replace the voice-prompt encoding
 * [n_tokens][hidden] (fp32, host) and recompute the cross K/V. n_tokens <= n_encode_length cap given at create. */
int    tts_hip_parler_set_text_encoding(tts_hip_ctx *ctx, const float *enc, uint32_t n_tokens);

/* ---- Parler decoder -------------------------------------------------------------------- */
/* pctx->reset + cache reuse (model.cpp:312-322,848-856): forget all sequences' positions. */
int tts_hip_parler_reset(tts_hip_ctx *ctx);
/* decode() with audio_generation=false (model.cpp:648-693 on a batch_from_sentence batch :473-498):
 * run `n` text-prompt ids of sequence `seq` at positions pos0..pos0+n-1 and append their K/V.
 * The prompt logits are never consumed by the reference (sampler only runs on audio steps,
 * model.cpp:774-776), so none are produced. */
int tts_hip_parler_prefill(tts_hip_ctx *ctx, uint32_t seq, const uint32_t *text_ids, uint32_t n, uint32_t pos0);
/* The same for n sequences in as few forwards as possible (extension): ids = the prompts concatenated, lens[n];
 * seqs[n] (NULL = 0..n-1) and pos0[n] (NULL = all 0).  Equivalent to n tts_hip_parler_prefill calls. */
int tts_hip_parler_prefill_batch(tts_hip_ctx *ctx, uint32_t n, const uint32_t *seqs, const uint32_t *text_ids,
                                 const uint32_t *lens, const uint32_t *pos0);
/* decode() with audio_generation=true for n_seqs sequences in lock-step:
 *   ids   [n_seqs][n_output_heads]  codebook ids fed this step (model.cpp:394-403,778-785)
 *   pos   [n_seqs]                  absolute position of each sequence (model.cpp:784)
 *   seqs  [n_seqs] or NULL          cache slot of each row (NULL = 0..n_seqs-1)
 *   logits_out [n_seqs][n_output_heads][output_vocab_size] fp32 host memory (model.cpp:455-456,682-683)
 * Blocks until the logits are in logits_out. */
int tts_hip_parler_step(tts_hip_ctx *ctx, uint32_t n_seqs, const uint32_t *ids, const uint32_t *pos,
                        const uint32_t *seqs, float *logits_out);
/* Same step, but sampler::max (src/sampler.cpp:185-204, first maximum wins, no repetition
 * penalty) is evaluated on the device; tokens_out [n_seqs][n_output_heads]. */
int tts_hip_parler_step_greedy(tts_hip_ctx *ctx, uint32_t n_seqs, const uint32_t *ids, const uint32_t *pos,
                               const uint32_t *seqs, uint32_t *tokens_out);
/* Device-resident greedy generation of `n_steps` audio steps for n_seqs sequences whose prompts
 * were prefetched with tts_hip_parler_prefill: the delay-pattern feed (model.cpp:778-785) and the
 * EOS bookkeeping (check_stopping :715-732) run on the device, the host synchronises once.
 *   start_pos [n_seqs]: position of the first audio step (prompt length)
 *   tokens_out [n_steps][n_seqs][n_output_heads] sampled ids, still delayed (pctx->output_tokens)
 *   steps_done [n_seqs] (may be NULL): number of steps executed before all heads saw EOS
 * bos/eos: audio.bos_token_id / audio.eos_token_id. */
int tts_hip_parler_generate_greedy(tts_hip_ctx *ctx, uint32_t n_seqs, const uint32_t *start_pos,
                                   uint32_t n_steps, uint32_t bos, uint32_t eos, uint32_t *tokens_out,
                                   uint32_t *steps_done);

/* sampler::sample on the device (src/sampler.cpp:3-69: softmax :82-116, topk :152-183, topp :118-150) for
 * output_vocab_size <= 2048.  repetition_penalty != 1 keeps sampler::last_token_ids / repetition_counts per
 * (sequence, head) on the device (reset at the start of a generation, sampler.cpp:71-80).  top_k == 0 or >= vocab disables top-k, top_p >= 1
 * disables top-p; the order of the fp32 sums follows the reference (see sample_kernel).  The U[0,1) draws are the
 * caller's (the reference draws them from std::minstd_rand, sampler.cpp:47-48). */
typedef struct tts_hip_sampling {
    uint32_t top_k;
    float    top_p;
    float    temperature;
    float    repetition_penalty;   /* 1 = off */
} tts_hip_sampling;
/* tts_hip_parler_generate_greedy with sampler::sample instead of sampler::max.
 *   uniforms [n_steps][n_seqs][n_output_heads]: draw for head h of sequence s at its k-th sampler call */
int tts_hip_parler_generate_sampled(tts_hip_ctx *ctx, uint32_t n_seqs, const uint32_t *start_pos,
                                    uint32_t n_steps, uint32_t bos, uint32_t eos, const tts_hip_sampling *sampling,
                                    const float *uniforms, uint32_t *tokens_out, uint32_t *steps_done);
/* The same loop in pieces, so that the host can work while steps run (the runner's chunked audio decodes codec windows meanwhile):
 *   gen_begin   stages n_seqs prefilled sequences as tts_hip_parler_generate_greedy / _sampled do (sampling == NULL: sampler::max;
 *               else sampler::sample with uniforms [max_steps][n_seqs][n_output_heads])
 *   gen_launch  enqueues up to n_steps more steps on the context's stream and returns at once (nothing once every sequence has stopped
 *               or max_steps have run)
 *   gen_wait    synchronises and looks in: steps_done [n_seqs] as in generate_greedy (0: still running), *ran = steps run so far, and —
 *               when tokens_out != NULL — the tokens of the steps no earlier gen_wait handed out, written at their places in
 *               tokens_out [max_steps][n_seqs][n_output_heads].  Finished rows are compacted out of the forward at a wait whose step
 *               count is a multiple of 32, whatever the launch sizes: the tokens equal those of generate_greedy / _sampled.
 * The generation is over when every steps_done is non-zero or *ran == max_steps.  While steps are in flight the context's codec may run
 * (tts_hip_dac_decode*: its own stream, no buffer shared with the decoder); any other decoder call needs a gen_wait first
 * (tts_hip_parler_reset waits for and drops an unfinished loop). */
int tts_hip_parler_gen_begin(tts_hip_ctx *ctx, uint32_t n_seqs, const uint32_t *start_pos, uint32_t max_steps, uint32_t bos, uint32_t eos,
                             const tts_hip_sampling *sampling, const float *uniforms);
int tts_hip_parler_gen_launch(tts_hip_ctx *ctx, uint32_t n_steps);
int tts_hip_parler_gen_wait(tts_hip_ctx *ctx, uint32_t *tokens_out, uint32_t *steps_done, uint32_t *ran);
/* The device sampler alone on caller-supplied logits [n_rows][n_output_heads][output_vocab_size]
 * (uniforms [n_rows][n_output_heads]) -> tokens_out [n_rows][n_output_heads]; for parity tests.
 * last_ids / rep_counts [n_rows][n_output_heads]: the repetition state, read and updated in place (may be NULL when
 * repetition_penalty == 1). */
int tts_hip_sample_logits(tts_hip_ctx *ctx, uint32_t n_rows, const float *logits, const tts_hip_sampling *sampling,
                          const float *uniforms, int32_t *last_ids, uint32_t *rep_counts, uint32_t *tokens_out);
/* The same selection with a sampler per row, as the slots of a mixed Dia session carry them (tts_hip_dia_stream_begin_mixed): row r runs with
 * sampling[r], NULL meaning sampler::max (first maximum wins; no uniform read, its state untouched).  Per row the contract of
 * tts_hip_sample_logits with that row's settings, and the same ids and state: uniforms may be NULL when every row is greedy, last_ids /
 * rep_counts when no row has a repetition penalty; the state of a row without one is left as it is. */
int tts_hip_sample_logits_rows_mixed(tts_hip_ctx *ctx, uint32_t n_rows, const float *logits, const tts_hip_sampling *const *sampling,
                                     const float *uniforms, int32_t *last_ids, uint32_t *rep_counts, uint32_t *tokens_out);

/* ---- T5 voice-prompt encoder (src/models/parler/t5/model.cpp) ---------------------------------
 * What parler_tts_runner::update_conditional_prompt runs (model.cpp:510-518): text_encoder_from_file ->
 * t5_runner::generate -> prep_cross_key_values.  A T5 context is its own tts_hip_ctx: create, tts_hip_upload
 * every "t5encoder.*" tensor of the encoder GGUF (names: t5/model.cpp:3-18), tts_hip_finalize(ctx, NULL),
 * tts_hip_t5_encode, then hand the result to the decoder context with tts_hip_parler_set_text_encoding. */
typedef struct tts_hip_t5_desc {
    uint32_t struct_size;      /* sizeof(tts_hip_t5_desc) */
    uint32_t hidden_size;      /* t5encoder.embedding_length      (t5/model.cpp:129-132) */
    uint32_t n_layers;         /* t5encoder.block_count           (:124-127) */
    uint32_t n_attn_heads;     /* t5encoder.attention.head_count  (:134-137); head size is 64 (t5/model.h:46) */
    uint32_t max_ctx_length;   /* t5encoder.context_length        (:139-142) */
    uint32_t n_buckets;        /* relative_attn_buckets, 32 (t5/model.h:48); 0 = 32 */
    uint32_t output_size;      /* t5encoder.output_size (:160-163), 0 = take it from the tensors */
    uint32_t gelu_mode;        /* as tts_hip_desc */
    uint32_t flags;            /* TTS_HIP_FLAG_VALU_GEMM | TTS_HIP_FLAG_DEQUANT_Q */
} tts_hip_t5_desc;
tts_hip_ctx *tts_hip_t5_create(int device, const tts_hip_t5_desc *desc);
/* t5_runner::run (t5/model.cpp:321-357): ids [n_tokens] (the caller appends EOS, :361-362) ->
 * out [n_tokens][output size] fp32 (final rms norm, then down_proj + bias when the GGUF has them) */
int tts_hip_t5_encode(tts_hip_ctx *ctx, const uint32_t *ids, uint32_t n_tokens, float *out);
int tts_hip_t5_output_size(tts_hip_ctx *ctx);   /* after tts_hip_finalize / tts_hip_arena_bytes; < 0 on error */

/* ---- Orpheus decoder: Llama-3 blocks (src/models/orpheus/model.cpp) --------------------------------------
 * Device side of orpheus_runner::decode (:298-325): create, tts_hip_upload every "orpheus.*" tensor (names :11-60),
 * tts_hip_finalize(ctx, NULL), then tts_hip_orpheus_decode per call of decode() — the prompt batch first, one token
 * per step after.  Tokenizer (BPE), prompt framing (:341-356), sampler and the 7-ids-per-frame -> SNAC level mapping
 * (:358-376) stay with the host. */
typedef struct tts_hip_orpheus_desc {
    uint32_t struct_size;
    uint32_t hidden_size;      /* orpheus.hidden_size (3072)   */
    uint32_t n_layers;         /* orpheus.layers (28)          */
    uint32_t n_attn_heads;     /* orpheus.attn_heads (24)      */
    uint32_t n_kv_heads;       /* orpheus.kv_attn_heads (8)    */
    uint32_t head_dim;         /* orpheus.head_dim (128)       */
    uint32_t vocab_size;       /* orpheus.vocab_size (156940)  */
    uint32_t n_ctx;            /* KV positions: max_context_length + max_generation_size (1024 + 2100, :176-177) */
    float    rope_base;        /* 500000 (:190,250); 0 = that  */
    uint32_t flags;            /* TTS_HIP_FLAG_VALU_GEMM | TTS_HIP_FLAG_DEQUANT_Q | TTS_HIP_FLAG_KV_F16 (fp16 K/V cache, see the flag; the e4m3 cache: kv_type below) */
    uint32_t max_seqs;         /* KV-cache slots for lock-step utterances (tts_hip_orpheus_generate_batch); 0 / 1: one sequence, as the reference's runner.
                                * At most 256 (= the rows one decoder forward carries); tts_hip_orpheus_step_batch, generate_batch, gen_* and stream_begin[_mixed] take
                                * up to max_seqs rows / slots.  Contexts of at most 64 slots are unchanged: same arena, same kernels.  A context of 65 .. 256
                                * slots also plans the transposed block scales of its GGUF-quantised matrices into the arena (share_with / broadcast carry them),
                                * and its forwards of more than 64 rows run those matrices on the LDS-tiled integer GEMM (F32 / F16 matrices: the 16-feature
                                * kernels, correct but slow).  A slot costs n_layers * n_ctx * n_kv_heads * head_dim * 2 cache elements: 0.72 GB at 3B shapes,
                                * 0.36 GB under TTS_HIP_FLAG_KV_F16, 0.18 GB under kv_type = TTS_HIP_KV_F8_E4M3; tts_hip_finalize fails with the slot count and the bytes
                                * it asked for when they do not fit. */
    uint32_t kv_type;          /* the cache element type (extension; appended last: a desc of the size before this field is accepted and reads as 0).
                                * 0: the flags decide, fp32 or fp16 under TTS_HIP_FLAG_KV_F16.  TTS_HIP_F16: the same as TTS_HIP_FLAG_KV_F16.
                                * TTS_HIP_KV_F8_E4M3: the cache is [slot][layer][position][kv width] with one byte per element, OCP e4m3fn (1 sign, 4 exponent,
                                * 3 mantissa bits, no inf) - a quarter of the fp32 cache memory and of the bytes every attention launch reads.  Rotated K and V
                                * are rounded once, to nearest-even, when they are appended; saturation at +-448: a larger magnitude is stored as +-448;
                                * subnormals below 2^-6 (steps of 2^-9), flush to zero below 2^-10.  All arithmetic stays fp32: query, scores, softmax and the
                                * P.V sums run on the cache rows widened exactly.  This costs accuracy fp16 does not (three mantissa bits: DESIGN.md has the
                                * measured logits distance); it is opt-in.  Fixed at create for every path of the context: decode, the captured step,
                                * step_batch / generate_batch, gen_*, stream_*, and the 65 .. 256-row forwards.  Any other value is refused by name, as is
                                * TTS_HIP_KV_F8_E4M3 together with TTS_HIP_FLAG_KV_F16.  Dia and Parler contexts have no fp8 cache: tts_hip_dia_create refuses
                                * every kv_type but TTS_HIP_F32 / TTS_HIP_F16, tts_hip_create reads anything but TTS_HIP_F16 as fp32. */
} tts_hip_orpheus_desc;
tts_hip_ctx *tts_hip_orpheus_create(int device, const tts_hip_orpheus_desc *desc);
/* n tokens at positions pos0 .. pos0+n-1 (KV cache appended); logits_out [vocab_size] of the LAST token (:287-290).
 * tokens_out (may be NULL): sampler::max of those logits (first maximum wins), evaluated on the device. */
int tts_hip_orpheus_decode(tts_hip_ctx *ctx, const uint32_t *ids, uint32_t n, uint32_t pos0, float *logits_out, uint32_t *token_out);
/* greedy generate_from_batch (:378-392 with sampler::max): decode the prompt, then feed back the arg-max until
 * stop_id or max_new ids; returns the count in *n_out */
int tts_hip_orpheus_generate_greedy(tts_hip_ctx *ctx, const uint32_t *prompt, uint32_t n_prompt, uint32_t max_new, uint32_t stop_id,
                                    uint32_t *tokens_out, uint32_t *n_out);
/* the same loop with sampler::sample (orpheus/model.cpp:389-398, src/sampler.cpp:3-69) on the device: top_k in 1..64 (the default
 * generation_configuration, include/common.h:45-55, has top_k 50, top_p 1), any top_p > 0, temperature and repetition penalty.
 * The reference sorts all 156 940 logits on the host at every step; here two kernels select the top_k candidates in the
 * reference's order (value descending; equal values by index) and run the softmax / inverse-CDF scan in the reference's
 * operation order.  top_p < 1 (nucleus sampling, sampler.cpp:22-27, 118-150): a third kernel first accumulates the softmax
 * total over the whole vocabulary in index order, as the reference's fp32 sum is, and the picks keep their full-vocabulary
 * probabilities (about 0.65 ms per token more).  uniforms [max_new]: the U[0,1) draw of the k-th sampler call (the caller's
 * std::minstd_rand).  top_k 0 or > 64 is refused: sample on the host from tts_hip_orpheus_decode's logits. */
int tts_hip_orpheus_generate_sampled(tts_hip_ctx *ctx, const uint32_t *prompt, uint32_t n_prompt, uint32_t max_new, uint32_t stop_id,
                                     const tts_hip_sampling *sampling, const float *uniforms, uint32_t *tokens_out, uint32_t *n_out);
/* Lock-step utterances (the reference runs N independent workers with a model copy each, examples/server/server.cpp:225-321): one forward
 * carries one row per live utterance, row r in cache slot slots[r] at position pos[r].  step_batch: logits_out [n][vocab_size] and / or tokens_out [n]
 * (sampler::max per row) may be NULL.  generate_batch: generate_from_batch (orpheus/model.cpp:378-392) for n_utt utterances at once — prompts are the
 * utterances' ids back to back (n_prompt[u] each), tokens_out [n_utt][max_new], n_out [n_utt]; sampling NULL = sampler::max, else sampler::sample with
 * uniforms [n_utt][max_new] (utterance u's k-th sampler call draws uniforms[u * max_new + k]) and one repetition state per utterance.  Every utterance
 * receives exactly the ids its own one-sequence generation produces.  The loop is the continuous session's (below) with slots 0 .. n_utt-1 admitted
 * at begin: runs of a fixed number of steps with no copy or synchronise inside; an utterance that finishes inside a run idles as padding until the
 * run ends and then leaves the rows.  The loop's device buffers stay on the context from one call to the next. */
int tts_hip_orpheus_step_batch(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots, const uint32_t *ids, const uint32_t *pos, float *logits_out, uint32_t *tokens_out);
int tts_hip_orpheus_generate_batch(tts_hip_ctx *ctx, uint32_t n_utt, const uint32_t *prompts, const uint32_t *n_prompt, uint32_t max_new, uint32_t stop_id,
                                   const tts_hip_sampling *sampling, const float *uniforms, uint32_t *tokens_out, uint32_t *n_out);
/* The generation loops in pieces, for callers that work on the ids while the decoder is still running (chunked audio); the three
 * generate_* calls above are built on them.  gen_begin: prompts / n_prompt / sampling / uniforms as for generate_batch (n_utt = 1: as for
 * generate_greedy / generate_sampled, uniforms [max_new]); it runs the prompts and makes the first selection.  gen_launch enqueues up to n_steps
 * more steps: for n_utt = 1 replays of the captured step, and the call returns while they run; for n_utt > 1 one run of the lock-step loop (what
 * tts_hip_orpheus_stream_run enqueues: rows staged once, n_steps x (forward, selection, advance), one copy of the slots' state), which returns
 * after the steps ran; rows that finished leave at this boundary.  gen_wait synchronises and hands out the ids no gen_wait handed out before: tokens_out
 * [n_utt][max_new] receives utterance u's new ids at their places ([u * max_new + old n_out[u]] onwards), n_out[u] its count so far and
 * done[u] whether it has ended (stopping token, max_new ids, or the end of the cache); done may be NULL.  The ids are those of the generate_*
 * calls whatever the launch sizes; steps a launch ran past an utterance's stopping token are discarded.  One gen_launch per gen_wait.
 * Between a gen_launch and its gen_wait the steps may still be running: every other tts_hip_orpheus_* call on the context (decode, step_batch,
 * sample_logits, generate_*, gen_begin, gen_launch) is refused with an error until gen_wait has been called.  After a gen_wait, gen_begin
 * or a generate_* call abandons the generation under way (its cache rows are overwritten from position 0). */
int tts_hip_orpheus_gen_begin(tts_hip_ctx *ctx, uint32_t n_utt, const uint32_t *prompts, const uint32_t *n_prompt, uint32_t max_new, uint32_t stop_id,
                              const tts_hip_sampling *sampling, const float *uniforms);
int tts_hip_orpheus_gen_launch(tts_hip_ctx *ctx, uint32_t n_steps);
int tts_hip_orpheus_gen_wait(tts_hip_ctx *ctx, uint32_t *tokens_out, uint32_t *n_out, uint8_t *done);
/* the device sampler alone on caller-supplied logits [vocab_size], for parity tests; last_id / rep_count: sampler::last_token_ids /
 * repetition_counts, read and updated in place (may be NULL when repetition_penalty == 1) */
int tts_hip_orpheus_sample_logits(tts_hip_ctx *ctx, const float *logits, const tts_hip_sampling *sampling, float uniform, int32_t *last_id,
                                  uint32_t *rep_count, uint32_t *token_out);
/* Continuous session: a lock-step generation that admits utterances into free cache slots while the others are running, on a device-driven loop.
 * The per-slot state (ids so far, finished flag, latest id and position, sampler state, uniforms) lives on the device; a run of k steps is
 * k x (forward, row-batched selection, row advance) enqueued back to back with no copy and no synchronise in between.
 *   begin    n_slots <= max_seqs cache slots, at most max_new ids per utterance, the stopping token, the sampler (sampling NULL: sampler::max; else the
 *            limits of tts_hip_orpheus_generate_sampled; every admission writes it into the slot's record and penalty table)
 *   admit    n utterances into free slots, between two runs: prompts back to back (n_prompt[i] ids each), uniforms [n][max_new] for a sampled session
 *            (utterance i's k-th sampler call draws uniforms[i * max_new + k]), else NULL.  Each slot's sampler state and counts are reset, its
 *            prompt runs, and the first id is selected from the prompt's last row, as gen_begin does.
 *   run      stages the live rows once, enqueues n_steps steps, synchronises and reads the slots' counts and flags in one copy.  Slots that finished
 *            (stopping token, max_new ids, or the end of the cache) — inside the run, or at their admission (max_new 0 or 1, a first id that stops) —
 *            are reported with their id counts and leave the rows of the next run.  A row that finishes inside a run idles as padding until the run
 *            ends: nothing it selects is emitted, its sampler state stands still.  With no live rows nothing is launched.
 *   launch   the enqueue half of run: the live rows staged once, min(n_steps, what the longest live row can still need) steps enqueued, and the call
 *            returns while they run, with no copy and no synchronise.  The session is in flight until a wait.  With no live rows nothing is launched.
 *   wait     the look-in: one launch (llama_loop_lookin_kernel, one workgroup per slot), one copy into pinned memory and one synchronise, whatever
 *            the slot count.  tokens_out [n_slots][max_new] receives each slot's ids that no earlier wait handed out, at their places (the contract
 *            of gen_wait); n_out[s] is the occupant's count so far (0 for a slot nobody occupies) and done[s] whether it has ended (both may be
 *            NULL).  Slots that ended are reported exactly as run reports them.  tokens_out NULL takes nothing: only the slots' headers are copied
 *            (they are the state array itself, so no kernel is launched: what run has always copied) and the handed-out marks stand still, so
 *            the next taking wait still delivers everything.  A wait with nothing in flight is a pure look-in.
 *   drop     frees n live slots without reporting them, between a wait and the next launch.  Nothing is launched: the rows of a run are staged from
 *            the host's state, so the slot has left the next run's rows, and the next admission rewrites its device state.  It is admissible at once.
 *   collect  the first `count` ids of a reported slot, before that slot is admitted again
 *   end      ends the session (its device buffers stay on the context for the next session or batch); with steps in flight it synchronises first
 * run is launch, a wait that takes nothing, and the report: one loop under both.  The ids the waits hand out tile each occupant's sequence
 * without gap or overlap whatever the launch sizes; they equal what run and collect return; a drop changes no other slot's ids
 * (tests/test_gpu_orpheus_stream_chunked.py).  While steps are in flight (between a launch and its wait), admit, collect, drop, run and a second
 * launch return non-zero before anything is launched and leave the session as it was; so does a drop of a slot that is not live, is >= n_slots
 * or is named twice.
 * An utterance's ids are those of tts_hip_orpheus_generate_batch for the same prompt, that is those of its own one-sequence generation
 * (tests/test_gpu_orpheus_stream.py).  Key split: the attention of step i of a run is sized by max over the live rows of (position at the look-in)
 * + i + 1, capped at n_ctx: the exact longest row as long as nobody finishes, an upper bound once someone has.  Below 256 keys that bound selects one
 * key split; beyond, the split count follows the bound, which can select another count than the exact longest live row would (another association
 * of the same softmax).  tts_hip_orpheus_generate_batch and gen_launch size their steps the same way.
 * Between begin and end every other tts_hip_orpheus_* generation call on the context (decode, step_batch, sample_logits, generate_*, gen_begin,
 * gen_launch) is refused with an error, as in the window between a gen_launch and its gen_wait; begin is refused in that window and while a
 * gen_* generation has unfinished utterances.  Every misuse (a busy slot, a slot >= n_slots, collect on a slot that has not been reported or for
 * more ids than it produced, n_slots > max_seqs, a prompt that does not fit) returns non-zero before anything is launched.
 * Mixed session: begin_mixed opens a session whose slots carry their own sampler, so utterances that differ in top_k, temperature, top_p or
 * repetition penalty, greedy ones among them, share one forward.  admit_mixed takes utterance i's sampler as sampling[i] (NULL: sampler::max; else
 * the limits of tts_hip_orpheus_generate_sampled, checked for all n before anything is launched) and its draws as uniforms[i * max_new ..] (ignored for
 * a greedy utterance; uniforms may be NULL when all n are greedy).  The slot's record {mode, top_k, temperature, top_p} and its own repetition-penalty
 * table [max_new] are rewritten at every admission, so nothing of the slot's previous utterance stays.  run, collect and end are the calls above.  Per
 * step a run enqueues the arg-max pair when a live row is greedy, the top-k kernels when one is sampled and the softmax total when a sampled one has
 * top_p < 1 (known when the run's rows are staged); each kernel skips the rows of the other mode.  The uniform session runs the same kernels: its admissions write the
 * session's one sampler into every slot's record.  So an utterance's ids are those of its own one-sequence generation with its own sampler
 * (tests/test_gpu_orpheus_stream_mixed.py).  admit_mixed on a session opened by begin, and admit on one opened by begin_mixed, return non-zero
 * with the session unchanged. */
int tts_hip_orpheus_stream_begin(tts_hip_ctx *ctx, uint32_t n_slots, uint32_t max_new, uint32_t stop_id, const tts_hip_sampling *sampling);
int tts_hip_orpheus_stream_admit(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots, const uint32_t *prompts, const uint32_t *n_prompt, const float *uniforms);
int tts_hip_orpheus_stream_begin_mixed(tts_hip_ctx *ctx, uint32_t n_slots, uint32_t max_new, uint32_t stop_id);
int tts_hip_orpheus_stream_admit_mixed(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots, const uint32_t *prompts, const uint32_t *n_prompt,
                                       const tts_hip_sampling *const *sampling, const float *uniforms);
int tts_hip_orpheus_stream_run(tts_hip_ctx *ctx, uint32_t n_steps, uint32_t *n_finished, uint32_t *finished_slots, uint32_t *finished_counts);
int tts_hip_orpheus_stream_launch(tts_hip_ctx *ctx, uint32_t n_steps);
int tts_hip_orpheus_stream_wait(tts_hip_ctx *ctx, uint32_t *tokens_out, uint32_t *n_out, uint8_t *done, uint32_t *n_finished, uint32_t *finished_slots,
                                uint32_t *finished_counts);
int tts_hip_orpheus_stream_drop(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots);
int tts_hip_orpheus_stream_collect(tts_hip_ctx *ctx, uint32_t slot, uint32_t count, uint32_t *tokens_out);
int tts_hip_orpheus_stream_end(tts_hip_ctx *ctx);
/* the session's row-batched selection alone on caller-supplied logits [n_rows][vocab_size] (n_rows <= max_seqs), for parity tests: per row the contract
 * of tts_hip_orpheus_sample_logits with uniforms[r], last_id[r], rep_count[r]; sampling NULL: sampler::max per row (uniforms / state may be NULL) */
int tts_hip_orpheus_sample_logits_rows(tts_hip_ctx *ctx, uint32_t n_rows, const float *logits, const tts_hip_sampling *sampling, const float *uniforms, int32_t *last_id,
                                       uint32_t *rep_count, uint32_t *tokens_out);
/* the mixed session's selection alone: row r with sampling[r] (NULL: sampler::max), per row the contract of tts_hip_orpheus_sample_logits */
int tts_hip_orpheus_sample_logits_rows_mixed(tts_hip_ctx *ctx, uint32_t n_rows, const float *logits, const tts_hip_sampling *const *sampling, const float *uniforms,
                                             int32_t *last_id, uint32_t *rep_count, uint32_t *tokens_out);

/* ---- Dia encoder + decoder step (src/models/dia/model.cpp) --------------------------------------------------------
 * Device side of dia_runner::decode (:730-757): create, tts_hip_upload every "dia.*" tensor (names
 * py-gguf/tts_encoders/dia_gguf_encoder.py:72-131), tts_hip_finalize(ctx, NULL), tts_hip_dia_encode once per sentence
 * (build_dia_encoder :383-440 + build_dia_cross_kv_store :505-541, both streams), then tts_hip_dia_step per token.
 * Tokenisation (:661-705), the sampler, check_stopping / the delay pattern (:767-808) stay with the host; the codec is
 * the DAC context (tts_hip_create with TTS_HIP_FLAG_NO_PARLER, "audio_encoder.*"). */
typedef struct tts_hip_dia_desc {
    uint32_t struct_size;
    uint32_t enc_hidden_size;   /* width of dia.encoder.embedding (1024; model.h:68, no GGUF key)        */
    uint32_t enc_layers;        /* dia.encoder.layers (12)                                               */
    uint32_t enc_attn_heads;    /* dia.encoder.attn_heads (16): heads x head_dim == dec_hidden_size       */
    uint32_t dec_hidden_size;   /* dia.decoder.hidden_size (2048)                                        */
    uint32_t dec_layers;        /* dia.decoder.layers (18)                                               */
    uint32_t dec_attn_heads;    /* dia.decoder.attn_heads (16) query heads                               */
    uint32_t dec_kv_heads;      /* attn_heads / dia.decoder.query_heads (16 / 4 = 4 k/v groups, :463,468) */
    uint32_t head_dim;          /* dia.attn_head_size (128)                                              */
    uint32_t n_output_heads;    /* dia.decoder.output_heads (9)                                          */
    uint32_t output_vocab_size; /* dia.decoder.output_vocab_size (1028)                                  */
    uint32_t max_ctx;           /* dia.encoder.max_context_length (1024): the encoder always runs all of it */
    uint32_t max_gen;           /* dia.decoder.max_generation_size (3072) self-attention cache positions  */
    float    cfg_scale;         /* dia.cfg_scale (3.0, model.h:82); 0 = that                             */
    uint32_t flags;             /* TTS_HIP_FLAG_VALU_GEMM | TTS_HIP_FLAG_DEQUANT_Q | TTS_HIP_FLAG_NO_GRAPH (the device loop's steps run
                                   eagerly instead of as replays of one captured graph; the same launches once max_gen reaches
                                   128 x the self-attention's key splits, 1024 by default) */
    uint32_t max_utterances;    /* extension: utterances decoded in lock-step (each is the reference's batch of 2 guidance streams,
                                   dia/model.cpp:330-341); 0 = 1.  Rows of a step = 2 x utterances.  At most 128 (one decoder forward
                                   carries 256 rows): tts_hip_dia_create refuses more with an error that names it and max_utterances.
                                   Up to 64 slots every step launches the streaming kernels (<= 16 rows) or the 16-feature GEMM;
                                   on a context of 65 .. 128 slots a step of more than 16 rows runs fp16 matrices (K % 128 == 0,
                                   N % 16 == 0, no TTS_HIP_FLAG_VALU_GEMM) on the LDS-tiled MFMA GEMM — tts_hip_tune
                                   "dia_tile_min_rows" below.  One slot of Dia-1.6B is 1.06 GB of caches (0.53 GB with kv_type =
                                   TTS_HIP_F16); caches that do not fit fail tts_hip_finalize with the slot count and the bytes */
    uint32_t kv_type;           /* extension (the reference keeps fp32 K/V, dia/model.cpp:329): TTS_HIP_F32 (0, so a zeroed desc) or
                                   TTS_HIP_F16: the self cache [layer][row slot][max_gen][kv width] and the cross cache
                                   [layer][row slot][max_ctx][heads * head_dim] are kept in fp16 — half the cache memory
                                   (Dia-1.6B: 1.06 GB -> 0.53 GB per utterance slot) and half the bytes both attention launches of a
                                   step read.  Rotated K and V are rounded once, to nearest-even, as they are stored (a plain
                                   fp32 -> fp16 conversion, as under TTS_HIP_FLAG_KV_F16): a magnitude above 65504 becomes inf, one
                                   below 6.1e-5 keeps fewer bits (fp16 subnormals).  All arithmetic stays fp32: query, scores,
                                   softmax and the P.V sums run on the cache rows widened exactly; the encoder's own K/V
                                   scratch stays fp32.  Fixed at create for every call of the context: tts_hip_dia_encode /
                                   _encode_slot (cross K/V), tts_hip_dia_step / _step_batch, tts_hip_dia_generate, gen_* and
                                   stream_* (self K/V appended, both caches read).  Any other value is refused with an error that
                                   names tts_hip_dia_create and kv_type. */
} tts_hip_dia_desc;
tts_hip_ctx *tts_hip_dia_create(int device, const tts_hip_dia_desc *desc);
/* tokens [max_ctx]: the sentence bytes then zeros; the all-zero second stream is added here (:700-703).  Fills the cross
 * K/V of every decoder layer (K only for the first sentence_len positions, the rest zero as in a freshly cleared cache)
 * and resets nothing else: self-attention cache rows are overwritten as positions are decoded.
 * enc_out (may be NULL): [2][max_ctx][enc_hidden_size] final-normed encoder states. */
int tts_hip_dia_encode(tts_hip_ctx *ctx, const uint32_t *tokens, uint32_t sentence_len, float *enc_out);
/* one decoder step at position pos with the n_output_heads ids of the previous step (both streams get the same ids).
 * logits_out [n_output_heads][output_vocab_size]: cond + cfg_scale * (cond - uncond) (util.cpp:194-196);
 * raw_out (may be NULL): [2][n_output_heads][output_vocab_size] conditional, unconditional. */
int tts_hip_dia_step(tts_hip_ctx *ctx, const uint32_t *ids, uint32_t pos, float *logits_out, float *raw_out);
/* Lock-step utterances (BASELINE config 3: batch 32 = 4 utterances per GPU x 8 GPUs; SURVEY.md §8e: M = 8 rows per GPU).  The
 * reference decodes one utterance = 2 guidance rows per graph (:330-341, :705-721); here utterance slot u owns rows 2u (text) and
 * 2u+1 (all-zero twin) of every cache, tts_hip_dia_encode_slot fills its cross K/V, and one step carries the rows of n_utt slots:
 * ids [n_utt][n_output_heads], pos [n_utt] (a slot that has finished keeps stepping on its last position; its rows are ignored by
 * the host), slots [n_utt] or NULL (= 0..n_utt-1), logits_out [n_utt][n_output_heads][vocab] guided, raw_out (may be NULL)
 * [n_utt][2][n_output_heads][vocab].  tts_hip_dia_encode / _step are the slot-0, one-utterance forms. */
int tts_hip_dia_encode_slot(tts_hip_ctx *ctx, uint32_t slot, const uint32_t *tokens, uint32_t sentence_len, float *enc_out);
int tts_hip_dia_step_batch(tts_hip_ctx *ctx, uint32_t n_utt, const uint32_t *slots, const uint32_t *ids, const uint32_t *pos,
                           float *logits_out, float *raw_out);
/* The whole generate_from_batch loop (dia/model.cpp:806-870) on the device for utterance slots 0..n_utt-1 (encoded with
 * tts_hip_dia_encode_slot): per step check_stopping (:767-785: EOS on head 0 or position max_gen - max_delay starts the countdown that
 * forces EOS / PAD into the delayed heads), the decoder step, guidance, sampler::sample (sampling != NULL; sample_kernel, any top_k /
 * top_p / temperature / repetition penalty at this vocabulary) or sampler::max (NULL), and the delay-pattern feedback (:795-803) run
 * as one captured graph; the host looks at the done flags every few steps.  An utterance whose countdown has ended is parked (see the
 * session below: it is the same loop with every slot live from the first step) while the others go on.  uniforms [max_gen][n_utt][n_output_heads]: the draw for
 * head h of utterance u at its k-th sampler call (ignored for sampler::max).  tokens_out [n_utt][max_gen][n_output_heads]: the
 * sampled ids in generation order (the runner's output_tokens before adjust_output_tokens); steps_out [n_utt]: sampler calls made. */
typedef struct tts_hip_dia_codes {
    uint32_t bos, eos, pad;        /* dia.bos_token_id 1026, eos 1024, pad 1025 (model.h:70-72) */
    uint32_t max_delay;            /* model.h:74 (15) */
    uint32_t delay_pattern[16];    /* per output head (model.h:66: 0,8,9,...,15) */
} tts_hip_dia_codes;
int tts_hip_dia_generate(tts_hip_ctx *ctx, uint32_t n_utt, uint32_t max_gen, const tts_hip_dia_codes *codes, const tts_hip_sampling *sampling,
                         const float *uniforms, uint32_t *tokens_out, uint32_t *steps_out);
/* The same loop in pieces, for callers that work on the ids while the decoder is still running (the runner's chunked audio un-delays
 * frames and decodes codec windows meanwhile); tts_hip_dia_generate is built on them.
 *   gen_begin   checks and stages what tts_hip_dia_generate does: uniforms, penalty table, loop state (every slot 0..n_utt-1 live: ids = BOS,
 *               position 0, budget max_gen, the whole text context as cross extent)
 *   gen_launch  enqueues up to n_steps replays of the captured step (eager under TTS_HIP_FLAG_NO_GRAPH / profiling; the very first step
 *               runs eagerly and is then captured) and returns without waiting.  Never more than the max_gen + 1 pre-steps
 *               tts_hip_dia_generate allows; nothing once a gen_wait has seen every utterance done.
 *   gen_wait    waits for the launched steps and looks in — one gather launch, one copy, one synchronisation whatever n_utt is:
 *               steps_done [n_utt] = sampler calls made so far, done [n_utt] = the countdown has ended, *ran = pre-steps launched so far
 *               (each may be NULL), and — when tokens_out != NULL — the tokens of the steps no earlier gen_wait handed out, written at
 *               their places in tokens_out [n_utt][max_gen][n_output_heads] (NULL: they stay for a later gen_wait).
 * The generation is over when every done flag is set or *ran == max_gen + 1.  The ids do not depend on the launch sizes.  While steps are
 * in flight the codec context may run (its own context and stream); any other call on this context needs a gen_wait first, except that
 * tts_hip_dia_encode* / tts_hip_dia_step* / gen_begin / tts_hip_dia_generate wait for an unfinished loop themselves and drop it. */
int tts_hip_dia_gen_begin(tts_hip_ctx *ctx, uint32_t n_utt, uint32_t max_gen, const tts_hip_dia_codes *codes, const tts_hip_sampling *sampling,
                          const float *uniforms);
int tts_hip_dia_gen_launch(tts_hip_ctx *ctx, uint32_t n_steps);
int tts_hip_dia_gen_wait(tts_hip_ctx *ctx, uint32_t *tokens_out, uint32_t *steps_done, uint8_t *done, uint32_t *ran);
/* Continuous session: the loop of tts_hip_dia_generate — the same kernels and host code, not a copy — with utterances entering and leaving
 * while the others keep going.  Fixed shape: every step of a session steps all n_slots slots = 2 * n_slots rows through the decoder step
 * tts_hip_dia_generate runs at n_utt == n_slots (kernel selection depends on the row count, so it never changes inside a session), as one
 * captured graph per session configuration (kept beside the one of the gen_* calls: alternating the two recaptures neither).  What belongs to a slot's occupant — its step budget, its uniforms, the parked flag — is device memory: an admission changes
 * values, never the captured launches.
 *   begin    n_slots <= max_utterances slots, every one parked; max_gen, codes and sampling as in tts_hip_dia_generate (sampling NULL:
 *            sampler::max), with its limits.  An unfinished gen_* loop is waited for and dropped.  Slots no encoder pass has filled get the one
 *            cross K/V position their parked rows attend over cleared.
 *   admit    n utterances into free slots, between two runs: tokens [n][max_ctx] and sentence_len [n] as for tts_hip_dia_encode_slot, budget [n]
 *            (NULL: max_gen) with max_delay < budget <= max_gen: the utterance runs as under tts_hip_dia_generate with max_gen = budget;
 *            uniforms [n][max_gen][n_output_heads] for a sampled session (utterance i, sampler call k, head h), else NULL.  Per utterance the
 *            encoder pass and cross K/V fill of its slot, then ONE launch for all n: ids = BOS, position 0, countdown not started, sampler::reset,
 *            budget, the whole text context as cross extent, the uniforms into the slot's column of the sampler's [call][n_slots][head] block.
 *   run      enqueues n_steps replays (no more than the live slots' budgets leave) with no copy and no synchronise in between, then one look-in
 *            — one launch, one copy, one synchronise — that reads every slot's sampler calls and parked flag.  Slots whose countdown ended are
 *            reported with their step counts.  (No budget ends at admission: budget = max_delay + 1 makes max_delay sampler calls and is reported
 *            by the run that contains them, like any other.)  With no live slot nothing is launched.
 *            run is launch followed by a wait that takes no rows.
 *   launch   what run enqueues — the same cap from the live budgets, the eager first step and the capture, the same graph — and returns without
 *            synchronising.  A launch must be followed by a wait.
 *   wait     waits for the launched steps and looks in — one gather launch, one copy into pinned memory, one synchronise, whatever n_slots is:
 *            steps_done [n_slots] = sampler calls each slot's occupant has made, done [n_slots] = the slot is parked (each may be NULL), the
 *            slots whose countdown ended as run reports them, and — when tokens_out != NULL — the history rows of every slot that no earlier
 *            wait handed out, written at their places in tokens_out [n_slots][max_gen][n_output_heads] (NULL: they stay for a later wait).
 *            A slot's rows start at 0 again once it is admitted again.  With nothing launched a wait is a pure look-in.
 *   drop     parks n live slots at once, between a wait and the next launch, in one launch: done, the step count, position 0, one cross key,
 *            sampler call 1 — what the parking pre-step writes.  The slots are free again without being reported.
 *   collect  the first `steps` history rows [steps][n_output_heads] of a reported slot, before that slot is admitted again; it works as before
 *            after waits that took rows
 *   end      ends the session (steps in flight are waited for and dropped); the slots stay encoded with their last occupants
 * Parking: a slot is free when it has finished, was never admitted, or has been collected and not admitted again.  The pre-step that ends a
 * slot's countdown parks it: both rows move to position 0 and their cross extent to one key, so from that step on its self-attention and its
 * cross-attention read one position each, it records nothing and its sampler state stands still.  A finished utterance of tts_hip_dia_generate
 * / gen_* is parked the same way.  Leaving the loop (end; for gen_*, the call that drops it) sets every cross extent back to the whole context.
 * Equality: an utterance's ids and step count are those of tts_hip_dia_generate on a context with n_utt = n_slots, the utterance in the same
 * slot, max_gen = its budget and its uniforms in that slot's column — the same forward at the same row count, whoever else is live, parked or
 * admitted meanwhile (tests/test_gpu_dia_stream.py); greedy, they are also those of its one-utterance tts_hip_dia_generate at the test shapes.
 * The rows the waits hand out for an occupant tile its history without gap or overlap; they are what collect returns and what the same session
 * returns through run / collect, whatever the launch sizes are — hence the ids of tts_hip_dia_generate at n_utt = n_slots — and dropping a slot
 * changes no other slot's ids (tests/test_gpu_dia_stream_chunked.py).
 * Ordering: admit, collect, drop, run or a second launch while steps are in flight return non-zero before anything is launched and leave the
 * session as it was; so does a drop of a slot that is not live, is >= n_slots or is named twice.
 * Between begin and end every other generation call on the context (tts_hip_dia_encode*, _step*, _generate, gen_begin / gen_launch / gen_wait)
 * is refused with an error, and so is a second begin.  Every misuse (n_slots > max_utterances, a busy slot, a slot >= n_slots or named twice,
 * collect on a slot that has not been reported or for more steps than it made, a budget outside (max_delay, max_gen], a sentence length outside
 * 1..max_ctx, a sampled session without uniforms, sampler limits) returns non-zero before anything is launched; the context stays usable.
 * Mixed session: begin_mixed is begin with every slot carrying its own sampler, so utterances that differ in top_k, top_p, temperature or
 * repetition penalty, greedy ones among them, share one loop; its checks are begin's (output_vocab_size <= 2048 also when every occupant
 * will be greedy).  The step is the session's — pre-step, forward, guidance, post-step — with ONE sample_kernel launch in place of the
 * arg-max / sampler alternative: every row reads its slot's record {mode, top_k, top_p, temperature, its own repetition-penalty table}; a greedy
 * row takes the kernel's first phase (sampler::max: first maximum wins, the id the arg-max kernel gives), reads no uniform and touches no sampler
 * state; a parked slot sits out as before.  admit_mixed is admit with sampling[i] per utterance (sampling NULL or sampling[i] NULL: sampler::max;
 * else the limits of tts_hip_dia_generate, checked for all n before anything is launched) and uniforms [n][max_gen][n_output_heads], where the
 * block of a greedy utterance is ignored; uniforms may be NULL when all n are greedy and is refused with a sampled one.  The ONE admission launch
 * also rewrites the slot's record, its own table [max_gen] (pow(penalty, count) in double, evaluated on the host) and its last_token_ids /
 * repetition_counts (sampler::reset), so nothing of the previous occupant survives.  run, launch, wait, drop, collect and end are the calls above
 * and work on either kind of session.  The mixed session has a captured graph of its own beside the fixed batch's and the uniform session's:
 * alternating the three recaptures none, and no admission ever recaptures.  admit_mixed on a session opened by begin, and admit on one opened by
 * begin_mixed, return non-zero with the session unchanged.
 * Equality (mixed): an utterance's ids and step count are those of tts_hip_dia_generate on a context with n_utt = n_slots, the utterance in the
 * same slot, max_gen = its budget, its own sampler (NULL for a greedy one) and its uniforms in that slot's column — whoever else is live, parked,
 * greedy or sampled in the other slots, and whatever the launch sizes (tests/test_gpu_dia_stream_mixed.py). */
int tts_hip_dia_stream_begin(tts_hip_ctx *ctx, uint32_t n_slots, uint32_t max_gen, const tts_hip_dia_codes *codes, const tts_hip_sampling *sampling);
int tts_hip_dia_stream_admit(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots, const uint32_t *tokens, const uint32_t *sentence_len, const uint32_t *budget,
                             const float *uniforms);
int tts_hip_dia_stream_begin_mixed(tts_hip_ctx *ctx, uint32_t n_slots, uint32_t max_gen, const tts_hip_dia_codes *codes);
int tts_hip_dia_stream_admit_mixed(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots, const uint32_t *tokens, const uint32_t *sentence_len,
                                   const uint32_t *budget, const tts_hip_sampling *const *sampling, const float *uniforms);
int tts_hip_dia_stream_run(tts_hip_ctx *ctx, uint32_t n_steps, uint32_t *n_finished, uint32_t *finished_slots, uint32_t *finished_steps);
int tts_hip_dia_stream_launch(tts_hip_ctx *ctx, uint32_t n_steps);
int tts_hip_dia_stream_wait(tts_hip_ctx *ctx, uint32_t *tokens_out, uint32_t *steps_done, uint8_t *done, uint32_t *n_finished, uint32_t *finished_slots,
                            uint32_t *finished_steps);
int tts_hip_dia_stream_drop(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots);
int tts_hip_dia_stream_collect(tts_hip_ctx *ctx, uint32_t slot, uint32_t steps, uint32_t *tokens_out);
int tts_hip_dia_stream_end(tts_hip_ctx *ctx);

/* ---- Kokoro (src/models/kokoro/model.cpp) ----------------------------------------------------------------------------
 * Device side of kokoro_duration_runner::run (:1069-1123) and kokoro_runner::run (:1277-1325): create, tts_hip_upload every
 * "kokoro.*" tensor (names py-gguf/tts_encoders/kokoro_gguf_encoder.py), tts_hip_finalize(ctx, NULL), then per clause
 * tts_hip_kokoro_durations (ALBERT + prosody predictor + duration head) and tts_hip_kokoro_generate (alignment ... iSTFT).
 * The phonemizer, the tokenizer, clause chunking (:1340-1388) and the source-noise draws (set_inputs :1255) stay with the host.
 * First version: plain fp32 kernels (csrc/kokoro_kernels.h). */
typedef struct tts_hip_kokoro_desc {
    uint32_t struct_size;
    uint32_t n_attn_heads;       /* kokoro.duration_predictor.albert.attn_heads (12) */
    uint32_t n_recurrence;       /* ...albert.recurrence (12): the one shared layer is applied this many times */
    uint32_t n_dp_layers;        /* kokoro.duration_predictor.layers (3) */
    uint32_t f0_n_blocks;        /* kokoro.duration_predictor.f0_n_blocks (3) */
    uint32_t n_conv_layers;      /* kokoro.text_encoder.layers (3) */
    uint32_t n_decoder_blocks;   /* kokoro.decoder.generator.layers (4) */
    uint32_t n_upsamples;        /* kokoro.decoder.generator.upsamples (2) */
    uint32_t n_kernels;          /* kokoro.decoder.generator.kernels (3) */
    uint32_t n_fft, hop;         /* kokoro.decoder.generator.{n_fft,hop} (20, 5) */
    uint32_t harmonic_num;       /* 8 (model.h:218) */
    uint32_t up_sampling_factor; /* kokoro.decoder.generator.up_sampling_factor (600 samples per duration frame) */
    uint32_t out_conv_padding;   /* kokoro.decoder.generator.padding (3) */
    uint32_t max_ctx;            /* ...albert.context_length (512) tokens per call */
    float    attn_scale;         /* 0.125 (model.h:196: not derived from the head size) */
    float    upsample_scale;     /* 300 (model.h:195) */
    float    sample_rate, sin_amp, noise_std, voice_threshold;   /* 24000, 0.1, 0.003, 10 (model.h:219-222) */
    uint32_t up_stride[4], up_padding[4];             /* kokoro.decoder.generator.up_convs.i.{stride,padding} */
    uint32_t noise_stride[4], noise_padding[4];       /* ...noise_blocks.i.{stride,padding} */
    uint32_t res_padding[16][3], res_dilation[16][3]; /* ...res_blocks.i.j.{padding,dilation} */
    uint32_t noise_res_padding[4][3], noise_res_dilation[4][3];   /* ...noise_blocks.i.res_block.j.{padding,dilation} */
    uint32_t flags;
} tts_hip_kokoro_desc;
tts_hip_ctx *tts_hip_kokoro_create(int device, const tts_hip_kokoro_desc *desc);
/* tokens [n] (bos, phoneme ids, eos); voice: the name after "kokoro.voice_tensors."; lens_out [n] = clamp(round(sum of the
 * duration sigmoids), 1, 50) (:1035-1037); hidden_out [n][duration hidden + style half] (:1029-1031) */
int tts_hip_kokoro_durations(tts_hip_ctx *ctx, const uint32_t *tokens, uint32_t n, const char *voice, float *lens_out, float *hidden_out);
#define TTS_HIP_KOKORO_ROWS_MAX 8
/* B clauses in one pass. tokens: the clauses' ids back to back; n[b] in 3..max_ctx; voices[b]: name after "kokoro.voice_tensors.".
 * lens_out [sum n], hidden_out [sum n][duration hidden + style half] (may be NULL), both in the caller's clause order.
 * Every clause's lens / hidden are bit for bit what tts_hip_kokoro_durations gives for that clause alone under the same tune keys.
 * Inside, the clauses are worked on sorted by non-increasing length (stable); the recurrences of all clauses advance in lock-step
 * (kk_lstm_rows_kernel, csrc/kokoro_kernels.h), so similar lengths waste the fewest steps. */
int tts_hip_kokoro_durations_batch(tts_hip_ctx *ctx, const uint32_t *tokens, const uint32_t *n, uint32_t B,
                                   const char *const *voices, float *lens_out, float *hidden_out);
/* lens [n]: whole numbers (the predicted ones, or forced); hidden [n][duration hidden + style half] from the call above;
 * noise [(harmonic_num + 1) * total * up_sampling_factor] uniform draws, total = sum(lens); pcm_out [total * up_sampling_factor].
 * hsrc_out / hsrc_in (may be NULL) [2 * (n_fft / 2 + 1)][2 * total * upsample_scale / hop + 1]: the STFT conditioning read out /
 * replaced (its phase channels wrap at +-pi, see oracle/kokoro_oracle.c). */
int tts_hip_kokoro_generate(tts_hip_ctx *ctx, const uint32_t *tokens, uint32_t n, const float *lens, const float *hidden, const char *voice, const float *noise,
                            float *pcm_out, float *hsrc_out, const float *hsrc_in);

/* ---- SNAC codec (src/decoder/snac_model.cpp; Orpheus' audio decoder) -------------------------------
 * A SNAC context is its own tts_hip_ctx: create, tts_hip_upload every "snac.*" tensor (names:
 * py-gguf/tts_encoders/orpheus_gguf_encoder.py:89-142), tts_hip_finalize(ctx, NULL), tts_hip_snac_decode. */
typedef struct tts_hip_snac_desc {
    uint32_t struct_size;
    uint32_t n_blocks;                          /* snac_model::n_layers (4) */
    uint32_t stride[TTS_HIP_MAX_DAC_BLOCKS];    /* snac.snac_layer_stride_i   (snac_model.cpp:26-48) */
    uint32_t padding[TTS_HIP_MAX_DAC_BLOCKS];   /* snac.snac_layer_padding_i  */
    uint32_t groups[TTS_HIP_MAX_DAC_BLOCKS];    /* snac.snac_layer_grouping_i: must equal the layer's channel count (depthwise, gnac.cpp:136-140) */
    uint32_t n_codebooks;                       /* snac.audio_token_channels (3) */
    uint32_t repeats[4];                        /* 4, 2, 1 (snac_model.h:17) */
    uint32_t max_frames;                        /* snac.max_generation_size: finest-level tokens per call */
    uint32_t flags;                             /* TTS_HIP_FLAG_VALU_GEMM */
} tts_hip_snac_desc;
tts_hip_ctx *tts_hip_snac_create(int device, const tts_hip_snac_desc *desc);
/* snac_runner::run (snac_model.cpp:180-208).  codes: level-major ids as set_inputs lays them out (:161-178): T/repeats[0]
 * of level 0, T/repeats[1] of level 1, ...; noise: per layer l, T * prod(stride_0..l) floats, concatenated (:131-137) —
 * the reference draws them from an unseeded normal generator (:177), here they are the caller's; NULL = no noise;
 * pcm_out: T * prod(strides) fp32 samples.  Every transposed conv must have 2 * padding == stride (each stage exactly `stride` times longer than
 * the one before, as in every SNAC release: padding ceil(s / 2), even strides); another layout is refused with an error.  Not to be called
 * between tts_hip_snac_decode_windows_begin and _end. */
int tts_hip_snac_decode(tts_hip_ctx *ctx, const uint32_t *codes, uint32_t T, const float *noise, float *pcm_out);
/* Chunked audio.  A SNAC frame is one group of 7 Orpheus ids = repeats[0] (4) finest-level tokens = 4 * prod(strides) samples.  The samples of
 * frame j depend on the codes and the noise of frames [j - h, j + h] only; h follows from the layout alone (no device): 3 for snac_24khz
 * (strides 8, 8, 4, 2), 5 for strides 4, 2.  -1 (tts_hip_last_error) for a layout the rule does not describe: other than three levels at
 * repeats 4 / 2 / 1, or a transposed conv whose padding is not half its stride. */
int tts_hip_snac_halo_frames(const tts_hip_snac_desc *desc);
/* n windows decoded in one pass as separate utterances, each cropped to the samples of its frames [keep0[i], keep1[i]) (relative to the
 * window); pcm_out receives the kept pieces back to back.  Per window the codes are level-major (T/4, T/2, T ids, T = 4 * frames[i]) and
 * the noise layer-major (per layer l, T * prod(stride_0..l) floats) as for tts_hip_snac_decode; windows are concatenated; noise NULL = no
 * noise block.  A window that reaches h frames beyond the kept ones on every side that is not an end of the utterance gives the kept
 * frames the samples of the whole utterance's decode (under the same noise samples).
 * _begin copies its inputs, enqueues the pass on the SNAC context's stream and returns; _end waits, after which pcm_out of _begin is
 * valid.  Between the two no other call on this context.  tts_hip_snac_decode_windows = _begin + _end. */
int tts_hip_snac_decode_windows(tts_hip_ctx *ctx, const uint32_t *codes, const uint32_t *frames, const uint32_t *keep0, const uint32_t *keep1, uint32_t n,
                                const float *noise, float *pcm_out);
int tts_hip_snac_decode_windows_begin(tts_hip_ctx *ctx, const uint32_t *codes, const uint32_t *frames, const uint32_t *keep0, const uint32_t *keep1, uint32_t n,
                                      const float *noise, float *pcm_out);
int tts_hip_snac_decode_windows_end(tts_hip_ctx *ctx);

/* ---- DAC codec --------------------------------------------------------------------------- */
/* dac_runner::run (dac_model.cpp:172-212): codes [frames][n_output_heads] (frame-major),
 * pcm_out: frames * prod(strides) fp32 samples in host memory.  Blocks until done. */
int tts_hip_dac_decode(tts_hip_ctx *ctx, const uint32_t *codes, uint32_t frames, float *pcm_out);
/* The same for n utterances in one pass (extension; the reference decodes one utterance per dac_runner::run).
 * codes: the utterances' code frames concatenated [sum(frames)][n_output_heads]; frames[n]; pcm_out: the PCM of
 * the utterances concatenated (frames[i] * prod(strides) samples each).  Results are identical to n single calls. */
int tts_hip_dac_decode_batch(tts_hip_ctx *ctx, const uint32_t *codes, const uint32_t *frames, uint32_t n, float *pcm_out);
/* Halo of the codec in code frames: the samples of frame j depend only on the codes of frames [j - h, j + h].  A pure function of
 * dac_n_blocks / dac_stride / dac_padding (no device); h = 10 for the DAC-44k layout (strides 8, 8, 4, 2).  -1 on a layout it does not
 * describe (padding > stride). */
int tts_hip_dac_halo_frames(const tts_hip_desc *desc);
/* n windows of code frames decoded in one pass as separate utterances (tts_hip_dac_decode_batch), each cropped to the samples of its frames
 * [keep0[i], keep1[i]).  codes: the windows' frames concatenated; pcm_out: (keep1[i] - keep0[i]) * prod(strides) samples per window,
 * concatenated.  A window that reaches h frames past its kept frames on each side (or the utterance's edge) reproduces the samples of
 * the whole utterance's decode.  Blocks until done. */
int tts_hip_dac_decode_windows(tts_hip_ctx *ctx, const uint32_t *codes, const uint32_t *frames, const uint32_t *keep0, const uint32_t *keep1,
                               uint32_t n, float *pcm_out);

/* ---- introspection (tests, bench) -------------------------------------------------------- */
/* Copy an internal buffer to the host.  what: "hidden" (final-normed hidden of the last forward,
 * [rows][H]), "k:<layer>:<seq>" / "v:<layer>:<seq>" (cache rows [n_pos][H] as fp32),
 * and, of the last attention launch of the last forward (these buffers outlive it, a graph replay included; without cross-attention it is
 * the last layer's self-attention, with cross-attention and fp32 matrices the last layer's cross-attention; reading them changes no
 * dispatch decision, unlike tts_hip_set_debug): "q" (the query rows it read) and "att" / "att16" (the fp32 / fp16 rows it left, the fp16
 * ones widened exactly), all [rows][H] with rows = max_floats / H; "pos" / "seq" (the rows' positions and cache slots as the device holds
 * them, as floats); "part:<nz>" (the key-slice partials of a launch with nz slices: [rows][heads][nz][66] = the slice's maximum (-inf:
 * an empty slice), its sum and its 64 unnormalised channels, rows = max_floats / (heads * nz * 66));
 * "dac:<stage>" (activation after DAC stage, see oracle stage numbering; requires
 * tts_hip_set_debug(ctx,1) before the decode); SNAC contexts: "snac:<stage>" (utterance 0's valid region
 * [C][tokens * rate] after the stage of the last pass, orc_snac_decode's numbering: 0 = the summed codebook levels, 1 = after
 * the input depthwise conv and the `up` conv, 2 + i = the end of block i, 2 + n_blocks = the PCM before the crop; requires
 * tts_hip_set_debug(ctx,1) before the decode); Orpheus contexts: "l_logits" (the logits row the last
 * step left), "l_k:<layer>[:<slot>]" / "l_v:<layer>[:<slot>]" (a cache slot of a layer, [n_ctx][kv width]; slot 0 by default; an fp16 or e4m3 cache
 * comes back widened to fp32, exact), "l_kv_elem" (the cache element size in bytes: 4, 2 or 1), and of the
 * last layer of the last forward — these buffers outlive it, a captured step included — "l_q" (the rotated queries the attention
 * kernel read) and "l_att" (the rows it left), both [rows][heads * head_dim] with rows = max_floats / (heads * head_dim), "l_pos" (the
 * rows' positions as floats; a captured step's selection has already advanced row 0 by one).
 * Dia contexts: with tts_hip_set_debug(ctx,1) an eager tts_hip_dia_step_batch keeps, per layer and per kind, what its attention launch
 * consumed and produced: "di_attn:<layer>:<self|cross>:q" (self: the rotated rows [R][ld]; cross: the raw query slabs, n_parts of them
 * part_stride floats apart, which the kernel sums in slab order and rotates at the row's position), ":out" ([R][heads * head_dim]) and
 * ":meta" (n_parts, part_stride, ld, R, then pos[R], kend[R], row_seq[R]).  "di_k:<layer>:<row slot>" / "di_v:..." are a row slot's
 * self-attention cache [max_gen][kv width], "di_ck:..." / "di_cv:..." its cross K / V [max_ctx][heads * head_dim] (fp16 caches, kv_type =
 * TTS_HIP_F16: the rows widened exactly); "di_kv_elem" is the caches' element size in bytes (4 or 2).  With debug off every
 * forward launches exactly what it launches without these items; nothing is kept during a graph capture.
 * Any context: "tile_pair" (two values: the tune key "tile_pair" as the tiled GEMM launches read it, i.e. what the default came to at the context's
 * first tiled launch, -1 before it; and the most LDS in bytes that a tiled GEMM launch of the context has asked for since the key was last set).
 * Returns number of floats written or <0. */
int64_t tts_hip_debug_read(tts_hip_ctx *ctx, const char *what, float *out, size_t max_floats);
int     tts_hip_set_debug(tts_hip_ctx *ctx, int on);
/* Test entry: one LDS-tiled GEMM y = W · a on the caller's fp16 operands (W [N][K], a [R][K], K a multiple of 128 and >= 256, N of 16), launched as a
 * decoder forward launches it, i.e. under the context's tile keys (tune "tile_force", "tile_deep", "tile_pair"), without a K split.  The context need not
 * be finalized.  epi: 0 store (out [R][N]); 1 q | k | v with cache append (N = 3 H: out = q [R][H], out2 = K | V caches [2][R][3][H] fp32, row r is
 * sequence r at position r % 3); 2 residual (out [R][N], read and written); 3 GELU (out [R][N], out2 the same rows as fp16, [R][N] uint16); 4 the
 * cross-attention inside the 64 x 64 tiles (N = H a multiple of 64, aux = K_c | V_c [2][E][H] fp32, E <= 32; out = the attended rows [R][H]; needs
 * tile_force = 3).  Returns 0 or -1 (tts_hip_last_error). */
int     tts_hip_debug_tile_gemm(tts_hip_ctx *ctx, int epi, int R, int N, int K, int H, int E, const void *W16, const void *A16, const float *aux, float *out, void *out2);

/* Per-kernel-class timing with HIP events on the context's stream.  While enabled, forwards are
 * launched eagerly and every launch of every class is bracketed by an event pair. */
enum tts_hip_kclass {
    TTS_HIP_K_EMBED = 0,        /* embed_rows_kernel */
    TTS_HIP_K_LN = 1,           /* ln_rows_kernel (LayerNorm as its own launch, > 8 rows) */
    TTS_HIP_K_GEMM_QKV = 2,     /* [LN +] fused q/k/v projection + KV-cache append */
    TTS_HIP_K_ATTN_SELF = 3,    /* attn_kernel (+ attn_combine_kernel) over the self-attention cache */
    TTS_HIP_K_GEMM_ATTN_OUT = 4,/* self_attn.out_proj + residual */
    TTS_HIP_K_GEMM_CROSS_Q = 5, /* [LN +] encoder_attn.q_proj */
    TTS_HIP_K_ATTN_CROSS = 6,   /* attn_kernel over the voice-prompt K/V */
    TTS_HIP_K_GEMM_CROSS_OUT = 7,/* encoder_attn.out_proj + residual */
    TTS_HIP_K_GEMM_FC1 = 8,     /* [LN +] fc1 + GELU */
    TTS_HIP_K_GEMM_FC2 = 9,     /* fc2 + residual */
    TTS_HIP_K_GEMM_HEADS = 10,  /* [LN +] 9 lm heads */
    TTS_HIP_K_SAMPLE = 11,      /* argmax_kernel + feed_kernel */
    TTS_HIP_K_GEMM_OTHER = 12,  /* cross K/V precompute */
    TTS_HIP_K_DAC_EMBED = 13,   /* dac_embed_kernel */
    TTS_HIP_K_DAC_CONV7 = 14,   /* conv1d k=7 (initial + residual units) */
    TTS_HIP_K_DAC_CONV1 = 15,   /* conv1d k=1 (+ residual add) */
    TTS_HIP_K_DAC_CONVT = 16,   /* ConvTranspose1d upsampling */
    TTS_HIP_K_DAC_FINAL = 17,   /* final Cout=1 conv + tanh */
    TTS_HIP_K_DAC_RESUNIT = 18, /* resunit_b3_kernel: one residual unit (snake, k=7 conv, snake, k=1 conv, + x) in one launch */
    TTS_HIP_K_KOKORO_CONV = 19, /* Kokoro's stride-1 "same" convolutions on conv1d_mfma_kernel (exact-fp32 MFMA) */
    TTS_HIP_K_COUNT = 20
};
typedef struct tts_hip_kstat {
    double   ms_total;      /* summed event-elapsed time */
    uint64_t launches;
    double   bytes_total;   /* ALGORITHMIC bytes (weights + activations + cache rows each launch must touch) */
    double   flops_total;   /* algorithmic flops */
} tts_hip_kstat;
/* Arithmetic of the codec convolutions of this context (bench.py prices each kernel family against the pipe it runs on): bit 0 = the
 * k = 7 convs of the wide classes as bf16 x 3 split products (TTS_HIP_DAC_BF16X3), bit 1 = residual units of 96 / 192 channels as one
 * launch, bf16 x 3 (TTS_HIP_DAC_FUSE), bit 2 = transposed convs as bf16 x 3 (TTS_HIP_DAC_CONVT_B3), bit 5 (32) = the wide classes keep their activations as bf16 x 3 split planes, so
 * their k = 1 convs are bf16 x 3 products too (TTS_HIP_DAC_PLANES; otherwise exact-fp32 MFMA); 8 = F16 tensors (fp16 im2col, fp16
 * MFMA); 16 = scalar-FMA cross-check kernels; 0 = exact-fp32 MFMA throughout or no codec. */
int tts_hip_dac_arith(tts_hip_ctx *ctx);
int tts_hip_profile(tts_hip_ctx *ctx, int enable);        /* 1: every launch, forwards run eagerly; 2: only the launches that are
                                                              never graph-captured (the DAC), decoder steps keep replaying their
                                                              hipGraph; 0: off.  Enabling clears the counters. */
int tts_hip_profile_get(tts_hip_ctx *ctx, int kclass, tts_hip_kstat *out);
const char *tts_hip_kclass_name(int kclass);

/* ---- continuous batching: a generation that admits new utterances while others are running -----------------------------------------
 * Replaces, for a serving loop, "form a batch from what is queued, run it to the end" (examples/server/server.cpp:126-158 is the queue this
 * widens; parler/model.cpp:762-792 the loop).  The context needs max_seqs >= n_slots + 1: cache slot n_slots pads the lock-step forward.
 *   begin   fixes n_slots, the per-utterance step budget max_steps (token buffer [max_steps][n_slots + 1][heads]), bos / eos and the sampler
 *           (sp == NULL: sampler::max; else sampler::sample on the device as in tts_hip_parler_generate_sampled)
 *   admit   n utterances into free slots: prompts concatenated in ids, lens[i] ids each (prefilled as one side batch, positions from 0);
 *           uniforms [n][max_steps][heads] for a sampled stream (the host-drawn std::minstd_rand sequence of each utterance), else NULL
 *   run     n_steps lock-step decode steps over the live utterances; then *n_finished slots whose check_stopping() fired (EOS on every head,
 *           position == the cached positions, or max_steps reached) are reported with their step counts and become free
 *           run is launch followed by a wait that takes no rows.
 *   launch  what run enqueues — the rows staged (ids, positions, cache slots, step counters, padding rows), the same choice of step (arg-max,
 *           sampled, mixed; with or without voices), the same captured graphs — and returns without synchronising.  A launch must be followed
 *           by a wait.
 *   wait    waits for the launched steps and looks in: the rows' state and steps_done come back, and a wait that takes rows adds one
 *           parler_stream_lookin_kernel launch and one copy of its block into pinned memory, whatever n_slots is; one synchronise.
 *           steps_done [n_slots] = decode steps each slot's occupant has recorded so far, done [n_slots] = the slot's check_stopping() has fired
 *           (each may be NULL), the finished slots as run reports them, and — when tokens_out != NULL — the token rows of every live or
 *           just-finished slot that no earlier wait handed out, written at their places in tokens_out [n_slots][max_steps][heads]; rows above
 *           steps_done are not touched (NULL: they stay for a later wait).  A slot that finishes inside an interval steps on to the interval's
 *           end; only its rows below its step count are handed out.  A slot's rows start at 0 again once it is admitted again.  With nothing
 *           launched a wait is a pure look-in.  The staging is sized by begin for 64 steps per slot: a wait that finds more enqueued since
 *           the last wait that took rows goes round again, one launch, copy and synchronise per 64; no wait allocates.
 *   drop    takes n live slots out at once, between a wait and the next launch.  The row list lives on the host and every launch stages it
 *           afresh, so nothing runs on the device.  The slots are free again without being reported.
 *   collect the tokens [steps][heads] of a finished slot (before the slot is admitted again); it works as before after waits that took rows
 *   end     ends the session (steps in flight are waited for and dropped); so does the tts_hip_parler_gen_begin / generate_* that ends one
 * An utterance's tokens are those of a solo tts_hip_parler_generate_* run of the same prompt (tests/test_gpu_runner.py).
 * The rows the waits hand out for an occupant tile its history without gap or overlap; they are what collect returns and what the same session
 * returns through run / collect, whatever the launch sizes are — under the proviso below about row counts that select another GEMM tile shape —
 * and dropping a slot changes no other slot's tokens (tests/test_gpu_parler_stream_chunked.py).
 * Ordering: admit, admit_mixed, collect, drop, run or a second launch while steps are in flight return non-zero before anything is launched
 * and leave the session as it was, and so do tts_hip_parler_voice_set and tts_hip_parler_seq_voices; so does a drop of a slot that is not
 * live, is >= n_slots or is named twice.  tts_hip_dac_decode_windows stays callable between a launch and its wait: that is where the audio
 * of the last look-in is decoded.
 * Mixed session: begin_mixed is begin with every slot carrying its own sampler, so utterances that differ in top_k, top_p, temperature or
 * repetition penalty, greedy ones among them, share one lock-step forward.  Its checks are begin's, and output_vocab_size <= 2048 also when every
 * occupant will be greedy.  It sizes, once, the uniforms [max_steps + 1][n_slots + 1][heads], a sampler record per slot {mode, top_k, top_p,
 * temperature, its own repetition-penalty table} — the padding slot's record is sampler::max for good — and the tables [n_slots][max_steps]; they
 * stay on the context from one session to the next, and no admission reallocates or recaptures.
 *   admit_mixed   admit with sampling[i] per utterance: sampling NULL or sampling[i] NULL means sampler::max, else the limits of
 *           tts_hip_parler_generate_sampled (temperature, top_p, repetition_penalty > 0).  uniforms is [n][max_steps][heads]; the block of a
 *           greedy utterance is ignored; uniforms may be NULL when all n are greedy and is refused with a sampled one.  Every check (admit's,
 *           the sampler limits, the uniforms) runs for all n before anything is launched: a refusal returns non-zero, the session unchanged.
 *           After the prompts' side batch ONE launch clears the slots' EOS flags and steps_done, resets last_token_ids /
 *           repetition_counts (sampler::reset), writes each slot's record and its own table (pow(penalty, count) in double, evaluated on the
 *           host) and scatters the draws into the slot's column, so nothing of the previous occupant survives.
 * run, collect and end are the calls above and serve either kind of session.  A run whose live slots are all greedy replays the captured step of
 * a uniform greedy session (the arg-max launch); any other run replays the mixed step, where ONE sample_kernel launch reads every row's record
 * through its cache slot: a greedy row takes the kernel's first phase (sampler::max: first maximum wins, the id the arg-max kernel gives), reads
 * no uniform and touches no sampler state.  Both graphs stay cached per row count: alternating between them recaptures nothing, and no
 * admission recaptures.  admit_mixed on a session opened by begin, and admit on one opened by begin_mixed, return non-zero, the session unchanged.
 * Equality (mixed): an utterance's tokens and step count are those of tts_hip_parler_generate_greedy / tts_hip_parler_generate_sampled for the
 * same prompt with its own sampler and uniforms — whoever else is live, greedy or sampled, and whenever it entered
 * (tests/test_gpu_parler_stream_mixed.py).  As for the uniform session this holds where the row count does not select another GEMM tile shape,
 * that is another fp32 summation order: the row-count rounding pins it for the decode steps, the tests pin it for the reference run. */
int tts_hip_parler_stream_begin(tts_hip_ctx *ctx, uint32_t n_slots, uint32_t max_steps, uint32_t bos, uint32_t eos, const tts_hip_sampling *sp);
int tts_hip_parler_stream_admit(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots, const uint32_t *ids, const uint32_t *lens, const float *uniforms);
int tts_hip_parler_stream_begin_mixed(tts_hip_ctx *ctx, uint32_t n_slots, uint32_t max_steps, uint32_t bos, uint32_t eos);
int tts_hip_parler_stream_admit_mixed(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots, const uint32_t *ids, const uint32_t *lens,
                                      const tts_hip_sampling *const *sampling, const float *uniforms);
int tts_hip_parler_stream_run(tts_hip_ctx *ctx, uint32_t n_steps, uint32_t *n_finished, uint32_t *finished_slots, uint32_t *finished_steps);
int tts_hip_parler_stream_launch(tts_hip_ctx *ctx, uint32_t n_steps);
int tts_hip_parler_stream_wait(tts_hip_ctx *ctx, uint32_t *tokens_out, uint32_t *steps_done, uint8_t *done, uint32_t *n_finished, uint32_t *finished_slots,
                               uint32_t *finished_steps);
int tts_hip_parler_stream_drop(tts_hip_ctx *ctx, uint32_t n, const uint32_t *slots);
int tts_hip_parler_stream_collect(tts_hip_ctx *ctx, uint32_t slot, uint32_t steps, uint32_t *tokens_out);
int tts_hip_parler_stream_end(tts_hip_ctx *ctx);

/* ---- per-request voice descriptions: rows of ONE lock-step forward attending over different descriptions -----------------------------
 * A context holds its own description (the arena's, or tts_hip_parler_set_text_encoding's): voice 0.  A voice bank adds voices 1 .. n_voices,
 * and every cache slot carries the voice its utterance attends over, so two requests with different voices share a prefill, a step, a
 * generation or a session run.
 *   voice_bank(n_voices)      room for voices 1 .. n_voices (1 .. 256): per voice [L][2][32][H] fp32 cross K / V and a length (Parler-Mini:
 *           6.3 MB), the device table of the slots' voices [max_seqs + padding slot] (all 0) and its host mirror.  Once per context (captured
 *           steps hold the addresses); a context on a shared arena has a bank of its own; tts_hip_destroy frees it.  Out of memory is
 *           reported with the context unchanged.
 *   voice_set(voice, enc, n)  the entry's K / V from the T5 output enc [n][H], by the launches that compute the context's own cross K / V
 *           (bit for bit what tts_hip_parler_set_text_encoding(enc, n) leaves in "cross:").  Refused: n outside 1..32 — a bank entry holds
 *           32 positions, what the short cross-attention body covers; voice 0 or a voice beyond the bank; a voice some live cache slot uses;
 *           steps in flight (between tts_hip_parler_gen_launch and its tts_hip_parler_gen_wait).
 *   seq_voices(n, seqs, voices)  the voice of n cache slots.  Allowed with no generation open, and inside a session between two runs for
 *           slots that are not live: a voice enters BEFORE tts_hip_parler_stream_admit*, whose prefill already attends.  Refused: a live
 *           slot (a session's live slot, a row of an open generation); a voice never set or beyond the bank; steps in flight; a session's
 *           padding slot (it stays at voice 0); a non-zero voice while the context's own description has more than 32 positions (voice 0
 *           then cannot join a mixed forward; tts_hip_parler_set_text_encoding refuses the other order).
 * Every misuse returns non-zero before anything is launched and leaves the context usable.
 * The forward: whether a prefill / step / generation / session run is "mixed" is decided on the host when its rows are staged — it is when
 * any slot involved carries a non-zero voice — and never inside a run (a generation keeps its choice through row compactions).  When none
 * does, the forward is the one-description forward, launch for launch.  A mixed forward runs the cross-q projection with a plain store,
 * tries neither cross-attention fold, and runs attn_short_voices_kernel where the unfolded chain runs the cross-attention: per row the
 * statements of attn_short_kernel, on the K / V base and length of the row's voice (voice 0: the context's own).  The out projection reads
 * the attended rows as the unfolded chain does, quantised matrices included.  No existing kernel is changed.
 * Equality: the logits (and so the tokens) of a row with voice v are bit for bit those of a context whose own description is v's encoding,
 * run with tune("cross_fold") = 0 over the same rows, ids and positions (tests/test_gpu_parler_voices.py).  Against the folded
 * one-description forward the project's tolerances hold (another summation order).
 * Captured steps: the mixed step has graph keys of its own beside the one-description step's.  The slots' voices, the lengths and the
 * bank are read through device pointers, so a call of seq_voices or voice_set never recaptures, and alternating one-voice and mixed runs recaptures
 * nothing after the first of each.
 * tts_hip_debug_read("voice:<v>:<layer>:<0|1>") returns an entry's K or V [len][H], like "cross:"; "graphs" the number of captured steps. */
int tts_hip_parler_voice_bank(tts_hip_ctx *ctx, uint32_t n_voices);
int tts_hip_parler_voice_set(tts_hip_ctx *ctx, uint32_t voice, const float *enc, uint32_t n_tokens);
int tts_hip_parler_seq_voices(tts_hip_ctx *ctx, uint32_t n, const uint32_t *seqs, const uint32_t *voices);

/* Tuning and fallback switches by name (profiles/ harnesses and the fallback parity test; call between tts_hip_create and the first
 * launch).  Unknown key: -1.  Not an environment variable on purpose: a deployment cannot flip a kernel path by accident.
 * Kokoro contexts (each 1 by default, 0 = the fallback; tests/test_gpu_kokoro.py runs every one against the oracle):
 *   kokoro_mfma         0: every convolution, linear and instance norm through the plain one-thread-per-output kernels
 *   kokoro_b3           0: the k = 3 / 5 / 7 / 11 same-convolutions on the exact-fp32 MFMA kernel instead of split products
 *   kokoro_split        0: those split products as three bf16 planes (six products) instead of fp16 hi + lo (three)
 *   kokoro_attn_lds     0: ALBERT's attention as one wave per (head, row) instead of keys staged through LDS
 *   kokoro_lstm_split   0: each LSTM direction in one workgroup instead of hid / 16 workgroups exchanging their hidden state
 *   kokoro_adain_split  0: instance-norm rows of 8192 positions and more in one workgroup per channel instead of slices over workgroups
 * Dia contexts:
 *   dia_tile_min_rows   decoder steps of at least this many rows, and more than 16, run fp16 matrices on the LDS-tiled MFMA GEMM (every
 *                       matrix and the heads F16 with K % 128 == 0 and N % 16 == 0, no TTS_HIP_FLAG_VALU_GEMM); 0 = never.  Default 0 on a
 *                       context of at most 64 utterance slots, 17 on a larger one.  tts_hip_debug_read("di_tiled") returns the tiled GEMM
 *                       launches of the last forward (0 on the other routes), "di_pending_max" the most K-slice slabs one GEMM left.
 *                       Like every key it is read when a step is issued: a loop graph captured before the call keeps replaying the route
 *                       it was captured with (set it before the first tts_hip_dia_generate / gen_* / stream_* of the context); the same
 *                       holds for tile_force and tile_ks.  The decoder must be at most 2048 wide for the route
 *   tile_force, tile_ks tile shape index (0..5, -1 = the cost model's) and K slices of the residual GEMMs (0 = the cost model's) of every
 *                       tiled GEMM: tests and tuning */
int tts_hip_tune(tts_hip_ctx *ctx, const char *key, int value);

/* stream / device handles for callers that need to order their own work (torch interop) */
void *tts_hip_stream(tts_hip_ctx *ctx);
int   tts_hip_synchronize(tts_hip_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* TTS_HIP_H */
