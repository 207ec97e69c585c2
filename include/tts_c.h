/*
 * tts_c.h — C ABI over the C++ runner API (tts.cpp_amd/host/common.h), for language bindings
 * (ctypes / cgo / JNI / N-API) and the parity tests.
 *
 * Each entry point corresponds to one call the reference's applications make on its C++ API
 * (file:line under /root/reference):
 *   tts_c_runner_from_file  -> runner_from_file()                      src/models/loaders.h:19-20, loaders.cpp:34-95
 *   tts_c_generate          -> tts_generation_runner::generate()       include/common.h:93, parler/model.cpp:838-858
 *   tts_c_sampling_rate     -> tts_runner::sampling_rate               include/common.h:70
 *   tts_c_arch              -> runner->loader.get().arch               examples/perf_battery/perf_battery.cpp:116
 *   tts_c_free              -> ~tts_generation_runner
 * plus test hooks for the host pieces that have no device dependency (tokenizer, sampler, GGUF reader).
 * Errors: the reference aborts (TTS_ABORT, src/util.cpp:14-22); through this ABI the same conditions are
 * returned as NULL / non-zero with tts_c_last_error().
 */
#ifndef TTS_C_H
#define TTS_C_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct tts_c_runner tts_c_runner;

/* generation_configuration (include/common.h:45-66) */
typedef struct tts_c_config {
    const char *voice;
    int         top_k;
    float       temperature;
    float       repetition_penalty;
    int         use_cross_attn;
    int         max_tokens;
    float       top_p;
    int         sample;
    uint64_t    seed; /* extension: 0 = unseeded like the reference (src/sampler.cpp:47) */
} tts_c_config;

void          tts_c_default_config(tts_c_config *cfg);
tts_c_runner *tts_c_runner_from_file(const char *path, int n_threads, const tts_c_config *cfg, int cpu_only);
/* *data stays owned by the runner and valid until the next generate (dac_model.cpp:190-191) */
int           tts_c_generate(tts_c_runner *r, const char *text, const tts_c_config *cfg, const float **data, size_t *n_outputs);
/* Extension: n utterances in lock-step on the runner's device (parler_runner::generate_batch).  texts[n];
 * data[i] / n_outputs[i] receive each utterance's PCM (runner-owned, valid until the next generate*). The runner
 * must have been loaded with TTS_HIP_MAX_SEQS >= n in the environment. */
int           tts_c_generate_batch(tts_c_runner *r, const char *const *texts, int n, const tts_c_config *cfg, const float **data,
                                   size_t *n_outputs);
/* Extension: any number of utterances through ONE continuous-batching session of the runner (tts_generation_runner::generate_stream): a row
 * freed by an utterance that finishes is refilled from texts[] at the next look-in point instead of idling until the longest one is done.
 * Parler-TTS, Orpheus and Dia have a session.  Parler-TTS: at most max_seqs - 1 utterances generate at a time (one cache slot pads the forward), a
 * look-in every 32 decode steps.  Orpheus: max_seqs utterances, a look-in every 28 ids (four SNAC frames) of a device-driven loop; a sampled
 * session needs the device sampler (top_k 1..64, top_p > 0) and is refused otherwise.  Dia: max_seqs utterances, a look-in every 16 steps; a slot
 * that finished is parked on the device (one attention position per step) until the next look-in refills it, an admission runs the text encoder
 * between two intervals, and the finished utterances of an interval share one codec pass (audio within 1e-5 of a tts_c_generate call's, ids
 * identical).  Kokoro has no session: its texts go through generate_batch in groups.  Same outputs as n generate() calls; data[i] valid until the next call.
 * Orpheus' SNAC noise block: the codec runs when an utterance finishes, so the never-reseeded noise engine's draws follow the order in which
 * utterances finish, not the order of texts[]; with TTS_SNAC_NO_NOISE every audio is bit for bit that of a tts_c_generate call of its own. */
int           tts_c_generate_stream(tts_c_runner *r, const char *const *texts, int n, const tts_c_config *cfg, const float **data,
                                    size_t *n_outputs);
/* tts_c_generate_stream with one configuration per text, cfgs[n] (tts_generation_runner::generate_stream with configurations).  Orpheus takes them all
 * into one session: the voice is a prompt prefix and every cache slot carries its own sampler, so texts that differ in voice, seed, sample, top_k,
 * temperature, top_p or repetition_penalty share the forward (a sampled text needs the device sampler, top_k 1..64 and top_p > 0, and fails the call
 * otherwise).  The other models run consecutive texts with equal configurations as one session each.  data[i] is the audio of
 * tts_c_generate(texts[i], &cfgs[i]) (Orpheus' SNAC noise block: as for tts_c_generate_stream). */
int           tts_c_generate_stream_configs(tts_c_runner *r, const char *const *texts, const tts_c_config *cfgs, int n, const float **data,
                                            size_t *n_outputs);
/* Extension: chunked audio (tts_generation_runner::generate_chunked).  fn receives the utterance's PCM in consecutive pieces of at most
 * chunk_frames codec frames while the utterance is still generating (pcm valid during the call only; utterance = 0 here, the text's index in
 * the batch form); their concatenation equals tts_c_generate's / tts_c_generate_batch's audio.  fn returning 0 stops the generation at the
 * next look-in point.  Returns 0 when done, 1 when fn stopped it, another value with tts_c_last_error() on error (chunk_frames == 0 is one).
 * Parler-TTS, Orpheus and Dia stream; Kokoro generates the whole utterance and hands it out as one chunk.
 * Dia: chunk_frames counts the frames the codec sees, after the un-delay dropped those that hold EOS / PAD.
 * Orpheus: chunk_frames counts SNAC frames (7 ids, 2048 samples at 24 kHz).  With TTS_SNAC_NO_NOISE the chunks concatenate to tts_c_generate's
 * PCM.  With the noise block they are a different realisation of the same distribution: generate() draws the noise layer by layer over the
 * whole utterance, chunked generation frame by frame (per frame, for layer l, 4 * prod(stride_0..l) normals) from the same engine, and the
 * chunks equal the whole utterance's decode under that re-laid noise; a completed call consumes exactly the draws generate() would. */
typedef int (*tts_c_chunk_fn)(void *user, int utterance, const float *pcm, size_t n);
int           tts_c_generate_chunked(tts_c_runner *r, const char *text, const tts_c_config *cfg, uint32_t chunk_frames, tts_c_chunk_fn fn, void *user);
int           tts_c_generate_batch_chunked(tts_c_runner *r, const char *const *texts, int n, const tts_c_config *cfg, uint32_t chunk_frames,
                                           tts_c_chunk_fn fn, void *user);
/* Extension: chunked audio out of the continuous session (tts_generation_runner::generate_stream_chunked): tts_c_generate_stream's loop with
 * every utterance's PCM handed to fn in consecutive pieces of at most chunk_frames codec frames; utterance = the text's index, the pieces of
 * different utterances interleave, those of one utterance arrive in order and concatenate to its tts_c_generate_stream audio.  fn returning 0
 * drops that utterance only; the others go on.  Returns 0 when done, 1 when fn dropped at least one utterance, another value with
 * tts_c_last_error() on error (chunk_frames == 0 is one).  Dia's session chunks while its slots keep running: the codec pass of the windows
 * that became final at one look-in runs under the next 16 decoder steps, and a dropped utterance's slot is parked at the next look-in.
 * Orpheus' session chunks the same way: chunk_frames counts SNAC frames, the windows of all slots go through one SNAC window pass under the next
 * 28 decoder steps, and a dropped utterance's slot is freed at the next look-in; the SNAC noise block is drawn as for tts_c_generate_chunked
 * (frame by frame; across utterances in slot order within a look-in), so with TTS_SNAC_NO_NOISE the pieces concatenate to tts_c_generate's PCM.
 * Parler-TTS' session chunks the same way with TTS_PARLER_STREAM_CHUNKS=1 in the environment (an opt-in): the windows of all slots go through one
 * DAC window pass under the next 32 decoder steps, and an utterance's slot is taken again only once its last piece is out.  Without the switch
 * Parler-TTS' session, and always Kokoro's groups, hand each finished utterance out as one chunk. */
int           tts_c_generate_stream_chunked(tts_c_runner *r, const char *const *texts, int n, const tts_c_config *cfg, uint32_t chunk_frames,
                                            tts_c_chunk_fn fn, void *user);
/* tts_c_generate_stream_chunked with one configuration per text, cfgs[n], as tts_c_generate_stream_configs takes them: a session takes every
 * following text whose configuration it accepts and is drained and reopened at the first one it cannot take. */
int           tts_c_generate_stream_chunked_configs(tts_c_runner *r, const char *const *texts, const tts_c_config *cfgs, int n, uint32_t chunk_frames,
                                                    tts_c_chunk_fn fn, void *user);
/* Test hook: the Parler runner's un-delay rule (parler_undelay) on delayed tokens [n_steps][n_heads] — the codes of the kept frames that are
 * final after n_steps steps (finished != 0: the generation is over, every frame is judged).  out [frames][n_heads] may be NULL to count;
 * returns the number of frames. */
int64_t       tts_c_parler_final_frames(const uint32_t *tokens, uint64_t n_steps, uint32_t n_heads, uint32_t audio_vocab, int finished, uint32_t *out,
                                        uint64_t cap_frames);
/* Placement of the NEXT tts_c_runner_from_file on the calling thread (host/common.h tts_load_options): device (< 0: TTS_HIP_DEVICE or
 * 0), lock-step KV slots (0: TTS_HIP_MAX_SEQS or 1), declare_only != 0: lay the model out without uploading its bytes — the weights
 * then arrive in tts_hip_arena_ptr(tts_c_runner_device_context(r)) by a collective and tts_hip_arena_filled() marks them present. */
void          tts_c_set_load_options(int device, int max_seqs, int declare_only);
/* the same plus share_with (tts_load_options::share_with): a loaded runner of the same model on the same device whose weight arena the
 * next runner uses instead of uploading its own (own KV cache, own stream, own voice prompt once it is updated); the reference's server
 * loads the file once per worker (examples/server/server.cpp:316-321).  Lifetime: the arena is reference counted in the device library, so
 * the runners may be freed in any order — the memory goes with the last of them.  Both calls apply to ONE load: tts_c_runner_from_file
 * resets the thread's options to the defaults when it returns. */
void          tts_c_set_load_options_ex(int device, int max_seqs, int declare_only, tts_c_runner *share_with);
/* the runner's tts_hip_ctx* (include/tts_hip.h: arena, profiling), or NULL when the architecture keeps several contexts */
void         *tts_c_runner_device_context(tts_c_runner *r);
/* bytes per element of the decoder's K/V cache as the device context reports them (Orpheus and Dia: 4, or 2 when TTS_HIP_KV_F16 was in the
 * environment at load, TTS_HIP_FLAG_KV_F16 / tts_hip_dia_desc::kv_type; Orpheus alone: 1 when TTS_HIP_KV_F8 was, the e4m3 cache of
 * tts_hip_orpheus_desc::kv_type - with both variables set the load fails, and a Parler or Dia load fails under TTS_HIP_KV_F8); 0 when the architecture does not report it */
uint32_t      tts_c_runner_kv_element_bytes(tts_c_runner *r);
/* utterances a continuous session of the runner holds at once (tts_generation_runner::stream_capacity: an Orpheus runner's max_seqs, at most 256;
 * 0: the runner has no session) */
uint32_t      tts_c_runner_stream_capacity(tts_c_runner *r);
/* the loaded runner's own tokenizer (Parler: unigram ids + EOS as batch_from_sentence builds them); returns the id count */
int           tts_c_runner_tokenize(tts_c_runner *r, const char *text, uint32_t *out, int cap);
float         tts_c_sampling_rate(tts_c_runner *r);
const char   *tts_c_arch(tts_c_runner *r);
void          tts_c_free(tts_c_runner *r);
const char   *tts_c_last_error(void);

/* ---- test hooks ---------------------------------------------------------------------------------- */
/* which = 0: prompt ids of the last generate (tokenised + EOS); 1: sampled ids, still delayed
 * (pctx->output_tokens); Dia, 16 + i: the still-delayed ids of utterance i of the last generate_batch / generate_stream; Orpheus, 16 + i: the ids
 * of utterance i of the last generate_batch, or of the last generate_stream_chunked whose session chunked (i below 4096); Parler, 16 + i: the
 * still-delayed ids of utterance i of the last generate_batch / generate_batch_chunked, or of the last generate_stream_chunked whose session
 * chunked (i below 4096).
 * Returns the count (copies at most cap). */
int tts_c_last_tokens(tts_c_runner *r, int which, uint32_t *out, int cap);
/* unigram tokenizer from the GGUF vocabulary + EOS, as batch_from_sentence builds it (model.cpp:473-498); a GGUF with
 * tokenizer.ggml.merges gets the byte-pair tokenizer instead (src/tokenizer.cpp:265-296; ids only, no framing) */
int tts_c_tokenize(const char *gguf_path, const char *text, uint32_t *out, int cap);

typedef struct tts_c_sampler_cfg {
    uint32_t n_output_heads, vocab_size, top_k;
    float    temperature, top_p, repetition_penalty;
    int      do_sample;
    uint64_t seed;
} tts_c_sampler_cfg;
/* sampler::sample (src/sampler.cpp:3-69); uniforms != NULL injects the per-head U[0,1) draws */
int tts_c_sampler_sample(const tts_c_sampler_cfg *cfg, const int32_t *last_ids, const uint32_t *counts, float *logits,
                         const float *uniforms, uint32_t *out);

/* tts_generation_runner::update_conditional_prompt (common.h:91; parler/model.cpp:510-518): encode `prompt` with the
 * T5 encoder GGUF at text_encoder_path and make it the voice prompt of every later generate().  which == 2 in
 * tts_c_last_tokens returns the ids it was encoded from. */
int tts_c_update_conditional_prompt(tts_c_runner *r, const char *text_encoder_path, const char *prompt);

/* tts_generation_runner::add_voice (an extension; Parler): encode `description` with the T5 encoder GGUF at text_encoder_path and keep it as the
 * voice `name` beside the runner's own description.  tts_c_config::voice == name then selects it per request — in tts_c_generate, the batch, the
 * chunked forms and the sessions, where requests with different voices share one lock-step forward; an unknown name fails the request and the
 * message lists the known ones.  At most 32 tokens and 64 voices; a known name is replaced.  A runner without voice descriptions refuses.
 * tts_c_list_voices writes the names, comma-separated, into out[0..cap) and returns the length of the whole list (< 0 on error). */
int tts_c_add_voice(tts_c_runner *r, const char *name, const char *text_encoder_path, const char *description);
int tts_c_list_voices(tts_c_runner *r, char *out, int cap);

/* ---- device pool: the server's worker pool (examples/server/server.cpp:126-330,885-895) with one worker per device
 * and dynamic lock-step batching of the queued requests (tts.cpp_amd/host/device_pool.h).  No HTTP. -------------- */
typedef struct tts_c_pool tts_c_pool;
/* n_workers workers (server --n-parallelism), worker w on devices[w % n_devices] (NULL: device 0); each worker decodes
 * up to max_batch compatible queued requests together, waiting batch_window_ms for more after the first. */
tts_c_pool *tts_c_pool_create(const char *model_path, int n_workers, const int *devices, int n_devices, int max_batch,
                              int batch_window_ms, const tts_c_config *load_cfg);
/* server --text-encoder-path: the T5 GGUF that CONDITIONAL_PROMPT tasks use; applies to pools created afterwards by
 * this thread (NULL / "" = none) */
void tts_c_pool_set_text_encoder(const char *path);
/* pool_options::continuous for pools created afterwards by this thread: a worker keeps one generation session per run of compatible requests
 * and admits queued requests into rows that free up while the others are still generating (continuous batching), instead of running each
 * batch to its end.  tts_c_pool_admitted_in_flight: how many requests entered a session that way. */
void     tts_c_pool_set_continuous(int on);
/* pool_options::continuous_yield_ms for pools created afterwards by this thread (default 2000): a continuous session stops admitting compatible
 * requests once a request it cannot take (another model, incompatible sampling parameters) has waited this long at the head of the queue */
void     tts_c_pool_set_continuous_yield_ms(int ms);
uint64_t tts_c_pool_admitted_in_flight(tts_c_pool *pool);
int  tts_c_pool_submit(tts_c_pool *pool, const char *text, const tts_c_config *cfg);   /* task id, < 0 on error */
/* CONDITIONAL_PROMPT task (server.cpp:263-271) fanned out to every worker; wait on the id like any task (no audio:
 * tts_c_pool_wait returns 0 with n_outputs == 0 on success, 1 + tts_c_last_error() otherwise) */
int  tts_c_pool_conditional_prompt(tts_c_pool *pool, const char *prompt);
/* add_voice on every worker's runner, with the path given to tts_c_pool_set_text_encoder; fanned out and waited for like CONDITIONAL_PROMPT */
int  tts_c_pool_add_voice(tts_c_pool *pool, const char *name, const char *description);
/* blocks until the task is done (timeout_ms < 0: forever).  0 = audio in data[0..n_outputs), valid until
 * tts_c_pool_release(id); 1 = finished without audio (tts_c_last_error says why); -1 = not finished */
int  tts_c_pool_wait(tts_c_pool *pool, int id, int timeout_ms, const float **data, size_t *n_outputs, int *batch_size, int *worker);
void tts_c_pool_release(tts_c_pool *pool, int id);
void tts_c_pool_stats(tts_c_pool *pool, uint64_t *tasks, uint64_t *batches, uint64_t *largest_batch, uint64_t *timed_out);
/* how the pool loaded its models: RCCL weight broadcasts performed (one per model when the workers span more than one device) and
 * workers that use their device's existing weight arena instead of uploading the file again */
void tts_c_pool_load_stats(tts_c_pool *pool, int *weight_broadcasts, int *shared_arena_loads);
void tts_c_pool_free(tts_c_pool *pool);

int tts_c_gguf_summary(const char *path, uint64_t *n_tensors, uint64_t *n_kv, uint64_t *data_offset, char *arch, int arch_cap);
int tts_c_gguf_tensor(const char *path, int index, char *name, int name_cap, int *type, int64_t ne[4], uint64_t *checksum);

/* ---- Dia host logic, callable without a device (host/dia_runner.h; reference src/models/dia/model.cpp) -------------
 * tokenize_sentence :661-705: out[max_ctx] = the sentence bytes ([S1]/[S2] -> 1/2) then zeros; returns the sentence length or -1 */
int tts_c_dia_tokenize(const char *sentence, uint32_t max_ctx, uint32_t *out);
/* check_stopping :767-785 with the default 9-head delay pattern; ids[9] may be rewritten; returns 1 when generation stops */
int tts_c_dia_check_stopping(uint32_t *ids, uint32_t eos, uint32_t pad, uint32_t max_delay, uint32_t current_position, uint32_t max_generation_size,
                             int *delay_steps);
/* adjust_output_tokens :787-808: tokens[n_steps][9] -> filtered frames [..][9]; returns the number of ids written */
int64_t tts_c_dia_adjust_output_tokens(const uint32_t *tokens, uint64_t n_ids, uint32_t audio_vocab, uint32_t max_delay, uint32_t *filtered);
/* the runner's incremental form of that rule (dia_undelay) fed tokens[n_steps][9] in pieces of `piece` steps (0: all at once), each call
 * continuing from the cursor the last one returned: the kept frames that are final after n_steps steps.  out [frames][9] may be NULL to
 * count; returns the number of frames. */
int64_t tts_c_dia_final_frames(const uint32_t *tokens, uint64_t n_steps, uint32_t audio_vocab, uint32_t max_delay, uint64_t piece, uint32_t *out,
                               uint64_t cap_frames);

/* ---- chunked audio, host logic callable without a device: the planner the Parler and Dia runners cut their codec windows with
 * (host/chunk_windows.h).  rule 0: Parler's un-delay over tokens[n_steps][n_heads] (audio_vocab; max_delay unused), 1: Dia's over
 * tokens[n_steps][9] (audio_vocab, max_delay; n_heads unused) — the arguments of the two *_final_frames calls.  The stream is fed to the planner
 * in pieces of `piece` steps (0: all at once), each a look-in of a generation that is still running, then once more marked finished.  Every
 * window cut, in order: windows[i] = (w0, w1, keep0, keep1) — the codec decodes frames [w0, w1) of the kept-frame sequence and keeps
 * [w0 + keep0, w0 + keep1) of them, as tts_hip_dac_decode_windows takes it; cut_at[i] = (steps fed when it was cut, 1 if that was the finished
 * call); codes = the kept frames' codes of all windows back to back, [*n_kept][heads].  windows, cut_at and codes may be NULL; at most
 * cap_windows windows and cap_frames frames are written.  Returns the number of windows, -1 on a bad argument. */
int64_t tts_c_chunk_windows(int rule, const uint32_t *tokens, uint64_t n_steps, uint32_t n_heads, uint32_t audio_vocab, uint32_t max_delay, uint32_t halo,
                            uint32_t chunk_frames, uint64_t piece, uint32_t *windows, uint32_t *cut_at, uint64_t cap_windows, uint32_t *codes,
                            uint64_t cap_frames, uint64_t *n_kept);

/* ---- Kokoro host logic, callable without a device (host/kokoro_runner.h; reference src/tokenizer.cpp:159-177,
 * src/models/kokoro/model.cpp:1340-1388) ------------------------------------------------------------------------------
 * single_pass_tokenizer::tokenize over the given vocabulary; returns the number of ids (out may be NULL to count) */
int tts_c_single_pass_tokenize(const char *const *vocab, int n_vocab, const char *text, uint32_t *out, int cap);
/* the clause / chunk split of kokoro_runner::generate (:1420-1446) for a phoneme string: out receives, per chunk, its length
 * followed by its ids (bos ... eos); returns the number of uint32 written (or needed, when larger than cap) */
int tts_c_kokoro_chunks(const char *const *vocab, int n_vocab, const char *phonemes, uint32_t max_ctx, uint32_t space_token_id, uint32_t *out, int cap);
/* the state of the reference's noise engine (random_uniform_gen, src/util.cpp:65-71: std::default_random_engine = minstd_rand0) after k more draws:
 * kokoro_runner::generate_batch hands every clause its stretch of the one stream this way (host/kokoro_runner.h) */
uint32_t tts_c_minstd0_jump(uint32_t state, uint64_t k);
/* generate_batch's plan for the duration passes (TTS_KOKORO_ROWS): the pieces sorted by non-increasing token count (stable), in consecutive groups of at most
 * max_per_group.  out receives, per group, its size followed by its piece indices; returns the number of uint32 written (or needed, when larger than cap) */
int tts_c_kokoro_duration_groups(const uint32_t *lengths, int n, int max_per_group, uint32_t *out, int cap);
/* starts_out[i] = the noise engine's state at the first draw of piece i, which draws frames[i] * per_frame values (pieces in clause order); returns the state
 * after the last piece */
uint32_t tts_c_kokoro_noise_starts(uint32_t state, const uint64_t *frames, int n, uint64_t per_frame, uint32_t *starts_out);
/* n draws of that engine through std::uniform_real_distribution<float>(0, 1) from `state`, drawn as `threads` parallel stretches (what the runner does for a
 * clause's source noise); returns the state afterwards */
uint32_t tts_c_minstd0_uniform(uint32_t state, uint64_t n, float *out, uint32_t threads);

/* ---- the quantize tool (examples/quantize/quantize_impl.h:5-15: quantization_params + quantize_gguf) ------------
 * Host only.  quantize_type is the ggml type number (F16 1, Q4_0 2, Q5_0 6, Q8_0 8; quantize.cpp:11-20). */
typedef struct tts_c_quantization_params {
    uint32_t n_threads;
    int      quantize_type;
    int      quantize_output_heads;
    int      quantize_text_embeddings;
    int      quantize_cross_attn_kv;
    int      convert_dac_to_f16;
    int      convert_non_quantizable_to_f16;
} tts_c_quantization_params;
int tts_c_quantize_gguf(const char *ifile, const char *ofile, const tts_c_quantization_params *params);  /* 0 / -1 */
/* the allow-list decision for one tensor name: 0 copied, 1 quantised to quantize_type, 2 converted to F16, -1 error */
int tts_c_quantize_decision(const char *arch, const char *tensor_name, int n_dims, const tts_c_quantization_params *params);
/* one call of the row quantisers (n values, n % 32 == 0 for the block types); returns bytes written or -1 */
int64_t tts_c_quantize_rows(int type, const float *src, void *dst, int64_t n_per_row, int64_t nrows, uint32_t n_threads);

#ifdef __cplusplus
}
#endif
#endif
