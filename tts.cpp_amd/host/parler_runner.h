// parler_runner.h — Parler-TTS generation runner on top of the HIP shim (include/tts_hip.h).
//
// Mirrors parler_tts_runner (/root/reference/src/models/parler/model.h:187-225, model.cpp:473-498,
// 704-858): tokenise -> text-prompt decode -> AR loop with the delay pattern, host sampling and EOS
// tracking -> un-delay -> DAC.  The ggml graph build/compute inside decode() and dac_runner::run() is
// replaced by calls into the C ABI; everything the reference keeps on the host stays on the host.
//
// generate, generate_batch and their chunked forms share one generation loop (run_rows) over the prefilled rows: the device loop
// (tts_hip_parler_gen_begin / _launch / _wait, a look-in every 32 steps) or, under TTS_HOST_LOOP or with more than 2048 logits per head,
// the host loop (tts_hip_parler_step + sampler::sample per step).  Chunked audio is a hook called at that loop's look-ins: the shared DAC
// chunker (chunk_windows.h) with parler_undelay as its rule.  The session's bookkeeping and its chunk hook come from stream_session.h.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../../include/tts_hip.h"
#include "chunk_windows.h"
#include "common.h"
#include "sampler.h"
#include "stream_session.h"
#include "tokenizer.h"

extern const struct parler_model_loader final : tts_model_loader {
    explicit parler_model_loader();
    std::unique_ptr<tts_generation_runner> from_file(gguf_file * meta, int n_threads, bool cpu_only,
                                                     const generation_configuration & config) const override;
} parler_loader;

struct parler_hparams {  // defaults = Parler TTS Mini v1 (model.h:66-83)
    uint32_t n_output_heads = 9, n_encode_length = 0, hidden_size = 1024, max_ctx_length = 4096, n_attn_heads = 16;
    uint32_t output_vocab_size = 1088, eos_token_id = 1024, audio_vocab_size = 1024, max_generation_size = 2580;
    uint32_t n_layers = 24, bos_token_id = 1025;
    uint32_t dac_n_layers = 4;  // dac_model.h:33
    uint32_t dac_stride[TTS_HIP_MAX_DAC_BLOCKS] = {0}, dac_padding[TTS_HIP_MAX_DAC_BLOCKS] = {0};
    uint32_t up_sampling_factor = 512;
};

// The delay pattern's per-frame rule (model.cpp:734-760): frame i takes head k's token from step i + k and is dropped when one of them lies
// past the end of the tokens or is no audio code (>= audio_vocab).  Frame i is final once step i + nh - 1 exists, so whether it is kept
// is known as soon as that step has run.  Judges frames [next, end) of tokens [steps][nh] — end = steps when the generation is over,
// else the frames already final (steps - nh + 1) — appends the kept ones' codes to `out` and returns end.  adjust_output_tokens is
// this with next = 0 and finished.
size_t parler_undelay(const uint32_t * toks, size_t steps, uint32_t nh, uint32_t audio_vocab, size_t next, bool finished, std::vector<uint32_t> & out);

struct parler_runner final : stream_session {
    parler_runner(const parler_hparams & hp, unigram_tokenizer * tok, int device, bool use_cross_attn);
    ~parler_runner() override;

    void assign_weight(const char * name, const gguf_tensor_view & tensor) override;
    void prepare_post_load() override;
    void generate(const char * sentence, tts_response & output, const generation_configuration & config) override;
    void update_conditional_prompt(const char * file_path, const char * prompt) override;
    // named voice descriptions (common.h): each lives in the device's voice bank (tts_hip_parler_voice_bank, created on first use with 64 entries)
    // and is selected per request by generation_configuration::voice; "" is the runner's own description.  More than 32 tokens abort.
    void add_voice(const char * name, const char * text_encoder_path, const char * description) override;
    std::vector<std::string_view> list_voices() override;

    // Extension (the reference generates one utterance per call; its only multi-utterance construct is the
    // server's pool of full replicas, examples/server/server.cpp:885-895): n utterances decoded in lock-step on
    // this runner's device — one pass over the weights per step for all of them, one batched DAC pass.
    // outputs[i].data points into a runner-owned buffer valid until the next generate/generate_batch.
    // Needs max_seqs >= n (TTS_HIP_MAX_SEQS at load time).  Results equal n separate generate() calls.
    void generate_batch(const std::vector<std::string> & sentences, std::vector<tts_response> & outputs,
                        const generation_configuration & config) override;
    uint32_t batch_capacity() const override { return max_seqs; }
    // continuous batching (common.h): max_seqs - 1 rows (one cache slot pads the lock-step forward), tts_hip_parler_stream_* underneath
    uint32_t stream_capacity() const override { return max_seqs > 1 ? max_seqs - 1 : 0; }
    void     stream_begin(const generation_configuration & config) override;
    uint32_t stream_free() const override { return (uint32_t) st_free.size(); }
    uint32_t stream_live() const override { return st_live + (uint32_t) st_codec.size(); }
    // With at most 2048 logits per head the session is a mixed one (tts_hip_parler_stream_begin_mixed): every slot carries its own sampler record
    // and penalty table, so a request may differ from the session's configuration in sample, seed, top_k, top_p, temperature and
    // repetition_penalty.  It is accepted when use_cross_attn is the load-time value and it is greedy or within the device sampler's limits; its
    // uniforms are drawn from its own seed, as a generate() call of its own draws them.  Its voice is empty (the runner's own description) or a name
    // add_voice has entered: the slot's voice is set before its admission (tts_hip_parler_seq_voices), so requests with different voices share
    // the session's forward; an unknown name is refused.
    bool     stream_accepts(const generation_configuration & config) const override;
    void     stream_submit(size_t ticket, const std::string & sentence, const generation_configuration & config) override;
    void     stream_step(std::vector<stream_result> & finished) override;
    void     stream_end() override;
    // chunked audio out of the session (the hook itself is stream_session's): with a hook set, stream_step launches its 32 steps
    // (tts_hip_parler_stream_launch), decodes the windows the last look-in planned while they run (one tts_hip_dac_decode_windows pass for all
    // slots) and hands their chunks out under the slots' tickets, then waits and takes the new rows of every live slot
    // (tts_hip_parler_stream_wait).  An utterance is reported in `finished` (no audio) once its last chunk is out, and its slot is free from then
    // on, not earlier: the chunker's rows are the slots.  on_chunk returning false drops that utterance only (tts_hip_parler_stream_drop),
    // reported with what it got.  last_batch_tokens[ticket] keeps an utterance's tokens for tickets below TOKEN_RECORD_TICKETS.
    void *   device_context() const override { return ctx; }
    // chunked audio (common.h): codec windows of the frames that became final are decoded while the next steps run
    void generate_chunked(const char * sentence, const generation_configuration & config, uint32_t chunk_frames,
                          const std::function<bool(const float *, size_t)> & on_chunk) override;
    void generate_batch_chunked(const std::vector<std::string> & sentences, const generation_configuration & config, uint32_t chunk_frames,
                                const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) override;
    bool          declare_only = false;   // tts_load_options at load time: no weight bytes uploaded by this runner
    tts_hip_ctx * share_ctx = nullptr;    // ... and whose arena it uses instead (same device)
    uint32_t max_seqs = 1;

    // pieces exposed for tests
    void                 adjust_output_tokens(const std::vector<uint32_t> & output_tokens, std::vector<uint32_t> & filtered) const;
    // stream_session's records: last_output_tokens is pctx->output_tokens of the last generate, last_batch_tokens per utterance, both still delayed

    parler_hparams                     hp;
    std::unique_ptr<unigram_tokenizer> tokenizer;
    sampler                            smp;
    tts_hip_ctx *                      ctx = nullptr;
    bool                               use_cross_attn;
    int                                device_id = 0;
    std::vector<uint32_t>              last_conditional_tokens;  // ids the voice prompt was encoded from (tests)
    std::vector<float>                 pcm;     // runner-owned output buffer (dctx->buf_output)

  private:
    static constexpr uint32_t VOICE_BANK = 64, VOICE_TOKENS = 32;   // bank entries; positions an entry holds
    std::vector<std::string> voice_names;   // voice i + 1 of the device's bank
    bool                     voice_bank_made = false;
    std::vector<uint32_t>    st_voice;      // slot -> voice of its occupant (session)
    // T5-encode a description with this runner's tokenizer: the ids (+ EOS) and the encoder's output [ids][hidden]
    std::vector<float> encode_description(const char * file_path, const char * prompt, const char * what, std::vector<uint32_t> & tokens);
    bool     voice_known(const std::string & voice) const;
    uint32_t voice_index(const std::string & voice, const char * what) const;   // "" -> 0; unknown: TTS_ABORT listing the names
    void     set_slot_voices(const std::vector<uint32_t> & slots, const std::vector<uint32_t> & voices, const char * what);
    bool tokenize_prompt(const std::string & sentence, std::vector<uint32_t> & prompt) const;
    bool prepare_single(const char * sentence, const generation_configuration & config, std::vector<uint32_t> & prompt);
    bool prepare_batch(const std::vector<std::string> & sentences, const generation_configuration & config, std::vector<uint32_t> & start,
                       std::vector<uint32_t> & row_of);
    int  dac_halo = -1;   // tts_hip_dac_halo_frames of the codec layout (-1: unknown; chunked audio then decodes whole utterances)
    dac_chunker make_chunker(uint32_t chunk_frames);   // the look-in hook of chunked audio: windows of the frames that became final -> codec -> callbacks
    // the one generation loop, over n prefilled rows (row i starts at start[i]); hook: nullptr, or planned and handed to on_chunk(row, ...) at every
    // look-in; tokens per row out
    std::vector<std::vector<uint32_t>> run_rows(const std::vector<uint32_t> & start, const generation_configuration & config, dac_chunker * hook,
                                                const std::function<bool(uint32_t, const float *, size_t)> & on_chunk = {});
    std::vector<tts_response> decode_frames(const std::vector<uint32_t> & codes, const std::vector<uint32_t> & frames);
    // session state of the continuous batching
    struct pending { size_t ticket; uint32_t slot; std::vector<uint32_t> prompt; generation_configuration cfg; uint32_t voice = 0; };
    struct decoded { size_t ticket; std::vector<uint32_t> frames; };   // un-delayed codes waiting for a codec pass
    bool                        st_mixed = false;    // the open session carries a sampler per slot
    uint32_t                    st_max_steps = 0;
    uint32_t                    st_codec_hold = 1;   // tts_load_options::stream_codec_hold at load time
    uint32_t                    st_codec_held = 0;   // stream_step calls the oldest undecoded finished utterance has waited for a codec group to fill
    std::vector<uint32_t>       st_start;           // slot -> prompt length
    std::vector<pending>        st_wait;            // submitted, not yet admitted (admitted as one side batch by the next stream_step)
    std::vector<decoded>        st_codec;
    std::vector<std::vector<float>> st_pcm;         // audio handed out by the last stream_step
    // ... with the chunk hook: the chunker's rows are the slots
    enum : uint8_t { SLOT_FREE = 0, SLOT_RUNNING = 1, SLOT_CLOSING = 2 };   // closing: ended, its last windows planned and not yet handed out
    bool session_chunks_ready(uint32_t chunk_frames) override;
    void stream_step_chunked(std::vector<stream_result> & finished);
    std::unique_ptr<dac_chunker>       st_hook;     // plan() / emit_session() over the slots
    std::vector<std::vector<uint32_t>> st_toks;     // slot -> the occupant's tokens so far, still delayed
    std::vector<bool>                  st_fin;      // slot -> its occupant has ended (plan() then cuts its tail)
    std::vector<uint8_t>               st_state;    // slot -> SLOT_*
    std::vector<size_t>                st_stopped;  // the slots whose occupant's on_chunk returned false
    std::vector<uint32_t>              st_buf;      // what tts_hip_parler_stream_wait writes: [slots][max_steps][heads]
};
