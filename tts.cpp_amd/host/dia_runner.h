// dia_runner.h — Dia generation runner on top of the HIP shim (include/tts_hip.h).
//
// Mirrors dia_runner (/root/reference/src/models/dia/model.h:187-216, model.cpp:661-858): byte tokenisation with the
// [S1] / [S2] speaker tags, one encoder pass over the padded text and an all-zero "unconditional" twin, an autoregressive
// loop over nine delayed codebook heads with classifier-free guidance inside every step, the end-of-sequence countdown of
// check_stopping, un-delay, DAC.  The ggml graphs inside decode() and dac_runner::run() are replaced by tts_hip_dia_* and
// tts_hip_dac_decode; tokenisation, sampling and the stopping logic stay on the host as in the reference.
//
// Chunked audio is the shared DAC chunker (chunk_windows.h) with dia_undelay as its rule; the session's bookkeeping and its chunk hook come
// from stream_session.h.
#pragma once
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tts_hip.h"
#include "chunk_windows.h"
#include "common.h"
#include "sampler.h"
#include "stream_session.h"

extern const struct dia_model_loader final : tts_model_loader {
    explicit dia_model_loader();
    std::unique_ptr<tts_generation_runner> from_file(gguf_file * meta, int n_threads, bool cpu_only,
                                                     const generation_configuration & config) const override;
} dia_loader;

struct dia_hparams {  // defaults = nari-labs/Dia-1.6B (dia/model.h:64-84)
    uint32_t n_output_heads = 9, n_encoder_layers = 12, n_decoder_layers = 18, encoder_hidden_size = 1024, decoder_hidden_size = 2048;
    uint32_t encoder_attn_heads = 16, decoder_attn_heads = 16, decoder_query_heads = 4, head_size = 128;
    uint32_t eos_token_id = 1024, pad_token_id = 1025, bos_token_id = 1026, output_vocab_size = 1028, audio_vocab_size = 1024;
    uint32_t max_generation_size = 3072, max_encoder_context_length = 1024, max_delay = 15;
    float    cfg_scale = 3.0f;
    std::vector<uint32_t> delay_pattern{0, 8, 9, 10, 11, 12, 13, 14, 15};   // model.h:84: not a GGUF key
    uint32_t dac_n_layers = 4;
    uint32_t dac_stride[TTS_HIP_MAX_DAC_BLOCKS] = {0}, dac_padding[TTS_HIP_MAX_DAC_BLOCKS] = {0};
    uint32_t up_sampling_factor = 512;
};

// host logic of the runner as free functions of the hyper-parameters (no device behind them; the runner and the CPU tests call these)
uint32_t dia_tokenize_sentence(const dia_hparams & hp, std::string sentence, std::vector<uint32_t> & tokens);                               // model.cpp:661-705
bool     dia_check_stopping(const dia_hparams & hp, std::vector<uint32_t> & audio_tokens, uint32_t current_position, uint32_t max_generation_size,
                            int & delay_steps);                                                                                             // :767-785
void     dia_adjust_output_tokens(const dia_hparams & hp, const std::vector<uint32_t> & output_tokens, std::vector<uint32_t> & filtered);   // :787-808
// the same rule from a cursor: toks [steps][heads] is the stream so far, `judged` frames were judged by earlier calls; appends the kept
// frames that became final (frame i is final once step i + max_delay exists) to `kept` and returns the new cursor.  A prefix of a stream
// yields a prefix of the whole stream's frames; dia_adjust_output_tokens is this from zero over everything.
size_t   dia_undelay(const dia_hparams & hp, const uint32_t * toks, size_t steps, size_t judged, std::vector<uint32_t> & kept);

struct dia_runner final : stream_session {
    dia_runner(const dia_hparams & hp, int device);
    ~dia_runner() override;

    void assign_weight(const char * name, const gguf_tensor_view & tensor) override;
    void prepare_post_load() override;
    void generate(const char * sentence, tts_response & output, const generation_configuration & config) override;
    // extension (BASELINE config 3: 4 utterances per GPU): n utterances in lock-step, each the reference's batch of two guidance streams
    // (model.cpp:330-341); per-utterance sampler, check_stopping countdown and un-delay; one batched DAC pass.  Needs max_seqs >= n at
    // load time (tts_load_options / TTS_HIP_MAX_SEQS).  Greedy results equal n separate generate() calls.
    void generate_batch(const std::vector<std::string> & sentences, std::vector<tts_response> & outputs,
                        const generation_configuration & config) override;
    // chunked audio (common.h): PCM in pieces of at most chunk_frames kept codec frames while the decoder is still running; the pieces
    // concatenate to generate()'s / generate_batch()'s audio, last_output_tokens / last_batch_tokens hold what was generated (also after
    // on_chunk stopped the call), and a fixed seed draws the uniforms of the one-call forms
    void generate_chunked(const char * sentence, const generation_configuration & config, uint32_t chunk_frames,
                          const std::function<bool(const float *, size_t)> & on_chunk) override;
    void generate_batch_chunked(const std::vector<std::string> & sentences, const generation_configuration & config, uint32_t chunk_frames,
                                const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) override;
    // extension: continuous batching (common.h) on tts_hip_dia_stream_*: max_seqs utterance slots stepped as one fixed lock-step forward; a slot
    // whose countdown ended is parked on the device and refilled at the next look-in (every 16 steps).  stream_submit tokenises and queues,
    // stream_step admits everything queued in one call (the encoder passes run there), runs one interval, un-delays and decodes what finished
    // in one batched codec pass.  An utterance's tokens are those of a generate() call of its own (a fixed seed draws that call's uniforms).
    // The session runs on the device loop only: stream_begin aborts under TTS_HOST_LOOP instead of falling back.
    uint32_t stream_capacity() const override { return max_seqs > 1 ? max_seqs : 0; }
    void     stream_begin(const generation_configuration & config) override;
    uint32_t stream_free() const override { return st_on ? (uint32_t) st_free.size() - (uint32_t) st_wait.size() : 0; }
    uint32_t stream_live() const override { return st_live + (uint32_t) st_wait.size() + (uint32_t) st_closing.size(); }
    // The session is a mixed one (tts_hip_dia_stream_begin_mixed): every slot carries its own sampler record, penalty table and step budget, so
    // a request may differ from the session's configuration in sample, seed, top_k, top_p, temperature, repetition_penalty and max_tokens.  It is
    // accepted when it is greedy or within the device sampler's limits and its generation length is at most the session's (the opening
    // configuration's); its uniforms are drawn from its own seed, as a generate() call of its own draws them.
    bool     stream_accepts(const generation_configuration & config) const override;
    void     stream_submit(size_t ticket, const std::string & sentence, const generation_configuration & config) override;
    void     stream_step(std::vector<stream_result> & finished) override;
    void     stream_end() override;
    // chunked audio out of the session: with a hook set, stream_step launches its 16 steps (tts_hip_dia_stream_launch), decodes the windows
    // cut at the last look-in in one tts_hip_dac_decode_windows pass on the codec context while they run, hands the chunks to on_chunk, then
    // waits and takes the new rows of every live slot (tts_hip_dia_stream_wait).  An utterance is reported in `finished` (no audio) once its
    // last chunk is out; on_chunk returning false drops that utterance only (tts_hip_dia_stream_drop), reported with what it got.  The hook
    // itself is stream_session's; this runner's part always says yes: with an unknown halo its chunker hands whole utterances out through the hook.
    bool     session_chunks_ready(uint32_t chunk_frames) override;
    uint32_t batch_capacity() const override { return max_seqs; }
    uint32_t kv_element_bytes() const override;   // 4, or 2 when TTS_HIP_KV_F16 was in the environment at load (tts_hip_dia_desc::kv_type)
    uint32_t max_seqs = 1;   // utterance slots of the decoder context (tts_load_options::max_seqs, at most 128: two guidance rows each, 256 rows per forward)

    dia_hparams        hp;
    sampler            smp;
    tts_hip_ctx *      lm = nullptr;    // encoder + decoder context
    tts_hip_ctx *      dac = nullptr;   // codec context
    std::vector<float> pcm, logits;
    int                dac_halo = -1;   // tts_hip_dac_halo_frames of the codec: frames of context a chunk's window needs on each side

  private:
    // session state of the continuous batching
    struct waiting { size_t ticket = 0; std::vector<uint32_t> prompt; uint32_t len = 0; generation_configuration cfg{}; };
    uint32_t                 st_max_gen = 0;
    std::vector<waiting>     st_wait;     // submitted, admitted by the next stream_step
    // ... with the chunk hook: the chunker's rows are the slots
    std::unique_ptr<dac_chunker>       st_hook;
    std::vector<std::vector<uint32_t>> st_toks;        // slot -> the occupant's still-delayed ids so far
    std::vector<bool>                  st_gen;         // slot -> its occupant is generating
    std::vector<uint32_t>              st_buf;         // what tts_hip_dia_stream_wait writes: [slots][max_gen][heads]
    std::vector<size_t>                st_win_ticket;  // planned window -> ticket
    std::vector<size_t>                st_closing;     // ended, rows on the host, last chunk not handed out yet
    std::vector<size_t>                st_stopped;     // on_chunk returned false for these
    void admit_waiting();
    void hand_out(std::vector<stream_result> & finished);
    void stream_step_chunked(std::vector<stream_result> & finished);
    uint32_t begin_call(const generation_configuration & config);   // sampler settings; -> the step budget (max_gen)
    bool     valid_max_tokens(const generation_configuration & config) const;    // begin_call's assertion
    uint32_t resolved_max_gen(const generation_configuration & config) const;    // the step budget begin_call returns
    bool     device_sampler(const generation_configuration & config) const;      // greedy, or within the limits of tts_hip_dia_generate
    tts_hip_dia_codes loop_codes() const;                           // the special ids and the delay pattern, as the device loop takes them
    void     draw_call_uniforms(uint64_t seed, uint32_t max_gen, float * out, size_t stride) const;
    void     encode_single(const char * sentence);
    void     encode_batch(const std::vector<std::string> & sentences);
    // the one generation loop under generate, generate_batch and their chunked forms
    dac_chunker make_chunker(uint32_t chunk_frames);
    std::vector<std::vector<uint32_t>> run_utterances(uint32_t n, uint32_t max_gen, const generation_configuration & config, dac_chunker * hook,
                                                      const std::function<bool(uint32_t, const float *, size_t)> & on_chunk = {});
};
