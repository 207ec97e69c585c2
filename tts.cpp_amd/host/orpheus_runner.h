// orpheus_runner.h — Orpheus generation runner on top of the HIP shim (include/tts_hip.h).
//
// Mirrors orpheus_runner (/root/reference/src/models/orpheus/model.h:104-140, model.cpp:341-448): frame the prompt
// (fixed leading / trailing ids, optional "voice: " prefix), byte-pair tokenise, autoregress one token at a time through
// the Llama-3 decoder until the stopping token, regroup every 7 ids into the three SNAC levels, decode with SNAC.
// The ggml graphs inside decode() and snac_runner::run() are replaced by tts_hip_orpheus_* / tts_hip_snac_*.
//
// Chunked audio cuts its windows and hands its chunks out with chunk_windows.h; the id regrouping and the frame-major noise block around them
// are this runner's.  The session's bookkeeping and its chunk hook come from stream_session.h.
#pragma once
#include <array>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/tts_hip.h"
#include "chunk_windows.h"
#include "common.h"
#include "sampler.h"
#include "stream_session.h"
#include "tokenizer.h"

extern const struct orpheus_model_loader final : tts_model_loader {
    explicit orpheus_model_loader();
    std::unique_ptr<tts_generation_runner> from_file(gguf_file * meta, int n_threads, bool cpu_only,
                                                     const generation_configuration & config) const override;
} orpheus_loader;

struct orpheus_hparams {  // defaults = canopylabs/orpheus-3b (orpheus/model.h:24-37) + hubertsiuzdak/snac_24khz (snac_model.h:10-21)
    uint32_t vocab_size = 156940, n_attn_heads = 24, n_kv_attn_heads = 8, head_size = 128, hidden_size = 3072, kv_hidden_size = 1024;
    uint32_t n_layers = 28, max_context_length = 1024, max_generation_size = 2100, stopping_token_id = 128258;
    uint32_t eos_token_id = 128001, bos_token_id = 128000;
    uint32_t audio_heads = 3;
    uint32_t heads[7] = {0, 1, 2, 2, 1, 2, 2};
    // "undocumented constants" the reference hard-codes (model.cpp:8-9, 371).  Extension: a GGUF may override them with
    // orpheus.{prepended_tokens,appended_tokens,audio_token_offset,audio_token_stride} (synthetic test models do).
    std::vector<uint32_t> prepended_tokens{128259, 128000};
    std::vector<uint32_t> appended_tokens{128009, 128260, 128261, 128257};
    uint32_t audio_token_offset = 128266, audio_token_stride = 4096;
    // SNAC
    uint32_t snac_layers = 4, snac_heads = 3, snac_up = 512, snac_max_generation = 2580;
    uint32_t snac_stride[TTS_HIP_MAX_DAC_BLOCKS] = {0}, snac_padding[TTS_HIP_MAX_DAC_BLOCKS] = {0}, snac_groups[TTS_HIP_MAX_DAC_BLOCKS] = {0};
    uint32_t snac_repeats[3] = {4, 2, 1};
};

struct orpheus_runner final : stream_session {
    orpheus_runner(const orpheus_hparams & hp, bpe_tokenizer * tok, int device);
    ~orpheus_runner() override;

    void assign_weight(const char * name, const gguf_tensor_view & tensor) override;
    void prepare_post_load() override;
    void generate(const char * sentence, tts_response & output, const generation_configuration & config) override;
    // extension: lock-step utterances (tts_hip_orpheus_generate_batch): every utterance's audio is that of a generate() call of its own, made in order
    void     generate_batch(const std::vector<std::string> & sentences, std::vector<tts_response> & outputs, const generation_configuration & config) override;
    uint32_t batch_capacity() const override { return max_seqs; }
    uint32_t kv_element_bytes() const override;
    // extension: chunked audio.  chunk_frames counts SNAC frames (7 ids, 4 * snac_up samples).  The decoder runs in pieces
    // (tts_hip_orpheus_gen_*); a chunk [f0, f1) is decoded once frames up to f1 + snac_halo exist or the utterance has ended, as the window
    // [f0 - halo, f1 + halo) on the codec's stream (tts_hip_snac_decode_windows_begin / _end) while the next piece of steps runs (one sequence;
    // a lock-step batch decodes and hands out its ready windows before the next piece, whose launch blocks).
    // The noise block: see chunk_state below.
    void     generate_chunked(const char * sentence, const generation_configuration & config, uint32_t chunk_frames,
                              const std::function<bool(const float *, size_t)> & on_chunk) override;
    void     generate_batch_chunked(const std::vector<std::string> & sentences, const generation_configuration & config, uint32_t chunk_frames,
                                    const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) override;
    // extension: continuous batching (common.h) on tts_hip_orpheus_stream_*: max_seqs slots, every one a row of the device-driven lock-step loop; a slot
    // that frees up is refilled at the next look-in.  An utterance's ids are those of a generate() call of its own, and with TTS_SNAC_NO_NOISE so is
    // its audio; with the noise block the engine's draws follow the order in which utterances finish.  A sampled session needs the device sampler
    // (top_k 1..64): generate_batch falls back to the host loop for other configurations, a session cannot, and stream_begin aborts.
    uint32_t stream_capacity() const override { return max_seqs > 1 ? max_seqs : 0; }
    void     stream_begin(const generation_configuration & config) override;
    uint32_t stream_free() const override { return (uint32_t) st_free.size(); }
    uint32_t stream_live() const override { return st_live; }
    // The session is a mixed one (tts_hip_orpheus_stream_begin_mixed): the voice is a prompt prefix and every slot carries its own sampler, so a
    // request may differ from the session's configuration in voice, seed, sample, top_k, temperature, top_p and repetition penalty.  It is accepted
    // when its voice is valid and it is greedy or within the device sampler's limits; its sampler is seeded as a generate() call of its own seeds it.
    bool     stream_accepts(const generation_configuration & config) const override;
    void     stream_submit(size_t ticket, const std::string & sentence, const generation_configuration & config) override;
    void     stream_step(std::vector<stream_result> & finished) override;
    void     stream_end() override;
    // extension: chunked audio out of the session (the hook itself is stream_session's).  With the hook set, a stream_step launches its 28
    // decoder steps (tts_hip_orpheus_stream_launch), decodes the windows cut at the previous look-in in one tts_hip_snac_decode_windows_begin / _end
    // pass on the codec context while they run (the windows of all slots in one pass), hands the chunks to on_chunk(ticket, ...), and then waits
    // taking the new ids (tts_hip_orpheus_stream_wait).  Right after the wait the ids go to the slots' chunk_state and the next windows are cut, with
    // slots as chunk_collect's rows: a slot whose occupant ended is free for the admission that precedes the next launch (stream_free() counts it
    // from here on), so its tail has to be in the windows by then; the windows carry the ticket they were cut for.  An utterance appears in
    // `finished`, with empty audio, once its last chunk is out, and stream_live() counts it until then.  When nothing generates after a wait, the
    // tails are decoded in the same stream_step.  on_chunk returning false ends that utterance only: its slot is dropped after the next wait
    // (tts_hip_orpheus_stream_drop) and it is reported with what it got.  last_output_tokens follows the utterances as they finish, and
    // last_batch_tokens[ticket] keeps an utterance's ids for tickets below TOKEN_RECORD_TICKETS.
    // The noise block: as in generate_chunked every frame is drawn once, frame-major, when it first enters a window.  The order of the draws across
    // utterances is the order of chunk_collect: slot order within a look-in, frames increasing.  With TTS_SNAC_NO_NOISE the chunks concatenate to
    // generate()'s PCM; a completed utterance consumes as many draws as its generate() would.
    bool     session_chunks_ready(uint32_t chunk_frames) override;
    std::vector<std::string_view> list_voices() override;

    void decode_audio(const std::vector<uint32_t> & output_tokens, std::vector<float> & audio);   // prepare_output_tokens + SNAC
    // pieces exposed for tests
    std::vector<uint32_t>              batch_from_sentence(const std::string & sentence, const std::string & voice) const;  // model.cpp:341-356
    std::vector<std::vector<uint32_t>> prepare_output_tokens(const std::vector<uint32_t> & output_tokens) const;           // :358-376
    // stream_session's records: last_batch_tokens holds the ids of every utterance of the last generate_batch, or of the chunked session

    orpheus_hparams                hp;
    std::unique_ptr<bpe_tokenizer> tokenizer;
    sampler                        smp;
    uint32_t                       max_seqs = 1;     // cache slots of the decoder context (tts_load_options::max_seqs, at most 256)
    tts_hip_ctx *                  lm = nullptr;     // Llama-3 decoder context
    tts_hip_ctx *                  snac = nullptr;   // SNAC codec context
    std::vector<float>             pcm, logits;
    std::default_random_engine     noise_engine;     // random_normal_gen's engine (util.cpp:74-80): default seed, never reseeded
    std::normal_distribution<float> noise_dist{0.0f, 1.0f};
    int                            snac_halo = -1;   // tts_hip_snac_halo_frames of the codec layout (-1: unknown; chunked audio then decodes whole utterances)

  private:
    // One utterance of a chunked generation.  generate() draws the SNAC noise layer-major over the whole utterance, so where layer 1's noise starts
    // depends on the final length, which is unknown while streaming.  Chunked generation draws frame-major from the same engine instead: frames in
    // increasing order, each once, when it first enters a window (kept or halo), and kept until no later window needs it; per frame, for layer
    // l = 0.., 4 * prod(stride_0..l) normals.  A completed call consumes exactly the draws generate() would.
    struct chunk_state {
        std::vector<uint32_t> ids;                 // the ids so far
        bool                  ended = false;
        uint32_t              next = 0;            // first frame not handed out yet
        uint32_t              noise0 = 0;          // frame of noise.front()
        std::vector<std::vector<float>> noise;     // frames [noise0, noise0 + size)
    };
    struct chunk_pass {                            // the windows of one look-in: one tts_hip_snac_decode_windows pass
        std::vector<uint32_t> utt, codes, frames, keep0, keep1;
        std::vector<float>    noise;
    };
    // session state of the continuous batching
    std::vector<std::vector<float>> st_pcm;      // audio handed out by the last stream_step
    // ... with the chunk hook: the chunker's rows are the slots
    std::vector<chunk_state>        st_rows;     // slot -> its occupant's ids and noise
    std::vector<uint8_t>            st_gen;      // slot -> its occupant is still generating
    std::vector<uint32_t>           st_buf;      // [slots][max_generation_size]: what the waits hand out
    chunk_pass                      st_pass;     // the windows cut at the last look-in ...
    std::vector<size_t>             st_pass_ticket;   // ... and the ticket each was cut for
    std::vector<size_t>             st_closing;  // utterances that ended at the last look-in: their tails are in st_pass
    std::vector<size_t>             st_stopped;  // utterances whose on_chunk returned false since the last look-in
    void stream_step_chunked(std::vector<stream_result> & finished);
    void session_hand_out(std::vector<stream_result> & finished);
    bool device_sampler(const generation_configuration & config) const;
    void sampler_setup(const generation_configuration & config);
    std::vector<uint32_t> checked_prompt(const std::string & sentence, const generation_configuration & config);
    void batch_inputs(const std::vector<std::string> & sentences, const generation_configuration & config, bool dev_sample,
                      std::vector<uint32_t> & prompts, std::vector<uint32_t> & lens, std::vector<float> & uni);
    bool chunk_collect(std::vector<chunk_state> & st, uint32_t chunk_frames, chunk_pass & P);
    void chunk_run(std::vector<chunk_state> & st, bool lockstep, uint32_t chunk_frames, const std::function<bool(uint32_t, const float *, size_t)> & on_chunk);
};
