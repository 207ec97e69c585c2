#include "orpheus_runner.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gguf.h"

// model.cpp:7: the voices are not in the model configuration
static constexpr std::array<const char *, 7> orpheus_voices{"zoe", "zac", "jess", "leo", "mia", "julia", "leah"};

orpheus_model_loader::orpheus_model_loader() : tts_model_loader{"orpheus"} {}
const orpheus_model_loader orpheus_loader{};
void orpheus_register() {}

// orpheus_model::prep_constants / prep_layers (model.cpp:62-120) + snac_model::prep_constants / prep_layers
// (snac_model.cpp:3-48): same keys, same defaults, same required keys.
static orpheus_hparams read_hparams(const gguf_file & m) {
    orpheus_hparams hp;
    m.get_u32({"orpheus.vocab_size"}, hp.vocab_size);
    m.get_u32({"orpheus.attn_heads"}, hp.n_attn_heads);
    m.get_u32({"orpheus.kv_attn_heads"}, hp.n_kv_attn_heads);
    m.get_u32({"orpheus.head_dim"}, hp.head_size);
    m.get_u32({"orpheus.stopping_token_id"}, hp.stopping_token_id);
    m.get_u32({"tokenizer.ggml.eos_token_id"}, hp.eos_token_id);
    m.get_u32({"tokenizer.ggml.bos_token_id"}, hp.bos_token_id);
    m.get_u32({"orpheus.hidden_size"}, hp.hidden_size);
    m.get_u32({"orpheus.kv_hidden_size"}, hp.kv_hidden_size);
    if (!m.get_u32({"orpheus.layers"}, hp.n_layers)) TTS_ABORT("the 'orpheus.layers' must be specified in the GGUF file.\n");
    // extensions (absent in the reference's files)
    m.get_u32({"orpheus.max_context_length"}, hp.max_context_length);
    m.get_u32({"orpheus.max_generation_size"}, hp.max_generation_size);
    m.get_u32({"orpheus.audio_token_offset"}, hp.audio_token_offset);
    m.get_u32({"orpheus.audio_token_stride"}, hp.audio_token_stride);
    auto u32_array = [&](const char * key, std::vector<uint32_t> & out) {
        if (const gguf_value * v = m.get(key)) {
            if (v->arr_data && v->arr_n && (v->elem_type == GGUF_U32 || v->elem_type == GGUF_I32)) out.assign((const uint32_t *) v->arr_data, (const uint32_t *) v->arr_data + v->arr_n);
        }
    };
    u32_array("orpheus.prepended_tokens", hp.prepended_tokens);
    u32_array("orpheus.appended_tokens", hp.appended_tokens);

    m.get_u32({"snac.audio_token_channels"}, hp.snac_heads);
    m.get_u32({"snac.up_sampling_factor"}, hp.snac_up);
    m.get_u32({"snac.max_generation_size"}, hp.snac_max_generation);
    // the reference fixes 4 layers (snac_model.h:12) and aborts on a missing key; like the DAC loader, the count here is
    // how many consecutive stride keys the file holds, so small synthetic codecs load too
    uint32_t n = 0, up = 1;
    for (uint32_t i = 0; i < TTS_HIP_MAX_DAC_BLOCKS; i++) {
        const std::string sk = "snac.snac_layer_stride_" + std::to_string(i), pk = "snac.snac_layer_padding_" + std::to_string(i),
                          gk = "snac.snac_layer_grouping_" + std::to_string(i);
        if (!m.get_u32({sk.c_str()}, hp.snac_stride[i])) {
            if (i == 0) TTS_ABORT("key %s must be specified in gguf file inorder to initialize the SNAC audio decoder.\n", sk.c_str());
            break;
        }
        if (!m.get_u32({pk.c_str()}, hp.snac_padding[i])) TTS_ABORT("key %s must be specified in gguf file inorder to initialize the SNAC audio decoder.\n", pk.c_str());
        if (!m.get_u32({gk.c_str()}, hp.snac_groups[i])) TTS_ABORT("key %s must be specified in gguf file inorder to initialize the SNAC audio decoder.\n", gk.c_str());
        up *= hp.snac_stride[i];
        n++;
    }
    hp.snac_layers = n;
    if (up != hp.snac_up) hp.snac_up = up;
    if (hp.snac_heads != 3) TTS_ABORT("SNAC with %u token channels is unsupported (3: 4/2/1 repeats, snac_model.h:17)\n", hp.snac_heads);
    return hp;
}

std::unique_ptr<tts_generation_runner> orpheus_model_loader::from_file(gguf_file * meta, int, bool, const generation_configuration &) const {
    const orpheus_hparams hp = read_hparams(*meta);
    const int device = tts_load_device();
    return std::make_unique<orpheus_runner>(hp, bpe_tokenizer_from_gguf(*meta), device);
}

orpheus_runner::orpheus_runner(const orpheus_hparams & hp_, bpe_tokenizer * tok, int device)
    : stream_session{orpheus_loader}, hp(hp_), tokenizer(tok) {
    tts_hip_orpheus_desc d{};
    d.struct_size = sizeof(d);
    d.hidden_size = hp.hidden_size; d.n_layers = hp.n_layers; d.n_attn_heads = hp.n_attn_heads; d.n_kv_heads = hp.n_kv_attn_heads;
    d.head_dim = hp.head_size; d.vocab_size = hp.vocab_size;
    d.n_ctx = hp.max_context_length + hp.max_generation_size;   // orpheus_kv_cache_init, model.cpp:176-177
    // up to 256 slots = the rows one decoder forward carries (tts_hip_orpheus_create); at 3B shapes a slot of the cache is 0.72 GB, 0.36 GB under TTS_HIP_KV_F16, 0.18 GB under TTS_HIP_KV_F8
    const uint32_t asked = std::max<uint32_t>(1, tts_load_max_seqs());
    max_seqs = std::min<uint32_t>(asked, 256);
    if (max_seqs != asked) fprintf(stderr, "orpheus: max_seqs %u exceeds what one decoder forward carries: loading with %u slots\n", asked, max_seqs);
    d.max_seqs = max_seqs;
    // both read once, here: the cache element type is fixed at create
    if (getenv("TTS_HIP_KV_F16") && getenv("TTS_HIP_KV_F8")) TTS_ABORT("orpheus: TTS_HIP_KV_F16 and TTS_HIP_KV_F8 are both set: one K/V cache element type per runner\n");
    if (getenv("TTS_HIP_KV_F16")) d.flags |= TTS_HIP_FLAG_KV_F16;   // the switch Parler's runner reads: fp16 K/V cache (extension, include/tts_hip.h)
    if (getenv("TTS_HIP_KV_F8")) d.kv_type = TTS_HIP_KV_F8_E4M3;    // one-byte e4m3 K/V cache (extension, tts_hip_orpheus_desc::kv_type)
    lm = tts_hip_orpheus_create(device, &d);
    if (!lm) TTS_ABORT("tts_hip_orpheus_create failed: %s\n", tts_hip_last_error());
    tts_hip_snac_desc s{};
    s.struct_size = sizeof(s);
    s.n_blocks = hp.snac_layers;
    for (uint32_t i = 0; i < hp.snac_layers; i++) { s.stride[i] = hp.snac_stride[i]; s.padding[i] = hp.snac_padding[i]; s.groups[i] = hp.snac_groups[i]; }
    s.n_codebooks = hp.snac_heads;
    for (uint32_t i = 0; i < 3; i++) s.repeats[i] = hp.snac_repeats[i];
    s.max_frames = hp.snac_max_generation;
    snac = tts_hip_snac_create(device, &s);
    if (!snac) {
        // the destructor does not run for a constructor that throws (TTS_ABORT under g_tts_throw_on_abort): release the decoder context
        tts_hip_destroy(lm);
        lm = nullptr;
        TTS_ABORT("tts_hip_snac_create failed: %s\n", tts_hip_last_error());
    }
    snac_halo = tts_hip_snac_halo_frames(&s);
    sampling_rate = 24000.0f;           // model.h:112
    supports_voices = true;
    smp.n_output_heads = 1;             // model.h:113-115
    smp.vocab_size = hp.vocab_size;
    smp.eos_token_id = hp.eos_token_id;
}

orpheus_runner::~orpheus_runner() {
    tts_hip_destroy(lm);
    tts_hip_destroy(snac);
}

void orpheus_runner::assign_weight(const char * name, const gguf_tensor_view & t) {
    // model.cpp:430-438: "snac." goes to the codec, "orpheus." to the decoder (the shim routes by the same prefixes)
    if (!strncmp(name, "snac.", 5)) hip_check(tts_hip_upload(snac, name, t.type, t.n_dims, t.ne, t.data), name);
    else if (!strncmp(name, "orpheus.", 8)) hip_check(tts_hip_upload(lm, name, t.type, t.n_dims, t.ne, t.data), name);
    else fprintf(stdout, "Warning: function %s encountered an unhandled tensor named '%s'.\n", __func__, name);
}

void orpheus_runner::prepare_post_load() {
    hip_check(tts_hip_finalize(lm, nullptr), "tts_hip_finalize(orpheus)");
    hip_check(tts_hip_finalize(snac, nullptr), "tts_hip_finalize(snac)");
    logits.resize(hp.vocab_size);
}

std::vector<std::string_view> orpheus_runner::list_voices() {
    return std::vector<std::string_view>(orpheus_voices.begin(), orpheus_voices.end());
}

std::vector<uint32_t> orpheus_runner::batch_from_sentence(const std::string & sentence, const std::string & voice) const {
    std::vector<uint32_t> tokens(hp.prepended_tokens);
    tokenizer->tokenize(voice.empty() ? sentence : voice + ": " + sentence, tokens);
    tokens.insert(tokens.end(), hp.appended_tokens.begin(), hp.appended_tokens.end());
    return tokens;
}

std::vector<std::vector<uint32_t>> orpheus_runner::prepare_output_tokens(const std::vector<uint32_t> & out) const {
    std::vector<std::vector<uint32_t>> levels(hp.audio_heads);
    const size_t chunks = out.size() / 7;
    for (size_t i = 0; i < chunks; i++)
        for (size_t ii = 0; ii < 7; ii++)
            levels[hp.heads[ii]].push_back(out[i * 7 + ii] - hp.audio_token_offset - (uint32_t) (ii % 7) * hp.audio_token_stride);
    return levels;
}

uint32_t orpheus_runner::kv_element_bytes() const {
    float v = 0.0f;
    return tts_hip_debug_read(lm, "l_kv_elem", &v, 1) == 1 ? (uint32_t) v : 0;
}

// what tts_hip_orpheus_generate_sampled's device sampler takes (top_k 1..64, any top_p > 0); TTS_HOST_LOOP forces the host sampler
bool orpheus_runner::device_sampler(const generation_configuration & config) const {
    return config.sample && !getenv("TTS_HOST_LOOP") && config.top_p > 0.0f && config.top_k >= 1 && config.top_k <= 64 && (uint32_t) config.top_k < hp.vocab_size;
}

// the sampler as a generate() call starts it: the call's parameters, n_calls = 0, reset
void orpheus_runner::sampler_setup(const generation_configuration & config) {
    smp.temperature = config.temperature;
    smp.repetition_penalty = config.repetition_penalty;
    smp.do_sample = config.sample;
    smp.top_k = (uint32_t) config.top_k;
    smp.top_p = config.top_p;
    smp.seed = config.seed;
    smp.n_calls = 0;
    smp.reset();
}

// voice check, framing and tokenisation, length check; the prompt is remembered in last_prompt_tokens
std::vector<uint32_t> orpheus_runner::checked_prompt(const std::string & sentence, const generation_configuration & config) {
    if (!config.voice.empty() && std::find(orpheus_voices.begin(), orpheus_voices.end(), config.voice) == orpheus_voices.end())
        TTS_ABORT("Voice '%s' is not a valid voice for Orpheus.\n", config.voice.c_str());
    std::vector<uint32_t> prompt = batch_from_sentence(sentence, config.voice);
    if (prompt.size() > hp.max_context_length)
        TTS_ABORT("The prompt was too large for the default context window. Try splitting up or shortenning the prompt.\n");
    last_prompt_tokens = prompt;
    return prompt;
}

// a lock-step batch's inputs: the checked prompts concatenated, their lengths and, for the device sampler, the uniforms [utterance][step]
void orpheus_runner::batch_inputs(const std::vector<std::string> & sentences, const generation_configuration & config, bool dev_sample,
                                  std::vector<uint32_t> & prompts, std::vector<uint32_t> & lens, std::vector<float> & uni) {
    const uint32_t n = (uint32_t) sentences.size(), M = hp.max_generation_size;
    for (uint32_t u = 0; u < n; u++) {
        const std::vector<uint32_t> p = checked_prompt(sentences[u], config);
        lens.push_back((uint32_t) p.size());
        prompts.insert(prompts.end(), p.begin(), p.end());
    }
    if (!dev_sample) return;
    uni.resize((size_t) n * M);
    for (uint32_t u = 0; u < n; u++) {   // generate() per utterance: same parameters, n_calls = 0, reset, then one draw per sampler call
        sampler_setup(config);
        for (uint32_t k = 0; k < M; k++) smp.draw_uniforms(&uni[(size_t) u * M + k]);
    }
}

void orpheus_runner::generate(const char * sentence, tts_response & output, const generation_configuration & config) {
    const std::vector<uint32_t> prompt = checked_prompt(sentence, config);
    sampler_setup(config);
    output.data = nullptr;
    output.n_outputs = 0;

    // generate_from_batch (model.cpp:378-392)
    std::vector<uint32_t> & out = last_output_tokens;
    out.clear();
    if (!config.sample) {
        out.resize(hp.max_generation_size);
        uint32_t n = 0;
        hip_check(tts_hip_orpheus_generate_greedy(lm, prompt.data(), (uint32_t) prompt.size(), hp.max_generation_size, hp.stopping_token_id, out.data(), &n),
                  "tts_hip_orpheus_generate_greedy");
        out.resize(n);
    } else if (device_sampler(config)) {
        // top_k in 1..64 (the default generation_configuration: top_k 50, top_p 1): sampler::sample runs on the device, two kernels pick the
        // top_k candidates out of the 156 940 logits (top_p < 1: a third accumulates the full-vocabulary softmax total in index order first,
        // round 5); the U[0,1) draws are made here, one generator per call as sampler.cpp:47-48
        std::vector<float> u(hp.max_generation_size);
        for (auto & v : u) smp.draw_uniforms(&v);
        tts_hip_sampling sp{(uint32_t) config.top_k, config.top_p, config.temperature, config.repetition_penalty};
        out.resize(hp.max_generation_size);
        uint32_t n = 0;
        hip_check(tts_hip_orpheus_generate_sampled(lm, prompt.data(), (uint32_t) prompt.size(), hp.max_generation_size, hp.stopping_token_id, &sp, u.data(), out.data(), &n),
                  "tts_hip_orpheus_generate_sampled");
        out.resize(n);
    } else {
        // a top_k the device sampler does not take (0 = off, or > 64: the reference sorts the whole vocabulary): logits come back,
        // sampler::sample runs here
        std::vector<uint32_t> batch = prompt;
        uint32_t pos = 0;
        while ((out.empty() || out.back() != hp.stopping_token_id) && out.size() < hp.max_generation_size) {
            hip_check(tts_hip_orpheus_decode(lm, batch.data(), (uint32_t) batch.size(), pos, logits.data(), nullptr), "tts_hip_orpheus_decode");
            pos += (uint32_t) batch.size();
            smp.sample(logits.data(), out);
            batch.assign(1, out.back());
        }
    }
    decode_audio(out, pcm);
    output.data = pcm.empty() ? nullptr : pcm.data();
    output.n_outputs = pcm.size();
}

// the 7-ids-per-frame stream -> SNAC levels -> audio (model.cpp:358-376, snac_runner::run)
void orpheus_runner::decode_audio(const std::vector<uint32_t> & out, std::vector<float> & audio) {
    audio.clear();
    if (out.size() >= hp.max_generation_size)
        fprintf(stdout, "Warning: generation hit its max default length. The generated audio may not contain the entire prompt.\n");
    const std::vector<std::vector<uint32_t>> levels = prepare_output_tokens(out);
    const uint32_t T = (uint32_t) levels[2].size();   // finest level: 4 ids per 7-id chunk (snac_runner::run :181)
    if (T == 0) return;
    std::vector<uint32_t> codes;
    for (auto & l : levels) codes.insert(codes.end(), l.begin(), l.end());
    // snac_runner::set_inputs (:177): noise_steps_sum * T standard normals from the never-reseeded engine
    size_t noise_len = 0, up = 1;
    for (uint32_t i = 0; i < hp.snac_layers; i++) { up *= hp.snac_stride[i]; noise_len += up * (size_t) T; }
    std::vector<float> noise;
    if (!getenv("TTS_SNAC_NO_NOISE")) {
        noise.resize(noise_len);
        for (auto & v : noise) v = noise_dist(noise_engine);
    }
    audio.assign((size_t) T * hp.snac_up, 0.0f);
    hip_check(tts_hip_snac_decode(snac, codes.data(), T, noise.empty() ? nullptr : noise.data(), audio.data()), "tts_hip_snac_decode");
}

// n utterances in lock-step on the device: one cache slot and one row of the forward per utterance (the reference: one worker and one model copy per
// concurrent request, examples/server/server.cpp:225-321).  Every utterance gets the ids a generate() call of its own would produce — the sampler is
// reset per utterance exactly as generate() does, so with config.sample every utterance draws the same uniform sequence its own call would —
// and the codec then runs utterance by utterance in order (the noise engine is never reseeded: the draws follow the order of sequential calls).
void orpheus_runner::generate_batch(const std::vector<std::string> & sentences, std::vector<tts_response> & outputs, const generation_configuration & config) {
    const uint32_t n = (uint32_t) sentences.size();
    const bool dev_sample = device_sampler(config);
    if (n <= 1 || max_seqs <= 1 || (config.sample && !dev_sample)) { tts_generation_runner::generate_batch(sentences, outputs, config); return; }
    if (n > max_seqs) TTS_ABORT("generate_batch: %u utterances but the runner was loaded with max_seqs=%u (TTS_HIP_MAX_SEQS)\n", n, max_seqs);
    std::vector<uint32_t> prompts, lens;
    std::vector<float> uni;
    batch_inputs(sentences, config, dev_sample, prompts, lens, uni);
    const uint32_t M = hp.max_generation_size;
    std::vector<uint32_t> toks((size_t) n * M), cnt(n);
    tts_hip_sampling sp{(uint32_t) config.top_k, config.top_p, config.temperature, config.repetition_penalty};
    hip_check(tts_hip_orpheus_generate_batch(lm, n, prompts.data(), lens.data(), M, hp.stopping_token_id, dev_sample ? &sp : nullptr, dev_sample ? uni.data() : nullptr, toks.data(),
                                             cnt.data()), "tts_hip_orpheus_generate_batch");
    outputs.assign(n, tts_response{});
    batch_store_.assign(n, {});
    last_batch_tokens.assign(n, {});
    for (uint32_t u = 0; u < n; u++) {
        last_batch_tokens[u].assign(toks.begin() + (size_t) u * M, toks.begin() + (size_t) u * M + cnt[u]);
        decode_audio(last_batch_tokens[u], batch_store_[u]);
        outputs[u].data = batch_store_[u].empty() ? nullptr : batch_store_[u].data();
        outputs[u].n_outputs = batch_store_[u].size();
    }
    last_output_tokens = last_batch_tokens[n - 1];
}

// ---- chunked audio -------------------------------------------------------------------------------------------------------------------
// The windows the ids known now make ready: per utterance one cut of chunk_windows.h over its whole frames.  Trailing ids that do not fill a group of 7 are dropped, as
// prepare_output_tokens does.  Returns whether there is a window.
bool orpheus_runner::chunk_collect(std::vector<chunk_state> & st, uint32_t chunk_frames, chunk_pass & P) {
    P = chunk_pass{};
    const uint32_t h = (uint32_t) snac_halo;
    const bool with_noise = !getenv("TTS_SNAC_NO_NOISE");
    std::vector<size_t> per_layer(hp.snac_layers);   // normals per frame and layer
    size_t per_frame = 0;
    { size_t up = 1; for (uint32_t l = 0; l < hp.snac_layers; l++) { up *= hp.snac_stride[l]; per_layer[l] = 4 * up; per_frame += 4 * up; } }
    for (uint32_t u = 0; u < st.size(); u++) {
        chunk_state & s = st[u];
        const uint32_t F = (uint32_t) (s.ids.size() / 7);
        const chunk_window c = cut_chunk_window(s.next, F, h, chunk_frames, s.ended);
        if (c.end == s.next) continue;
        const uint32_t f1 = c.end, w0 = c.w0, w1 = c.w1;
        const std::vector<uint32_t> part(s.ids.begin() + (size_t) 7 * w0, s.ids.begin() + (size_t) 7 * w1);
        for (auto & l : prepare_output_tokens(part)) P.codes.insert(P.codes.end(), l.begin(), l.end());
        P.utt.push_back(u); P.frames.push_back(w1 - w0); P.keep0.push_back(c.keep0); P.keep1.push_back(c.keep1);
        if (with_noise) {
            while (s.noise0 + s.noise.size() < w1) {   // frames enter in increasing order, each drawn once
                s.noise.emplace_back(per_frame);
                for (auto & v : s.noise.back()) v = noise_dist(noise_engine);
            }
            size_t off = 0;
            for (uint32_t l = 0; l < hp.snac_layers; l++) {   // the window's noise, layer-major
                for (uint32_t f = w0; f < w1; f++) {
                    const float * src = s.noise[f - s.noise0].data() + off;
                    P.noise.insert(P.noise.end(), src, src + per_layer[l]);
                }
                off += per_layer[l];
            }
            const uint32_t keep_from = f1 > h ? f1 - h : 0;   // the next window starts here
            if (keep_from > s.noise0) { s.noise.erase(s.noise.begin(), s.noise.begin() + (keep_from - s.noise0)); s.noise0 = keep_from; }
        }
        s.next = f1;
    }
    return !P.utt.empty();
}

static size_t chunk_samples(const std::vector<uint32_t> & keep0, const std::vector<uint32_t> & keep1, uint32_t up) {
    size_t k = 0;
    for (size_t i = 0; i < keep0.size(); i++) k += keep1[i] - keep0[i];
    return std::max<size_t>(1, k * 4 * up);
}

// the look-in loop over a generation that tts_hip_orpheus_gen_begin has started.  One sequence: launch the next piece of decoder steps (the call
// returns while they run), decode the windows the previous look-in made ready on the codec's stream, call back, then look at the piece's ids.
// A lock-step launch returns only after its steps ran, so there the ready windows are decoded and handed out first: hiding a codec pass of a few
// ms behind a piece of blocking steps would hold every chunk back by that piece (15 ms at chunk_frames 1, 120 ms at 16 for 8 rows of Orpheus-3B).
void orpheus_runner::chunk_run(std::vector<chunk_state> & st, bool lockstep, uint32_t chunk_frames, const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) {
    const uint32_t n = (uint32_t) st.size(), M = hp.max_generation_size;
    const uint32_t piece = 7 * std::min<uint32_t>(chunk_frames, 8);   // decoder steps per look-in: one chunk's ids, at most 8 frames'
    std::vector<uint32_t> toks((size_t) n * M), cnt(n, 0);
    std::vector<uint8_t> done(n, 0);
    auto look = [&]() {
        hip_check(tts_hip_orpheus_gen_wait(lm, toks.data(), cnt.data(), done.data()), "tts_hip_orpheus_gen_wait");
        for (uint32_t u = 0; u < n; u++) {
            st[u].ids.assign(toks.begin() + (size_t) u * M, toks.begin() + (size_t) u * M + cnt[u]);
            st[u].ended = done[u] != 0;
        }
    };
    look();
    chunk_pass P;
    bool go_on = true;
    bool in_flight = false;   // a launch no look() has followed yet
    try {
    while (go_on) {
        bool all_done = true;
        for (auto & s : st) all_done = all_done && s.ended;
        const bool have = chunk_collect(st, chunk_frames, P);
        if (all_done && !have) break;
        const bool launch = !all_done;
        if (launch && !lockstep) { hip_check(tts_hip_orpheus_gen_launch(lm, piece), "tts_hip_orpheus_gen_launch"); in_flight = true; }
        if (have) {
            pcm.resize(chunk_samples(P.keep0, P.keep1, hp.snac_up));
            hip_check(tts_hip_snac_decode_windows_begin(snac, P.codes.data(), P.frames.data(), P.keep0.data(), P.keep1.data(), (uint32_t) P.utt.size(),
                                                        P.noise.empty() ? nullptr : P.noise.data(), pcm.data()), "tts_hip_snac_decode_windows");
            hip_check(tts_hip_snac_decode_windows_end(snac), "tts_hip_snac_decode_windows");
            go_on = hand_out_rows(P.keep0, P.keep1, P.utt, chunk_frames, (size_t) 4 * hp.snac_up, pcm.data(), on_chunk);
        }
        if (launch && lockstep && go_on) hip_check(tts_hip_orpheus_gen_launch(lm, piece), "tts_hip_orpheus_gen_launch");
        if (launch) { in_flight = false; look(); }
    }
    } catch (...) {
        // an error (the codec refusing an id) or a throwing callback: the steps under way are waited for, so the decoder context stays usable
        if (in_flight) (void) tts_hip_orpheus_gen_wait(lm, toks.data(), cnt.data(), done.data());
        throw;
    }
}

void orpheus_runner::generate_chunked(const char * sentence, const generation_configuration & config, uint32_t chunk_frames,
                                      const std::function<bool(const float *, size_t)> & on_chunk) {
    if (chunk_frames == 0) TTS_ABORT("generate_chunked: chunk_frames must be >= 1\n");
    if (snac_halo < 0) { tts_generation_runner::generate_chunked(sentence, config, chunk_frames, on_chunk); return; }
    const std::vector<uint32_t> prompt = checked_prompt(sentence, config);
    sampler_setup(config);
    const uint32_t M = hp.max_generation_size, n_prompt = (uint32_t) prompt.size();
    std::vector<chunk_state> st(1);
    const auto cb = [&](uint32_t, const float * p, size_t k) { return on_chunk(p, k); };
    const bool dev_sample = device_sampler(config);
    if (!config.sample || dev_sample) {
        std::vector<float> u;
        tts_hip_sampling sp{(uint32_t) config.top_k, config.top_p, config.temperature, config.repetition_penalty};
        if (dev_sample) {
            u.resize(M);
            for (auto & v : u) smp.draw_uniforms(&v);
        }
        hip_check(tts_hip_orpheus_gen_begin(lm, 1, prompt.data(), &n_prompt, M, hp.stopping_token_id, dev_sample ? &sp : nullptr, dev_sample ? u.data() : nullptr),
                  "tts_hip_orpheus_gen_begin");
        chunk_run(st, false, chunk_frames, cb);
    } else {
        // the host sampler: logits come back at every step, so the windows are decoded between two steps (no overlap)
        const uint32_t piece = 7 * std::min<uint32_t>(chunk_frames, 8);
        std::vector<uint32_t> batch = prompt, & out = st[0].ids;
        uint32_t pos = 0;
        chunk_pass P;
        bool go_on = true;
        while (go_on) {
            st[0].ended = !((out.empty() || out.back() != hp.stopping_token_id) && out.size() < M);
            if (st[0].ended || out.size() % piece == 0) {
                if (chunk_collect(st, chunk_frames, P)) {
                    pcm.resize(chunk_samples(P.keep0, P.keep1, hp.snac_up));
                    hip_check(tts_hip_snac_decode_windows(snac, P.codes.data(), P.frames.data(), P.keep0.data(), P.keep1.data(), 1, P.noise.empty() ? nullptr : P.noise.data(), pcm.data()),
                              "tts_hip_snac_decode_windows");
                    go_on = hand_out_rows(P.keep0, P.keep1, P.utt, chunk_frames, (size_t) 4 * hp.snac_up, pcm.data(), cb);
                }
            }
            if (st[0].ended || !go_on) break;
            hip_check(tts_hip_orpheus_decode(lm, batch.data(), (uint32_t) batch.size(), pos, logits.data(), nullptr), "tts_hip_orpheus_decode");
            pos += (uint32_t) batch.size();
            smp.sample(logits.data(), out);
            batch.assign(1, out.back());
        }
    }
    last_output_tokens = st[0].ids;
    if (last_output_tokens.size() >= M)
        fprintf(stdout, "Warning: generation hit its max default length. The generated audio may not contain the entire prompt.\n");
}

void orpheus_runner::generate_batch_chunked(const std::vector<std::string> & sentences, const generation_configuration & config, uint32_t chunk_frames,
                                            const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) {
    if (chunk_frames == 0) TTS_ABORT("generate_batch_chunked: chunk_frames must be >= 1\n");
    const uint32_t n = (uint32_t) sentences.size();
    const bool dev_sample = device_sampler(config);
    if (snac_halo < 0) { tts_generation_runner::generate_batch_chunked(sentences, config, chunk_frames, on_chunk); return; }
    if (n <= 1 || max_seqs <= 1 || (config.sample && !dev_sample)) {   // as generate_batch: one utterance after the other, each one streaming
        last_batch_tokens.assign(n, {});
        bool go_on = true;
        for (uint32_t u = 0; u < n && go_on; u++) {
            generate_chunked(sentences[u].c_str(), config, chunk_frames, [&](const float * p, size_t k) { return go_on = on_chunk(u, p, k); });
            last_batch_tokens[u] = last_output_tokens;
        }
        return;
    }
    if (n > max_seqs) TTS_ABORT("generate_batch_chunked: %u utterances but the runner was loaded with max_seqs=%u (TTS_HIP_MAX_SEQS)\n", n, max_seqs);
    std::vector<uint32_t> prompts, lens;
    std::vector<float> uni;
    batch_inputs(sentences, config, dev_sample, prompts, lens, uni);
    const uint32_t M = hp.max_generation_size;
    tts_hip_sampling sp{(uint32_t) config.top_k, config.top_p, config.temperature, config.repetition_penalty};
    hip_check(tts_hip_orpheus_gen_begin(lm, n, prompts.data(), lens.data(), M, hp.stopping_token_id, dev_sample ? &sp : nullptr, dev_sample ? uni.data() : nullptr),
              "tts_hip_orpheus_gen_begin");
    std::vector<chunk_state> st(n);
    chunk_run(st, true, chunk_frames, on_chunk);
    last_batch_tokens.assign(n, {});
    for (uint32_t u = 0; u < n; u++) last_batch_tokens[u] = st[u].ids;
    last_output_tokens = last_batch_tokens[n - 1];
}

// ---- continuous batching (common.h; tts_hip_orpheus_stream_* underneath) ---------------------------------------------------------------
// Decoder steps between two look-ins.  A multiple of 7 ids, so an utterance admitted at a look-in is looked at on SNAC frame boundaries; four frames:
// a finished row idles as padding for at most 27 steps (about 1 % of a 2100-id utterance, 14 steps on average) and a queued request waits at most
// 28 steps (about 0.1 s at 8 rows of Orpheus-3B) for a free slot, while a look-in's staging copies, synchronise and state copy (tens of
// microseconds) are spread over 28 forwards of a few milliseconds each.
static constexpr uint32_t ORPHEUS_STREAM_STEPS = 28;

void orpheus_runner::stream_begin(const generation_configuration & config) {
    if (stream_capacity() == 0) TTS_ABORT("stream_begin: the runner was loaded with max_seqs=%u; a session needs >= 2 (TTS_HIP_MAX_SEQS)\n", max_seqs);
    if (getenv("TTS_HOST_LOOP")) TTS_ABORT("stream_begin: TTS_HOST_LOOP asks for the host loop; a session runs on the device\n");
    if (config.sample && !device_sampler(config))
        TTS_ABORT("stream_begin: the device sampler takes top_k in 1..64 and top_p > 0 (got top_k %d, top_p %g); a session cannot sample on the host\n", config.top_k, config.top_p);
    if (st_on) stream_end();
    {   // a chunked generation that its callback stopped is abandoned here, as a generate() call would abandon it
        const uint32_t one = 1, id = 0;
        hip_check(tts_hip_orpheus_gen_begin(lm, 1, &id, &one, 0, hp.stopping_token_id, nullptr, nullptr), "tts_hip_orpheus_gen_begin");
    }
    const uint32_t slots = stream_capacity();
    hip_check(tts_hip_orpheus_stream_begin_mixed(lm, slots, hp.max_generation_size, hp.stopping_token_id), "tts_hip_orpheus_stream_begin_mixed");
    session_open(config, slots);
    st_pcm.clear();
}

// chunked audio out of the session (common.h): this runner's part of stream_session's hook
bool orpheus_runner::session_chunks_ready(uint32_t) {
    if (!st_on) TTS_ABORT("stream_chunks: no session (stream_begin)\n");
    if (st_live != 0) TTS_ABORT("stream_chunks: after stream_begin and before the first stream_submit\n");
    if (snac_halo < 0) return false;   // no window pass for this codec layout: whole utterances, as without the hook
    const uint32_t slots = stream_capacity();
    st_rows.assign(slots, {});
    st_gen.assign(slots, 0);
    st_buf.assign((size_t) slots * hp.max_generation_size, 0u);
    st_pass = chunk_pass{};
    st_pass_ticket.clear();
    st_closing.clear();
    st_stopped.clear();
    last_batch_tokens.clear();
    return true;
}

bool orpheus_runner::stream_accepts(const generation_configuration & config) const {
    if (!st_on) return false;
    if (!config.voice.empty() && std::find(orpheus_voices.begin(), orpheus_voices.end(), config.voice) == orpheus_voices.end()) return false;
    return !config.sample || device_sampler(config);
}

void orpheus_runner::stream_submit(size_t ticket, const std::string & sentence, const generation_configuration & config) {
    if (!st_on) TTS_ABORT("stream_submit: no session (stream_begin)\n");
    if (st_free.empty()) TTS_ABORT("stream_submit: no free row (stream_free() == 0)\n");
    if (config.sample && !device_sampler(config))
        TTS_ABORT("stream_submit: the device sampler takes top_k in 1..64 and top_p > 0 (got top_k %d, top_p %g); a session cannot sample on the host\n", config.top_k, config.top_p);
    const std::vector<uint32_t> prompt = checked_prompt(sentence, config);
    const uint32_t M = hp.max_generation_size, n_prompt = (uint32_t) prompt.size();
    std::vector<float> uni;
    if (config.sample) {   // as batch_inputs: the sampler as a generate() call of this utterance's own starts it, one draw per sampler call
        uni.resize(M);
        sampler_setup(config);
        for (auto & v : uni) smp.draw_uniforms(&v);
    }
    const uint32_t slot = st_free.back();
    const tts_hip_sampling sp{(uint32_t) config.top_k, config.top_p, config.temperature, config.repetition_penalty};
    const tts_hip_sampling * spp = config.sample ? &sp : nullptr;
    hip_check(tts_hip_orpheus_stream_admit_mixed(lm, 1, &slot, prompt.data(), &n_prompt, &spp, config.sample ? uni.data() : nullptr), "tts_hip_orpheus_stream_admit_mixed");
    st_free.pop_back();
    st_ticket[slot] = ticket;
    st_live++;
    if (st_chunk_frames) {   // a new occupant: its ids and its chunker row start at zero
        st_rows[slot] = {};
        st_gen[slot] = 1;
    }
}

// the windows the last look-in cut, through the codec in one pass and out chunk by chunk, each under the ticket it was cut for; then the utterances
// that had ended at that look-in have had their last chunk.  An utterance whose callback returns false gets nothing more.
void orpheus_runner::session_hand_out(std::vector<stream_result> & finished) {
    const chunk_pass & P = st_pass;
    if (!P.utt.empty()) {
        pcm.resize(chunk_samples(P.keep0, P.keep1, hp.snac_up));
        hip_check(tts_hip_snac_decode_windows_begin(snac, P.codes.data(), P.frames.data(), P.keep0.data(), P.keep1.data(), (uint32_t) P.utt.size(),
                                                    P.noise.empty() ? nullptr : P.noise.data(), pcm.data()), "tts_hip_snac_decode_windows");
        hip_check(tts_hip_snac_decode_windows_end(snac), "tts_hip_snac_decode_windows");
        hand_out_session(P.keep0, P.keep1, st_pass_ticket, st_chunk_frames, (size_t) 4 * hp.snac_up, pcm.data(), st_on_chunk, st_stopped);
    }
    st_pass = chunk_pass{};
    st_pass_ticket.clear();
    for (size_t ticket : st_closing) {
        report_no_audio(finished, ticket);
        st_live--;
    }
    st_closing.clear();
}

// stream_step with the hook (orpheus_runner.h): the codec pass of the windows cut at the last look-in runs on the codec context while this
// interval's decoder steps run on the decoder's.
void orpheus_runner::stream_step_chunked(std::vector<stream_result> & finished) {
    const uint32_t slots = stream_capacity(), M = hp.max_generation_size;
    std::vector<uint32_t> fs(slots), fn(slots), cnt(slots);
    std::vector<uint8_t> done(slots);
    uint32_t nf = 0;
    hip_check(tts_hip_orpheus_stream_launch(lm, ORPHEUS_STREAM_STEPS), "tts_hip_orpheus_stream_launch");
    try {
        session_hand_out(finished);
    } catch (...) {
        // an error (the codec refusing an id) or a throwing callback: the steps under way are waited for, so the decoder context stays usable
        (void) tts_hip_orpheus_stream_wait(lm, nullptr, nullptr, nullptr, &nf, fs.data(), fn.data());
        throw;
    }
    hip_check(tts_hip_orpheus_stream_wait(lm, st_buf.data(), cnt.data(), done.data(), &nf, fs.data(), fn.data()), "tts_hip_orpheus_stream_wait");
    std::vector<uint32_t> drop;
    std::vector<uint8_t> ended(slots, 0);
    bool generating = false;
    for (uint32_t s = 0; s < slots; s++) {
        if (!st_gen[s]) continue;
        chunk_state & row = st_rows[s];
        const uint32_t * b = st_buf.data() + (size_t) s * M;
        row.ids.insert(row.ids.end(), b + row.ids.size(), b + cnt[s]);
        const bool stopped = std::find(st_stopped.begin(), st_stopped.end(), st_ticket[s]) != st_stopped.end();
        if (!done[s] && !stopped) { generating = true; continue; }
        // the occupant leaves: its ids are on the host, the slot is free for the next admission
        remember_tokens(st_ticket[s], row.ids);
        if (row.ids.size() >= M) fprintf(stdout, "Warning: generation hit its max default length. The generated audio may not contain the entire prompt.\n");
        st_gen[s] = 0;
        st_free.push_back(s);
        if (stopped) {   // on_chunk ended it: reported with what it got, nothing more is decoded for it
            if (!done[s]) drop.push_back(s);
            row = {};
            report_no_audio(finished, st_ticket[s]);
            st_live--;
        } else {
            row.ended = true;
            ended[s] = 1;
            st_closing.push_back(st_ticket[s]);
        }
    }
    st_stopped.clear();
    if (!drop.empty()) hip_check(tts_hip_orpheus_stream_drop(lm, (uint32_t) drop.size(), drop.data()), "tts_hip_orpheus_stream_drop");
    chunk_collect(st_rows, st_chunk_frames, st_pass);   // the noise draws: slot order, frames increasing
    for (uint32_t s : st_pass.utt) st_pass_ticket.push_back(st_ticket[s]);
    for (uint32_t s = 0; s < slots; s++)
        if (ended[s]) st_rows[s] = {};   // its tail is in the windows
    if (!generating) {   // nothing to run the codec under: the tails now
        session_hand_out(finished);
        st_stopped.clear();   // only utterances that had ended could be stopped here
    }
}

void orpheus_runner::stream_step(std::vector<stream_result> & finished) {
    if (!st_on) TTS_ABORT("stream_step: no session (stream_begin)\n");
    finished.clear();
    if (st_chunk_frames) return stream_step_chunked(finished);
    std::vector<uint32_t> fs(stream_capacity()), fn(stream_capacity());
    uint32_t nf = 0;
    hip_check(tts_hip_orpheus_stream_run(lm, ORPHEUS_STREAM_STEPS, &nf, fs.data(), fn.data()), "tts_hip_orpheus_stream_run");
    st_pcm.assign(nf, {});
    for (uint32_t i = 0; i < nf; i++) {   // in slot order; the codec runs utterance by utterance, as in generate_batch
        const uint32_t slot = fs[i];
        std::vector<uint32_t> ids(fn[i]);
        hip_check(tts_hip_orpheus_stream_collect(lm, slot, fn[i], ids.data()), "tts_hip_orpheus_stream_collect");
        st_free.push_back(slot);
        st_live--;
        decode_audio(ids, st_pcm[i]);   // ids the codec refuses abort here, as they do in generate()
        last_output_tokens = std::move(ids);
        stream_result r;
        r.ticket = st_ticket[slot];
        r.audio.data = st_pcm[i].empty() ? nullptr : st_pcm[i].data();
        r.audio.n_outputs = st_pcm[i].size();
        finished.push_back(r);
    }
}

void orpheus_runner::stream_end() {
    if (!st_on) return;
    (void) tts_hip_orpheus_stream_end(lm);
    session_close();
    st_pass = chunk_pass{};
    st_pass_ticket.clear();
    st_closing.clear();
    st_stopped.clear();
}
