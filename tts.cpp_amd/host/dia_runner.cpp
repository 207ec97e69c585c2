#include "dia_runner.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gguf.h"

dia_model_loader::dia_model_loader() : tts_model_loader{"dia"} {}
const dia_model_loader dia_loader{};
void dia_register() {}

// dia_model::prep_constants (model.cpp:168-268) + dac_model::prep_constants / prep_layers (dac_model.cpp:15-55): same keys
// and defaults.  The encoder's hidden size has no key in the reference (model.h:68); it is the embedding's row length.
static dia_hparams read_hparams(const gguf_file & m) {
    dia_hparams hp;
    m.get_u32({"dia.decoder.output_heads"}, hp.n_output_heads);
    m.get_u32({"dia.decoder.layers"}, hp.n_decoder_layers);
    m.get_u32({"dia.encoder.layers"}, hp.n_encoder_layers);
    m.get_u32({"dia.decoder.hidden_size"}, hp.decoder_hidden_size);
    m.get_u32({"dia.decoder.attn_heads"}, hp.decoder_attn_heads);
    m.get_u32({"dia.decoder.query_heads"}, hp.decoder_query_heads);
    m.get_u32({"dia.encoder.attn_heads"}, hp.encoder_attn_heads);
    m.get_u32({"dia.attn_head_size"}, hp.head_size);
    m.get_u32({"dia.eos_token_id"}, hp.eos_token_id);
    m.get_u32({"dia.bos_token_id"}, hp.bos_token_id);
    m.get_u32({"dia.pad_token_id"}, hp.pad_token_id);
    m.get_u32({"dia.encoder.max_context_length"}, hp.max_encoder_context_length);
    m.get_u32({"dia.decoder.output_vocab_size"}, hp.output_vocab_size);
    m.get_u32({"dia.decoder.audio_vocab_size"}, hp.audio_vocab_size);
    m.get_u32({"dia.decoder.max_generation_size"}, hp.max_generation_size);
    m.get_u32({"dia.max_delay"}, hp.max_delay);
    if (const gguf_value * v = m.get("dia.cfg_scale")) hp.cfg_scale = (float) v->f;
    for (const gguf_tensor_view & t : m.tensors)
        if (!strcmp(t.name, "dia.encoder.embedding")) hp.encoder_hidden_size = (uint32_t) t.ne[0];
    if (hp.n_output_heads != hp.delay_pattern.size())
        TTS_ABORT("Dia with %u output heads is unsupported: the delay pattern is fixed at %zu heads (dia/model.h:84)\n", hp.n_output_heads, hp.delay_pattern.size());
    if (hp.decoder_query_heads == 0 || hp.decoder_attn_heads % hp.decoder_query_heads)
        TTS_ABORT("dia.decoder.attn_heads must be a multiple of dia.decoder.query_heads\n");
    m.get_u32({"dac.up_sampling_factor", "up_sampling_factor"}, hp.up_sampling_factor);
    uint32_t n_found = 0, up = 1;
    for (uint32_t i = 0; i < TTS_HIP_MAX_DAC_BLOCKS; i++) {   // same rule as the Parler loader: as many blocks as stride keys
        const std::string sk = "dac_layer_stride_" + std::to_string(i), pk = "dac_layer_padding_" + std::to_string(i);
        const std::string dsk = "dac." + sk, dpk = "dac." + pk;
        if (!m.get_u32({dsk.c_str(), sk.c_str()}, hp.dac_stride[i])) {
            if (i == 0) TTS_ABORT("key %s must be specified in gguf file inorder to initialize the DAC audio decoder.\n", dsk.c_str());
            break;
        }
        if (!m.get_u32({dpk.c_str(), pk.c_str()}, hp.dac_padding[i]))
            TTS_ABORT("key %s must be specified in gguf file inorder to initialize the DAC audio decoder.\n", dpk.c_str());
        up *= hp.dac_stride[i];
        n_found++;
    }
    hp.dac_n_layers = n_found;
    hp.up_sampling_factor = up;
    return hp;
}

std::unique_ptr<tts_generation_runner> dia_model_loader::from_file(gguf_file * meta, int, bool, const generation_configuration &) const {
    const dia_hparams hp = read_hparams(*meta);
    const int device = tts_load_device();
    return std::make_unique<dia_runner>(hp, device);
}

dia_runner::dia_runner(const dia_hparams & hp_, int device) : stream_session{dia_loader}, hp(hp_) {
    tts_hip_dia_desc d{};
    d.struct_size = sizeof(d);
    d.enc_hidden_size = hp.encoder_hidden_size; d.enc_layers = hp.n_encoder_layers; d.enc_attn_heads = hp.encoder_attn_heads;
    d.dec_hidden_size = hp.decoder_hidden_size; d.dec_layers = hp.n_decoder_layers; d.dec_attn_heads = hp.decoder_attn_heads;
    d.dec_kv_heads = hp.decoder_attn_heads / hp.decoder_query_heads;   // model.cpp:463: k/v are projected to attn_heads / query_heads groups
    d.head_dim = hp.head_size; d.n_output_heads = hp.n_output_heads; d.output_vocab_size = hp.output_vocab_size;
    d.max_ctx = hp.max_encoder_context_length; d.max_gen = hp.max_generation_size; d.cfg_scale = hp.cfg_scale;
    const uint32_t asked = tts_load_max_seqs();
    max_seqs = std::min<uint32_t>(asked, 128);   // two guidance rows per utterance, 256 rows per decoder forward (tts_hip_dia_create)
    if (max_seqs != asked) fprintf(stderr, "dia: max_seqs %u exceeds what one decoder forward carries: loading with %u slots\n", asked, max_seqs);
    d.max_utterances = max_seqs;
    // the fp8 cache is the Orpheus decoder's alone: a silent fp32 cache here would be worse than a failed load
    if (getenv("TTS_HIP_KV_F8")) TTS_ABORT("dia: TTS_HIP_KV_F8 is set, and a Dia decoder has no fp8 K/V caches (TTS_HIP_KV_F16 selects its fp16 ones)\n");
    if (getenv("TTS_HIP_KV_F16")) d.kv_type = TTS_HIP_F16;   // the switch the Parler and Orpheus runners read: fp16 self and cross K/V caches (extension, include/tts_hip.h)
    lm = tts_hip_dia_create(device, &d);
    if (!lm) TTS_ABORT("tts_hip_dia_create failed: %s\n", tts_hip_last_error());
    tts_hip_desc a{};
    a.struct_size = sizeof(a);
    a.dac_n_blocks = hp.dac_n_layers;
    for (uint32_t i = 0; i < hp.dac_n_layers; i++) { a.dac_stride[i] = hp.dac_stride[i]; a.dac_padding[i] = hp.dac_padding[i]; }
    a.dac_max_frames = hp.max_generation_size;
    a.max_seqs = 1;
    a.flags = TTS_HIP_FLAG_NO_PARLER;
    dac_halo = tts_hip_dac_halo_frames(&a);
    dac = tts_hip_create(device, &a);
    if (!dac) {
        // the destructor does not run for a constructor that throws (TTS_ABORT under g_tts_throw_on_abort): release the model context
        tts_hip_destroy(lm);
        lm = nullptr;
        TTS_ABORT("tts_hip_create (codec) failed: %s\n", tts_hip_last_error());
    }
    sampling_rate = 44100.0f;
    smp.n_output_heads = hp.n_output_heads;
    smp.vocab_size = hp.output_vocab_size;   // model.h:191
    smp.eos_token_id = hp.eos_token_id;
}

dia_runner::~dia_runner() {
    tts_hip_destroy(lm);
    tts_hip_destroy(dac);
}

uint32_t dia_runner::kv_element_bytes() const {
    float v = 0.0f;
    return tts_hip_debug_read(lm, "di_kv_elem", &v, 1) == 1 ? (uint32_t) v : 0;
}

void dia_runner::assign_weight(const char * name, const gguf_tensor_view & t) {
    // model.cpp:892-898: "audio_encoder." goes to the codec, everything else to the Dia model
    if (!strncmp(name, "audio_encoder.", 14)) hip_check(tts_hip_upload(dac, name, t.type, t.n_dims, t.ne, t.data), name);
    else if (!strncmp(name, "dia.", 4)) hip_check(tts_hip_upload(lm, name, t.type, t.n_dims, t.ne, t.data), name);
    else TTS_ABORT("Unrecognized tensor '%s' when loading Dia from GGUF file.", name);
}

void dia_runner::prepare_post_load() {
    hip_check(tts_hip_finalize(lm, nullptr), "tts_hip_finalize(dia)");
    hip_check(tts_hip_finalize(dac, nullptr), "tts_hip_finalize(dac)");
    logits.resize((size_t) hp.n_output_heads * hp.output_vocab_size);
}

uint32_t dia_tokenize_sentence(const dia_hparams & hp, std::string sentence, std::vector<uint32_t> & tokens) {
    const size_t b = sentence.find_first_not_of(' '), e = sentence.find_last_not_of(' ');   // strip(), util.cpp:273-281
    sentence = b == std::string::npos ? std::string() : sentence.substr(b, e - b + 1);
    const std::string start = sentence.substr(0, 4);
    if (start != "[S1]" && start != "[S2]") sentence = "[S1] " + sentence;
    if (sentence[sentence.size() - 1] != '.') sentence += ".";
    for (const auto & tag : {std::pair<const char *, char>{"[S1]", 1}, {"[S2]", 2}})
        for (size_t p = sentence.find(tag.first); p != std::string::npos; p = sentence.find(tag.first)) sentence.replace(p, 4, std::string(1, tag.second));
    if (sentence.size() > hp.max_encoder_context_length)
        TTS_ABORT("Dia currently only supports a max of %d characters and received an input of %d characters.", (int) hp.max_encoder_context_length, (int) sentence.size());
    tokens.assign(hp.max_encoder_context_length, 0u);
    // bytes as unsigned values: the reference casts a (signed) char, which turns UTF-8 bytes >= 0x80 into row indices far
    // outside the 256-row embedding (:694); the byte value is what the model was trained on
    for (size_t i = 0; i < sentence.size(); i++) tokens[i] = (uint32_t) (unsigned char) sentence[i];
    if (sentence.size() <= 100)
        fprintf(stdout, "Your prompt has fewer than 100 tokens. Please note that Dia's generation with prompts that are fewer than 100 tokens is highly inconsistent.\n");
    return (uint32_t) sentence.size();
}

bool dia_check_stopping(const dia_hparams & hp, std::vector<uint32_t> & audio_tokens, uint32_t current_position, uint32_t max_generation_size, int & delay_steps) {
    if (delay_steps == -1 && (audio_tokens[0] == hp.eos_token_id || current_position >= max_generation_size - hp.max_delay)) delay_steps = (int) hp.max_delay;
    if (delay_steps > 0) {
        const int step_after_eos = (int) hp.max_delay - delay_steps;
        for (size_t i = 0; i < hp.delay_pattern.size(); i++) {
            if (step_after_eos == (int) hp.delay_pattern[i]) audio_tokens[i] = hp.eos_token_id;
            else if (step_after_eos > (int) hp.delay_pattern[i]) audio_tokens[i] = hp.pad_token_id;
        }
        delay_steps -= 1;
    }
    return delay_steps == 0;
}

// adjust_output_tokens (model.cpp:787-808) from a cursor.  After `steps` steps the frames i < steps - max_delay can be judged, and judging
// frame i reads tokens up to step i + max_delay only: what a prefix of the stream yields stays what the whole stream yields.  `judged`
// frames have been judged by earlier calls; the kept ones of [judged, steps - max_delay) are appended to `kept`.  Returns the new cursor.
size_t dia_undelay(const dia_hparams & hp, const uint32_t * toks, size_t steps, size_t judged, std::vector<uint32_t> & kept) {
    const size_t nh = hp.n_output_heads, size = steps * nh;
    const size_t end = steps > hp.max_delay ? steps - hp.max_delay : 0;
    for (size_t i = judged; i < end; i++) {
        bool skip_step = false;
        for (size_t ii = 0; ii < nh; ii++) {
            const size_t next_index = i * nh + hp.delay_pattern[ii] * nh + ii;
            if (next_index >= size || toks[next_index] >= hp.audio_vocab_size) { skip_step = true; break; }
        }
        if (skip_step) continue;
        for (size_t ii = 0; ii < nh; ii++) kept.push_back(toks[i * nh + hp.delay_pattern[ii] * nh + ii]);
    }
    return std::max(end, judged);
}

void dia_adjust_output_tokens(const dia_hparams & hp, const std::vector<uint32_t> & output_tokens, std::vector<uint32_t> & filtered) {
    filtered.clear();
    filtered.reserve(output_tokens.size());
    dia_undelay(hp, output_tokens.data(), output_tokens.size() / hp.n_output_heads, 0, filtered);
}

// ---- chunked audio (common.h; the windows and the chunker: chunk_windows.h) ------------------------------------------------------------------
// Frames are counted after the un-delay dropped those with EOS / PAD in them: that is the sequence the codec sees.  run_utterances calls the
// hook at its look-ins: plan() un-delays what became final and cuts the next windows, emit_rows() decodes them — one codec pass for every
// utterance, on the codec context's stream while the decoder's next steps run — and hands out.
static constexpr uint32_t LOOK_IN = 16;   // decode steps between two look-ins (what tts_hip_dia_generate uses)

dac_chunker dia_runner::make_chunker(uint32_t chunk_frames) {
    return dac_chunker{[this](const uint32_t * toks, size_t steps, size_t judged, bool, std::vector<uint32_t> & kept) { return dia_undelay(hp, toks, steps, judged, kept); },
                       hp.n_output_heads, hp.up_sampling_factor, dac_halo >= 0 ? (uint32_t) dac_halo : hp.max_generation_size, chunk_frames, dac, pcm};
}

// what every form of generate() does before the loop: the sampler's settings (n_calls = 0: a seeded sampler draws the sequence of a call of
// its own) and the step budget
bool dia_runner::valid_max_tokens(const generation_configuration & config) const { return config.max_tokens == 0 || config.max_tokens > (int) hp.max_delay; }

uint32_t dia_runner::resolved_max_gen(const generation_configuration & config) const {
    const uint32_t max_gen = config.max_tokens > (int) hp.max_delay ? (uint32_t) config.max_tokens : hp.max_generation_size;
    return std::min(max_gen, hp.max_generation_size);   // the self-attention cache holds max_generation_size positions (:300-301)
}

bool dia_runner::device_sampler(const generation_configuration & config) const {
    return !config.sample || (config.temperature > 0.0f && config.top_p > 0.0f && config.repetition_penalty > 0.0f);
}

uint32_t dia_runner::begin_call(const generation_configuration & config) {
    if (!valid_max_tokens(config)) TTS_ABORT("TTS_ASSERT(config.max_tokens == 0 || config.max_tokens > model->max_delay) failed\n");
    smp.temperature = config.temperature;
    smp.repetition_penalty = config.repetition_penalty;
    smp.do_sample = config.sample;
    smp.top_k = (uint32_t) config.top_k;
    smp.top_p = config.top_p;
    smp.seed = config.seed;
    smp.n_calls = 0;
    return resolved_max_gen(config);
}

tts_hip_dia_codes dia_runner::loop_codes() const {
    tts_hip_dia_codes codes{};
    codes.bos = hp.bos_token_id; codes.eos = hp.eos_token_id; codes.pad = hp.pad_token_id; codes.max_delay = hp.max_delay;
    for (size_t i = 0; i < hp.delay_pattern.size() && i < 16; i++) codes.delay_pattern[i] = hp.delay_pattern[i];
    return codes;
}

// the U[0,1) values a generate() call of one utterance's own would draw in max_gen sampler calls, call k at out + k * stride.  Every call seeds
// its sampler the same way, so under a fixed seed every utterance draws the same values; with seed == 0 (std::random_device per draw, the
// reference's behaviour) every utterance draws its own.
void dia_runner::draw_call_uniforms(uint64_t seed, uint32_t max_gen, float * out, size_t stride) const {
    sampler s = smp;
    s.seed = seed; s.n_calls = 0;
    for (uint32_t k = 0; k < max_gen; k++) s.draw_uniforms(out + (size_t) k * stride);
}

void dia_runner::encode_single(const char * sentence) {
    const uint32_t sentence_length = dia_tokenize_sentence(hp, sentence, last_prompt_tokens);
    last_output_tokens.clear();
    hip_check(tts_hip_dia_encode(lm, last_prompt_tokens.data(), sentence_length, nullptr), "tts_hip_dia_encode");
}

void dia_runner::encode_batch(const std::vector<std::string> & sentences) {
    const uint32_t n = (uint32_t) sentences.size();
    if (n > max_seqs) TTS_ABORT("generate_batch: %u utterances but the runner was loaded with max_seqs=%u (TTS_HIP_MAX_SEQS)\n", n, max_seqs);
    std::vector<uint32_t> prompt;
    for (uint32_t u = 0; u < n; u++) {
        const uint32_t len = dia_tokenize_sentence(hp, sentences[u], prompt);
        hip_check(tts_hip_dia_encode_slot(lm, u, prompt.data(), len, nullptr), "tts_hip_dia_encode_slot");
    }
    last_batch_tokens.assign(n, {});
}

// generate_from_batch (model.cpp:806-870) for the utterances encoded in slots 0..n-1 -> the still-delayed tokens of each.  The device loop
// (tts_hip_dia_gen_*: check_stopping, the step, the sampler and the delay-pattern feedback replay as one captured graph, the host looks in
// every 16 steps), or under TTS_HOST_LOOP the reference's shape: logits back every step, sampler::sample and check_stopping here.  With a
// hook, the look-ins hand out chunked audio.
// Device loop: every utterance gets the draws a separate generate() call would make (draw_call_uniforms), as the host loop's per-utterance
// samplers and the Parler batch path do.
std::vector<std::vector<uint32_t>> dia_runner::run_utterances(uint32_t n, uint32_t max_gen, const generation_configuration & config, dac_chunker * hook,
                                                              const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) {
    const uint32_t nh = hp.n_output_heads;
    std::vector<std::vector<uint32_t>> toks(n);
    std::vector<bool> finished(n, false);
    bool go = true;   // false: the hook's caller stopped the generation
    if (!getenv("TTS_HOST_LOOP")) {
        const tts_hip_dia_codes codes = loop_codes();
        std::vector<float> u;
        const tts_hip_sampling sp{(uint32_t) config.top_k, config.top_p, config.temperature, config.repetition_penalty};
        if (config.sample) {   // uniforms [call][utterance][head]
            u.resize((size_t) max_gen * n * nh);
            for (uint32_t i = 0; i < n; i++) draw_call_uniforms(config.seed, max_gen, u.data() + (size_t) i * nh, (size_t) n * nh);
        }
        hip_check(tts_hip_dia_gen_begin(lm, n, max_gen, &codes, config.sample ? &sp : nullptr, config.sample ? u.data() : nullptr), "tts_hip_dia_gen_begin");
        std::vector<uint32_t> buf((size_t) n * max_gen * nh), steps(n);
        std::vector<uint8_t>  done(n);
        uint32_t ran = 0;
        hip_check(tts_hip_dia_gen_launch(lm, LOOK_IN), "tts_hip_dia_gen_launch");
        for (;;) {
            if (hook) go = hook->emit_rows(on_chunk);   // the codec windows of the last look-in, while the steps run
            hip_check(tts_hip_dia_gen_wait(lm, buf.data(), steps.data(), done.data(), &ran), "tts_hip_dia_gen_wait");
            bool all = true;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t * b = buf.data() + (size_t) i * max_gen * nh;
                toks[i].insert(toks[i].end(), b + toks[i].size(), b + (size_t) steps[i] * nh);
                finished[i] = done[i] != 0;
                all = all && finished[i];
            }
            if (all || ran >= max_gen + 1 || !go) break;
            hip_check(tts_hip_dia_gen_launch(lm, LOOK_IN), "tts_hip_dia_gen_launch");
            if (hook) hook->plan(toks, finished);
        }
    } else {
        // per utterance: its own sampler state (n separate generate() calls would each reset and seed theirs), tokens, countdown.  A hook's
        // windows are planned and decoded at the same look-in points, without overlap.
        std::vector<sampler> smps(n, smp);
        for (sampler & s : smps) s.reset();
        std::vector<std::vector<uint32_t>> audio(n, std::vector<uint32_t>(nh, hp.bos_token_id));
        std::vector<uint32_t> pos(n, 0), ids((size_t) n * nh);
        std::vector<int>      delay(n, -1);
        std::vector<float>    lg((size_t) n * nh * hp.output_vocab_size);
        for (uint32_t step = 1; go; step++) {
            // check_stopping (:767-785) per utterance before each decode, as generate_from_batch's while condition (:817)
            bool any = false;
            for (uint32_t u = 0; u < n; u++) {
                if (!finished[u] && dia_check_stopping(hp, audio[u], pos[u], max_gen, delay[u])) finished[u] = true;
                any = any || !finished[u];
            }
            if (!any) break;
            for (uint32_t u = 0; u < n; u++) std::copy(audio[u].begin(), audio[u].end(), ids.begin() + (size_t) u * nh);
            // a finished utterance keeps its rows in the step (lock-step shapes stay fixed); its logits are ignored and its position stays
            hip_check(tts_hip_dia_step_batch(lm, n, nullptr, ids.data(), pos.data(), lg.data(), nullptr), "tts_hip_dia_step_batch");
            for (uint32_t u = 0; u < n; u++) {
                if (finished[u]) continue;
                std::vector<uint32_t> & out = toks[u];
                smps[u].sample(lg.data() + (size_t) u * nh * hp.output_vocab_size, out);
                pos[u] += 1;
                const uint32_t * last = out.data() + out.size() - nh;
                for (uint32_t i = 0; i < nh; i++) audio[u][i] = pos[u] > i ? last[i] : hp.bos_token_id;
            }
            if (hook && step % LOOK_IN == 0) {
                hook->plan(toks, finished);
                go = hook->emit_rows(on_chunk);
            }
        }
    }
    if (hook && go) {   // what is left once every utterance is done
        finished.assign(n, true);
        hook->plan(toks, finished);
        (void) hook->emit_rows(on_chunk);
    }
    return toks;
}

void dia_runner::generate(const char * sentence, tts_response & output, const generation_configuration & config) {
    const uint32_t max_gen = begin_call(config);
    output.data = nullptr;
    output.n_outputs = 0;
    encode_single(sentence);
    last_output_tokens = std::move(run_utterances(1, max_gen, config, nullptr)[0]);

    std::vector<uint32_t> filtered;
    dia_adjust_output_tokens(hp, last_output_tokens, filtered);
    const uint32_t frames = (uint32_t) (filtered.size() / hp.n_output_heads);
    if (frames == 0) return;
    pcm.assign((size_t) frames * hp.up_sampling_factor, 0.0f);
    hip_check(tts_hip_dac_decode(dac, filtered.data(), frames, pcm.data()), "tts_hip_dac_decode");
    output.data = pcm.data();
    output.n_outputs = pcm.size();
}

void dia_runner::generate_batch(const std::vector<std::string> & sentences, std::vector<tts_response> & outputs, const generation_configuration & config) {
    const uint32_t n = (uint32_t) sentences.size(), nh = hp.n_output_heads;
    outputs.assign(n, tts_response{});
    if (n == 0) return;
    if (n > max_seqs) TTS_ABORT("generate_batch: %u utterances but the runner was loaded with max_seqs=%u (TTS_HIP_MAX_SEQS)\n", n, max_seqs);
    const uint32_t max_gen = begin_call(config);
    encode_batch(sentences);
    last_batch_tokens = run_utterances(n, max_gen, config, nullptr);

    std::vector<uint32_t> codes, frames(n);
    for (uint32_t u = 0; u < n; u++) {
        std::vector<uint32_t> f;
        dia_adjust_output_tokens(hp, last_batch_tokens[u], f);
        frames[u] = (uint32_t) (f.size() / nh);
        codes.insert(codes.end(), f.begin(), f.end());
    }
    size_t total = 0;
    for (uint32_t f : frames) total += (size_t) f * hp.up_sampling_factor;
    pcm.assign(total, 0.0f);
    if (total) hip_check(tts_hip_dac_decode_batch(dac, codes.data(), frames.data(), n, pcm.data()), "tts_hip_dac_decode_batch");   // one batched codec pass
    size_t off = 0;
    for (uint32_t u = 0; u < n; u++) {
        outputs[u].data = frames[u] ? pcm.data() + off : nullptr;
        outputs[u].n_outputs = (size_t) frames[u] * hp.up_sampling_factor;
        off += outputs[u].n_outputs;
    }
}

void dia_runner::generate_chunked(const char * sentence, const generation_configuration & config, uint32_t chunk_frames,
                                  const std::function<bool(const float *, size_t)> & on_chunk) {
    if (chunk_frames == 0) TTS_ABORT("generate_chunked: chunk_frames must be >= 1\n");
    const uint32_t max_gen = begin_call(config);
    encode_single(sentence);
    const std::function<bool(uint32_t, const float *, size_t)> cb = [&](uint32_t, const float * p, size_t k) { return on_chunk(p, k); };
    dac_chunker hook = make_chunker(chunk_frames);
    last_output_tokens = std::move(run_utterances(1, max_gen, config, &hook, cb)[0]);
}

void dia_runner::generate_batch_chunked(const std::vector<std::string> & sentences, const generation_configuration & config, uint32_t chunk_frames,
                                        const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) {
    if (chunk_frames == 0) TTS_ABORT("generate_batch_chunked: chunk_frames must be >= 1\n");
    const uint32_t n = (uint32_t) sentences.size();
    if (n == 0) return;
    if (n > max_seqs) TTS_ABORT("generate_batch: %u utterances but the runner was loaded with max_seqs=%u (TTS_HIP_MAX_SEQS)\n", n, max_seqs);
    const uint32_t max_gen = begin_call(config);
    encode_batch(sentences);
    dac_chunker hook = make_chunker(chunk_frames);
    last_batch_tokens = run_utterances(n, max_gen, config, &hook, on_chunk);
}

// ---- continuous batching (common.h; tts_hip_dia_stream_* underneath) -------------------------------------------------------------------
// Decoder steps between two look-ins: the distance tts_hip_dia_generate and run_utterances use.  A parked slot waits at most 15 steps for its
// successor, a look-in (one launch, one small copy, one synchronise) is spread over 16 steps of about 2 ms.
void dia_runner::stream_begin(const generation_configuration & config) {
    if (stream_capacity() == 0) TTS_ABORT("stream_begin: the runner was loaded with max_seqs=%u; a session needs >= 2 (TTS_HIP_MAX_SEQS)\n", max_seqs);
    if (getenv("TTS_HOST_LOOP")) TTS_ABORT("stream_begin: TTS_HOST_LOOP asks for the host loop; a session runs on the device\n");
    if (st_on) stream_end();
    st_max_gen = begin_call(config);
    if (!device_sampler(config)) TTS_ABORT("stream_begin: temperature, top_p and repetition_penalty must be > 0 for a sampled session\n");
    // one path: the mixed session, whose slots carry their own sampler; a request with the opening configuration is one among the others
    const tts_hip_dia_codes codes = loop_codes();
    const uint32_t slots = stream_capacity();
    hip_check(tts_hip_dia_stream_begin_mixed(lm, slots, st_max_gen, &codes), "tts_hip_dia_stream_begin_mixed");
    session_open(config, slots);
    st_wait.clear();
    st_hook.reset();
    st_closing.clear();
    st_stopped.clear();
    last_batch_tokens.clear();
}

// chunked audio out of the session (common.h), this runner's part of stream_session's hook: the chunker's rows are the slots.  An unknown halo
// is no refusal: the chunker then cuts one window per utterance once it has ended, and the whole utterance goes out through the hook.
bool dia_runner::session_chunks_ready(uint32_t chunk_frames) {
    if (!st_on) TTS_ABORT("stream_chunks: no session (stream_begin)\n");
    if (st_live != 0 || !st_wait.empty()) TTS_ABORT("stream_chunks: after stream_begin and before the first stream_submit\n");
    const uint32_t slots = stream_capacity();
    st_hook = std::make_unique<dac_chunker>(make_chunker(chunk_frames));
    st_hook->rows.assign(slots, {});
    st_toks.assign(slots, {});
    st_gen.assign(slots, false);
    st_buf.assign((size_t) slots * st_max_gen * hp.n_output_heads, 0u);
    return true;
}

bool dia_runner::stream_accepts(const generation_configuration & config) const {
    return st_on && device_sampler(config) && valid_max_tokens(config) && resolved_max_gen(config) <= st_max_gen;
}

void dia_runner::stream_submit(size_t ticket, const std::string & sentence, const generation_configuration & config) {
    if (!st_on) TTS_ABORT("stream_submit: no session (stream_begin)\n");
    if (stream_free() == 0) TTS_ABORT("stream_submit: no free row (stream_free() == 0)\n");
    if (!device_sampler(config)) TTS_ABORT("stream_submit: temperature, top_p and repetition_penalty must be > 0 (got %g, %g, %g)\n", config.temperature, config.top_p, config.repetition_penalty);
    if (!valid_max_tokens(config)) TTS_ABORT("stream_submit: max_tokens %d must be 0 or exceed max_delay %u\n", config.max_tokens, hp.max_delay);
    if (resolved_max_gen(config) > st_max_gen)
        TTS_ABORT("stream_submit: the request generates up to %u steps, the session was opened for %u (max_tokens)\n", resolved_max_gen(config), st_max_gen);
    waiting w;
    w.ticket = ticket;
    w.cfg = config;
    w.len = dia_tokenize_sentence(hp, sentence, w.prompt);
    st_wait.push_back(std::move(w));
}

// everything queued, in one admission
void dia_runner::admit_waiting() {
    const uint32_t nh = hp.n_output_heads, S = hp.max_encoder_context_length;
    if (st_wait.empty()) return;
    const uint32_t n = (uint32_t) st_wait.size();
    std::vector<uint32_t> slots(n), tokens((size_t) n * S, 0u), lens(n), budgets(n);
    std::vector<tts_hip_sampling>         sps(n);
    std::vector<const tts_hip_sampling *> spp(n, nullptr);
    std::vector<float>    uni;
    bool any_sampled = false;
    for (const waiting & w : st_wait) any_sampled = any_sampled || w.cfg.sample;
    if (any_sampled) uni.assign((size_t) n * st_max_gen * nh, 0.0f);
    for (uint32_t i = 0; i < n; i++) {
        const generation_configuration & cfg = st_wait[i].cfg;
        slots[i] = st_free[st_free.size() - 1 - i];
        lens[i] = st_wait[i].len;
        budgets[i] = resolved_max_gen(cfg);   // the utterance runs as under a generate() call of its own
        std::copy(st_wait[i].prompt.begin(), st_wait[i].prompt.begin() + std::min<size_t>(S, st_wait[i].prompt.size()), tokens.begin() + (size_t) i * S);
        if (!cfg.sample) continue;
        sps[i] = tts_hip_sampling{(uint32_t) cfg.top_k, cfg.top_p, cfg.temperature, cfg.repetition_penalty};
        spp[i] = &sps[i];
        draw_call_uniforms(cfg.seed, budgets[i], uni.data() + (size_t) i * st_max_gen * nh, nh);   // its own seed, the calls its budget allows
    }
    hip_check(tts_hip_dia_stream_admit_mixed(lm, n, slots.data(), tokens.data(), lens.data(), budgets.data(), spp.data(), any_sampled ? uni.data() : nullptr),
              "tts_hip_dia_stream_admit_mixed");
    for (uint32_t i = 0; i < n; i++) {
        st_ticket[slots[i]] = st_wait[i].ticket;
        st_free.pop_back();
        if (st_hook) {   // a new occupant: its rows and its chunker row start at zero
            st_toks[slots[i]].clear();
            st_hook->rows[slots[i]] = {};
            st_gen[slots[i]] = true;
        }
    }
    st_live += n;
    st_wait.clear();
}

// the windows the last plan cut, through the codec and out; then the utterances that ended before that plan have had their last chunk
void dia_runner::hand_out(std::vector<stream_result> & finished) {
    st_hook->emit_session(st_win_ticket, st_on_chunk, st_stopped);
    st_win_ticket.clear();
    for (size_t ticket : st_closing) report_no_audio(finished, ticket);
    st_closing.clear();
}

// stream_step with a hook: the codec pass of the windows cut at the last look-in runs on the codec context while this interval's steps run.
// The rows are un-delayed and cut into windows right after the wait that brought them (host work on at most 16 rows per slot) rather than
// under the next launch: a slot that finished is handed to the next occupant by the admission that precedes that launch, so its tail has to
// be out of the slot's row by then.
void dia_runner::stream_step_chunked(std::vector<stream_result> & finished) {
    const uint32_t nh = hp.n_output_heads, slots = stream_capacity();
    admit_waiting();
    hip_check(tts_hip_dia_stream_launch(lm, LOOK_IN), "tts_hip_dia_stream_launch");
    hand_out(finished);
    std::vector<uint32_t> fs(slots), fn(slots), steps(slots);
    uint32_t nf = 0;
    hip_check(tts_hip_dia_stream_wait(lm, st_buf.data(), steps.data(), nullptr, &nf, fs.data(), fn.data()), "tts_hip_dia_stream_wait");
    std::vector<bool> ended(slots, false);
    for (uint32_t i = 0; i < nf; i++) ended[fs[i]] = true;
    std::vector<uint32_t> drop;
    for (uint32_t s = 0; s < slots; s++) {
        if (!st_gen[s]) continue;
        const uint32_t * b = st_buf.data() + (size_t) s * st_max_gen * nh;
        st_toks[s].insert(st_toks[s].end(), b + st_toks[s].size(), b + (size_t) steps[s] * nh);
        const bool stopped = std::find(st_stopped.begin(), st_stopped.end(), st_ticket[s]) != st_stopped.end();
        if (!ended[s] && !stopped) continue;
        // the occupant leaves: its rows are on the host, the slot is free for the next admission
        remember_tokens(st_ticket[s], st_toks[s]);
        st_gen[s] = false;
        st_free.push_back(s);
        st_live--;
        if (stopped) {   // on_chunk ended it: reported with what it got, nothing more is decoded for it
            if (!ended[s]) drop.push_back(s);
            st_toks[s].clear();
            st_hook->rows[s] = {};
            report_no_audio(finished, st_ticket[s]);
            ended[s] = false;
        } else {
            st_closing.push_back(st_ticket[s]);
        }
    }
    st_stopped.clear();
    if (!drop.empty()) hip_check(tts_hip_dia_stream_drop(lm, (uint32_t) drop.size(), drop.data()), "tts_hip_dia_stream_drop");
    st_hook->plan(st_toks, ended);
    for (uint32_t s : st_hook->row_of) st_win_ticket.push_back(st_ticket[s]);
    for (uint32_t s = 0; s < slots; s++)
        if (ended[s]) { st_toks[s].clear(); st_hook->rows[s] = {}; }   // its tail is in the windows
    if (st_live == 0) {   // nothing to run the codec under: the tails now
        hand_out(finished);
        st_stopped.clear();   // only utterances that had ended could be stopped here
    }
}

void dia_runner::stream_step(std::vector<stream_result> & finished) {
    if (!st_on) TTS_ABORT("stream_step: no session (stream_begin)\n");
    finished.clear();
    if (st_hook) return stream_step_chunked(finished);
    const uint32_t nh = hp.n_output_heads;
    admit_waiting();
    std::vector<uint32_t> fs(stream_capacity()), fn(stream_capacity());
    uint32_t nf = 0;
    hip_check(tts_hip_dia_stream_run(lm, LOOK_IN, &nf, fs.data(), fn.data()), "tts_hip_dia_stream_run");
    if (nf == 0) return;
    std::vector<uint32_t> codes, frames(nf);
    for (uint32_t i = 0; i < nf; i++) {   // in slot order
        std::vector<uint32_t> ids((size_t) fn[i] * nh), f;
        hip_check(tts_hip_dia_stream_collect(lm, fs[i], fn[i], ids.data()), "tts_hip_dia_stream_collect");
        st_free.push_back(fs[i]);
        st_live--;
        dia_adjust_output_tokens(hp, ids, f);
        frames[i] = (uint32_t) (f.size() / nh);
        codes.insert(codes.end(), f.begin(), f.end());
        remember_tokens(st_ticket[fs[i]], ids);
    }
    size_t total = 0;
    for (uint32_t f : frames) total += (size_t) f * hp.up_sampling_factor;
    pcm.assign(total, 0.0f);
    if (total) hip_check(tts_hip_dac_decode_batch(dac, codes.data(), frames.data(), nf, pcm.data()), "tts_hip_dac_decode_batch");   // one batched codec pass
    size_t off = 0;
    for (uint32_t i = 0; i < nf; i++) {
        stream_result r;
        r.ticket = st_ticket[fs[i]];
        r.audio.data = frames[i] ? pcm.data() + off : nullptr;
        r.audio.n_outputs = (size_t) frames[i] * hp.up_sampling_factor;
        off += r.audio.n_outputs;
        finished.push_back(r);
    }
}

void dia_runner::stream_end() {
    if (!st_on) return;
    (void) tts_hip_dia_stream_end(lm);
    session_close();
    st_wait.clear();
    st_hook.reset();
    st_closing.clear();
    st_stopped.clear();
    st_win_ticket.clear();
}
