#include "parler_runner.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gguf.h"

parler_model_loader::parler_model_loader() : tts_model_loader{"parler-tts"} {}
const parler_model_loader parler_loader{};
void parler_register() {}

// parler_tts_model::prep_constants (model.cpp:51-108) + dac_model::prep_constants/prep_layers
// (dac_model.cpp:15-55): same keys, same aliases, same defaults.
static parler_hparams read_hparams(const gguf_file & m) {
    parler_hparams hp;
    if (!m.get_u32({"parler-tts.decoder.encode_length", "encode_length"}, hp.n_encode_length))
        TTS_ABORT("key 'parler-tts.decoder.encode_length' must be specified in gguf file.\n");
    m.get_u32({"parler-tts.decoder.hidden_size", "hidden_size"}, hp.hidden_size);
    m.get_u32({"parler-tts.decoder.output_heads", "output_heads"}, hp.n_output_heads);
    m.get_u32({"parler-tts.decoder.context_length", "ctx_length"}, hp.max_ctx_length);
    m.get_u32({"parler-tts.decoder.attention.head_count", "attn_heads"}, hp.n_attn_heads);
    m.get_u32({"parler-tts.decoder.out_vocab_size", "out_vocab_size"}, hp.output_vocab_size);
    m.get_u32({"parler-tts.decoder.audio_vocab_size", "audio_vocab_size"}, hp.audio_vocab_size);
    m.get_u32({"parler-tts.decoder.max_generation", "max_generation"}, hp.max_generation_size);
    m.get_u32({"parler-tts.decoder.num_hidden_layers", "num_hidden_layers"}, hp.n_layers);
    m.get_u32({"audio.bos_token_id", "bos_token_id"}, hp.bos_token_id);
    m.get_u32({"audio.eos_token_id", "eos_token_id"}, hp.eos_token_id);
    // the converter writes dac.up_scaling_factor but the reference reads dac.up_sampling_factor, so the
    // default 512 always applies there (dac_model.cpp:21-24); kept, and cross-checked against the strides below
    m.get_u32({"dac.up_sampling_factor", "up_sampling_factor"}, hp.up_sampling_factor);
    // The reference fixes the codec at 4 decoder blocks (dac_model.h:33) and aborts when one of their
    // stride/padding keys is missing (dac_model.cpp:37-47).  Extension: the block count is taken from how many
    // consecutive dac_layer_stride_i keys the file holds (>= 1), so non-standard codecs load too.
    uint32_t up = 1, n_found = 0;
    for (uint32_t i = 0; i < TTS_HIP_MAX_DAC_BLOCKS; i++) {
        const std::string sk = "dac_layer_stride_" + std::to_string(i), pk = "dac_layer_padding_" + std::to_string(i);
        const std::string dsk = "dac." + sk, dpk = "dac." + pk;
        if (!m.get_u32({dsk.c_str(), sk.c_str()}, hp.dac_stride[i])) {
            if (i == 0) TTS_ABORT("key %s must be specified in gguf file inorder to initialize the DAC audio decoder.\n", sk.c_str());
            break;
        }
        if (!m.get_u32({dpk.c_str(), pk.c_str()}, hp.dac_padding[i]))
            TTS_ABORT("key %s must be specified in gguf file inorder to initialize the DAC audio decoder.\n", pk.c_str());
        up *= hp.dac_stride[i];
        n_found++;
    }
    hp.dac_n_layers = n_found;
    if (up != hp.up_sampling_factor) hp.up_sampling_factor = up;  // non-standard codec: trust the layer strides
    // a file whose metadata cannot describe a model is refused here, not by a division further down
    if (hp.n_output_heads == 0 || hp.output_vocab_size == 0 || hp.hidden_size == 0 || hp.n_attn_heads == 0 || hp.hidden_size % hp.n_attn_heads ||
        hp.n_layers == 0 || hp.max_generation_size < 2 || hp.up_sampling_factor == 0)
        TTS_ABORT("parler-tts metadata out of range: %u output heads, vocabulary %u, hidden %u over %u heads, %u layers, max_generation %u\n", hp.n_output_heads,
                  hp.output_vocab_size, hp.hidden_size, hp.n_attn_heads, hp.n_layers, hp.max_generation_size);
    return hp;
}

std::unique_ptr<tts_generation_runner> parler_model_loader::from_file(gguf_file * meta, int, bool cpu_only,
                                                                      const generation_configuration & config) const {
    const parler_hparams hp = read_hparams(*meta);
    const int device = tts_load_device();
    (void) cpu_only;
    return std::make_unique<parler_runner>(hp, unigram_tokenizer_from_gguf(*meta), device, config.use_cross_attn);
}

parler_runner::parler_runner(const parler_hparams & hp_, unigram_tokenizer * tok, int device, bool cross)
    : stream_session{parler_loader}, hp(hp_), tokenizer(tok), use_cross_attn(cross), device_id(device) {
    tts_hip_desc d{};
    d.struct_size = sizeof(d);
    d.hidden_size = hp.hidden_size; d.n_layers = hp.n_layers; d.n_attn_heads = hp.n_attn_heads;
    d.n_output_heads = hp.n_output_heads; d.output_vocab_size = hp.output_vocab_size; d.max_ctx_length = hp.max_ctx_length;
    d.n_encode_length = hp.n_encode_length; d.use_cross_attn = cross ? 1 : 0;
    d.dac_n_blocks = hp.dac_n_layers;
    for (uint32_t i = 0; i < hp.dac_n_layers; i++) { d.dac_stride[i] = hp.dac_stride[i]; d.dac_padding[i] = hp.dac_padding[i]; }
    d.dac_max_frames = hp.max_generation_size;
    max_seqs = tts_load_max_seqs();
    st_codec_hold = (uint32_t) std::max(1, tts_thread_load_options().stream_codec_hold);
    d.max_seqs = max_seqs;
    {
        const tts_load_options & lo = tts_thread_load_options();
        if (lo.share_with) {
            share_ctx = (tts_hip_ctx *) lo.share_with->device_context();
            if (!share_ctx) TTS_ABORT("load: share_with names a runner that cannot share its weights\n");
        }
        declare_only = lo.declare_only || share_ctx != nullptr;
    }
    // the fp8 cache is the Orpheus decoder's alone: a silent fp32 cache here would be worse than a failed load
    if (getenv("TTS_HIP_KV_F8")) TTS_ABORT("parler: TTS_HIP_KV_F8 is set, and a Parler decoder has no fp8 K/V cache (TTS_HIP_KV_F16 selects its fp16 one)\n");
    d.kv_type = getenv("TTS_HIP_KV_F16") ? TTS_HIP_F16 : TTS_HIP_F32;
    d.gelu_mode = 1;
    // one utterance: the reference layout (max_ctx_length positions, model.cpp:368-369); lock-step batches keep only
    // the positions generation can reach (check_stopping stops at max_generation, model.cpp:720-722)
    d.kv_positions = max_seqs > 1 ? hp.max_generation_size : 0;
    dac_halo = tts_hip_dac_halo_frames(&d);
    ctx = tts_hip_create(device, &d);
    if (!ctx) TTS_ABORT("tts_hip_create failed: %s\n", tts_hip_last_error());
    smp.n_output_heads = hp.n_output_heads;
    smp.vocab_size = hp.output_vocab_size;
    smp.eos_token_id = hp.eos_token_id;
    sampling_rate = 44100.0f;
}

parler_runner::~parler_runner() { tts_hip_destroy(ctx); }

void parler_runner::assign_weight(const char * name, const gguf_tensor_view & t) {
    // model.cpp:500-508 routes "audio_encoder." / "decoder." prefixes; the shim does the same by name
    // declare-only: the shape is all the device needs to lay its arena out; the bytes come from another context
    hip_check(tts_hip_upload(ctx, name, t.type, t.n_dims, t.ne, declare_only ? nullptr : t.data), name);
}

void parler_runner::prepare_post_load() {
    // prep_cross_key_values + kv cache init + graph reserve (model.cpp:704-713) all live in finalize
    if (share_ctx) {
        // same model, same device: use the loaded runner's arena (weights + precomputed cross K/V); own KV cache and stream
        if (tts_hip_arena_bytes(ctx) != tts_hip_arena_bytes(share_ctx)) TTS_ABORT("load: the runner to share weights with holds a different model\n");
        hip_check(tts_hip_finalize(ctx, tts_hip_arena_ptr(share_ctx)), "tts_hip_finalize(shared arena)");
        hip_check(tts_hip_arena_filled(ctx), "tts_hip_arena_filled");
    } else
    hip_check(tts_hip_finalize(ctx, nullptr), "tts_hip_finalize");
    pcm.reserve((size_t) hp.max_generation_size * hp.up_sampling_factor);
}

// model.cpp:510-518: text_encoder_from_file (t5/model.cpp:365-402) with THIS runner's tokenizer, t5_runner::generate
// (:359-364: tokenize + EOS, run), then prep_cross_key_values with the response.  The encoder lives in its own device
// context for the duration of the call, as the reference builds and deletes a t5_runner per call.
std::vector<float> parler_runner::encode_description(const char * file_path, const char * prompt, const char * what, std::vector<uint32_t> & tokens) {
    std::string err;
    std::shared_ptr<gguf_file> meta = gguf_file::open(file_path, err);
    if (!meta) TTS_ABORT("text_encoder_from_file failed for file %s: %s\n", file_path, err.c_str());
    // t5_encoder::prep_constants (t5/model.cpp:123-164); defaults t5/model.h:43-52
    tts_hip_t5_desc td{};
    td.struct_size = sizeof(td);
    td.n_layers = 24; td.n_attn_heads = 32; td.hidden_size = 2048; td.max_ctx_length = 512; td.n_buckets = 32; td.output_size = 1536;
    uint32_t eos = 1, vocab = 0;
    meta->get_u32({"t5encoder.block_count"}, td.n_layers);
    meta->get_u32({"t5encoder.embedding_length"}, td.hidden_size);
    meta->get_u32({"t5encoder.attention.head_count"}, td.n_attn_heads);
    meta->get_u32({"t5encoder.context_length"}, td.max_ctx_length);
    meta->get_u32({"tokenizer.ggml.eos_token_id"}, eos);
    if (!meta->get_u32({"t5encoder.vocab_size"}, vocab)) TTS_ABORT("key 't5encoder.vocab_size' must be specified in gguf file.\n");
    meta->get_u32({"t5encoder.output_size"}, td.output_size);
    td.gelu_mode = 1;
    if (td.output_size != hp.hidden_size)
        TTS_ABORT("%s: the encoder's output size %u differs from the decoder's hidden size %u\n", what, td.output_size, hp.hidden_size);

    tts_hip_ctx * t5 = tts_hip_t5_create(device_id, &td);
    if (!t5) TTS_ABORT("tts_hip_t5_create failed: %s\n", tts_hip_last_error());
    struct guard { tts_hip_ctx * c; ~guard() { tts_hip_destroy(c); } } g{t5};
    for (const gguf_tensor_view & t : meta->tensors) {
        if (!t.data || !*t.name) continue;
        hip_check(tts_hip_upload(t5, t.name, t.type, t.n_dims, t.ne, t.data), t.name);  // assign_to_t5_encoder keeps "t5encoder.*"
    }
    hip_check(tts_hip_finalize(t5, nullptr), "tts_hip_finalize(t5)");

    tokens.clear();
    tokenizer->tokenize(prompt, tokens);
    tokens.push_back(eos);
    if (tokens.size() > td.max_ctx_length || tokens.size() > 512)   // max_encode_length, model.h:69
        TTS_ABORT("%s: %zu prompt tokens exceed the encoder context %u\n", what, tokens.size(), td.max_ctx_length);
    std::vector<float> enc(tokens.size() * (size_t) td.output_size);
    hip_check(tts_hip_t5_encode(t5, tokens.data(), (uint32_t) tokens.size(), enc.data()), "tts_hip_t5_encode");
    return enc;
}

void parler_runner::update_conditional_prompt(const char * file_path, const char * prompt) {
    std::vector<uint32_t> tokens;
    const std::vector<float> enc = encode_description(file_path, prompt, "update_conditional_prompt", tokens);
    hip_check(tts_hip_parler_set_text_encoding(ctx, enc.data(), (uint32_t) tokens.size()), "tts_hip_parler_set_text_encoding");
    last_conditional_tokens = tokens;
}

void parler_runner::add_voice(const char * name, const char * text_encoder_path, const char * description) {
    if (!name || !*name) TTS_ABORT("add_voice: a voice needs a name (the empty name is the runner's own description)\n");
    if (!use_cross_attn) TTS_ABORT("add_voice: the model was loaded without cross attention\n");
    size_t idx = 0;
    while (idx < voice_names.size() && voice_names[idx] != name) idx++;
    if (idx == VOICE_BANK) TTS_ABORT("add_voice: the bank holds %u voices\n", VOICE_BANK);
    if (st_on && idx < voice_names.size()) {
        for (const pending & p : st_wait)
            if (p.voice == idx + 1) TTS_ABORT("add_voice: voice '%s' is in use by a request waiting for its admission\n", name);
        for (uint32_t s = 0; s < (uint32_t) st_voice.size(); s++) {
            bool free_slot = false;
            for (uint32_t f : st_free) free_slot = free_slot || f == s;
            if (!free_slot && st_voice[s] == idx + 1) TTS_ABORT("add_voice: voice '%s' is in use by a session slot\n", name);
        }
    }
    std::vector<uint32_t> tokens;
    const std::vector<float> enc = encode_description(text_encoder_path, description, "add_voice", tokens);
    if (tokens.size() > VOICE_TOKENS)
        TTS_ABORT("add_voice: the description of '%s' has %zu tokens; a voice holds at most %u\n", name, tokens.size(), VOICE_TOKENS);
    if (!voice_bank_made) {
        hip_check(tts_hip_parler_voice_bank(ctx, VOICE_BANK), "tts_hip_parler_voice_bank");
        voice_bank_made = true;
        voice_names.reserve(VOICE_BANK);   // list_voices hands out views
    }
    hip_check(tts_hip_parler_voice_set(ctx, (uint32_t) idx + 1, enc.data(), (uint32_t) tokens.size()), "tts_hip_parler_voice_set");
    if (idx == voice_names.size()) voice_names.emplace_back(name);
    last_conditional_tokens = tokens;
}

std::vector<std::string_view> parler_runner::list_voices() {
    return std::vector<std::string_view>(voice_names.begin(), voice_names.end());
}

bool parler_runner::voice_known(const std::string & voice) const {
    if (voice.empty()) return true;
    for (const std::string & v : voice_names) if (v == voice) return true;
    return false;
}

uint32_t parler_runner::voice_index(const std::string & voice, const char * what) const {
    if (voice.empty()) return 0;
    std::string known;
    for (size_t i = 0; i < voice_names.size(); i++) {
        if (voice_names[i] == voice) return (uint32_t) i + 1;
        known += (i ? ", " : "") + voice_names[i];
    }
    TTS_ABORT("%s: unknown voice '%s' (known: %s)\n", what, voice.c_str(), known.empty() ? "none; add_voice enters one" : known.c_str());
}

// a runner without added voices never calls into the bank: every slot is at voice 0 as it always was
void parler_runner::set_slot_voices(const std::vector<uint32_t> & slots, const std::vector<uint32_t> & voices, const char * what) {
    if (voice_names.empty() || slots.empty()) return;
    hip_check(tts_hip_parler_seq_voices(ctx, (uint32_t) slots.size(), slots.data(), voices.data()), what);
}

// model.cpp:734-760, including the `next_index > size` bound (an index == size would read one past the
// end in the reference; such a frame is dropped here, the only defined outcome).
size_t parler_undelay(const uint32_t * toks, size_t steps, uint32_t nh, uint32_t audio_vocab, size_t next, bool finished, std::vector<uint32_t> & out) {
    const size_t size = steps * nh, end = finished ? steps : (steps >= nh ? steps - nh + 1 : 0);
    for (size_t i = next; i < end; i++) {
        bool remove = false;
        for (size_t ii = 0; ii < nh; ii++) {
            const size_t idx = i * nh + ii * nh + ii;
            if (idx >= size || toks[idx] >= audio_vocab) { remove = true; break; }
        }
        if (remove) continue;
        for (size_t ii = 0; ii < nh; ii++) out.push_back(toks[i * nh + ii * nh + ii]);
    }
    return std::max(end, next);
}

void parler_runner::adjust_output_tokens(const std::vector<uint32_t> & toks, std::vector<uint32_t> & filtered) const {
    filtered.reserve(toks.size());
    parler_undelay(toks.data(), toks.size() / hp.n_output_heads, hp.n_output_heads, hp.audio_vocab_size, 0, true, filtered);
}

// the sampler's settings as a generate() call starts it (n_calls = 0: a seeded sampler draws the sequence of a call of its own)
static void sampler_setup(sampler & s, const generation_configuration & config) {
    s.temperature = config.temperature;
    s.repetition_penalty = config.repetition_penalty;
    s.do_sample = config.sample;
    s.top_k = (uint32_t) config.top_k;
    s.top_p = config.top_p;
    s.seed = config.seed;
    s.n_calls = 0;
}

// the U[0,1) draws sample() would make in `steps` calls (sampler.cpp:47-50) on one utterance's own sampler, seeded as a generate() call of
// its own, drawn ahead for a device loop: step s at u + s * stride (stride = rows * heads in the [step][row][head] layout)
static void draw_row_uniforms(sampler si, uint64_t seed, uint32_t steps, size_t stride, float * u) {
    si.seed = seed;
    si.n_calls = 0;
    for (uint32_t s = 0; s < steps; s++) si.draw_uniforms(u + s * stride);
}

// batch_from_sentence (model.cpp:473-498): tokenise + EOS.  false: the prompt leaves no room for generation (the response is empty).
bool parler_runner::tokenize_prompt(const std::string & sentence, std::vector<uint32_t> & prompt) const {
    prompt.clear();
    tokenizer->tokenize(sentence, prompt);
    prompt.push_back(tokenizer->eos_token);
    return prompt.size() < hp.max_generation_size && prompt.size() < hp.max_ctx_length;
}

// generate() up to the prefill: the sampler's settings, the prompt into cache slot 0.  false: no room for generation.
bool parler_runner::prepare_single(const char * sentence, const generation_configuration & config, std::vector<uint32_t> & prompt) {
    sampler_setup(smp, config);
    if (config.use_cross_attn != use_cross_attn)
        TTS_ABORT("generate(): use_cross_attn differs from the value the model was loaded with (the reference only "
                  "loads the encoder_attn tensors when it is set at load time, model.cpp:202-237)\n");
    const uint32_t voice = voice_index(config.voice, "generate()");
    const bool room = tokenize_prompt(sentence, prompt);
    last_prompt_tokens = prompt;
    last_output_tokens.clear();
    smp.reset();
    hip_check(tts_hip_parler_reset(ctx), "tts_hip_parler_reset");
    if (!room) {
        fprintf(stderr, "prompt of %zu tokens leaves no room for generation\n", prompt.size());
        return false;
    }
    set_slot_voices({0}, {voice}, "tts_hip_parler_seq_voices");
    hip_check(tts_hip_parler_prefill(ctx, 0, prompt.data(), (uint32_t) prompt.size(), 0), "tts_hip_parler_prefill");
    return true;
}

// generate_batch() up to the prefill: the utterances that have room for generation as rows (row_of: the utterance of a row, start: its prompt
// length), their prompts prefilled as one batch.  false: no row.
bool parler_runner::prepare_batch(const std::vector<std::string> & sentences, const generation_configuration & config,
                                  std::vector<uint32_t> & start, std::vector<uint32_t> & row_of) {
    const uint32_t n_all = (uint32_t) sentences.size();
    start.clear(); row_of.clear();
    last_batch_tokens.assign(n_all, {});
    if (n_all == 0) return false;
    if (n_all > max_seqs) TTS_ABORT("generate_batch: %u utterances but the runner was loaded with max_seqs=%u (TTS_HIP_MAX_SEQS)\n", n_all, max_seqs);
    if (config.use_cross_attn != use_cross_attn) TTS_ABORT("generate_batch: use_cross_attn differs from load time\n");
    const uint32_t voice = voice_index(config.voice, "generate_batch");
    // an utterance whose prompt leaves no room gets an empty response, exactly as generate() does
    std::vector<uint32_t> ids, p;
    for (uint32_t i = 0; i < n_all; i++) {
        if (!tokenize_prompt(sentences[i], p)) {
            fprintf(stderr, "prompt %u of %zu tokens leaves no room for generation\n", i, p.size());
            continue;
        }
        row_of.push_back(i);
        start.push_back((uint32_t) p.size());
        ids.insert(ids.end(), p.begin(), p.end());
    }
    const uint32_t n = (uint32_t) row_of.size();
    if (n == 0) return false;
    hip_check(tts_hip_parler_reset(ctx), "tts_hip_parler_reset");
    {
        std::vector<uint32_t> rows(n);
        for (uint32_t i = 0; i < n; i++) rows[i] = i;
        set_slot_voices(rows, std::vector<uint32_t>(n, voice), "tts_hip_parler_seq_voices");
    }
    hip_check(tts_hip_parler_prefill_batch(ctx, n, nullptr, ids.data(), start.data(), nullptr), "tts_hip_parler_prefill_batch");
    return true;
}

// ---- chunked audio (common.h; the windows and the chunker: chunk_windows.h) ------------------------------------------------------------------
// run_rows calls the hook at its look-ins: plan() un-delays the frames that became final and cuts the next windows, emit_rows() decodes them
// (one codec pass for every utterance, on the codec's stream while the device loop's next steps run) and hands the chunks out.
static constexpr uint32_t LOOK_IN = 32;   // decode steps between two look-ins: the device compacts its rows at multiples of 32 steps

dac_chunker parler_runner::make_chunker(uint32_t chunk_frames) {
    const uint32_t nh = hp.n_output_heads, av = hp.audio_vocab_size;
    return dac_chunker{[nh, av](const uint32_t * toks, size_t steps, size_t judged, bool finished, std::vector<uint32_t> & kept) {
                           return parler_undelay(toks, steps, nh, av, judged, finished, kept);
                       },
                       nh, hp.up_sampling_factor, dac_halo >= 0 ? (uint32_t) dac_halo : hp.max_generation_size, chunk_frames, ctx, pcm};
}

// generate_from_batch (model.cpp:762-792) over n prefilled rows (row i starts at position start[i]) -> the still-delayed tokens of each row.
// Every row gets the steps generate() would give it alone (max_generation - its own prompt) and its own sampler, seeded as a generate() call
// of its own; the loop runs as long as the shortest prompt needs.  With a hook, the look-ins every 32 steps hand out chunked audio.
std::vector<std::vector<uint32_t>> parler_runner::run_rows(const std::vector<uint32_t> & start, const generation_configuration & config, dac_chunker * hook,
                                                           const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) {
    const uint32_t n = (uint32_t) start.size(), nh = hp.n_output_heads, V = hp.output_vocab_size;
    const uint32_t max_steps = hp.max_generation_size - *std::min_element(start.begin(), start.end());
    std::vector<std::vector<uint32_t>> toks(n);
    std::vector<bool> finished(n, false);
    bool go = true;   // false: the hook's caller stopped the generation

    // the sampler runs on the device (unless a head has more than 2048 logits).  Greedy never sees the repetition
    // penalty: sampler::max only reads last_token_ids, which stay -1 after reset() (sampler.cpp:71-80,185-204)
    if (!getenv("TTS_HOST_LOOP") && (!config.sample || V <= 2048)) {
        // sampler::max / sampler::sample, the delay-pattern feed and the EOS flags run on the device; the host looks in every 32 steps to
        // learn whether check_stopping() has fired, and fetches the tokens once at the end (with a hook: the new steps' at every look-in)
        std::vector<float> u;
        const tts_hip_sampling sp{(uint32_t) config.top_k, config.top_p, config.temperature, config.repetition_penalty};
        if (config.sample) {   // uniforms [step][row][head]
            u.resize((size_t) max_steps * n * nh);
            for (uint32_t i = 0; i < n; i++) draw_row_uniforms(smp, config.seed, max_steps, (size_t) n * nh, u.data() + (size_t) i * nh);
        }
        hip_check(tts_hip_parler_gen_begin(ctx, n, start.data(), max_steps, hp.bos_token_id, hp.eos_token_id, config.sample ? &sp : nullptr,
                                           config.sample ? u.data() : nullptr), "tts_hip_parler_gen_begin");
        std::vector<uint32_t> buf((size_t) max_steps * n * nh), done(n);
        uint32_t ran = 0;
        // check_stopping per row: EOS on every head (done), or position == max_generation
        auto cap = [&](uint32_t i) { return std::min(done[i] ? done[i] : max_steps, hp.max_generation_size - start[i]); };
        auto collect = [&]() {   // the steps of buf [step][row][head] that the rows do not hold yet
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t s = (uint32_t) (toks[i].size() / nh), e = std::min(ran, cap(i)); s < e; s++)
                    toks[i].insert(toks[i].end(), buf.begin() + ((size_t) s * n + i) * nh, buf.begin() + ((size_t) s * n + i + 1) * nh);
        };
        hip_check(tts_hip_parler_gen_launch(ctx, LOOK_IN), "tts_hip_parler_gen_launch");
        for (;;) {
            if (hook) go = hook->emit_rows(on_chunk);   // the codec windows of the last look-in, while the steps run
            hip_check(tts_hip_parler_gen_wait(ctx, hook ? buf.data() : nullptr, done.data(), &ran), "tts_hip_parler_gen_wait");
            bool all = true;
            for (uint32_t i = 0; i < n; i++) {
                finished[i] = ran >= cap(i);
                all = all && finished[i];
            }
            if (hook) collect();
            if (all || !go) break;
            hip_check(tts_hip_parler_gen_launch(ctx, LOOK_IN), "tts_hip_parler_gen_launch");
            if (hook) hook->plan(toks, finished);
        }
        if (!hook) {   // one copy of all the tokens
            hip_check(tts_hip_parler_gen_wait(ctx, buf.data(), done.data(), &ran), "tts_hip_parler_gen_wait");
            collect();
        }
    } else {
        // host sampling, one sampler state per row; finished rows keep stepping on EOS inputs (their tokens are no longer recorded) until
        // all are done.  A hook's windows are planned and decoded at the same look-in points, without overlap.
        std::vector<sampler> smps(n, smp);
        for (sampler & s : smps) {
            sampler_setup(s, config);
            s.reset();
        }
        std::vector<uint32_t> in_ids((size_t) n * nh, hp.bos_token_id), pos(start);
        std::vector<std::vector<bool>> eos_seen(n, std::vector<bool>(nh, false));
        std::vector<float> lg((size_t) n * nh * V);
        for (uint32_t step = 1; step <= max_steps && go; step++) {
            bool all_done = true;
            for (uint32_t i = 0; i < n; i++) {
                // check_stopping (model.cpp:715-732)
                if (finished[i]) continue;
                auto & t = toks[i];
                if (!t.empty()) {
                    if (start[i] + t.size() / nh >= hp.max_generation_size) { finished[i] = true; continue; }
                    bool all = true;
                    for (uint32_t h = 0; h < nh; h++) {
                        eos_seen[i][h] = eos_seen[i][h] || t[t.size() - nh + h] == hp.eos_token_id;
                        all = all && eos_seen[i][h];
                    }
                    if (all) { finished[i] = true; continue; }
                }
                all_done = false;
            }
            if (all_done) break;
            hip_check(tts_hip_parler_step(ctx, n, in_ids.data(), pos.data(), nullptr, lg.data()), "tts_hip_parler_step");
            for (uint32_t i = 0; i < n; i++) {
                if (pos[i] + 1 < hp.max_generation_size) pos[i] += 1;  // finished rows idle on their last position
                if (finished[i]) continue;
                auto & t = toks[i];
                smps[i].sample(lg.data() + (size_t) i * nh * V, t);
                const uint32_t * last = t.data() + t.size() - nh;
                for (uint32_t h = 0; h < nh; h++)
                    in_ids[(size_t) i * nh + h] = step > h ? (eos_seen[i][h] ? hp.eos_token_id : last[h]) : hp.bos_token_id;
            }
            if (hook && step % LOOK_IN == 0) {
                hook->plan(toks, finished);
                go = hook->emit_rows(on_chunk);
            }
        }
    }
    if (hook && go) {   // what is left once every row is done
        finished.assign(n, true);
        hook->plan(toks, finished);
        (void) hook->emit_rows(on_chunk);
    }
    return toks;
}

// un-delayed codes of frames.size() utterances, concatenated, through the codec in one pass: the audio of each, pointing into `pcm`
std::vector<tts_response> parler_runner::decode_frames(const std::vector<uint32_t> & codes, const std::vector<uint32_t> & frames) {
    size_t total = 0;
    for (uint32_t f : frames) total += (size_t) f * hp.up_sampling_factor;
    pcm.assign(total, 0.0f);
    if (total) hip_check(tts_hip_dac_decode_batch(ctx, codes.data(), frames.data(), (uint32_t) frames.size(), pcm.data()), "tts_hip_dac_decode_batch");
    std::vector<tts_response> audio(frames.size());
    size_t off = 0;
    for (size_t i = 0; i < frames.size(); i++) {
        audio[i].data = pcm.data() + off;
        audio[i].n_outputs = (size_t) frames[i] * hp.up_sampling_factor;
        off += audio[i].n_outputs;
    }
    return audio;
}

void parler_runner::generate(const char * sentence, tts_response & output, const generation_configuration & config) {
    std::vector<uint32_t> prompt, codes;
    output.data = nullptr;
    output.n_outputs = 0;
    if (!prepare_single(sentence, config, prompt)) return;
    last_output_tokens = std::move(run_rows({(uint32_t) prompt.size()}, config, nullptr)[0]);
    adjust_output_tokens(last_output_tokens, codes);
    const tts_response audio = decode_frames(codes, {(uint32_t) (codes.size() / hp.n_output_heads)})[0];
    output.data = audio.data;
    output.n_outputs = audio.n_outputs;
}

void parler_runner::generate_batch(const std::vector<std::string> & sentences, std::vector<tts_response> & outputs,
                                   const generation_configuration & config) {
    outputs.assign(sentences.size(), tts_response{});
    std::vector<uint32_t> start, row_of;
    if (!prepare_batch(sentences, config, start, row_of)) return;
    std::vector<std::vector<uint32_t>> row_tokens = run_rows(start, config, nullptr);
    std::vector<uint32_t> codes, frames;
    for (size_t i = 0; i < row_of.size(); i++) {
        const size_t before = codes.size();
        adjust_output_tokens(row_tokens[i], codes);
        frames.push_back((uint32_t) ((codes.size() - before) / hp.n_output_heads));
        last_batch_tokens[row_of[i]] = std::move(row_tokens[i]);
    }
    const std::vector<tts_response> audio = decode_frames(codes, frames);
    for (size_t i = 0; i < row_of.size(); i++) outputs[row_of[i]] = audio[i];
}

void parler_runner::generate_chunked(const char * sentence, const generation_configuration & config, uint32_t chunk_frames,
                                     const std::function<bool(const float *, size_t)> & on_chunk) {
    if (chunk_frames == 0) TTS_ABORT("generate_chunked: chunk_frames must be >= 1\n");
    std::vector<uint32_t> prompt;
    if (!prepare_single(sentence, config, prompt)) return;
    const std::function<bool(uint32_t, const float *, size_t)> cb = [&](uint32_t, const float * p, size_t k) { return on_chunk(p, k); };
    dac_chunker hook = make_chunker(chunk_frames);
    last_output_tokens = std::move(run_rows({(uint32_t) prompt.size()}, config, &hook, cb)[0]);
}

void parler_runner::generate_batch_chunked(const std::vector<std::string> & sentences, const generation_configuration & config, uint32_t chunk_frames,
                                           const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) {
    if (chunk_frames == 0) TTS_ABORT("generate_batch_chunked: chunk_frames must be >= 1\n");
    std::vector<uint32_t> start, row_of;
    if (!prepare_batch(sentences, config, start, row_of)) return;
    const std::function<bool(uint32_t, const float *, size_t)> cb = [&](uint32_t row, const float * p, size_t k) { return on_chunk(row_of[row], p, k); };
    dac_chunker hook = make_chunker(chunk_frames);
    std::vector<std::vector<uint32_t>> row_tokens = run_rows(start, config, &hook, cb);
    for (size_t i = 0; i < row_of.size(); i++) last_batch_tokens[row_of[i]] = std::move(row_tokens[i]);
}

// ---- continuous batching (common.h; tts_hip_parler_stream_* underneath) ----------------------------------------------------------------
static constexpr uint32_t STREAM_CHUNK = 32;     // decode steps between two look-in points (what generate_loop's compaction uses)
static constexpr size_t   STREAM_CODEC_GROUP = 64;   // finished utterances per codec pass (the device's pass size); flushed when the session drains

// the limits of the device sampler (tts_hip_parler_stream_admit_mixed); a greedy request never reads them
static bool device_sampler(const generation_configuration & config) {
    return !config.sample || (config.temperature > 0.0f && config.top_p > 0.0f && config.repetition_penalty > 0.0f);
}

void parler_runner::stream_begin(const generation_configuration & config) {
    if (stream_capacity() == 0) TTS_ABORT("stream_begin: the runner was loaded with max_seqs=%u; a session needs >= 2 (TTS_HIP_MAX_SEQS)\n", max_seqs);
    if (config.use_cross_attn != use_cross_attn) TTS_ABORT("stream_begin: use_cross_attn differs from load time\n");
    if (config.sample && hp.output_vocab_size > 2048) TTS_ABORT("stream_begin: sampling over %u logits per head is host-only\n", hp.output_vocab_size);
    (void) voice_index(config.voice, "stream_begin");
    if (st_on) stream_end();
    const uint32_t slots = stream_capacity();
    st_max_steps = hp.max_generation_size - 1;   // an utterance ends at position max_generation (check_stopping): at most this many steps after a 1-id prompt
    // the device sampler's vocabulary: every slot carries its own sampler record (stream_accepts); above it the session is greedy with one setting
    st_mixed = hp.output_vocab_size <= 2048;
    if (st_mixed) {
        if (!device_sampler(config)) TTS_ABORT("stream_begin: temperature, top_p and repetition_penalty must be > 0 (got %g, %g, %g)\n", config.temperature, config.top_p, config.repetition_penalty);
        hip_check(tts_hip_parler_stream_begin_mixed(ctx, slots, st_max_steps, hp.bos_token_id, hp.eos_token_id), "tts_hip_parler_stream_begin_mixed");
    } else {
        hip_check(tts_hip_parler_stream_begin(ctx, slots, st_max_steps, hp.bos_token_id, hp.eos_token_id, nullptr), "tts_hip_parler_stream_begin");
    }
    session_open(config, slots);
    st_start.assign(slots, 0);
    st_voice.assign(slots, 0);
    st_wait.clear(); st_codec.clear(); st_pcm.clear();
    st_codec_held = 0;
    st_hook.reset();
}

// chunked audio out of the session (common.h): this runner's part of stream_session's hook
bool parler_runner::session_chunks_ready(uint32_t chunk_frames) {
    if (!st_on) TTS_ABORT("stream_chunks: no session (stream_begin)\n");
    if (st_live != 0 || !st_wait.empty() || !st_codec.empty()) TTS_ABORT("stream_chunks: after stream_begin and before the first stream_submit\n");
    if (dac_halo < 0) return false;   // no window pass for this codec layout: whole utterances, as without the hook
    // Opt-in (TTS_PARLER_STREAM_CHUNKS, read here like TTS_HOST_LOOP in run_rows): without it generate_stream_chunked on a Parler runner keeps
    // handing each finished utterance out as one chunk, out of the codec groups of 64, which callers and tests/test_gpu_dia_stream_chunked.py rely on
    const char * on = getenv("TTS_PARLER_STREAM_CHUNKS");
    if (!on || !*on || !strcmp(on, "0")) return false;
    const uint32_t slots = stream_capacity();
    st_hook = std::make_unique<dac_chunker>(make_chunker(chunk_frames));
    st_hook->rows.assign(slots, {});
    st_toks.assign(slots, {});
    st_fin.assign(slots, false);
    st_state.assign(slots, SLOT_FREE);
    st_stopped.clear();
    st_buf.assign((size_t) slots * st_max_steps * hp.n_output_heads, 0u);
    last_batch_tokens.clear();
    return true;
}

bool parler_runner::stream_accepts(const generation_configuration & config) const {
    return st_on && st_mixed && config.use_cross_attn == use_cross_attn && device_sampler(config) && voice_known(config.voice);
}

void parler_runner::stream_submit(size_t ticket, const std::string & sentence, const generation_configuration & config) {
    if (!st_on) TTS_ABORT("stream_submit: no session (stream_begin)\n");
    if (st_free.empty()) TTS_ABORT("stream_submit: no free row (stream_free() == 0)\n");
    if (config.use_cross_attn != use_cross_attn) TTS_ABORT("stream_submit: use_cross_attn differs from load time\n");
    if (st_mixed && !device_sampler(config))
        TTS_ABORT("stream_submit: temperature, top_p and repetition_penalty must be > 0 (got %g, %g, %g)\n", config.temperature, config.top_p, config.repetition_penalty);
    pending p;
    p.ticket = ticket;
    p.cfg = st_mixed ? config : st_cfg;   // a session without per-slot samplers runs everything with the configuration it was opened with
    p.voice = voice_index(p.cfg.voice, "stream_submit");
    if (!tokenize_prompt(sentence, p.prompt)) {
        // generate() answers such a prompt with an empty response: the session does the same at its next step
        fprintf(stderr, "prompt of %zu tokens leaves no room for generation\n", p.prompt.size());
        st_codec.push_back(decoded{ticket, {}});
        return;
    }
    p.slot = st_free.back();
    st_free.pop_back();
    if (st_chunk_frames) {   // a new occupant: its tokens and its chunker row start at zero
        st_hook->rows[p.slot] = {};
        st_toks[p.slot].clear();
        st_fin[p.slot] = false;
        std::erase(st_stopped, (size_t) p.slot);
        st_state[p.slot] = SLOT_RUNNING;
    }
    st_wait.push_back(std::move(p));
    st_live++;
}

// stream_step with the hook (parler_runner.h), the newcomers admitted: the codec pass of the windows planned at the last look-in runs on the
// codec's stream while this interval's decoder steps run on the decoder's.
void parler_runner::stream_step_chunked(std::vector<stream_result> & finished) {
    const uint32_t slots = stream_capacity(), nh = hp.n_output_heads;
    for (const decoded & d : st_codec) report_no_audio(finished, d.ticket);   // prompts that left no room for generation: an empty answer, as generate() gives
    st_codec.clear();
    std::vector<uint32_t> fs(slots), fn(slots), cnt(slots);
    std::vector<uint8_t> done(slots);
    uint32_t nf = 0;
    bool running = false;
    for (uint32_t s = 0; s < slots; s++) running = running || st_state[s] == SLOT_RUNNING;
    // nothing live but windows still planned: they are decoded without a launch
    if (running) hip_check(tts_hip_parler_stream_launch(ctx, STREAM_CHUNK), "tts_hip_parler_stream_launch");
    try {
        // a window's key is its row, here the slot: the slot keeps its ticket until its last piece is out
        st_hook->emit_session(std::vector<size_t>(st_hook->row_of.begin(), st_hook->row_of.end()),
                              [this](size_t slot, const float * p, size_t k) { return st_on_chunk(st_ticket[slot], p, k); }, st_stopped);
    } catch (...) {
        // an error of the codec pass or a throwing callback: the steps under way are waited for, so the context stays usable
        if (running) (void) tts_hip_parler_stream_wait(ctx, nullptr, nullptr, nullptr, &nf, fs.data(), fn.data());
        throw;
    }
    for (uint32_t s = 0; s < slots; s++) {   // those that had ended at the last look-in have had their last piece: the slot is free from here on
        if (st_state[s] != SLOT_CLOSING) continue;
        report_no_audio(finished, st_ticket[s]);
        st_state[s] = SLOT_FREE;
        st_free.push_back(s);
        st_live--;
    }
    if (!running) return;
    hip_check(tts_hip_parler_stream_wait(ctx, st_buf.data(), cnt.data(), done.data(), &nf, fs.data(), fn.data()), "tts_hip_parler_stream_wait");
    std::vector<uint32_t> drop;
    for (uint32_t s = 0; s < slots; s++) {
        if (st_state[s] != SLOT_RUNNING) continue;
        std::vector<uint32_t> & t = st_toks[s];
        const uint32_t steps = std::min(cnt[s], hp.max_generation_size - st_start[s]);   // what generate() would have run alone
        const uint32_t * b = st_buf.data() + (size_t) s * st_max_steps * nh;
        if ((size_t) steps * nh > t.size()) t.insert(t.end(), b + t.size(), b + (size_t) steps * nh);
        if (std::find(st_stopped.begin(), st_stopped.end(), s) != st_stopped.end()) {   // on_chunk ended it: reported with what it got, nothing more is decoded for it
            if (!done[s]) drop.push_back(s);
            remember_tokens(st_ticket[s], t);
            report_no_audio(finished, st_ticket[s]);
            st_hook->rows[s] = {};
            t.clear();
            st_state[s] = SLOT_FREE;
            st_free.push_back(s);
            st_live--;
        } else if (done[s]) {   // ended: plan() cuts its tail, the next step hands it out
            remember_tokens(st_ticket[s], t);
            st_fin[s] = true;
            st_state[s] = SLOT_CLOSING;
        }
    }
    if (!drop.empty()) hip_check(tts_hip_parler_stream_drop(ctx, (uint32_t) drop.size(), drop.data()), "tts_hip_parler_stream_drop");
    st_hook->plan(st_toks, st_fin);
}

void parler_runner::stream_step(std::vector<stream_result> & finished) {
    if (!st_on) TTS_ABORT("stream_step: no session (stream_begin)\n");
    finished.clear();
    const uint32_t nh = hp.n_output_heads;
    if (!st_wait.empty()) {   // the newcomers: one prefill side batch, then rows of the lock-step forward
        std::vector<uint32_t> slots, ids, lens, voices;
        std::vector<float> uni;
        std::vector<tts_hip_sampling> sps(st_wait.size());
        std::vector<const tts_hip_sampling *> spp(st_wait.size(), nullptr);
        bool any_sampled = false;
        for (const auto & p : st_wait) any_sampled = any_sampled || p.cfg.sample;
        if (st_mixed && any_sampled) uni.assign(st_wait.size() * (size_t) st_max_steps * nh, 0.0f);   // [n][max_steps][heads]; a greedy utterance's block is ignored
        for (size_t i = 0; i < st_wait.size(); i++) {
            const pending & p = st_wait[i];
            slots.push_back(p.slot);
            voices.push_back(p.voice);
            st_voice[p.slot] = p.voice;
            lens.push_back((uint32_t) p.prompt.size());
            ids.insert(ids.end(), p.prompt.begin(), p.prompt.end());
            st_ticket[p.slot] = p.ticket;
            st_start[p.slot] = (uint32_t) p.prompt.size();
            if (!st_mixed || !p.cfg.sample) continue;
            // the utterance's own sampler and draws, seeded as a generate() call of its own would be
            sps[i] = tts_hip_sampling{(uint32_t) p.cfg.top_k, p.cfg.top_p, p.cfg.temperature, p.cfg.repetition_penalty};
            spp[i] = &sps[i];
            draw_row_uniforms(smp, p.cfg.seed, st_max_steps, nh, uni.data() + i * (size_t) st_max_steps * nh);
        }
        set_slot_voices(slots, voices, "tts_hip_parler_seq_voices");   // before the admission: its prefill already attends
        if (st_mixed)
            hip_check(tts_hip_parler_stream_admit_mixed(ctx, (uint32_t) slots.size(), slots.data(), ids.data(), lens.data(), spp.data(), any_sampled ? uni.data() : nullptr),
                      "tts_hip_parler_stream_admit_mixed");
        else
            hip_check(tts_hip_parler_stream_admit(ctx, (uint32_t) slots.size(), slots.data(), ids.data(), lens.data(), nullptr), "tts_hip_parler_stream_admit");
        st_wait.clear();
    }
    if (st_chunk_frames) return stream_step_chunked(finished);
    std::vector<uint32_t> fs(stream_capacity()), fn(stream_capacity());
    uint32_t nf = 0;
    hip_check(tts_hip_parler_stream_run(ctx, STREAM_CHUNK, &nf, fs.data(), fn.data()), "tts_hip_parler_stream_run");
    for (uint32_t i = 0; i < nf; i++) {
        const uint32_t slot = fs[i];
        const uint32_t steps = std::min(fn[i], hp.max_generation_size - st_start[slot]);   // what generate() would have run alone
        std::vector<uint32_t> toks((size_t) steps * nh);
        hip_check(tts_hip_parler_stream_collect(ctx, slot, steps, toks.data()), "tts_hip_parler_stream_collect");
        decoded d;
        d.ticket = st_ticket[slot];
        adjust_output_tokens(toks, d.frames);
        st_codec.push_back(std::move(d));
        st_free.push_back(slot);
        st_live--;
    }
    // the codec: whole groups of 64 as they fill (the device's pass size); what is left goes out when nothing is generating any more, and in any case
    // one look-in interval after it finished — a finished utterance waits at most STREAM_CHUNK decode steps for company, never for a group to fill
    // (round 4 held a finished request's audio until 63 more utterances had finished: under steady arrivals with fewer than 64 rows, for ever)
    const bool drain = st_live == 0;
    size_t take = st_codec.size() >= STREAM_CODEC_GROUP ? st_codec.size() / STREAM_CODEC_GROUP * STREAM_CODEC_GROUP : 0;
    if (!take && !st_codec.empty() && (drain || st_codec_held >= st_codec_hold)) take = st_codec.size();
    st_codec_held = (take < st_codec.size()) ? (take ? 0 : st_codec_held + 1) : 0;
    if (take) {
        std::vector<uint32_t> codes, frames(take);
        for (size_t i = 0; i < take; i++) {
            frames[i] = (uint32_t) (st_codec[i].frames.size() / nh);
            codes.insert(codes.end(), st_codec[i].frames.begin(), st_codec[i].frames.end());
        }
        const std::vector<tts_response> audio = decode_frames(codes, frames);
        for (size_t i = 0; i < take; i++) {
            stream_result r;
            r.ticket = st_codec[i].ticket;
            r.audio = audio[i];
            finished.push_back(r);
        }
        st_codec.erase(st_codec.begin(), st_codec.begin() + (std::ptrdiff_t) take);
    }
}

void parler_runner::stream_end() {
    if (!st_on) return;
    (void) tts_hip_parler_stream_end(ctx);
    session_close();
    st_wait.clear(); st_codec.clear();
    st_hook.reset();
    st_buf.clear(); st_buf.shrink_to_fit();
}
