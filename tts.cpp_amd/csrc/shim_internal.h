// shim_internal.h — what the translation units of libtts_hip.so share: error plumbing, the arena / tensor records, the device
// context (tts_hip_ctx) and the few host functions one unit calls in another.  Kernel headers are included by the unit that launches them.
#pragma once
#include "../../include/tts_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <mutex>
#include <string>
#include <vector>

#include <unordered_map>
#define LLAMA_GREEDY_CHUNK 8

#include "session_slots.h"   // set_err (shim_core.hip: thread-local message behind tts_hip_last_error()), SlotLedger, penalty_table
// TTS_HIP_FLAG_KV_F16 is tts_hip_orpheus_create's alone: every other create call refuses it by name (true: refused, the message is set)
static inline bool refuse_kv_f16(uint32_t flags, const char *call) {
    if (!(flags & TTS_HIP_FLAG_KV_F16)) return false;
    set_err("%s: TTS_HIP_FLAG_KV_F16 is not accepted here: it selects the fp16 K/V cache of tts_hip_orpheus_create (Parler's is tts_hip_desc::kv_type)", call);
    return true;
}
#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) return set_err("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
    } while (0)
#define CHK(expr)                       \
    do {                                \
        int _r = (expr);                \
        if (_r != 0) return _r;         \
    } while (0)

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
#define TTS_HIP_Q8I 100  // device-side: int8 block integers [N][K] followed by fp16 block scales [N][K/32]

struct Tensor {
    int type = 0;  // type as stored on the device (F32, F16 or TTS_HIP_Q8I)
    int n_dims = 0;
    int64_t ne[4] = {1, 1, 1, 1};
    size_t nbytes = 0;
    int src_type = 0;  // ggml type the tensor had in the GGUF
    void *tmp = nullptr;  // device staging copy until finalize
    bool has_data = false;
    int64_t nelem() const { return ne[0] * ne[1] * ne[2] * ne[3]; }
};

struct W {  // a matrix living in the arena
    size_t off = 0;
    size_t soff = 0;  // TTS_HIP_Q8I: block scales
    int type = 0;
    int64_t K = 0, N = 0;
    bool src_q4 = false;            // every stacked source tensor was Q4_0 in the GGUF
    const uint8_t *q4 = nullptr;    // TTS_HIP_Q4_NATIVE: the 4-bit codes repacked next to the int8 expansion (gemv_q4_rows_kernel)
    size_t stoff = 0;               // TTS_HIP_Q8I matrices of the Parler decoder and of Orpheus contexts of more than 64 slots: the block scales once more, transposed (float [K/32][ldw]) for qgemm_tile_kernel
    int ldw = 0;
};

// where a tiled integer GEMM's epilogue leaves its result rows as Q8_0 blocks for the next quantised matrix (set by the caller right before run_gemm)
struct QTileOut { int8_t *q = nullptr; float *dT = nullptr; int ldq = 0; const void *stands_for = nullptr; };   // stands_for: the fp32 buffer the consumer names as its input

struct PLayer {
    W qkv, o, cq, ck, cv, co, fc1, fc2;
    size_t sa_w = 0, sa_b = 0, ca_w = 0, ca_b = 0, f_w = 0, f_b = 0;
};

struct DRes { size_t in_alpha, in_w, in_b, out_alpha, out_w, out_b; };
struct DBlock { int stride, padding, cin, cout; size_t alpha, w, b; DRes res[3]; };

struct CopyItem { size_t dst; std::string src; size_t src_off = 0; size_t bytes = 0; };  // bytes == 0: the whole tensor

struct ProfEv { hipEvent_t a, b; int kclass; };

// Codec activation buffers of a device.  Codec passes of one device take turns (g_dac_pass_mutex: a pass fills the chip), so every
// context of the device works in the same buffers instead of holding its own three activation buffers (197 KB per frame and utterance of
// a pass each: 12.6 GB per context for 64 x 248 frames, 38.6 GB at 1016 frames); they are freed when the device's last codec context goes.
constexpr int GRAPH_KEY_ROWS = 8192;   // captured decode steps are keyed mode * GRAPH_KEY_ROWS + rows (run_step, drop_gen_graphs)

struct DacBuffers {
    float *dbuf[3] = {nullptr, nullptr, nullptr};
    size_t dbuf_elems = 0;       // capacity of each buffer in floats
    size_t cap_codes = 0;        // ids d_codes holds (frames summed over a batch, padded to the longest, x codebooks)
    float *dplanes = nullptr;    // second planes buffer of the wide classes (the first lives in dbuf[2])
    uint32_t *d_codes = nullptr;
    float *h_pcm = nullptr;
    size_t h_pcm_elems = 0;
    int users = 0;
};
extern DacBuffers g_dac_buffers[64];
extern std::mutex g_dac_pass_mutex[64];

struct tts_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t dac_stream = nullptr;  // low-priority queue for the codec (NULL: same stream)
    tts_hip_desc d{};
    std::map<std::string, Tensor> tensors;
    bool planned = false, finalized = false, weights_present = false;
    bool has_parler = false, has_dac = false;

    // arena
    char *arena = nullptr;
    size_t arena_bytes = 0;
    bool arena_external = false;
    bool arena_counted = false;   // the external arena is another context's allocation and this context holds a reference (shim_core.hip: g_arena_refs)
    std::vector<CopyItem> copies;

    // parler model
    int H = 0, L = 0, NH = 0, F = 0, V = 0, NO = 0, NCTX = 0, E = 0, ECAP = 0, PV = 0, EROWS = 0, NPOS = 0, KVPOS = 0;
    W embed_prompts, embed_tokens, heads;
    size_t pos_embed = 0, text_enc = 0, ln_w = 0, ln_b = 0, cross_kv = 0;
    // The voice-prompt encoding and the cross K/V computed from it are the only arena entries that change after load
    // (tts_hip_parler_set_text_encoding).  Contexts of one device may share an arena (tts_hip_finalize(ctx, arena of another context)),
    // so a context that gets a new prompt moves both into allocations of its own and the arena stays immutable: a sibling in the middle
    // of a generation keeps reading the prompt it started with (the reference keeps a whole model per worker, server.cpp:316-321).
    char *cond_text_enc = nullptr, *cond_cross_kv = nullptr;   // private copies, or NULL = the arena's
    char *text_enc_ptr() const { return cond_text_enc ? cond_text_enc : arena + text_enc; }
    char *cross_kv_ptr() const { return cond_cross_kv ? cond_cross_kv : arena + cross_kv; }
    std::vector<PLayer> layers;
    // Per-request voice descriptions (tts_hip_parler_voice_bank): voices 1 .. vb_n, each [L][2][VOICE_POS][H] fp32 cross K / V plus a length; voice 0 is the
    // description above.  The context's own, also on a shared arena.  Captured launches hold vb_kv / vb_len / vb_seq by pointer: none is ever reallocated.
    enum { VOICE_POS = 32, VOICE_MAX = 256 };   // 32: what attn_short_body<32> covers
    int vb_n = 0;
    float *vb_kv = nullptr, *vb_enc = nullptr;   // the bank; staging for one description's T5 output [VOICE_POS][H]
    int *vb_len = nullptr;                       // device [vb_n + 1]
    uint32_t *vb_seq = nullptr;                  // device [max_seqs + 1]: voice of a cache slot
    std::vector<int> vb_len_h;                   // host mirrors
    std::vector<uint32_t> vb_seq_h;
    bool fwd_voices = false;                     // the forward being staged has a row whose slot carries a non-zero voice: enqueue_forward's "voices" variant
    size_t voice_stride() const { return (size_t) L * 2 * VOICE_POS * H; }
    bool slot_voiced(uint32_t s) const { return s < vb_seq_h.size() && vb_seq_h[s] != 0; }

    // dac model
    int d_ncb = 0, d_cbsize = 0, d_cbdim = 0, d_latent = 0, d_c0 = 0, d_clast = 0, d_up = 1;
    size_t d_codebook = 0, d_projw = 0, d_projb = 0, d_initw = 0, d_initb = 0, d_falpha = 0, d_fw = 0, d_fb = 0;
    std::vector<DBlock> dblocks;

    // runtime buffers
    int RMAX = 0;
    void *kcache = nullptr, *vcache = nullptr;  // [L][max_seqs][NCTX][H]
    float *x = nullptr, *q = nullptr, *att = nullptr, *u32 = nullptr, *logits = nullptr, *part = nullptr, *dbg = nullptr;
    _Float16 *u16 = nullptr, *xn16 = nullptr, *att16 = nullptr;
    int ln_fuse_max = 8;  // rows up to which LayerNorm stays fused in the GEMM prologue
    float *partials = nullptr;  // [8][RMAX][H] split-K slabs of the residual GEMMs
    int8_t *aq = nullptr;       // Q8_0-quantised activation rows [RMAX][max(H,F)]
    float *ad = nullptr;        // their block scales
    bool all_q8i = false;       // every decoder matrix is on the integer path (all GEMMs go through run_qgemm)
    int q_fuse_max = 16;        // rows up to which the integer GEMM quantises its own activations
    bool q4_native = false;     // TTS_HIP_Q4_NATIVE (with TTS_HIP_GEMV_ROWS; default on for Orpheus contexts): Q4_0 matrices are read as 4-bit codes
    std::vector<void *> q4_bufs;
    bool q4_rms = true;         // tune("q4_rms")=0: the rms norms in front of the q/k/v and gate|up projections keep their own launches
    bool q4_silu = true;        // tune("q4_silu")=0: gate|up, silu * up and the down projection stay three launches
    bool q4_rope = true;        // tune("q4_rope")=0: the Llama q/k/v projection keeps its separate rope + cache-append launch
    bool q4_lds = true;         // tune("q4_lds")=0: Q4_0 row products stay on gemv_q4_rows_kernel (one feature per wave, activations from L2)
    int q_stream = 31;          // tune("q_stream"): which quantised projections of a 5 .. 64 row Llama step take qgemv_stream_kernel instead of qgemm16_kernel
                                // (bits: 1 qkv, 2 o, 4 gate|up, 8 down, 16 head; 0 none, 1 = all)
    bool gemv_stream = true;    // tune("gemv_stream")=0: <= 16-row F16 GEMMs of the Dia step stay on gemm16_kernel (gemv_stream_kernels.h otherwise)
    bool llama_graph = false;   // TTS_HIP_LLAMA_GRAPH (default on for Orpheus contexts): the greedy step as one captured graph
    bool gemv_rows = false;     // TTS_HIP_GEMV_ROWS (default on for Orpheus contexts): 1..4 rows go through the streaming one-wave-per-feature kernels (gemv_kernels.h)
    // ---- Orpheus decoder context (tts_hip_orpheus_create) ----
    bool has_llama = false;
    tts_hip_orpheus_desc lm{};
    struct LLayer { size_t in_norm = 0, post_norm = 0; W qkv, o, gu, down; };
    std::vector<LLayer> l_layers;
    size_t l_embd = 0, l_out_norm = 0, l_ropef = 0;
    W l_head;
    int l_V = 0, l_Vpad = 0, l_kvH = 0, l_ksplit = 1;
    float *l_x = nullptr, *l_xn = nullptr, *l_qkv = nullptr, *l_att = nullptr, *l_gu = nullptr, *l_g = nullptr, *l_logits = nullptr, *l_parts = nullptr;
    void *l_kc = nullptr, *l_vc = nullptr;   // [slot][layer][position][kv width] of l_kv_esz bytes per element
    int l_kv_esz = 4;                        // 2 under TTS_HIP_FLAG_KV_F16, 1 under kv_type = TTS_HIP_KV_F8_E4M3 (fixed at create: the captured graphs never see it change)
    uint32_t *l_ids = nullptr, *l_pos = nullptr, *l_tok = nullptr;
    uint32_t *l_seq = nullptr, *l_btok = nullptr, *l_bpi = nullptr;   // lock-step utterances: row -> cache slot, selected tokens [rows], arg-max partials
    float *l_bpv = nullptr;
    int l_pending = 0;
    int64_t l_pstride = 0;   // floats between the pending slabs (0: RMAX * H)
    // ---- Dia context (tts_hip_dia_create) ----
    bool has_dia = false;
    tts_hip_dia_desc dia{};
    struct DiaEnc { size_t sa_norm = 0, mlp_norm = 0; W qkv, o, gu, out; };
    struct DiaDec { size_t sa_norm = 0, ca_norm = 0, mlp_norm = 0; W sqkv, so, cq, ckv, co, gu, out; };
    std::vector<DiaEnc> di_enc;
    std::vector<DiaDec> di_dec;
    size_t di_enc_embd = 0, di_enc_norm = 0, di_dec_norm = 0, di_embd[16] = {0};
    W di_heads;
    int di_EH = 0, di_EF = 0, di_DF = 0, di_A = 0, di_kvH = 0, di_V = 0, di_Vpad = 0, di_ksplit = 1, di_pending = 0, di_evocab = 0;
    float *di_ex = nullptr, *di_exn = nullptr, *di_eqkv = nullptr, *di_eatt = nullptr, *di_egu = nullptr, *di_eg = nullptr, *di_ek = nullptr, *di_ev = nullptr;
    float *di_ckv = nullptr;
    void *di_ck = nullptr, *di_cv = nullptr, *di_k = nullptr, *di_v = nullptr;   // cross [L][2U][max_ctx][A] and self [L][2U][max_gen][kv width] of di_kv_esz bytes per element
    int di_kv_esz = 4;   // 2 under tts_hip_dia_desc::kv_type = TTS_HIP_F16 (fixed at create: the captured graphs never see it change)
    float *di_x = nullptr, *di_xn = nullptr, *di_qkv = nullptr, *di_q = nullptr, *di_att = nullptr, *di_gu = nullptr, *di_g = nullptr, *di_parts = nullptr;
    float *di_logits = nullptr, *di_guided = nullptr;
    uint32_t *di_tok = nullptr, *di_epos = nullptr, *di_eseq = nullptr, *di_kbeg = nullptr, *di_kend = nullptr;
    uint32_t *di_ids = nullptr, *di_pos = nullptr, *di_seq = nullptr, *di_cend = nullptr;
    // device-resident generation loop: sampled ids [U][NO], countdown [U] / parked [U] / sampler call [U] / history rows handed out [U] in di_loop,
    // history [U][G][NO]; a look-in packs per slot {sampler calls, parked, new history rows} into di_look, which travels to h_di_look (pinned)
    // in one copy
    uint32_t *di_stok = nullptr, *di_loop = nullptr, *di_hist = nullptr;
    uint32_t *di_look = nullptr, *h_di_look = nullptr;
    _Float16 *di_e16 = nullptr;   // [2 * max_ctx][max(EH, A, EF)] the encoder activations rounded to fp16 for gemm_tile_kernel
    // the tiled route (decoder steps of more than 16 rows on gemm_tile_kernel, shim_llama.hip: dia_forward_tiled)
    _Float16 *di_h16 = nullptr;   // [2 * di_U][max(DH, A, DF)] the fp16 rows the next tiled GEMM reads (one producer, one consumer, stream order); NULL while the key is 0 (dia_tiled_buffers)
    int dia_tile_min_rows = 0;    // tune("dia_tile_min_rows"): steps of at least this many rows (and more than 16) take the route; 0 = never.  0 up to 64 slots, 17 above
    int di_tiled = 0;             // gemm_tile_kernel launches of the last dia_forward (debug_read "di_tiled")
    int di_pending_max = 0;       // most K-slice slabs one GEMM of the last dia_forward left in di_parts (debug_read "di_pending_max")
    int di_U = 1;                        // utterance slots (rows = 2 per slot)
    // One loop, two ways in.  BATCH (tts_hip_dia_gen_begin / _launch / _wait, tts_hip_dia_generate): n encoded slots, all live from the first
    // step with the budget max_gen, until the last one has parked.  SESSION (tts_hip_dia_stream_*): n slots that begin parked; admissions
    // make them live, reports and collections free them again.
    struct DiaLoop : SlotLedger {         // ENDED: seen parked by a look-in, not yet reported
        enum Mode : uint8_t { NONE = 0, BATCH = 1, SESSION = 2 };
        Mode mode = NONE;
        bool sampled = false, rep = false;
        bool mixed = false;              // SESSION opened by tts_hip_dia_stream_begin_mixed: every slot carries its own sampler (di_srec)
        bool all_done = false;           // the last look-in found no live slot
        uint32_t n = 0, max_gen = 0;     // utterances (BATCH) or slots (SESSION)
        tts_hip_dia_codes codes{};
        tts_hip_sampling sp{};
        std::vector<uint32_t> steps;     // per slot at the last look-in: sampler calls made
        std::vector<uint32_t> budget;    // per slot: the occupant's step budget
        std::vector<uint32_t> handed;    // per slot: history rows of the occupant handed out (the host's copy of di_loop's fourth array)
        uint32_t launched = 0;           // steps enqueued so far (BATCH: at most max_gen + 1)
    } dl;
    // what the captured step of a mode holds by value: a begin that changes any of it drops that mode's graph (and only that one, so a
    // caller alternating tts_hip_dia_generate, a session and a mixed session keeps all three)
    struct DiaBaked { const void *uni = nullptr, *pen = nullptr; tts_hip_sampling sp{}; int sampled = -1; uint32_t n = 0, max_gen = 0; tts_hip_dia_codes codes{}; };
    DiaBaked di_baked[3];                // [0] BATCH, [1] SESSION, [2] mixed SESSION (sampled = 2, pen = di_srec)
    uint32_t *di_sbud = nullptr;         // device [2][U]: budget, steps
    uint32_t *di_sadm = nullptr;         // device [2][U]: slots, budgets of one admission
    float *di_suni = nullptr;            // device: the admitted utterances' uniforms before they move into their columns
    size_t di_suni_cap = 0;
    // a mixed session: the slots' sampler records and penalty tables, and where one admission stages its utterances' before the admit launch
    // moves them into the slots' places.  di_srec is allocated once (the captured sample_kernel launch holds it); the tables are reached
    // through the records only, so they may move when a session asks for more
    void *di_srec = nullptr, *di_srec_in = nullptr;   // device SampleRow [U] each
    double *di_spen = nullptr, *di_spen_in = nullptr; // device [U][di_spen_len] each
    size_t di_spen_cap = 0;                           // doubles either holds
    int di_spen_len = 0;                              // entries per slot in the open mixed session (its max_gen)
    std::vector<uint8_t> di_slot_encoded;   // tts_hip_dia_encode_slot has run for the slot
    uint32_t *h_di = nullptr;            // pinned staging: ids / pos / seq of a step
    // ---- Kokoro context (tts_hip_kokoro_create) ----
    bool has_kokoro = false;
    tts_hip_kokoro_desc ko{};
    struct KTensor { size_t off = 0; int64_t ne[4] = {1, 1, 1, 1}; };
    std::unordered_map<std::string, KTensor> k_tensors;   // every "kokoro.*" tensor, fp32, by GGUF name
    // ---- SNAC codec context (tts_hip_snac_create) ----
    bool has_snac = false;
    tts_hip_snac_desc snac{};
    struct SRes { size_t in_alpha = 0, in_w = 0, in_b = 0, out_alpha = 0, out_w = 0, out_b = 0; };
    struct SBlock { int stride = 0, padding = 0, cin = 0, cout = 0; size_t alpha = 0, w = 0, b = 0, noise_w = 0; SRes res[3]; };
    std::vector<SBlock> sblocks;
    size_t s_codebook = 0, s_projw = 0, s_projb = 0, s_inw = 0, s_inb = 0, s_upw = 0, s_upb = 0, s_falpha = 0, s_fw = 0, s_fb = 0;
    int s_latent = 0, s_c0 = 0, s_cbdim = 0, s_cbsize = 0, s_up = 1, s_clast = 0;
    float *sbuf[3] = {nullptr, nullptr, nullptr};
    bool snac_packed = false;
    // one pass (tts_hip_snac_decode / _decode_windows): segment table, codes and noise travel in one block, h_in (pinned) -> s_in; the
    // cropped PCM comes back s_out -> h_out (pinned).  Capacities in 4-byte elements; sbuf holds dac_cap_frames tokens.
    uint32_t *s_in = nullptr, *h_in = nullptr;
    float *s_out = nullptr, *h_out = nullptr;
    size_t s_in_cap = 0, s_out_cap = 0;
    struct { bool active = false; float *pcm_out = nullptr; size_t n = 0; } snac_pending;   // between _decode_windows_begin and _end
    // ---- Orpheus generation in pieces (tts_hip_orpheus_gen_begin / _launch / _wait), one sequence: the captured step; several utterances are ls in BATCH mode ----
    struct LlamaGen {
        bool active = false, sampled = false, done = false;
        uint32_t max_new = 0, stop_id = 0;
        tts_hip_sampling sp{};
        uint32_t pending = 0;                       // steps enqueued by gen_launch that no gen_wait has read yet
        uint32_t pos = 0, cur = 0;                  // next position, latest id
        std::vector<uint32_t> toks;                 // ids so far
        uint32_t handed = 0;                        // ... of which a gen_wait has handed out
    } lg;
    // ---- The Orpheus lock-step loop: per-slot state on the device, the host keeps the copy of the last look-in.  One loop, two ways in.  BATCH
    // (tts_hip_orpheus_gen_begin / _launch / _wait at n_utt > 1, tts_hip_orpheus_generate_batch): slots 0 .. n-1, all admitted at begin.  SESSION
    // (tts_hip_orpheus_stream_*): admissions fill the slots, reports and collections free them again.  The device buffers stay on the context from
    // one loop to the next (cap_slots x cap_new) and grow when a begin asks for more ----
    struct LlamaStream : SlotLedger {               // ENDED: finished, not yet reported (SESSION) / done (BATCH)
        enum Mode : uint8_t { NONE = 0, BATCH = 1, SESSION = 2 };
        Mode mode = NONE;
        bool sampled = false;
        bool mixed = false;                         // begin_mixed: the admissions bring a sampler per utterance; otherwise every admission takes sp (sampled) or sampler::max
        uint32_t n_slots = 0, max_new = 0, stop_id = 0;
        tts_hip_sampling sp{};
        std::vector<uint32_t> count, cur, pos;      // per slot at the last look-in: ids so far, latest id, its position
        std::vector<uint32_t> handed;               // ids of the occupant that a gen_wait (BATCH) or a stream_wait (SESSION, mirrored in d_handed) has handed out
        std::vector<uint32_t> rows;                 // live slots in slot order (= the rows of the next run)
        std::vector<uint8_t> slot_sampled, slot_nucleus;   // per slot, what its occupant selects with: sampler::sample / ... with top_p < 1
        size_t cap_slots = 0, cap_new = 0;          // what the buffers below hold
        uint32_t *state = nullptr;                  // device [slots][LLAMA_SLOT_STATE]
        uint32_t *tokens = nullptr;                 // device [slots][max_new]
        uint32_t *smp = nullptr;                    // device [slots][3] sampler state
        float *uni = nullptr;                       // device [slots][max_new]
        unsigned long long *cand = nullptr;         // device [slots][TOPK_PARTS][TOPK_MAXK]
        float *total = nullptr;                     // device [slots]
        uint32_t *h_state = nullptr;                // pinned [slots][LLAMA_SLOT_STATE]: an admission's look at its slot
        uint32_t *d_handed = nullptr;               // device [slots] ids llama_loop_lookin_kernel has taken from the occupant
        uint32_t *look = nullptr, *h_look = nullptr;   // device / pinned [slots][LLAMA_SLOT_STATE + max_new] the look-in's block
        void *samp = nullptr;                       // device [slots] llama_slot_sampler
        double *pen = nullptr;                      // device [slots][max_new] pow(penalty, count); first entry 0: penalty 1
    } ls;
    uint32_t l_batch_run = 7;     // tune("orpheus_batch_run"): steps per launch of tts_hip_orpheus_generate_batch: padding rows against look-ins, 7 / 14 / 28 / 56 measured (DESIGN)
    uint32_t *h_hist = nullptr;   // pinned: the ids of the steps of one gen_launch
    size_t h_hist_cap = 0;
    // ---- T5 voice-prompt encoder context (tts_hip_t5_create) ----
    bool has_t5 = false;
    tts_hip_t5_desc t5{};
    struct T5Layer { size_t attn_norm = 0, mlp_norm = 0; W qkv, o, wi, wo; };
    std::vector<T5Layer> t5_layers;
    size_t t5_embd = 0, t5_relb = 0, t5_out_norm = 0, t5_down_b = 0;
    W t5_down;
    bool t5_has_down = false, t5_has_down_b = false;
    int t5_vocab = 0, t5_out = 0;
    int *t5_bucket = nullptr;          // bucket of (key - query) + (n_ctx - 1), host-computed with the reference's arithmetic
    float *t5_x = nullptr, *t5_qkv = nullptr, *t5_att = nullptr, *t5_ug = nullptr, *t5_g = nullptr, *t5_y = nullptr;
    uint32_t *t5_ids = nullptr;
    tts_hip_sampling smp{};     // parameters baked into the captured MODE_GEN_SAMPLE graphs
    float *d_uniforms = nullptr;  // [calls][R][n_out] host-drawn U[0,1) for sample_kernel
    unsigned long long *l_cand = nullptr;   // Orpheus sampler: [TOPK_PARTS][TOPK_MAXK] stage-1 survivors
    uint32_t *l_smp = nullptr;              // Orpheus sampler: [0] last token (int32), [1] repetition count, [2] sampler call index
    struct { const void *uni = nullptr, *pen = nullptr; uint32_t k = 0; float temp = 0, top_p = 1.0f; } l_smp_baked;   // what the captured sampled step holds
    double *d_pen = nullptr;      // pow(repetition_penalty, count) table (host-evaluated)
    int pen_len = 0;
    int32_t *d_last = nullptr;    // [RMAX][n_out] sampler::last_token_ids
    uint32_t *d_repc = nullptr;   // [RMAX][n_out] sampler::repetition_counts
    size_t uniforms_cap = 0;
    uint32_t g_bos = 0xFFFFFFFFu, g_eos = 0xFFFFFFFFu;  // ids baked into the captured feed kernel
    int pending_parts = 0;      // slabs waiting to be folded into x by the next LayerNorm launch
    uint32_t *d_ids = nullptr, *d_pos = nullptr, *d_seq = nullptr, *d_tok = nullptr, *d_step = nullptr, *d_steps_done = nullptr;
    uint32_t *d_gather = nullptr;   // scratch of the row compaction: map [R] + ids [R][n_out] + pos / seq / step [R] each
    // continuous batching (tts_hip_parler_stream_*): the rows' state between two stream_run calls lives on the host
    struct GenStream {
        bool active = false, sampled = false;
        bool mixed = false;              // opened by tts_hip_parler_stream_begin_mixed: every slot carries its own sampler (gs_rec)
        uint32_t n_slots = 0, max_steps = 0, bos = 0, eos = 0;
        std::vector<uint8_t> slot_live;
        std::vector<uint8_t> slot_sampled;   // mixed: the slot's occupant is sampled (a run whose live slots are all greedy replays MODE_GEN)
        std::vector<uint32_t> row_slot, pos, step, ids;   // live rows: cache slot, next position, step counter, next input ids [rows][heads]
        // launch / wait / drop (audio in chunks while the slots keep running)
        bool unwaited = false;           // a stream_launch has enqueued steps that no stream_wait has waited for
        uint32_t launched_live = 0;      // live rows of that launch
        uint32_t unread = 0;             // steps enqueued since the last wait that took rows: no slot holds more un-taken rows than this
        std::vector<uint32_t> slot_sofar;   // [n_slots] steps the occupant has recorded (the step counter advances with every enqueued step: known without a read)
        std::vector<uint32_t> slot_done;    // [n_slots] the occupant's steps_done once check_stopping() has fired (0: not yet), until the next admission
        std::vector<uint32_t> slot_handed;  // [n_slots] host mirror of gs_handed: rows of the occupant a wait has handed out
        std::vector<uint8_t> slot_pend;     // [n_slots] finished and reported, rows not all handed out yet (until taken, collected over by an admission, or dropped)
        // a newcomer with a prompt of len ids: live, a row at position len, step 1, bos in every head
        void push_row(uint32_t s, uint32_t len, int n_out) {
            slot_live[s] = 1;
            row_slot.push_back(s); pos.push_back(len); step.push_back(1);
            ids.insert(ids.end(), (size_t) n_out, bos);
        }
        // the rows whose slot keep(slot) accepts stay, in order, and take position, step and ids [row][n_out] from the arrays given (the session's own, or
        // what the device left); keep is called once per row, in row order
        template <class Keep>
        void keep_rows(Keep keep, const uint32_t *pos_src, const uint32_t *step_src, const uint32_t *ids_src, int n_out) {
            size_t w = 0;
            for (size_t r = 0; r < row_slot.size(); r++) {
                if (!keep(row_slot[r])) continue;
                row_slot[w] = row_slot[r]; pos[w] = pos_src[r]; step[w] = step_src[r];
                memmove(ids.data() + w * n_out, ids_src + r * n_out, (size_t) n_out * 4);
                w++;
            }
            row_slot.resize(w); pos.resize(w); step.resize(w); ids.resize(w * n_out);
        }
    } gs;
    // the look-in of a session wait that takes rows (parler_stream_lookin_kernel): the slots to look at {slot, steps so far} go up from h_gs_look_in,
    // one dense block [entries][2 + cap * heads] comes back into h_gs_look; sized by stream_begin for GS_LOOK_ROWS steps, no wait allocates
    uint32_t *gs_handed = nullptr;       // device [slots + 1]: rows handed out per slot, reset by the admission
    uint32_t *gs_look_in = nullptr, *gs_look = nullptr, *h_gs_look_in = nullptr, *h_gs_look = nullptr;
    size_t gs_look_slots = 0, gs_look_words = 0;   // capacity: slots of gs_handed / gs_look_in, words of gs_look
    // a mixed session's sampler records and penalty tables, kept from one session to the next.  gs_rec [slots + 1] is what the captured
    // MODE_GEN_MIXED sample_kernel launch holds (the padding slot's record stays SAMPLE_ROW_MAX); the tables [slots][gs_pen_len] are reached
    // through the records' pointers.  The *_in copies and gs_adm / gs_uni_in stage one admission for parler_stream_admit_kernel.
    void *gs_rec = nullptr, *gs_rec_in = nullptr;
    size_t gs_rec_cap = 0;               // records either holds
    double *gs_pen = nullptr, *gs_pen_in = nullptr;
    size_t gs_pen_cap = 0, gs_pen_in_cap = 0;   // doubles
    int gs_pen_len = 0;                  // entries per slot in the open mixed session (its max_steps)
    uint32_t *gs_adm = nullptr;          // device [gs_rec_cap]: the slots of one admission
    float *gs_uni_in = nullptr;          // device: the admitted utterances' uniforms before they move into their columns
    size_t gs_uni_in_cap = 0;
    uint32_t gs_baked_steps = 0;    // ... and the step budget they carry
    bool gs_graphs = false;         // the captured generation graphs were made for a stream (feed_kernel's padding slot baked in)
    // the generation loop between tts_hip_parler_gen_begin and its last gen_wait: launch enqueues steps, wait looks in
    struct GenLoop {
        bool active = false, done = false;
        bool voices = false;     // some utterance's slot carried a non-zero voice at gen_begin: every step is the "voices" variant
        bool unwaited = false;   // a gen_launch has enqueued steps that no gen_wait has waited for
        int mode = 0;
        uint32_t n = 0, n_steps = 0, bos = 0, eos = 0;
        uint32_t R = 0;          // rows of the forward (<= n after a compaction)
        uint32_t launched = 0;   // steps enqueued so far
        uint32_t copied = 0;     // steps whose tokens a gen_wait has handed out
        std::vector<uint32_t> start, row_utt;   // start position per utterance; utterance of row r
    } gl;
    int gen_total = 0;              // utterances of the generation loop under way (rows of the forward <= this after a compaction)
    bool gen_compact = true;        // TTS_HIP_GEN_COMPACT=0: finished utterances keep idling in the lock-step forward
    uint32_t *d_tokens_out = nullptr;
    size_t tokens_out_cap = 0;
    uint8_t *d_eos = nullptr;
    // pinned staging
    uint32_t *h_ids = nullptr, *h_pos = nullptr, *h_seq = nullptr, *h_tok = nullptr;
    float *h_logits = nullptr;
    std::vector<uint32_t> host_pos;  // positions per row of the forward being enqueued (for byte accounting)

    // dac: the activation buffers are the device's (g_dac_buffers)
    size_t dac_frame_elems = 0;  // largest activation per frame over all stages (C * L / frames)
    size_t dac_cap_frames = 0;   // SNAC: frames its own buffers hold
    uint32_t *d_frames = nullptr;
    size_t d_frames_cap = 0;
    bool debug = false;
    std::map<int, std::vector<float>> dac_dbg;
    // Dia, tts_hip_set_debug: what every attention launch of the last eager tts_hip_dia_step_batch consumed and produced, key = layer * 2 + (cross ? 1 : 0)
    // (self-attention writes di_att and cross-attention overwrites it, so the rows are copied out between the two)
    struct DiaAttnSnap { std::vector<float> q, out, meta; };
    std::map<int, DiaAttnSnap> dia_attn_dbg;
    std::vector<float> win_pcm;    // tts_hip_dac_decode_windows: the windows' whole PCM before the crop
    std::map<size_t, float *> packed;  // arena offset of a conv weight -> its MFMA-tile-packed copy
    std::set<size_t> packed_direct;    // ... of those, the k = 1 weights packed as [cin][cout] for conv1x1_direct_kernel
    std::map<size_t, _Float16 *> packed16;  // same, fp16 images (dac_f16)
    std::map<size_t, __bf16 *> packed_b3;   // k = 7 conv weights as three bf16 planes (dac_b3, experiment)
    std::map<size_t, __bf16 *> packed_ru;   // residual unit (keyed by its k = 7 weight) -> stage stream of resunit_b3_kernel
    std::map<size_t, __bf16 *> packed_p;    // conv weight -> bf16 planes in stage order for conv_b3p_kernel (k = 7: 64-channel tiles, k = 1: 128-channel tiles)
    int dac_split = 1;          // tune("dac_split") / TTS_HIP_DAC_SPLIT: operand split of the codec's plane kernels for F32 tensors: 1 (default since round 6) = fp16 hi + lo, three
                                // products; 0 = bf16 x 3, six products (rounds 3 - 5).  64 x 248-frame pass 132.4 -> 84.6 ms, every DAC bar held (profiles/r06/dac_split_call1.txt)
    int dac_f16_planes = 1;     // tune("dac_f16_planes")=0: F16 codec tensors stay on round 2's fp16 tile kernels (conv1d_mfma16_kernel / convt1d_mfma16_kernel) instead of the plane kernels with one fp16 plane
    int dac_tap7 = 1;           // tune("dac_tap7")=0: the k = 7 convs on planes keep the tap-pair k-steps (8 slots for 7 taps) instead of one tap per k-step
    int dac_wdma = 1;           // tune("dac_wdma")=0: the fused units as in round 5 (weight stages through registers + ds_write_b128, the k = 1 operand rebuilt per pass)
    int dac_planes = 1;         // tune("dac_planes")=0: the wide classes (channels % 128 == 0, no fused unit) keep fp32 activations and stage snake + split per tile
    bool dac_buf_user = false;  // counted in g_dac_buffers[device].users
    std::map<size_t, __bf16 *> packed_ct;   // transposed conv weight -> bf16 planes of convt_b3_kernel
    int dac_convt_planes = 1;   // tune("dac_convt_planes") = 0: the bf16 x 3 transposed convs always stage fp32 input (snake + split per workgroup) instead of the producer's planes
    int dac_convt_b3 = 1;       // tune("dac_convt_b3")=0: the transposed convs stay on the exact-fp32 MFMA kernel
    int dac_fuse = 1;           // tune("dac_fuse")=0: residual units at 96 / 192 channels stay two launches (k = 7 conv, k = 1 conv + residual)
    int dac_b3 = 2;             // TTS_HIP_DAC_BF16X3 / tune("dac_exact_fp32") (default 2 since round 3; 0 = exact-fp32 MFMA convs): k = 7 convs of F32 tensors as six bf16 MFMAs per product (conv1d_mfma_b3_kernel); 1 = only the layers with 64-channel tiles, 2 = also the 96-channel tile (both measured and in the parity tests since round 3)
    bool kk_lstm_split = true;  // tune("kokoro_lstm_split")=0: the bidirectional LSTMs through the one-workgroup-per-direction kernel
    char *kk_pool = nullptr;    // Kokoro scratch pool (KScratch): grows to the largest call
    size_t kk_pool_cap = 0, kk_pool_next = 0;
    int *kk_stuck = nullptr;    // set by kk_lstm_split_kernel when a granule never arrives (bounded spin)
    bool kk_b3 = true;          // tune("kokoro_b3") = 0: Kokoro's k = 3 / 5 / 7 / 11 same-convolutions stay on the exact-fp32 MFMA kernel instead of bf16 x 3 split products
    bool kk_attn_lds = true;    // tune("kokoro_attn_lds") = 0: ALBERT's attention as one wave per (head, row) walking the K rows from memory (kk_albert_attn_kernel)
    int kk_split = 1;           // tune("kokoro_split"): the operand split of those convolutions — 1 = fp16 hi + lo, three products (round 6), 0 = three bf16 planes, six products
    bool kk_adain_split = true; // tune("kokoro_adain_split")=0: instance-norm rows of 8192 positions and more stay on one workgroup per channel (kk_adain_kernel) instead of the sliced kk_adain_split_kernel
    bool kk_mfma = true;        // tune("kokoro_mfma")=0: every Kokoro convolution through the one-thread-per-output kernel
    bool attn_short = true;     // tune("attn_short")=0: cross-attention through the general kernel
    int dac_group = 64;         // TTS_HIP_DAC_GROUP: utterances per codec pass (16: 451, 32: 458, 64: 461, 128: 460, 384: 462 audio-s/s at 3 x 384)
    bool dac_conv1_direct = true;   // tune("dac_conv1_direct")=0: the 96- / 192-channel k=1 convs stay on conv1d_mfma_kernel<1,...>
    int attn_rows_min = 256;    // tune("attn_rows_min") / TTS_HIP_ATTN_ROWS: forwards with at least this many rows run the self-attention one workgroup per ROW (attn_rows_kernel); 0 = never
    int attn_rows_u = 2;        // tune("attn_rows_u") / TTS_HIP_ATTN_ROWS_U: keys in flight per lane of attn_rows_kernel, 2 / 4 / 8 = 32 / 48 / 80 VGPRs; same arithmetic in the same key order.  2: a wave fits beside every codec kernel of another context (measured in profiles/attn_beside_codec.txt)
    int tile_min_rows = 33;     // forwards with at least this many rows take the LDS-tiled GEMM (gemm_tile_kernels.h); 0 = never
    int tile_force = -1;        // TTS_HIP_TILE_FORCE: tile shape index for every tiled GEMM (tuning)
    int tile_force_ks = 0;      // TTS_HIP_TILE_KS: k slices for the residual GEMMs (tuning)
    uint64_t tile_launches = 0; // gemm_tile_kernel launches of this context so far (launch_tile_form)
    const void *aq_src = nullptr;  // activation rows whose Q8_0 blocks already sit in aq / ad (written by the producing kernel)
    // many rows on quantised matrices (qgemm_tile_kernels.h): activation block scales transposed, float [max(H, F) / 32][ldr]
    float *adT = nullptr;
    int ldr = 0;
    int8_t *aq2 = nullptr;      // second set: blocks written by a GEMM epilogue (GELU output, attended cross rows) while that GEMM reads the first
    float *adT2 = nullptr;
    int aqt_set = 0;            // which set holds the blocks of aqt_src
    int qtile_min_rows = 65;    // tune("qtile_min_rows"): forwards with at least this many rows take the LDS-tiled integer GEMM; 0 = never (the 16-feature kernel, <= 256 rows)
    int qtile_shape = -1;       // tune("qtile_shape"): tile shape index for every tiled integer GEMM (tuning / tests)
    int qtile_big = 0;          // tune("qtile_big"): tile shape of the GEMMs with at least two 64 x 64 tiles per CU (0: 64 x 64; 1: 128 x 128; 2: 128 x 64; 3: 64 x 128)
    int qtile_ks = 0;           // tune("qtile_ks"): k slices of the residual GEMMs (tuning / tests)
    bool qtile_fuse = true;     // tune("qtile_fuse")=0: LayerNorm, GELU and the attentions hand fp32 rows to a quantising launch of their own instead of writing Q8_0 blocks themselves
    const void *aqt_src = nullptr; // activation rows whose Q8_0 blocks already sit in aq / adT
    QTileOut qtile_out;         // request for the next run_gemm: Q8_0 output (EPI_GELU / EPI_CROSS on the tiled integer path); cleared by it
    int attn_fold = 1;          // tune("attn_fold") = 0: Dia's step keeps attn_gqa_combine_kernel and silu_mul_kernel as launches of their own.  1 (default): the consuming
                                // projections merge the attention's key slices / apply silu * up while they stage their rows (gemv_stream_kernel<.., PRO_ATTN8 / PRO_SILU, ..>)
    bool cross_fold = true;     // tune("cross_fold")=0: the cross-attention of a many-row forward stays a launch of its own (attn_short_kernel) instead of the cross-q GEMM's epilogue
    bool cross_folded = false;  // set by run_gemm: the EPI_CROSS request was served by the 64 x 64 tile
    bool attn_wave = true;      // tune("attn_wave")=0: the split decode attention of a Llama step and the cross-attention of a Dia step through the SPLIT form of attn_gqa_kernel (rounds 2-4) instead of attn_gqa_wave_kernel
    int attn_split_max = 8;     // tune("attn_split"): key splits of the decode attention of the Llama / Dia steps (1 = off)
    float *attn_part = nullptr; // [rows][heads][splits][130] partial softmax results
    size_t attn_part_cap = 0;   // in (row, head, split) triples
    int tile_deep = 1;          // tune("tile_deep")=0: always the 64-wide k-tiles / 4 buffers form (half the LDS per workgroup)
    int tile_pair = -1;         // tune("tile_pair") / TTS_HIP_TILE_PAIR: tile forms of at most 72 KB of LDS and 80 VGPRs, so that a GEMM workgroup fits a CU beside another one (of this
                                // context's launch or of another context's) or beside a codec workgroup.  0 = off; 1 = 128 x 128 tiles with two 64-wide buffers (64 KB), 128 x 64 with
                                // three (72 KB), the smaller shapes as under tile_deep = 0; 2 = as 1, a 128 x 128 choice takes 128 x 64 tiles instead.  Same k order per output element:
                                // the same bits.  -1 (default): 1 when another context reads this context's weight arena (the runners of one device), else 0, decided at the first
                                // tiled launch (tile_pair_of, shim_decoder.hip): a captured step keeps its kernels.  Measured in profiles/gemm_two_per_cu.txt
    int tile_pair_auto = -1;    // what the default came to: -1 until the first tiled launch, then 0 or 1; tune("tile_pair") resets it
    int tile_lds_max = 0;       // the most LDS in bytes a tiled GEMM launch asked for since tune("tile_pair") (debug_read "tile_pair": the tests' "which forms ran")
    bool dac_f16 = false;      // every codec conv kernel arrived as F16: fp16 im2col x fp16 kernel, fp32 accumulate (ggml)
    bool dac_packed = false;

    // graphs
    std::map<int, hipGraphExec_t> graphs;

    // profiling
    bool prof = false;       // full per-launch event timing: forwards run eagerly
    bool prof_light = false; // event pairs only around launches that are never graph-captured (the DAC)
    std::vector<ProfEv> prof_events;
    bool prof_cur = false;
    tts_hip_kstat kstat[TTS_HIP_K_COUNT]{};
    int attn_nsplit_override = 0;
    // batch-1 chain (<= 4 rows; timeline in profiles/r03/b1_chain.txt):
    bool b1_fc2_split = true;        // tune("b1_fc2_split")=0: fc2 stays 64 workgroups x 128 KB of weights (7.4 us) instead of 256 x 32 KB writing four K-slice slabs
    bool b1_defer_combine = true;    // tune("b1_defer_combine")=0: the split-T self-attention folds its partials itself (last workgroup, +3.3 us) instead of out_proj's prologue
    bool b1_stamps_want = false;     // tts_hip_tune("b1_stamps") or TTS_HIP_B1_STAMPS=1 before finalize
    long long *b1_stamps = nullptr;  // TTS_HIP_B1_STAMPS=1: 16 s_memrealtime stamps per launch of a <= 4-row forward (debug_read "stamps", profiles/b1_chain.py)
    int b1_stamp_slot = 0;
    bool attn_fused = true;          // tune("attn_fused")=0: split-T self-attention keeps its separate combine launch and small batches stay unsplit
    uint32_t *attn_cnt = nullptr;    // [RMAX][heads] arrival counters of the fused combine (attn_kernel)
};

// One captured graph: begin-capture on the context's stream, `enqueue` (a callable returning 0 or an error code), end-capture, instantiate.
// The exec is kept in c->graphs under `key` and handed back.  What has to run outside a capture (an eager pass that sets per-kernel
// attributes) is the caller's business.
template <class F>
static int capture_graph(tts_hip_ctx *c, int key, F enqueue, hipGraphExec_t *out) {
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    const hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (rc != 0 || e != hipSuccess) {
        if (graph) (void) hipGraphDestroy(graph);
        return rc != 0 ? rc : set_err("hipStreamEndCapture: %s", hipGetErrorString(e));
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void) hipGraphDestroy(graph);
    if (ei != hipSuccess) return set_err("hipGraphInstantiate: %s", hipGetErrorString(ei));
    c->graphs.emplace(key, exec);
    *out = exec;
    return 0;
}

// Orpheus contexts of more than LLAMA_STREAM_ROWS slots carry forwards of 65 .. LLAMA_MAX_SEQS rows: their quantised matrices get the transposed scale
// tables and the forward routes those rows to qgemm_tile_kernel.  Contexts of at most 64 slots plan, allocate and launch what they always have.
enum { LLAMA_STREAM_ROWS = 64, LLAMA_MAX_SEQS = 256 };
static inline bool llama_many_rows(const tts_hip_ctx *c) { return c->has_llama && c->lm.max_seqs > LLAMA_STREAM_ROWS; }

// ---- shim_core.hip
void free_dev(void *p);
template <typename T>
static int dmalloc(T **p, size_t n) {   // n zeroed elements
    HIPCHK(hipMalloc((void **) p, n * sizeof(T)));
    HIPCHK(hipMemset(*p, 0, n * sizeof(T)));
    return 0;
}
// Buffers that grow when a call asks for more than they hold.  The buffers of a group share one capacity, in elements: all are freed and nulled
// and the capacity zeroed BEFORE `need` elements of each are allocated, and the capacity is recorded only once all exist, so a failed
// allocation leaves (NULL, 0) and never a stale capacity.  Nothing is synchronised (a caller whose stream may still read the old buffer does
// that first); *moved says whether the addresses changed, for callers whose captured graphs hold them.  pinned(&p): a host-pinned member.
template <class T> struct PinnedRef { T **p; };
template <class T> static PinnedRef<T> pinned(T **p) { return {p}; }
template <class T> static void buf_release(T **p) { free_dev(*p); *p = nullptr; }
template <class T> static void buf_release(PinnedRef<T> h) { if (*h.p) (void) hipHostFree(*h.p); *h.p = nullptr; }
template <class T> static hipError_t buf_alloc(T **p, size_t n) { return hipMalloc((void **) p, n * sizeof(T)); }
template <class T> static hipError_t buf_alloc(PinnedRef<T> h, size_t n) { return hipHostMalloc((void **) h.p, n * sizeof(T)); }
template <class Cap, class... B>
static int grow_bufs(Cap *cap, size_t need, bool *moved, B... bufs) {
    if (moved) *moved = false;
    if (need <= (size_t) *cap) return 0;
    (buf_release(bufs), ...);
    *cap = 0;
    if (moved) *moved = true;
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? buf_alloc(bufs, need) : e), ...);
    if (e != hipSuccess) return set_err("growing a buffer to %zu elements -> %s", need, hipGetErrorString(e));
    *cap = (Cap) need;
    return 0;
}
template <class T, class Cap> static int grow_dev(T **p, Cap *cap, size_t need, bool *moved = nullptr) { return grow_bufs(cap, need, moved, p); }
template <class T, class Cap> static int grow_pinned(T **p, Cap *cap, size_t need) { return grow_bufs(cap, need, nullptr, pinned(p)); }
void arena_own(tts_hip_ctx *c);
void arena_share(tts_hip_ctx *c);
int arena_sharers(tts_hip_ctx *c);   // contexts that hold a reference on c's arena (1: c alone)
void arena_release(tts_hip_ctx *c);
bool starts_with(const std::string &s, const char *pre);
int plan(tts_hip_ctx *c);
// ---- shim_decoder.hip (launch plumbing, the Parler forward, generation loop)
bool attr_needed(std::atomic<uint64_t> &done, int device);
int prof_begin(tts_hip_ctx *c, int kclass, double bytes, double flops);
int prof_end(tts_hip_ctx *c);
int dia_tiled_buffers(tts_hip_ctx *c);   // di_h16 once tune("dia_tile_min_rows") is above 0 (finalize, or the tune call after it)
int ready(tts_hip_ctx *c, const char *who);
int stage_uniforms(tts_hip_ctx *c, const float *uniforms, size_t count);
int stage_penalty(tts_hip_ctx *c, float penalty, int n);
// ---- shim_qtile.hip (the tiled integer GEMM: its own unit, built without SLP vectorisation and with MFMA results in VGPRs)
int qtile_transpose_scales(tts_hip_ctx *c, const W &w);
int qtile_quant_rows(tts_hip_ctx *c, const float *x, int lda, int K, int R);   // fp32 rows -> Q8_0 blocks in c->aq / c->adT
// ---- shim_codec.hip
int dac_row_stride(const tts_hip_ctx *c, int L);

