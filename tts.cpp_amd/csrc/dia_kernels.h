// dia_kernels.h — the pieces of the Dia step that are not shared with the Orpheus decoder (llama_kernels.h: rms norm,
// NEOX rope + cache append, grouped-query attention with key ranges, silu*up) or the GEMMs (parler_kernels.h).
//   dia_embed_kernel   build_dia_decoder_inp_embd: sum of the n_out codebook embeddings, the same row for both streams
//                      (/root/reference/src/models/dia/model.cpp:337-350, set_inputs :724-726)
//   dia_cfg_kernel     cfg_scale map at the end of the graph: cond + scale * (cond - uncond) (src/util.cpp:175-200; the
//                      "r > max_output -> -inf" statement there is overwritten by the next one, so nothing is masked)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "parler_kernels.h"   // SampleRow: the per-slot sampler record of a mixed session

struct DiaEmbedArgs {
    const float *table[16];   // [V][H] fp32 each
    const uint32_t *ids;      // [n_utt][n_out]
    int n_out, H;
    float *x;                 // [2 * n_utt][H]: rows 2u (text stream) and 2u+1 (all-zero twin) of utterance u get the same embedding
};

static __global__ __launch_bounds__(256) void dia_embed_kernel(DiaEmbedArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
    if (e >= a.H) return;
    float acc = 0.0f;
    for (int i = 0; i < a.n_out; i++) {   // embds[0] first, then embds[i] + running (:343-347)
        const float v = a.table[i][(int64_t) a.ids[u * a.n_out + i] * a.H + e];
        acc = i == 0 ? v : v + acc;
    }
    a.x[(int64_t) (2 * u) * a.H + e] = acc;
    a.x[(int64_t) (2 * u + 1) * a.H + e] = acc;
}

// raw [2 * n_utt][ld] (ld >= n: the fused heads are padded to a multiple of 16 rows) -> guided [n_utt][n]; blockIdx.y = utterance
static __global__ __launch_bounds__(256) void dia_cfg_kernel(const float *raw, int ld, int n, float scale, float *guided) {
    const int i = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
    if (i >= n) return;
    const float cr = raw[(int64_t) (2 * u) * ld + i], ur = raw[(int64_t) (2 * u + 1) * ld + i];
    guided[(int64_t) u * n + i] = cr + scale * (cr - ur);
}

// [R][ld] fp32 -> [R][K] fp16 (round to nearest even): the rounding ggml_mul_mat applies to the activations of an F16-weight product
// (vec_dot_type conversion of src1), done once here so that the encoder's 2 x 1024 rows can go through gemm_tile_kernel
static __global__ __launch_bounds__(256) void rows_to_f16_kernel(const float *x, int ld, int K, int64_t n8, _Float16 *y) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;   // one thread = 8 consecutive values
    if (i >= n8) return;
    const int64_t r = i / (K >> 3), c8 = i - r * (K >> 3);
    const float4 a = *(const float4 *) (x + r * ld + c8 * 8), b = *(const float4 *) (x + r * ld + c8 * 8 + 4);
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    h8 h;
    h[0] = (_Float16) a.x; h[1] = (_Float16) a.y; h[2] = (_Float16) a.z; h[3] = (_Float16) a.w;
    h[4] = (_Float16) b.x; h[5] = (_Float16) b.y; h[6] = (_Float16) b.z; h[7] = (_Float16) b.w;
    *(h8 *) (y + r * K + c8 * 8) = h;
}

// ------------------------------------------------------------------------------------------------
// device-resident generation loop (dia_runner::generate_from_batch, dia/model.cpp:806-870 with check_stopping :767-785 and the
// delay-pattern feedback :795-803): one thread per utterance slot keeps what the host loop keeps — the n_out input ids, the position,
// the countdown, the sampled history — so that a step (pre-step, forward, guidance, sampler, post-step) replays as one hipGraph and
// neither logits nor ids cross PCIe inside the loop.  One loop serves the fixed batch (tts_hip_dia_gen_*, tts_hip_dia_generate: n
// encoded slots, all live from the first step, each with the budget max_gen) and the continuous session (tts_hip_dia_stream_*: n slots
// that utterances enter and leave while the others keep going).  What differs per slot and per occupant lives in device memory, so an
// admission never drops the captured graph:
//   budget[u]   the occupant's max_gen (max_delay < budget <= max_gen of the loop); the history stride stays the loop's max_gen
//   steps[u]    sampler calls the occupant made, written when the slot parks (its position does not survive parking)
//   done[u]     the parked flag: set when the countdown ends, set for every slot by a session's begin, cleared by an admission
// Parking: the pre-step that ends a countdown moves both rows of the slot to position 0 and their cross extent to one key, so from that
// step on the slot's self-attention and cross-attention read one position each while its rows stay in the step (lock-step shapes stay
// fixed); the post-step records nothing for it and sample_kernel leaves its state alone (SampleArgs::idle).  Whoever leaves the loop
// sets the cross extents back to the whole text context.
//   dia_loop_prestep_kernel   check_stopping before each decode: start the countdown when head 0 produced EOS or the position reaches
//                             budget - max_delay; during it force EOS / PAD into the heads whose delay has passed; park the slot when
//                             the countdown reaches 0.  Also publishes the 1-based sampler call index of this step.
//   dia_loop_poststep_kernel  record the sampled ids, advance the position (both guidance rows), feed head i its id once pos > i, BOS before.
//   dia_loop_lookin_kernel    the look-in: {sampler calls, parked flag, the history rows no earlier look-in took} of every slot into one block
//   dia_stream_admit_kernel   one launch for all admitted slots: loop state and sampler state reset, uniforms into the slot's column; in a
//                             mixed session also the occupant's sampler record and its own penalty table
//   dia_stream_clear_kernel   begin: zero cross K/V at position 0 of the slots no encoder pass has filled (what their parked rows attend over)
//   dia_stream_drop_kernel    parks live slots at once, between a look-in and the next step (what the parking pre-step writes)
// ------------------------------------------------------------------------------------------------
struct DiaLoopArgs {
    int n_utt, n_out;
    uint32_t bos, eos, pad, max_delay, max_gen;
    uint32_t delay_pattern[16];
    uint32_t *ids;        // [n_utt][n_out] the step's input ids (audio_tokens of the host loop)
    uint32_t *pos;        // [2 * n_utt] position of rows 2u, 2u+1
    int32_t *delay;       // [n_utt] countdown, -1 = not started
    uint32_t *done;       // [n_utt]
    uint32_t *call;       // [n_utt] 1-based index of the sampler call this step makes (sample_kernel's row_step)
    const uint32_t *tok;  // [n_utt][n_out] ids the sampler produced this step
    uint32_t *hist;       // [n_utt][max_gen][n_out]
    const uint32_t *budget;   // [n_utt]
    uint32_t *steps;          // [n_utt]
    uint32_t *cend;           // [2 * n_utt] cross-attention extent of rows 2u, 2u+1
};

static __global__ void dia_loop_prestep_kernel(DiaLoopArgs a) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.n_utt || a.done[u]) return;
    uint32_t *aud = a.ids + u * a.n_out;
    const uint32_t p = a.pos[2 * u];
    int d = a.delay[u];
    if (d == -1 && (aud[0] == a.eos || p >= a.budget[u] - a.max_delay)) d = (int) a.max_delay;
    if (d > 0) {
        const int after = (int) a.max_delay - d;
        for (int i = 0; i < a.n_out; i++) {
            if (after == (int) a.delay_pattern[i]) aud[i] = a.eos;
            else if (after > (int) a.delay_pattern[i]) aud[i] = a.pad;
        }
        d -= 1;
    }
    a.delay[u] = d;
    a.call[u] = p + 1;
    if (d == 0) {   // park: this step's forward already reads one position per attention
        a.done[u] = 1;
        a.steps[u] = p;
        a.pos[2 * u] = 0; a.pos[2 * u + 1] = 0;
        a.cend[2 * u] = 1; a.cend[2 * u + 1] = 1;
        a.call[u] = 1;
    }
}

static __global__ void dia_loop_poststep_kernel(DiaLoopArgs a) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.n_utt || a.done[u]) return;
    const uint32_t p = a.pos[2 * u];
    for (int i = 0; i < a.n_out; i++) a.hist[((int64_t) u * a.max_gen + p) * a.n_out + i] = a.tok[u * a.n_out + i];
    const uint32_t np = p + 1;
    a.pos[2 * u] = np;
    a.pos[2 * u + 1] = np;
    for (int i = 0; i < a.n_out; i++) a.ids[u * a.n_out + i] = np > (uint32_t) i ? a.tok[u * a.n_out + i] : a.bos;
}

// A look-in: one workgroup per slot packs {sampler calls so far, parked flag, the history rows no earlier look-in took} into its slot of
// one contiguous block, so that the host learns everything from one launch, one copy and one synchronisation however many slots there
// are.  The count so far is steps[u] once the slot has parked (parking moved its position to 0).  A session slot's rows restart at 0 with
// every admission (dia_stream_admit_kernel resets handed[u]); the rows of a parked slot stay in hist until then, so a look-in after the
// parking step still finds them.  take = 0: the header only (the rows stay for a later look-in).
struct DiaLookArgs {
    int n_utt, n_out;
    uint32_t max_gen;
    uint32_t cap;            // rows a slot holds: the steps enqueued since the last look-in that took rows
    int take;
    const uint32_t *pos;     // [2 * n_utt]
    const uint32_t *done;    // [n_utt]
    const uint32_t *steps;   // [n_utt]
    const uint32_t *hist;    // [n_utt][max_gen][n_out]
    uint32_t *handed;        // [n_utt] history rows taken so far
    uint32_t *block;         // [n_utt][2 + cap * n_out]
};

static __global__ __launch_bounds__(64) void dia_loop_lookin_kernel(DiaLookArgs a) {
    const int u = blockIdx.x;
    if (u >= a.n_utt) return;
    const uint32_t parked = a.done[u];
    const uint32_t from = a.handed[u], to = min(parked ? a.steps[u] : a.pos[2 * u], a.max_gen);
    const uint32_t rows = a.take && to > from ? min(to - from, a.cap) : 0u;
    uint32_t *slot = a.block + (int64_t) u * (2 + (int64_t) a.cap * a.n_out);
    const uint32_t *src = a.hist + ((int64_t) u * a.max_gen + from) * a.n_out;
    for (uint32_t i = threadIdx.x; i < rows * (uint32_t) a.n_out; i += blockDim.x) slot[2 + i] = src[i];
    __syncthreads();   // every thread has read handed[u]
    if (threadIdx.x == 0) {
        slot[0] = to;   // sampler calls made so far; the host derives `rows` from it as this kernel does
        slot[1] = parked;
        a.handed[u] = from + rows;
    }
}

struct DiaAdmitArgs {
    int n, n_slots, n_out;
    uint32_t bos, max_gen, max_ctx;
    const uint32_t *slots;    // [n]
    const uint32_t *budgets;  // [n]
    const float *uni_in;      // [n][max_gen][n_out] or NULL
    float *uni;               // [max_gen][n_slots][n_out] what sample_kernel reads
    int32_t *last;            // [n_slots][n_out] or NULL (no repetition penalty)
    uint32_t *repc;
    uint32_t *ids, *pos, *done, *call, *handed, *budget, *steps, *cend;
    int32_t *delay;
    // a mixed session (tts_hip_dia_stream_admit_mixed): the occupant's sampler record and its own penalty table move into the slot's places
    // (rec_in NULL: a uniform session, the sampler is the launch's)
    const SampleRow *rec_in;  // [n]; pen_table already points at the slot's table, or is NULL (penalty 1, or sampler::max)
    SampleRow *rec;           // [n_slots] what sample_kernel reads
    const double *pen_in;     // [n][pen_len]
    double *pen;              // [n_slots][pen_len]
    int pen_len;
};

// blockIdx.y = admitted utterance; thread 0 of block x == 0 resets the slot, then admit_sampler_state (parler_kernels.h): all threads move its penalty table and its uniforms
static __global__ __launch_bounds__(256) void dia_stream_admit_kernel(DiaAdmitArgs a) {
    const int i = blockIdx.y;
    if (i >= a.n) return;
    const uint32_t u = a.slots[i];
    if (blockIdx.x == 0 && threadIdx.x < (unsigned) a.n_out) {
        a.ids[u * a.n_out + threadIdx.x] = a.bos;
        if (a.last) { a.last[u * a.n_out + threadIdx.x] = -1; a.repc[u * a.n_out + threadIdx.x] = 0; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.pos[2 * u] = 0; a.pos[2 * u + 1] = 0;
        a.cend[2 * u] = a.max_ctx; a.cend[2 * u + 1] = a.max_ctx;
        a.delay[u] = -1; a.done[u] = 0; a.call[u] = 1; a.handed[u] = 0;
        a.budget[u] = a.budgets[i]; a.steps[u] = 0;
    }
    admit_sampler_state(a.rec_in, a.rec, a.pen_in, a.pen, a.pen_len, a.uni_in, a.uni, a.max_gen, a.n_slots, a.n_out, i, u, a.uni_in != nullptr);
}

// cross K/V [L][rows][S][A] of KV = float or _Float16 elements (tts_hip_dia_desc::kv_type): position 0 of rows 2u, 2u+1 of the flagged slots.
// grid (ceil(A / 256), 2 * n_slots, L)
template <typename KV>
__global__ __launch_bounds__(256) void dia_stream_clear_kernel(KV *ck, KV *cv, uint64_t clear, int rows, int64_t S, int A) {
    const int e = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, l = blockIdx.z;   // clear: bit u = slot u of the launch's group of 64 (ck / cv start at the group's first row)
    if (e >= A || !((clear >> (r >> 1)) & 1)) return;
    const int64_t at = ((int64_t) l * rows + r) * S * A + e;
    ck[at] = (KV) 0.0f;
    cv[at] = (KV) 0.0f;
}

struct DiaDropArgs {
    int n;
    const uint32_t *slots;   // [n] distinct live slots
    uint32_t *pos, *done, *call, *steps, *cend;
};

// one thread per dropped slot: the values the parking pre-step writes.  The slot's history rows stay where they are.
static __global__ void dia_stream_drop_kernel(DiaDropArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t u = a.slots[i];
    if (a.done[u]) return;   // parked by the last step before the host saw it: steps[u] is already the occupant's
    a.steps[u] = a.pos[2 * u];
    a.done[u] = 1;
    a.pos[2 * u] = 0; a.pos[2 * u + 1] = 0;
    a.cend[2 * u] = 1; a.cend[2 * u + 1] = 1;
    a.call[u] = 1;
}
