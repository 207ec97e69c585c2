// chunk_windows.h — chunked audio, the host arithmetic the three streaming runners share: where the next codec window of an utterance is cut,
// how a pass' PCM is handed out chunk by chunk, and the DAC chunker of the Parler and Dia runners.
//
// A codec's samples of frame j depend on the codes of frames [j - h, j + h] only (tts_hip_dac_halo_frames / tts_hip_snac_halo_frames).  So once
// frames [e, f + h) of an utterance are final, the window [e - h, f + h) decoded as an utterance of its own yields the samples of [e, f) exactly
// as the whole utterance's decode does; at the utterance's true edges the window is clipped and sees the same zero padding.  Frames are counted
// as the codec sees them: after the un-delay dropped the ones with a non-audio id in them (Parler, Dia), in groups of 7 ids (Orpheus).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/tts_hip.h"
#include "common.h"

// ---- the cut ---------------------------------------------------------------------------------------------------------------------------------
// Of an utterance with `have` final frames of which `emitted` are out: the kept frames [emitted, end) are the whole chunks whose right halo is
// final too, or everything left once the utterance has ended (end == emitted: nothing to cut yet).  They are decoded inside the window
// [w0, w1) = [emitted - halo, end + halo) clipped to the utterance; keep0 / keep1 mark them inside the window, as the codec's window pass takes them.
struct chunk_window { uint32_t end, w0, w1, keep0, keep1; };

inline chunk_window cut_chunk_window(uint32_t emitted, uint32_t have, uint32_t halo, uint32_t chunk_frames, bool ended) {
    uint32_t end = emitted;
    if (ended) end = std::max(have, emitted);
    else if ((uint64_t) have >= (uint64_t) emitted + halo + chunk_frames) end = emitted + (have - halo - emitted) / chunk_frames * chunk_frames;
    const uint32_t w0 = emitted > halo ? emitted - halo : 0, w1 = (uint32_t) std::min<uint64_t>((uint64_t) end + halo, have);
    return {end, w0, w1, emitted - w0, end - w0};
}

// ---- the hand-out ----------------------------------------------------------------------------------------------------------------------------
// The PCM of one window pass (the windows' kept frames back to back, `per` samples a frame) to to(window, samples, count), every window in pieces
// of at most chunk_frames frames; a false ends that window.
template <class To>
void hand_out_windows(const std::vector<uint32_t> & keep0, const std::vector<uint32_t> & keep1, uint32_t chunk_frames, size_t per, const float * pcm, To && to) {
    size_t off = 0;
    for (size_t w = 0; w < keep0.size(); w++) {
        const uint32_t nf = keep1[w] - keep0[w];
        bool more = true;
        for (uint32_t f = 0; f < nf && more; f += std::min(chunk_frames, nf - f)) more = to(w, pcm + off + (size_t) f * per, (size_t) std::min(chunk_frames, nf - f) * per);
        off += (size_t) nf * per;
    }
}

// a generation's policy (run_rows, run_utterances, chunk_run): window w belongs to row row_of[w]; a false stops the whole generation, so nothing
// after it is handed out.  Returns whether to go on.
inline bool hand_out_rows(const std::vector<uint32_t> & keep0, const std::vector<uint32_t> & keep1, const std::vector<uint32_t> & row_of, uint32_t chunk_frames,
                          size_t per, const float * pcm, const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) {
    bool go = true;
    hand_out_windows(keep0, keep1, chunk_frames, per, pcm, [&](size_t w, const float * p, size_t k) { return go = go && on_chunk(row_of[w], p, k); });
    return go;
}

// a session's policy: window w belongs to the utterance key_of[w] (a ticket, or a slot that keeps its occupant until the last piece is out); a
// false ends that utterance only — its key goes into `stopped`, it gets nothing more and the other windows go on
inline void hand_out_session(const std::vector<uint32_t> & keep0, const std::vector<uint32_t> & keep1, const std::vector<size_t> & key_of, uint32_t chunk_frames,
                             size_t per, const float * pcm, const std::function<bool(size_t, const float *, size_t)> & to, std::vector<size_t> & stopped) {
    hand_out_windows(keep0, keep1, chunk_frames, per, pcm, [&](size_t w, const float * p, size_t k) {
        if (std::find(stopped.begin(), stopped.end(), key_of[w]) != stopped.end()) return false;
        if (to(key_of[w], p, k)) return true;
        stopped.push_back(key_of[w]);
        return false;
    });
}

// ---- the DAC chunker (parler_runner, dia_runner) -----------------------------------------------------------------------------------------------
// A generation loop calls it at its look-ins: plan() un-delays the frames of every row that became final and cuts the next windows, decode()
// sends them through the codec in one tts_hip_dac_decode_windows pass — on the codec's stream, while the decoder's next steps run — and the
// emit_* forms hand the chunks out.  The rows are a batch's utterances or a session's slots.
struct dac_chunker {
    // the runner's un-delay rule from a cursor: judges the frames of toks [steps][heads] that are final and not judged yet (`finished`: the
    // generation is over), appends the kept ones' codes and returns the new cursor (parler_undelay, dia_undelay)
    using undelay_fn = std::function<size_t(const uint32_t * toks, size_t steps, size_t judged, bool finished, std::vector<uint32_t> & kept)>;
    struct row {
        std::vector<uint32_t> frames;     // codes of the kept frames that are final [frames][heads]
        size_t   judged = 0;              // the rule's cursor
        uint32_t emitted = 0;             // kept frames handed out
    };
    const undelay_fn     undelay;
    const uint32_t       heads, up, halo, chunk_frames;   // up: samples per frame; halo: the utterance's maximum length where the layout's is unknown (whole utterances once they are done)
    tts_hip_ctx * const  codec;                           // nullptr: plan() only (tts_c_chunk_windows)
    std::vector<float> & pcm;                             // the runner's output buffer
    std::vector<row>      rows;
    std::vector<uint32_t> codes, frames, keep0, keep1, row_of;   // the planned windows: one tts_hip_dac_decode_windows pass
    dac_chunker(undelay_fn rule, uint32_t heads_, uint32_t up_, uint32_t halo_, uint32_t chunk_frames_, tts_hip_ctx * codec_, std::vector<float> & pcm_)
        : undelay(std::move(rule)), heads(heads_), up(up_), halo(halo_), chunk_frames(chunk_frames_), codec(codec_), pcm(pcm_) {}

    void plan(const std::vector<std::vector<uint32_t>> & toks, const std::vector<bool> & finished) {
        rows.resize(toks.size());
        for (uint32_t i = 0; i < toks.size(); i++) {
            row & r = rows[i];
            r.judged = undelay(toks[i].data(), toks[i].size() / heads, r.judged, finished[i], r.frames);
            const chunk_window c = cut_chunk_window(r.emitted, (uint32_t) (r.frames.size() / heads), halo, chunk_frames, finished[i]);
            if (c.end == r.emitted) continue;
            codes.insert(codes.end(), r.frames.begin() + (size_t) c.w0 * heads, r.frames.begin() + (size_t) c.w1 * heads);
            frames.push_back(c.w1 - c.w0);
            keep0.push_back(c.keep0);
            keep1.push_back(c.keep1);
            row_of.push_back(i);
            r.emitted = c.end;
        }
    }
    void clear() { codes.clear(); frames.clear(); keep0.clear(); keep1.clear(); row_of.clear(); }
    // the planned windows through the codec into pcm, window after window; false: nothing was planned
    bool decode() {
        if (row_of.empty()) return false;
        size_t total = 0;
        for (size_t w = 0; w < row_of.size(); w++) total += (size_t) (keep1[w] - keep0[w]) * up;
        pcm.resize(total);
        hip_check(tts_hip_dac_decode_windows(codec, codes.data(), frames.data(), keep0.data(), keep1.data(), (uint32_t) row_of.size(), pcm.data()),
                  "tts_hip_dac_decode_windows");
        return true;
    }
    // decode, then hand_out_rows with a window's row; false: the caller stopped the generation
    bool emit_rows(const std::function<bool(uint32_t, const float *, size_t)> & on_chunk) {
        const bool go = !decode() || hand_out_rows(keep0, keep1, row_of, chunk_frames, up, pcm.data(), on_chunk);
        clear();
        return go;
    }
    // decode, then hand_out_session with key_of[w] the utterance of planned window w
    void emit_session(const std::vector<size_t> & key_of, const std::function<bool(size_t, const float *, size_t)> & to, std::vector<size_t> & stopped) {
        if (decode()) hand_out_session(keep0, keep1, key_of, chunk_frames, up, pcm.data(), to, stopped);
        clear();
    }
};
