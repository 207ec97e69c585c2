// orpheus_session.h — the chunk hook of the Orpheus continuous session (common.h: "chunked audio out of a session").
//
// A small base between tts_generation_runner and orpheus_runner: it declares the override of the session's chunk hook and keeps what the hook
// stores, the chunk size and the callback.  orpheus_runner stays final and does the work in stream_step (orpheus_runner.h, "chunked audio out
// of the session").
#pragma once
#include <functional>

#include "common.h"

struct orpheus_session : tts_generation_runner {
    using tts_generation_runner::tts_generation_runner;

    // Between stream_begin and the first stream_submit.  chunk_frames counts SNAC frames (7 ids, 4 * snac_up samples); 0 aborts.  Returns false
    // when the codec layout has no known halo (session_chunks_ready): the session then hands out whole utterances, as it does without the hook.
    bool stream_chunks(uint32_t chunk_frames, std::function<bool(size_t ticket, const float *, size_t)> on_chunk) override;

  protected:
    uint32_t                                           st_chunk_frames = 0;   // 0: no hook, stream_step hands out whole utterances
    std::function<bool(size_t, const float *, size_t)> st_on_chunk;
    // the runner's part of the hook: aborts unless a session is open and empty; false: this session cannot cut windows; true: its per-slot
    // chunk state is set up for st_chunk_frames
    virtual bool session_chunks_ready(uint32_t chunk_frames) = 0;
};
