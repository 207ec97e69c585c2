// parler_session.h — the chunk hook of the Parler continuous session (common.h: "chunked audio out of a session").
//
// A small base between tts_generation_runner and parler_runner: it declares the override of the session's chunk hook and keeps what the hook
// stores, the chunk size and the callback.  parler_runner stays final and does the work in stream_step (parler_runner.h, "chunked audio out
// of the session").
#pragma once
#include <functional>

#include "common.h"

struct parler_session : tts_generation_runner {
    using tts_generation_runner::tts_generation_runner;

    // Between stream_begin and the first stream_submit.  chunk_frames counts codec frames (up_sampling_factor samples each); 0 aborts.  Returns
    // false when the codec layout reports no halo, or when TTS_PARLER_STREAM_CHUNKS is not set in the environment (session_chunks_ready): the
    // session then hands out whole utterances, as it does without the hook.  The switch is an opt-in because the whole-utterance answer is
    // what generate_stream_chunked has given for a Parler runner so far.
    bool stream_chunks(uint32_t chunk_frames, std::function<bool(size_t ticket, const float *, size_t)> on_chunk) override;

  protected:
    uint32_t                                           st_chunk_frames = 0;   // 0: no hook, stream_step hands out whole utterances
    std::function<bool(size_t, const float *, size_t)> st_on_chunk;
    // the runner's part of the hook: aborts unless a session is open and empty; false: this session cannot cut windows; true: its per-slot
    // chunk state is set up for chunk_frames
    virtual bool session_chunks_ready(uint32_t chunk_frames) = 0;
};
