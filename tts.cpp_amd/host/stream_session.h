// stream_session.h — what the continuous sessions of parler_runner, orpheus_runner and dia_runner have in common (common.h: "continuous batching",
// "chunked audio out of a session").
//
// A base between tts_generation_runner and the three runners, which stay final: the slot bookkeeping of an open session, the one override of
// the session's chunk hook, the submit that takes the session's own configuration, and the token records the tests read.  What differs stays
// in the runners: when a slot is free again, what stream_live() counts, where a submission is admitted, and every stream_step.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "common.h"

struct stream_session : tts_generation_runner {
    using tts_generation_runner::tts_generation_runner;
    using tts_generation_runner::stream_submit;

    // Between stream_begin and the first stream_submit.  chunk_frames counts codec frames (Orpheus: SNAC frames of 7 ids, 4 * snac_up samples);
    // 0 aborts.  Returns false when this session cannot cut windows (session_chunks_ready): it then hands out whole utterances, as it does
    // without the hook.
    bool stream_chunks(uint32_t chunk_frames, std::function<bool(size_t ticket, const float *, size_t)> on_chunk) override;
    // with the configuration the session was opened with
    void stream_submit(size_t ticket, const std::string & sentence) override { stream_submit(ticket, sentence, st_cfg); }

    // token records (tests, through tts_c_last_tokens): the last prompt, the last utterance's ids, and per utterance of the last batch or
    // chunked session.  A session keeps last_batch_tokens[ticket] only for tickets below TOKEN_RECORD_TICKETS.  A ticket is the caller's handle:
    // generate_stream_chunked numbers its sentences from 0, which the record is for; a host with its own queue may use any size_t (a request
    // id, a pointer), and the vector must not grow to it.
    static constexpr size_t TOKEN_RECORD_TICKETS = 4096;
    std::vector<uint32_t>              last_prompt_tokens, last_output_tokens;
    std::vector<std::vector<uint32_t>> last_batch_tokens;

  protected:
    bool                     st_on = false;
    generation_configuration st_cfg{};
    uint32_t                 st_live = 0;
    std::vector<uint32_t>    st_free;     // free slots
    std::vector<size_t>      st_ticket;   // slot -> ticket
    uint32_t                 st_chunk_frames = 0;   // 0: no hook, stream_step hands out whole utterances
    std::function<bool(size_t, const float *, size_t)> st_on_chunk;
    // the runner's part of the hook: aborts unless a session is open and empty; false: this session cannot cut windows; true: its per-slot
    // chunk state is set up for chunk_frames
    virtual bool session_chunks_ready(uint32_t chunk_frames) = 0;

    // stream_begin, once the device's session is open: every slot free, no hook
    void session_open(const generation_configuration & config, uint32_t slots) {
        st_cfg = config;
        st_free.clear();
        for (uint32_t s = slots; s-- > 0;) st_free.push_back(s);   // pop_back hands out slot 0 first
        st_ticket.assign(slots, 0);
        st_live = 0;
        st_chunk_frames = 0;
        st_on_chunk = nullptr;
        st_on = true;
    }
    void session_close() {
        st_on = false;
        st_free.clear();
        st_ticket.clear();
        st_live = 0;
        st_chunk_frames = 0;
        st_on_chunk = nullptr;
    }
    // an utterance of the session has ended (or was stopped): its ids, still delayed where the model delays them
    void remember_tokens(size_t ticket, const std::vector<uint32_t> & ids) {
        if (ticket < TOKEN_RECORD_TICKETS) {   // generate_stream_chunked's tickets are the sentence indices: last_batch_tokens[i] as after generate_batch
            if (last_batch_tokens.size() <= ticket) last_batch_tokens.resize(ticket + 1);
            last_batch_tokens[ticket] = ids;
        }
        last_output_tokens = ids;
    }
    // an utterance whose audio went through the hook, or that has none: its ticket, no audio
    static void report_no_audio(std::vector<stream_result> & finished, size_t ticket) {
        stream_result r;
        r.ticket = ticket;
        finished.push_back(r);
    }
};

inline bool stream_session::stream_chunks(uint32_t chunk_frames, std::function<bool(size_t, const float *, size_t)> on_chunk) {
    if (chunk_frames == 0) TTS_ABORT("stream_chunks: chunk_frames must be >= 1\n");
    if (!session_chunks_ready(chunk_frames)) return false;
    st_chunk_frames = chunk_frames;
    st_on_chunk = std::move(on_chunk);
    return true;
}
