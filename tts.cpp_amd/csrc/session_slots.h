// session_slots.h — the host bookkeeping every continuous session shares: which slot holds what (SlotLedger), the check of a caller's slot
// list, and the repetition-penalty table.  No HIP in here: tests/session_slots_main.cpp builds it with the host compiler alone.
#pragma once
#include <stdint.h>
#include <math.h>
#include <vector>

int set_err(const char *fmt, ...);   // keeps the message, returns non-zero

// pow(penalty, count) for count = 0 .. len-1 in double with the host libm: the arithmetic sampler.cpp:90 performs, and the one place csrc/
// evaluates it (the device only ever reads the table).  Bit parity with the reference sampler rests on this being libm's double pow.
static inline void penalty_table(double *dst, float penalty, int len) {
    for (int k = 0; k < len; k++) dst[k] = pow((double) penalty, (double) k);
}

// A caller's list of n slots against the per-slot states: in range, in a state of `allowed` (bit s = state s passes), named once — in that order
// per entry, all n before the caller changes anything.  `ge` and `refused` are the pieces of the texts that differ between the sessions.
static inline int check_slot_list(const char *what, uint32_t n, const uint32_t *slots, const std::vector<uint8_t> &state, unsigned allowed, const char *ge,
                                  const char *refused) {
    for (uint32_t i = 0; i < n; i++) {
        if (slots[i] >= state.size()) return set_err("%s: slot %u %s %u", what, slots[i], ge, (uint32_t) state.size());
        if (!((allowed >> state[slots[i]]) & 1u)) return set_err("%s: slot %u %s", what, slots[i], refused);
        for (uint32_t j = 0; j < i; j++) if (slots[j] == slots[i]) return set_err("%s: slot %u named twice", what, slots[i]);
    }
    return 0;
}

// The slots of a device-driven session (Orpheus, Dia).  An admission makes a slot LIVE, a look-in that finds it finished ENDED, the report of
// that REPORTED; a collect reads a REPORTED slot, a drop or the next admission frees it.
struct SlotLedger {
    enum : uint8_t { FREE = 0, LIVE = 1, ENDED = 2, REPORTED = 3 };   // ENDED: seen finished by a look-in, not yet reported
    enum Want { ADMIT, DROP };
    std::vector<uint8_t> slot;   // per slot, one of the above
    uint32_t in_flight = 0;      // steps enqueued by a launch that no look-in has waited for
    uint32_t unread = 0;         // steps enqueued since the last look-in that took rows: bounds what a look-in can find

    // between a launch and its wait the steps may still be running: nothing else touches the session
    int idle(const char *what, const char *wait_name) const {
        return in_flight ? set_err("%s: %u steps are in flight (%s first)", what, in_flight, wait_name) : 0;
    }
    int check_list(const char *what, uint32_t n, const uint32_t *slots, Want want) const {
        return want == ADMIT ? check_slot_list(what, n, slots, slot, (1u << FREE) | (1u << REPORTED),">= n_slots", "is busy")
                             : check_slot_list(what, n, slots, slot, 1u << LIVE, ">= n_slots", "is not live");
    }
    // slots a look-in saw finished and no call has reported yet, in slot order, with counts[slot]
    void report(const std::vector<uint32_t> &counts, uint32_t *n_finished, uint32_t *finished_slots, uint32_t *finished_counts) {
        *n_finished = 0;
        for (uint32_t s = 0; s < slot.size(); s++) {
            if (slot[s] != ENDED) continue;
            finished_slots[*n_finished] = s;
            finished_counts[*n_finished] = counts[s];
            (*n_finished)++;
            slot[s] = REPORTED;
        }
    }
    // a collect of `asked` entries from a reported slot; "<verb> %u <unit>" is the model's wording ("produced %u ids", "made %u steps")
    int check_collect(const char *what, uint32_t s, uint32_t asked, const std::vector<uint32_t> &counts, const char *run_name, const char *verb, const char *unit) const {
        if (s >= slot.size()) return set_err("%s: slot %u >= n_slots %u", what, s, (uint32_t) slot.size());
        if (slot[s] != REPORTED) return set_err("%s: slot %u has not finished (%s reports it)", what, s, run_name);
        if (asked > counts[s]) return set_err("%s: slot %u %s %u %s, %u asked for", what, s, verb, counts[s], unit, asked);
        return 0;
    }
};
