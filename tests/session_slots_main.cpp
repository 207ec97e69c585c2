// The host bookkeeping of the continuous sessions (tts.cpp_amd/csrc/session_slots.h), without a device: slot-list validation with the texts
// the Orpheus, Dia and Parler entry points produce, report and collect, and the penalty table against libm's pow.  Exits non-zero at the
// first failed check.  Built and run by tests/test_session_slots_cpu.py.
#include "../tts.cpp_amd/csrc/session_slots.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static char g_err[512];
int set_err(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return -1;
}

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s (last message: %s)\n", __FILE__, __LINE__, #cond, g_err); exit(1); } \
    } while (0)

static bool refused(int rc, const char *text) { return rc != 0 && std::string(g_err) == text; }

static SlotLedger ledger(std::initializer_list<uint8_t> states) {
    SlotLedger g;
    g.slot.assign(states);
    return g;
}

static void slot_lists() {
    const char *adm = "tts_hip_orpheus_stream_admit", *drop = "tts_hip_dia_stream_drop";
    SlotLedger g = ledger({SlotLedger::FREE, SlotLedger::LIVE, SlotLedger::FREE});
    const std::vector<uint8_t> before = g.slot;
    {   // out of range, as the last of three: the two good ones before it change nothing
        const uint32_t s[3] = {0, 2, 3};
        CHECK(refused(g.check_list(adm, 3, s, SlotLedger::ADMIT), "tts_hip_orpheus_stream_admit: slot 3 >= n_slots 3"));
        CHECK(refused(g.check_list(drop, 3, s, SlotLedger::DROP), "tts_hip_dia_stream_drop: slot 0 is not live"));   // state of [0] before range of [2]
        const uint32_t far[1] = {0xFFFFFFFFu};
        CHECK(refused(g.check_list(drop, 1, far, SlotLedger::DROP), "tts_hip_dia_stream_drop: slot 4294967295 >= n_slots 3"));
    }
    {   // a busy slot as the second of two: nothing changed, and slot 0 is still admissible
        const uint32_t s[2] = {0, 1};
        CHECK(refused(g.check_list(adm, 2, s, SlotLedger::ADMIT), "tts_hip_orpheus_stream_admit: slot 1 is busy"));
        CHECK(g.slot == before);
        CHECK(g.check_list(adm, 1, s, SlotLedger::ADMIT) == 0);
    }
    {   // ENDED is busy too (finished, not yet reported); REPORTED is admissible (the admission collects over it)
        SlotLedger e = ledger({SlotLedger::ENDED, SlotLedger::REPORTED, SlotLedger::FREE});
        const uint32_t s[2] = {1, 0};
        CHECK(e.check_list(adm, 1, s, SlotLedger::ADMIT) == 0);
        CHECK(refused(e.check_list(adm, 2, s, SlotLedger::ADMIT), "tts_hip_orpheus_stream_admit: slot 0 is busy"));
    }
    {   // named twice: after range and state of the same entry
        const uint32_t s[3] = {2, 0, 2};
        CHECK(refused(g.check_list(adm, 3, s, SlotLedger::ADMIT), "tts_hip_orpheus_stream_admit: slot 2 named twice"));
        const uint32_t l[2] = {1, 1};
        CHECK(refused(g.check_list(drop, 2, l, SlotLedger::DROP), "tts_hip_dia_stream_drop: slot 1 named twice"));
    }
    {   // dropping a slot that is not live: FREE, ENDED and REPORTED alike
        const uint32_t s[2] = {1, 2};
        CHECK(refused(g.check_list(drop, 2, s, SlotLedger::DROP), "tts_hip_dia_stream_drop: slot 2 is not live"));
        CHECK(g.check_list(drop, 1, s, SlotLedger::DROP) == 0);
        SlotLedger e = ledger({SlotLedger::ENDED, SlotLedger::REPORTED, SlotLedger::LIVE});
        const uint32_t a[1] = {0}, b[1] = {1};
        CHECK(refused(e.check_list(drop, 1, a, SlotLedger::DROP), "tts_hip_dia_stream_drop: slot 0 is not live"));
        CHECK(refused(e.check_list(drop, 1, b, SlotLedger::DROP), "tts_hip_dia_stream_drop: slot 1 is not live"));
    }
    // the empty list
    CHECK(g.check_list(adm, 0, nullptr, SlotLedger::ADMIT) == 0 && g.check_list(drop, 0, nullptr, SlotLedger::DROP) == 0);
    CHECK(g.slot == before);
    {   // Parler's dialect: its own live flags (0 / 1 = FREE / LIVE) and texts
        const std::vector<uint8_t> live = {0, 1, 0};
        const uint32_t s[2] = {0, 1}, far[1] = {3}, twice[2] = {2, 2}, l[2] = {1, 0};
        const char *who = "tts_hip_parler_stream_drop";
        CHECK(refused(check_slot_list("stream_admit", 2, s, live, 1u << SlotLedger::FREE, ">=", "is still generating"), "stream_admit: slot 1 is still generating"));
        CHECK(refused(check_slot_list("stream_admit", 1, far, live, 1u << SlotLedger::FREE, ">=", "is still generating"), "stream_admit: slot 3 >= 3"));
        CHECK(refused(check_slot_list("stream_admit", 2, twice, live, 1u << SlotLedger::FREE, ">=", "is still generating"), "stream_admit: slot 2 named twice"));
        CHECK(check_slot_list("stream_admit", 1, s, live, 1u << SlotLedger::FREE, ">=", "is still generating") == 0);
        CHECK(refused(check_slot_list(who, 1, far, live, 1u << SlotLedger::LIVE, ">=", "is not live"), "tts_hip_parler_stream_drop: slot 3 >= 3"));
        CHECK(refused(check_slot_list(who, 2, l, live, 1u << SlotLedger::LIVE, ">=", "is not live"), "tts_hip_parler_stream_drop: slot 0 is not live"));
        CHECK(check_slot_list(who, 1, l, live, 1u << SlotLedger::LIVE, ">=", "is not live") == 0);
    }
}

static void report_and_collect() {
    SlotLedger g = ledger({SlotLedger::LIVE, SlotLedger::ENDED, SlotLedger::FREE, SlotLedger::REPORTED, SlotLedger::ENDED});
    const std::vector<uint32_t> counts = {5, 7, 0, 9, 11};
    uint32_t n = 99, slots[5] = {99, 99, 99, 99, 99}, cnt[5] = {99, 99, 99, 99, 99};
    g.report(counts, &n, slots, cnt);
    CHECK(n == 2 && slots[0] == 1 && cnt[0] == 7 && slots[1] == 4 && cnt[1] == 11 && slots[2] == 99);
    CHECK((g.slot == std::vector<uint8_t>{SlotLedger::LIVE, SlotLedger::REPORTED, SlotLedger::FREE, SlotLedger::REPORTED, SlotLedger::REPORTED}));
    g.report(counts, &n, slots, cnt);
    CHECK(n == 0);
    const char *oc = "tts_hip_orpheus_stream_collect", *orun = "tts_hip_orpheus_stream_run", *dc = "tts_hip_dia_stream_collect", *drun = "tts_hip_dia_stream_run";
    CHECK(refused(g.check_collect(oc, 0, 1, counts, orun, "produced", "ids"), "tts_hip_orpheus_stream_collect: slot 0 has not finished (tts_hip_orpheus_stream_run reports it)"));
    CHECK(refused(g.check_collect(dc, 2, 0, counts, drun, "made", "steps"), "tts_hip_dia_stream_collect: slot 2 has not finished (tts_hip_dia_stream_run reports it)"));
    CHECK(refused(g.check_collect(oc, 5, 0, counts, orun, "produced", "ids"), "tts_hip_orpheus_stream_collect: slot 5 >= n_slots 5"));
    CHECK(refused(g.check_collect(oc, 1, 8, counts, orun, "produced", "ids"), "tts_hip_orpheus_stream_collect: slot 1 produced 7 ids, 8 asked for"));
    CHECK(refused(g.check_collect(dc, 4, 12, counts, drun, "made", "steps"), "tts_hip_dia_stream_collect: slot 4 made 11 steps, 12 asked for"));
    CHECK(g.check_collect(oc, 1, 7, counts, orun, "produced", "ids") == 0 && g.check_collect(dc, 3, 0, counts, drun, "made", "steps") == 0);
    // steps in flight
    CHECK(g.idle("tts_hip_dia_stream_admit", "tts_hip_dia_stream_wait") == 0);
    g.in_flight = 16;
    CHECK(refused(g.idle("tts_hip_dia_stream_admit", "tts_hip_dia_stream_wait"), "tts_hip_dia_stream_admit: 16 steps are in flight (tts_hip_dia_stream_wait first)"));
    CHECK(refused(g.idle("tts_hip_orpheus_stream_drop", "tts_hip_orpheus_stream_wait"), "tts_hip_orpheus_stream_drop: 16 steps are in flight (tts_hip_orpheus_stream_wait first)"));
}

static void penalty_tables() {
    const float pens[3] = {1.1f, 1.3f, 0.5f};
    const int lens[3] = {1, 2, 37};
    for (float p : pens)
        for (int len : lens) {
            std::vector<double> got((size_t) len + 1, -7.0), want((size_t) len);
            penalty_table(got.data(), p, len);
            for (int k = 0; k < len; k++) want[(size_t) k] = pow((double) p, (double) k);
            CHECK(memcmp(got.data(), want.data(), (size_t) len * sizeof(double)) == 0);
            CHECK(got[0] == 1.0 && got[(size_t) len] == -7.0);   // entry 0 exactly 1; nothing past len is written
        }
}

int main() {
    slot_lists();
    report_and_collect();
    penalty_tables();
    printf("session_slots: ok\n");
    return 0;
}
