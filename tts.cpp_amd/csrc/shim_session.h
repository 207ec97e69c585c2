// shim_session.h — what the mixed sessions of shim_decoder.hip and shim_llama.hip stage alike: the per-slot sampler records of sample_kernel.
#pragma once
#include "shim_internal.h"
#include "parler_kernels.h"   // SampleRow

// Utterance i's record into recs[i] (sampling NULL, or an entry NULL: sampler::max) and, where its penalty is not 1, its table pow(penalty, k),
// k < len, into tabs[i * len ...]; the record then points at table_of(i), the device address the table will have.  tabs stays empty while no
// utterance is penalised.  any_sampled / any_rep are only ever set.  The limits of a sampler are the caller's to check, before this.
template <class TableOf>
static void build_sample_rows(uint32_t n, const tts_hip_sampling *const *sampling, int len, TableOf table_of, std::vector<SampleRow> &recs, std::vector<double> &tabs,
                              bool *any_sampled, bool *any_rep) {
    recs.assign(n, SampleRow{SAMPLE_ROW_MAX, 0u, 1.0f, 1.0f, nullptr, len, 0});
    for (uint32_t i = 0; i < n; i++) {
        const tts_hip_sampling *sp = sampling ? sampling[i] : nullptr;
        if (!sp) continue;
        *any_sampled = true;
        recs[i].mode = SAMPLE_ROW_SAMPLE; recs[i].top_k = sp->top_k; recs[i].top_p = sp->top_p; recs[i].temperature = sp->temperature;
        if (sp->repetition_penalty == 1.0f) continue;
        *any_rep = true;
        tabs.resize((size_t) n * len);
        recs[i].pen_table = table_of(i);
        penalty_table(tabs.data() + (size_t) i * len, sp->repetition_penalty, len);
    }
}
