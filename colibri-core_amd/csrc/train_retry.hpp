// The retry ladder of colibri_train: what a training run does next after an engine gave up, a buffer ran out or a check failed. Plain C++ on purpose (nothing of HIP,
// nothing of the context): tests/test_train_retry.py walks event sequences through it on the CPU. DESIGN.md §4b has the ladder as a table.
#pragma once

#include <cstdint>

namespace colibri_retry {

// colibri_stats.fallback_reason (the COLIBRI_FALLBACK_* of include/colibri_hip.h; the driver asserts that they agree)
constexpr int kReasonBin = 2, kReasonOrder2 = 4, kReasonSplit = 8, kReasonChain = 16, kReasonResults = 32, kReasonPairs = 64, kReasonLdsOrder = 128;

// what one attempt runs with: colibri_train applies the flags to the context before the attempt and clears them after it
struct Attempt {
    bool force_table    = false;  // the global table (options.table_mode 1)
    bool b2_disabled    = false;  // no second-generation order 2
    bool chain_disabled = false;  // no chained orders >= 3
    bool small_passes   = false;  // the earlier, smaller pass size
};

enum class Loop { kPlain, kEnqueued, kPerPass };  // which order loop met the event
enum class What {
    kOverflow,  // DevState.radix_overflow after a loop (plain, enqueued) or a pass (per pass): 1 region, 2 bin, 3 ids, 4 order 2, 8 split, 16 chain
    kToTable,   // a skipgram pass asked for the table (kRerunOnTable), or the logged skipgram passes overflowed
    kPairs,     // finalize_index: the pair buffer was too small (it has been enlarged)
    kRanks,     // finalize_index: a checked rank disagreed (the context now matches every rank with ballots)
    kResults,   // colibri_train: the result buffers were too small
};
struct Event {
    What     what       = What::kOverflow;
    Loop     loop       = Loop::kPlain;
    uint32_t overflow   = 0;      // DevState.radix_overflow when the event was met (names the reason of a table repeat)
    bool     bi2_synced = false;  // per-pass loop: the run has the second-generation order 2
    bool     radix      = false;  // per-pass loop: the run counts on the radix path
};

enum class Verdict { kGoOn, kRepeat, kFail };  // kGoOn: the event asks for nothing; kFail: COLIBRI_ERR_OVERFLOW, the radix path overflowed under table_mode 2
struct Step {
    Verdict verdict = Verdict::kGoOn;
    Attempt next;                     // kRepeat: the attempt to run
    int     reason          = 0;      // ... and the COLIBRI_FALLBACK_* to note
    bool    set_split_exact = false;  // ... after making the exact split sticky for this corpus
};

// cur: the attempt that met the event; split_exact: the sticky flag of the corpus; table_mode: the caller's option; small_passes_apply: retry_with_small_passes(npos)
// as the attempt saw it. Flags only accumulate — except for kResults: the repeat with more room starts clean. kPairs / kRanks: the same attempt again
inline Step next_attempt(const Attempt& cur, bool split_exact, int table_mode, bool small_passes_apply, const Event& ev) {
    Step           st;
    const uint32_t v = ev.overflow;
    const bool     plain = ev.loop == Loop::kPlain, per_pass = ev.loop == Loop::kPerPass;
    st.next    = cur;
    st.verdict = Verdict::kRepeat;
    switch (ev.what) {
    case What::kResults: st.next = Attempt{}; st.reason = kReasonResults; return st;
    case What::kPairs: st.reason = kReasonPairs; return st;
    case What::kRanks: st.reason = kReasonLdsOrder; return st;
    case What::kToTable: break;
    case What::kOverflow:  // the per-pass loop acts on order 2's overflow only under bi2_synced, on any other only in a run on the radix path
        if (v == 0 || (per_pass && !(ev.bi2_synced && v == 4) && !ev.radix)) {
            st.verdict = Verdict::kGoOn;
        } else if (plain && v == 8 && !split_exact) {
            st.set_split_exact = true;
            st.reason          = kReasonSplit;
        } else if (!per_pass && v == 16) {
            st.next.chain_disabled = true;
            st.reason              = kReasonChain;
        } else if (v == 4 && (!per_pass || ev.bi2_synced)) {  // a corpus beyond the earlier pass size gets that size back before anything slower is tried
            (small_passes_apply ? st.next.small_passes : st.next.b2_disabled) = true;
            st.reason = kReasonOrder2;
        } else if (plain && table_mode == 2) {
            st.verdict = Verdict::kFail;
        } else {
            break;
        }
        return st;
    }
    st.next.force_table = true;  // the global table; the reason names what overflowed
    st.reason           = v >= 1 && v <= 3 ? (int)v : kReasonBin;
    return st;
}

// the state of one colibri_train call between attempts, and one step of the ladder with the bookkeeping of a repeat done
struct Ladder {
    Attempt attempt;
    int     first_reason = 0;  // colibri_stats.fallback_reason: of the first repeat
    int     retries      = 0;  // colibri_stats.retries: all repeats
};
inline Step advance(Ladder& l, bool split_exact, int table_mode, bool small_passes_apply, const Event& ev) {
    const Step st = next_attempt(l.attempt, split_exact, table_mode, small_passes_apply, ev);
    if (st.verdict == Verdict::kRepeat) {
        l.attempt = st.next;
        if (l.retries++ == 0) l.first_reason = st.reason;
    }
    return st;
}

}  // namespace colibri_retry
