// Walks a sequence of events through the retry ladder of colibri_train (colibri-core_amd/csrc/train_retry.hpp) the way colibri_train does, and prints the state after
// each step. Built and run by tests/test_train_retry.py.
//
//   train_retry_walk TABLE_MODE SPLIT_EXACT BIG EVENT...
//     TABLE_MODE   the caller's options.table_mode
//     SPLIT_EXACT  1: the corpus already has the exact split (sticky)
//     BIG          1: a corpus beyond the small pass size (small passes apply until an attempt runs with them)
//     EVENT        plain:V | enq:V | pass:V[:bi2][:radix]   DevState.radix_overflow = V after that loop (per pass: with the run's guards)
//                  totable:V | pairs | ranks | results
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "train_retry.hpp"

using namespace colibri_retry;

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int  table_mode  = atoi(argv[1]);
    bool       split_exact = atoi(argv[2]) != 0;
    const bool big         = atoi(argv[3]) != 0;
    Ladder     ladder;
    for (int i = 4; i < argc; ++i) {
        const std::string a = argv[i];
        Event             ev;
        const size_t      colon = a.find(':');
        const std::string kind  = a.substr(0, colon);
        if (colon != std::string::npos) ev.overflow = (uint32_t)strtoul(a.c_str() + colon + 1, nullptr, 10);
        if (kind == "plain")
            ev.loop = Loop::kPlain;
        else if (kind == "enq")
            ev.loop = Loop::kEnqueued;
        else if (kind == "pass") {
            ev.loop       = Loop::kPerPass;
            ev.bi2_synced = a.find(":bi2") != std::string::npos;
            ev.radix      = a.find(":radix") != std::string::npos;
        } else if (kind == "totable")
            ev.what = What::kToTable;
        else if (kind == "pairs")
            ev.what = What::kPairs;
        else if (kind == "ranks")
            ev.what = What::kRanks;
        else if (kind == "results")
            ev.what = What::kResults;
        else
            return 2;
        const Step st = advance(ladder, split_exact, table_mode, big && !ladder.attempt.small_passes, ev);
        if (st.set_split_exact) split_exact = true;
        const char* verdict = st.verdict == Verdict::kRepeat ? "repeat" : st.verdict == Verdict::kFail ? "fail" : "goon";
        printf("%s reason=%d first=%d retries=%d table=%d b2off=%d chainoff=%d small=%d split=%d\n", verdict, st.verdict == Verdict::kRepeat ? st.reason : 0, ladder.first_reason,
               ladder.retries, (int)ladder.attempt.force_table, (int)ladder.attempt.b2_disabled, (int)ladder.attempt.chain_disabled, (int)ladder.attempt.small_passes, (int)split_exact);
        if (st.verdict == Verdict::kFail) break;
    }
    return 0;
}
