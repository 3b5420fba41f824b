// chain_step_check.cpp — csrc/chain_step.hpp on the host, compiled and run by tests/test_chain_step.py.
// Prints "checked <n> mismatches <m>" and up to ten failing cases; exit status 1 when any case fails. The checks:
//   the entry:  pack / pairs / bucket give back every (pairs, bucket) with pairs = 0 .. 2048 (a step holds at most 2048) and 65 535, bucket = 0 .. 1023 and 65 535;
//   the runs:   for run = 1, 2, 4, 8, blocks per XCD nper = 1, 2, 3, 96, 128 and tables of ns = 0 .. 3 run nper + 5 entries, the blocks' walks
//               (chain_run_first, then chain_run_next while below ns) visit every entry below ns exactly once, each block in ascending order and in whole runs:
//               a block's entries are consecutive inside a run and the block after it takes the next run;
//   run = 1 is the walk k, k + nper, k + 2 nper, ...
#include <cstdint>
#include <cstdio>
#include <vector>

#include "chain_step.hpp"

using namespace colibri;

static uint64_t checked = 0, bad = 0;
static void     fail(const char* what, uint64_t a, uint64_t b, uint64_t c) {
    if (bad++ < 10) printf("FAIL %s %llu %llu %llu\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
}

int main() {
    const uint32_t pairs[] = {0, 1, 2, 511, 512, 2047, 2048, 65535}, buckets[] = {0, 1, 7, 8, 512, 1022, 1023, 65535};
    for (uint32_t p = 0; p <= 2048; ++p)
        for (uint32_t b = 0; b < 1024; ++b) {
            const uint32_t y = chain_step_pack(p, b);
            ++checked;
            if (chain_step_pairs(y) != p || chain_step_bucket(y) != b) fail("pack", p, b, y);
        }
    for (uint32_t p : pairs)
        for (uint32_t b : buckets) {
            const uint32_t y = chain_step_pack(p, b);
            ++checked;
            if (chain_step_pairs(y) != p || chain_step_bucket(y) != b) fail("pack-edge", p, b, y);
        }
    const uint32_t runs[] = {1, 2, 4, 8}, npers[] = {1, 2, 3, 96, 128};
    for (uint32_t run : runs)
        for (uint32_t nper : npers)
            for (uint32_t ns = 0; ns <= 3 * run * nper + 5; ++ns) {
                std::vector<uint32_t> owner(ns, 0xFFFFFFFFu);
                for (uint32_t k = 0; k < nper; ++k) {
                    uint32_t prev = 0xFFFFFFFFu;
                    for (uint32_t s = chain_run_first(k, run); s < ns; s = chain_run_next(s, nper, run)) {
                        ++checked;
                        if (owner[s] != 0xFFFFFFFFu) fail("taken twice", run, nper, s);
                        owner[s] = k;
                        if ((s / run) % nper != k) fail("not this block's run", run, nper, s);
                        if (prev != 0xFFFFFFFFu && s <= prev) fail("not ascending", run, nper, s);
                        if (prev != 0xFFFFFFFFu && s % run != 0 && s != prev + 1) fail("a run is not consecutive", run, nper, s);
                        if (run == 1 && prev != 0xFFFFFFFFu && s != prev + nper) fail("run 1 is the strided walk", run, nper, s);
                        prev = s;
                    }
                }
                for (uint32_t s = 0; s < ns; ++s) {
                    ++checked;
                    if (owner[s] == 0xFFFFFFFFu) fail("not taken", run, nper, s);
                }
            }
    printf("checked %llu mismatches %llu\n", (unsigned long long)checked, (unsigned long long)bad);
    return bad ? 1 : 0;
}
