// fmt_g6_check.cpp — csrc/fmt_g6.hpp against snprintf("%.6g", a / (double)b), compiled and run by tests/test_print.py.
// Prints one line "checked <n> mismatches <m>" and up to ten mismatching cases; exit status 1 when any case differs.
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <initializer_list>

#include "fmt_g6.hpp"

static uint64_t checked = 0, bad = 0;

static void check(uint64_t a, uint64_t b) {
    char want[64], got[64];
    snprintf(want, sizeof want, "%.6g", (double)a / (double)b);
    const int n = colibri::fmt_g6(a, b, got);
    got[n]      = 0;
    ++checked;
    if (n > colibri::kFmtG6Max || strcmp(want, got) != 0) {
        if (bad++ < 10) printf("MISMATCH %llu / %llu: want %s got %s\n", (unsigned long long)a, (unsigned long long)b, want, got);
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

int main() {
    // every 0 <= a <= 3b, 1 <= b <= 1500
    for (uint64_t b = 1; b <= 1500; ++b)
        for (uint64_t a = 0; a <= 3 * b; ++a) check(a, b);
    // exponent form, both doubles of a row
    const uint64_t bs[5] = {10000000ull, 100000000ull, 1000000000ull, 4000000000ull, 1ull << 40};
    for (uint64_t b : bs)
        for (uint64_t a = 1; a <= 2000; ++a) check(a, b);
    for (uint64_t a = 999990; a <= 1000010; ++a) check(a, 1);  // the switch to exponent form at 10^6
    for (uint64_t a : {1000000ull, 999999500ull, 999999499ull, 123456789012ull, (1ull << 53) - 1}) {
        check(a, 1);
        check(a, 1000);
        check(1, a);
    }
    // exact decimal ties at the seventh digit, and the ratios just either side of them
    struct Tie {
        uint64_t a, b;
    };
    const Tie ties[] = {{1234565, 10000000ull}, {1234575, 10000000ull}, {9999995, 10000000ull}, {99999950, 1000000000000ull}, {999999500, 10000000000000ull},
                        {1000005, 10000000ull}, {1000015, 10000000ull}, {5000005, 10000000ull}, {2500025, 10000000ull},       {1999995, 10000000ull}};
    for (const Tie& t : ties) {
        check(t.a, t.b);
        check(t.a * 1000 - 1, t.b * 1000);
        check(t.a * 1000 + 1, t.b * 1000);
        check(t.a * 1000, t.b * 1000);
    }
    for (uint64_t k = 1; k <= 4000; ++k) {  // 5 / 10^6 * k forms: ties at every scale
        check(5 * k, 1000000ull);
        check(10 * k + 5, 10000000ull);
        check(1000000ull + 10 * k + 5, 10000000ull);
        check(100000 * k + 5, 10ull);     // ties above 10^6: the integer branch
        check(1000000 * k + 50, 100ull);
        check(100000 * k + 5, 10000ull);
    }
    // ties that are exact in binary: (2j + 1) / 2^s
    for (uint64_t s = 1; s <= 24; ++s)
        for (uint64_t j = 0; j < 300; ++j) check(2 * j + 1, 1ull << s);
    // random pairs under 2^40
    for (int i = 0; i < 2000000; ++i) {
        const uint64_t a = rng() >> 24, b = (rng() >> 24) | 1u;
        check(a, b);
    }
    for (int i = 0; i < 200000; ++i) {  // and of very different sizes, up to 2^53
        const uint64_t a = rng() >> (11 + rng() % 50), b = (rng() >> (11 + rng() % 50)) | 1u;
        check(a, b);
    }
    check(5, 0);
    check(0, 0);
    printf("checked %llu mismatches %llu\n", (unsigned long long)checked, (unsigned long long)bad);
    return bad ? 1 : 0;
}
