// bi2_mix_check.cpp — csrc/bi2_mix.hpp on the host, compiled and run by tests/test_bi2_mix.py.
//   (no argument)  the checks below; prints "checked <n> mismatches <m>" and up to ten failing cases; exit status 1 when any case fails
//   vectors        prints the vectors that pin tests/bin_models.py: "M <K> <x> <bi2_mix(x, K)>" and "B <lgb> <key> <bi2_bucket_of(key, lgb, 2^lgb - 1)>"
// The checks: the mix is a bijection of the K-bit integers —
//   K = 17 .. 24   every one of the 2^K values: the image is below 2^K and no image repeats (a bitmap);
//   K = 25 .. 56   10^6 seeded random values each: the four Feistel rounds undone in reverse order (unmix, written out here) give the value back;
//   K = 17, 18, 24, 28, 34, 42, 48   the same for the smallest inputs, the largest and those around the half boundary 1 << (K >> 1);
// and the two forms of the round function's product (the device's 24-bit multiply, the host's 64-bit one) are the same integer: the low 32 bits of r x c, r cut to 24 bits.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bi2_mix.hpp"

using colibri::bi2_mix;
using colibri::bi2_mix_f;
using colibri::kBi2MixC;

static uint64_t checked = 0, bad = 0;
static void     fail(const char* what, uint32_t K, uint64_t x, uint64_t y) {
    if (bad++ < 10) printf("FAIL %s K=%u x=%llu y=%llu\n", what, K, (unsigned long long)x, (unsigned long long)y);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

// the low 32 bits of (r mod 2^24) x c for a 24-bit c, three ways: as the host form of bi2_mix_f computes it, as a 24-bit multiply instruction does (32-bit product of the
// two operands cut to 24 bits), and from 12-bit limbs
static uint32_t prod64(uint32_t r, uint32_t c) { return (uint32_t)((uint64_t)(r & 0xFFFFFFu) * c); }
static uint32_t prod24(uint32_t r, uint32_t c) { return (r & 0xFFFFFFu) * (c & 0xFFFFFFu); }
static uint32_t prod12(uint32_t r, uint32_t c) {
    const uint32_t r0 = r & 0xFFFu, r1 = (r >> 12) & 0xFFFu, c0 = c & 0xFFFu, c1 = (c >> 12) & 0xFFFu;
    return r0 * c0 + ((r0 * c1 + r1 * c0) << 12) + ((r1 * c1) << 24);
}
static void check_products(uint32_t r) {
    for (int k = 0; k < 4; ++k) {
        const uint32_t c = kBi2MixC[k], a = prod64(r, c);
        ++checked;
        if (a != prod24(r, c) || a != prod12(r, c)) fail("product", 0, r, c);
        for (uint32_t ob = 8; ob <= 24; ++ob)
            if (bi2_mix_f(r, c, ob) != a >> (32u - ob)) fail("bi2_mix_f", ob, r, c);
    }
}

// bi2_mix undone: the rounds in reverse order (a round (L, R) -> (L ^ F(R), R) is its own inverse)
static uint64_t unmix(uint64_t y, uint32_t K) {
    const uint32_t h = K >> 1, hb = K - h;
    const uint32_t fl = h > 24u ? 24u : h, fh = hb > 24u ? 24u : hb;
    uint32_t       lo = (uint32_t)y & ((1u << h) - 1u), hi = (uint32_t)(y >> h);
    lo ^= bi2_mix_f(hi, kBi2MixC[3], fl);
    hi ^= bi2_mix_f(lo, kBi2MixC[2], fh);
    lo ^= bi2_mix_f(hi, kBi2MixC[1], fl);
    hi ^= bi2_mix_f(lo, kBi2MixC[0], fh);
    return ((uint64_t)hi << h) | lo;
}
static void check_round_trip(uint64_t x, uint32_t K) {
    const uint64_t y = bi2_mix(x, K);
    ++checked;
    if (y >> K) fail("range", K, x, y);
    if (unmix(y, K) != x) fail("round trip", K, x, y);
}

static const uint32_t kEdgeK[7] = {17, 18, 24, 28, 34, 42, 48};
// the smallest inputs, the largest, and those around the half boundary (where the low half wraps into the high one)
static void edge_inputs(uint32_t K, uint32_t n, std::vector<uint64_t>& out) {
    const uint64_t top = (1ull << K) - 1, half = 1ull << (K >> 1);
    for (uint32_t i = 0; i < n; ++i) {
        out.push_back(i);
        out.push_back(top - i);
        out.push_back(half - n / 2 + i);
    }
}

static int print_vectors() {
    for (uint32_t K : kEdgeK) {
        std::vector<uint64_t> xs;
        edge_inputs(K, 40, xs);
        for (int i = 0; i < 1500; ++i) xs.push_back(rng() & ((1ull << K) - 1));
        for (uint64_t x : xs) printf("M %u %llu %llu\n", K, (unsigned long long)x, (unsigned long long)bi2_mix(x, K));
    }
    for (int lgb = 6; lgb <= 8; ++lgb) {
        const uint32_t bmask = (1u << lgb) - 1u;
        for (int i = 0; i < 1200; ++i) {
            const uint32_t key = i < 64 ? (uint32_t)i : i < 128 ? 0x7FFFFFFFu - (uint32_t)(i - 64) : (uint32_t)rng() & 0x7FFFFFFFu;
            printf("B %d %u %u\n", lgb, key, colibri::bi2_bucket_of(key, lgb, bmask));
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "vectors") == 0) return print_vectors();
    // every K-bit value, K = 17 .. 24
    for (uint32_t K = 17; K <= 24; ++K) {
        std::vector<uint64_t> seen(((size_t)1 << K) / 64, 0);
        for (uint64_t x = 0; x < (1ull << K); ++x) {
            const uint64_t y = bi2_mix(x, K);
            ++checked;
            if (y >> K) {
                fail("range", K, x, y);
                continue;
            }
            if (seen[y >> 6] >> (y & 63) & 1) fail("repeat", K, x, y);
            seen[y >> 6] |= 1ull << (y & 63);
        }
    }
    // random values, K = 25 .. 56
    for (uint32_t K = 25; K <= 56; ++K)
        for (int i = 0; i < 1000000; ++i) check_round_trip(rng() & ((1ull << K) - 1), K);
    for (uint32_t K : kEdgeK) {
        std::vector<uint64_t> xs;
        edge_inputs(K, 4096, xs);
        for (uint64_t x : xs) check_round_trip(x & ((1ull << K) - 1), K);
    }
    // the product forms: the ends of the 24-bit range, operands with bits above it (which both forms drop), random operands
    for (uint32_t r = 0; r < 4096; ++r) {
        check_products(r);
        check_products(0xFFFFFFu - r);
        check_products(0xFFFFFFFFu - r);
        check_products(0x1000000u + r);
    }
    for (int i = 0; i < 1000000; ++i) check_products((uint32_t)rng());
    printf("checked %llu mismatches %llu\n", (unsigned long long)checked, (unsigned long long)bad);
    return bad ? 1 : 0;
}
