// keep_rows_check.cpp — host/include/keep_rows.h against a naive rebuild of the kept rows, compiled with -fsanitize=address,undefined and run by
// tests/test_subsume.py. Prints one line "checked <n> mismatches <m>"; exit status 1 when any case differs.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "keep_rows.h"

struct Model {
    std::vector<uint64_t>      key_off, ref_off;
    std::vector<unsigned char> key_bytes;
    std::vector<uint32_t>      counts, ref_sentence;
    std::vector<uint16_t>      ref_token;
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

// n patterns of 1..6 key bytes; indexed: 0..4 references each (a count is then the number of references)
static Model make(size_t n, bool indexed) {
    Model m;
    m.key_off.push_back(0);
    if (indexed) m.ref_off.push_back(0);
    for (size_t j = 0; j < n; ++j) {
        const size_t len = 1 + rng() % 6;
        for (size_t k = 0; k < len; ++k) m.key_bytes.push_back((unsigned char)(rng() & 0xFF));
        m.key_off.push_back(m.key_bytes.size());
        if (indexed) {
            const size_t r = rng() % 5;
            for (size_t k = 0; k < r; ++k) {
                m.ref_sentence.push_back((uint32_t)rng());
                m.ref_token.push_back((uint16_t)rng());
            }
            m.ref_off.push_back(m.ref_sentence.size());
            m.counts.push_back((uint32_t)r);
        } else {
            m.counts.push_back((uint32_t)rng());
        }
    }
    m.key_bytes.push_back(0);  // the exports' element of slack
    if (indexed) {
        m.ref_sentence.push_back(0);
        m.ref_token.push_back(0);
    }
    return m;
}

static Model naive(const Model& m, const std::vector<uint8_t>& keep) {
    Model      o;
    const bool indexed = !m.ref_off.empty();
    o.key_off.push_back(0);
    if (indexed) o.ref_off.push_back(0);
    for (size_t j = 0; j < m.counts.size(); ++j) {
        if (!keep[j]) continue;
        for (uint64_t k = m.key_off[j]; k < m.key_off[j + 1]; ++k) o.key_bytes.push_back(m.key_bytes[k]);
        o.key_off.push_back(o.key_bytes.size());
        o.counts.push_back(m.counts[j]);
        if (indexed) {
            for (uint64_t k = m.ref_off[j]; k < m.ref_off[j + 1]; ++k) {
                o.ref_sentence.push_back(m.ref_sentence[k]);
                o.ref_token.push_back(m.ref_token[k]);
            }
            o.ref_off.push_back(o.ref_sentence.size());
        }
    }
    return o;
}

template <class T>
static bool same_prefix(const std::vector<T>& got, const std::vector<T>& want, size_t slack) {
    if (got.size() != want.size() + slack) return false;
    for (size_t k = 0; k < want.size(); ++k)
        if (got[k] != want[k]) return false;
    return true;
}

static unsigned checked = 0, bad = 0;

static void check(const char* what, size_t n, bool indexed, const std::vector<uint8_t>& keep) {
    Model       m    = make(n, indexed);
    const Model want = naive(m, keep);
    const size_t kept = colibri_host::keep_rows(m.key_off, m.key_bytes, m.counts, m.ref_off, m.ref_sentence, m.ref_token, keep.data());
    ++checked;
    const bool ok = kept == want.counts.size() && m.key_off == want.key_off && m.counts == want.counts && same_prefix(m.key_bytes, want.key_bytes, 1) && m.ref_off == want.ref_off &&
                    (!indexed || (same_prefix(m.ref_sentence, want.ref_sentence, 1) && same_prefix(m.ref_token, want.ref_token, 1)));
    if (!ok && bad++ < 10) printf("MISMATCH %s: %zu patterns, %s\n", what, n, indexed ? "indexed" : "unindexed");
}

int main() {
    for (int indexed = 0; indexed < 2; ++indexed) {
        check("empty model", 0, indexed, std::vector<uint8_t>(1, 1));
        for (size_t n : {1u, 2u, 7u, 100u, 1000u}) {
            check("keep all", n, indexed, std::vector<uint8_t>(n, 1));
            check("keep none", n, indexed, std::vector<uint8_t>(n, 0));
            std::vector<uint8_t> alt(n), ends(n, 1), rnd(n);
            for (size_t j = 0; j < n; ++j) alt[j] = (uint8_t)(j & 1), rnd[j] = (uint8_t)(rng() % 3 == 0 ? 0 : 255);
            ends[0] = ends[n - 1] = 0;  // the first and the last pattern go
            check("alternating", n, indexed, alt);
            for (auto& k : alt) k = !k;
            check("alternating, the first stays", n, indexed, alt);
            check("first and last go", n, indexed, ends);
            check("random", n, indexed, rnd);
        }
    }
    printf("checked %u mismatches %u\n", checked, bad);
    return bad != 0;
}
