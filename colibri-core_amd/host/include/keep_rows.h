#ifndef COLIBRI_AMD_KEEP_ROWS_H
#define COLIBRI_AMD_KEEP_ROWS_H
// keep_rows — the rows of a model in export layout whose flag is set, compacted in place and in order. It stands alone (no device layer,
// no other header of the C++ face): colibri_host::keep_patterns (patternmodel.h) applies it to a TrainResult, tests/keep_rows_check.cpp runs it
// under the sanitizers.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace colibri_host {

/** keep[j] != 0: pattern j stays. key_off (n + 1) / key_bytes and counts (n) always; ref_off (n + 1) / ref_sentence / ref_token of an indexed
 *  model, ref_off empty otherwise. One linear pass over every array; the byte and reference arrays keep one element of slack, as the exports
 *  leave them. Returns the patterns kept. */
inline size_t keep_rows(std::vector<uint64_t>& key_off, std::vector<unsigned char>& key_bytes, std::vector<uint32_t>& counts, std::vector<uint64_t>& ref_off,
                        std::vector<uint32_t>& ref_sentence, std::vector<uint16_t>& ref_token, const uint8_t* keep) {
    const size_t n       = counts.size();
    const bool   indexed = !ref_off.empty();
    if (key_off.size() < n + 1 || (indexed && ref_off.size() < n + 1)) return n;  // (not a model in export layout: left alone)
    size_t   w  = 0;
    uint64_t kb = 0, nr = 0;
    for (size_t j = 0; j < n; ++j) {
        if (!keep[j]) continue;
        const uint64_t a = key_off[j], b = key_off[j + 1];
        if (b > a) std::memmove(key_bytes.data() + kb, key_bytes.data() + a, (size_t)(b - a));
        counts[w] = counts[j];
        if (indexed) {
            const uint64_t ra = ref_off[j], rb = ref_off[j + 1];
            if (rb > ra) {
                std::memmove(ref_sentence.data() + nr, ref_sentence.data() + ra, (size_t)(rb - ra) * sizeof(uint32_t));
                std::memmove(ref_token.data() + nr, ref_token.data() + ra, (size_t)(rb - ra) * sizeof(uint16_t));
            }
            ref_off[w] = nr;
            nr += rb - ra;
        }
        key_off[w] = kb;
        kb += b - a;
        ++w;
    }
    key_off[w] = kb;
    key_off.resize(w + 1);
    key_bytes.resize((size_t)kb + 1);
    counts.resize(w);
    if (indexed) {
        ref_off[w] = nr;
        ref_off.resize(w + 1);
        ref_sentence.resize((size_t)nr + 1);
        ref_token.resize((size_t)nr + 1);
    }
    return w;
}

}  // namespace colibri_host
#endif
