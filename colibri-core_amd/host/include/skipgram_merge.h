#ifndef COLIBRI_AMD_SKIPGRAM_MERGE_H
#define COLIBRI_AMD_SKIPGRAM_MERGE_H
// skipgram_merge — installing the answer of colibri_modelskip (the skipgrams of a model that holds its n-grams) in a model: the
// patterns whose keep byte is 0 leave, the skipgrams enter with their reference lists. On the flat arrays of a run that has not been turned into
// map nodes (skipgram_merge_flat), or through two callbacks on whatever holds the patterns (skipgram_merge_each: IndexedPatternModel's map). A
// malformed answer is refused before anything is touched. It stands alone (no device layer, no other header of the C++ face but keep_rows.h):
// tests/skipgram_merge_check.cpp runs it under the sanitizers.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "keep_rows.h"

namespace colibri_host {

/** what colibri_modelskip_fetch fills: the kept skipgrams in export layout with their skip-type counts, and one keep byte per pattern of the model */
struct SkipgramAnswer {
    std::vector<uint64_t>      key_off;  // size() + 1
    std::vector<unsigned char> key_bytes;
    std::vector<uint32_t>      counts, types;
    std::vector<uint64_t>      ref_off;  // size() + 1
    std::vector<uint32_t>      ref_sentence;
    std::vector<uint16_t>      ref_token;
    std::vector<uint8_t>       keep;     // one per pattern of the model the answer was computed on
    size_t size() const { return counts.size(); }
};

/** NULL when the answer is well-formed for a model of np patterns, else what is wrong with it */
inline const char* skipgram_answer_fault(const SkipgramAnswer& a, size_t np) {
    const size_t ns = a.size();
    if (a.keep.size() != np) return "the keep bytes are not one per pattern of the model";
    if (a.types.size() != ns || a.key_off.size() != ns + 1 || a.ref_off.size() != ns + 1) return "the arrays' lengths disagree";
    if (a.key_off[0] != 0 || a.ref_off[0] != 0) return "an offset array does not start at 0";
    for (size_t j = 0; j < ns; ++j) {
        if (a.key_off[j + 1] <= a.key_off[j]) return "a key offset does not ascend (an empty key)";
        if (a.ref_off[j + 1] < a.ref_off[j]) return "a reference offset descends";
        if (a.ref_off[j + 1] - a.ref_off[j] != a.counts[j]) return "a count is not the length of its reference list";
    }
    if (a.key_off[ns] > a.key_bytes.size()) return "the key offsets run past the key bytes";
    if (a.ref_off[ns] > a.ref_sentence.size() || a.ref_off[ns] > a.ref_token.size()) return "the reference offsets run past the references";
    return NULL;
}

/** no skipgram to insert and no pattern to erase: installing the answer would leave the model as it is */
inline bool skipgram_answer_changes_nothing(const SkipgramAnswer& a) {
    if (a.size() != 0) return false;
    for (uint8_t k : a.keep)
        if (!k) return false;
    return true;
}

/** on the flat arrays of an indexed model in export layout (key_off / ref_off: n + 1, counts: n; the byte and reference arrays with one element of
 *  slack, as the exports leave them): keep_rows by the keep bytes, then the skipgrams behind. false, with nothing touched: a malformed answer or
 *  arrays that are not such a model. *erased (optional) = the patterns that left. */
inline bool skipgram_merge_flat(std::vector<uint64_t>& key_off, std::vector<unsigned char>& key_bytes, std::vector<uint32_t>& counts, std::vector<uint64_t>& ref_off,
                                std::vector<uint32_t>& ref_sentence, std::vector<uint16_t>& ref_token, const SkipgramAnswer& a, size_t* erased = NULL) {
    const size_t n = counts.size();
    if (key_off.size() != n + 1 || ref_off.size() != n + 1 || skipgram_answer_fault(a, n) != NULL) return false;
    if (key_off[n] > key_bytes.size() || ref_off[n] > ref_sentence.size() || ref_off[n] > ref_token.size()) return false;
    const size_t kept = keep_rows(key_off, key_bytes, counts, ref_off, ref_sentence, ref_token, a.keep.data());
    if (erased) *erased = n - kept;
    const size_t   ns = a.size();
    const uint64_t kb = key_off[kept], nr = ref_off[kept], skb = a.key_off[ns], snr = a.ref_off[ns];
    key_bytes.resize((size_t)(kb + skb) + 1);
    ref_sentence.resize((size_t)(nr + snr) + 1);
    ref_token.resize((size_t)(nr + snr) + 1);
    if (skb) std::memcpy(key_bytes.data() + kb, a.key_bytes.data(), (size_t)skb);
    if (snr) {
        std::memcpy(ref_sentence.data() + nr, a.ref_sentence.data(), (size_t)snr * sizeof(uint32_t));
        std::memcpy(ref_token.data() + nr, a.ref_token.data(), (size_t)snr * sizeof(uint16_t));
    }
    key_off.resize(kept + ns + 1);
    ref_off.resize(kept + ns + 1);
    counts.resize(kept + ns);
    for (size_t j = 0; j < ns; ++j) {
        key_off[kept + j + 1] = kb + a.key_off[j + 1];
        ref_off[kept + j + 1] = nr + a.ref_off[j + 1];
        counts[kept + j]      = a.counts[j];
    }
    return true;
}

/** on any holder of the np patterns the answer was computed on: erase(j) for every pattern j whose keep byte is 0, then
 *  insert(key, keylen, ref_sentence, ref_token, nrefs) for every skipgram. false, with no callback made: a malformed answer. */
template <class Erase, class Insert>
bool skipgram_merge_each(const SkipgramAnswer& a, size_t np, Erase erase, Insert insert) {
    if (skipgram_answer_fault(a, np) != NULL) return false;
    for (size_t j = 0; j < np; ++j)
        if (!a.keep[j]) erase(j);
    for (size_t j = 0; j < a.size(); ++j)
        insert(a.key_bytes.data() + a.key_off[j], (size_t)(a.key_off[j + 1] - a.key_off[j]), a.ref_sentence.data() + a.ref_off[j], a.ref_token.data() + a.ref_off[j],
               (size_t)(a.ref_off[j + 1] - a.ref_off[j]));
    return true;
}

}  // namespace colibri_host
#endif
