// relations.hpp — pattern relations of an indexed model: IndexedPatternModel::getsubchildren / getsubparents / getleftneighbours /
// getrightneighbours (reference include/patternmodel.h:3166-3352) summed over the model.
//
// For every reference (s, t) of a pattern A in A's own forward index, the occurrences (i, B) the reverse index holds in sentence s (the B list
// of cooc.hpp: every window of MINLENGTH..MAXLENGTH tokens the model has, and for n >= 3 that window under every gap mask of the model's
// skipgrams of that length; with a threshold, B's own count >= it) count when
//   getrightneighbours  i == t + n(A)
//   getleftneighbours   i + n(B) == t
//   getsubchildren      t <= i < t + n(A), n(B) <= n(A) - (i - t), B != A
//   getsubparents       i <= t, n(B) >= n(A) + (t - i), B != A
// and, for the two subsumption kinds when A or B is a skipgram, the reference's own test (kept as it is, not as its comments describe it):
//   getsubchildren  Pattern(A, i, n(B)) slices A at the corpus token index i (src/pattern.cpp:911-970): past A's end that slice is all of an
//                   n-gram A (no skipgram B is an instance of an n-gram) or empty for a skipgram A; otherwise it is A's tokens [i, i + n(B)),
//                   and B.instanceof(slice) (:1764-1784) needs n(B) tokens, each under a gap of the slice or equal to the corpus token there;
//                   a slice without a gap needs B to be an n-gram
//   getsubparents   A.instanceof(B) of the whole patterns: B's tokens, sliced from the corpus, are never gaps, so only an n-gram A with
//                   n(B) == n(A) (B starts at t, on A's own tokens) passes
//   B != A          PatternPointer::operator== (:1067-1103): equal masks, equal byte lengths, equal non-gap tokens; the corpus bytes of a gapped
//                   token count, so a skipgram B whose gap holds a multi-byte token differs from A even when it is A
// Two more kinds belong to skipgrams (getinstances :3127-3157, gettemplates :3086-3118); they look at the single position t, and a reference
// whose window [t, t + n(A)) leaves its sentence has no rows (the reference reads past the sentence there):
//   getinstances    i == t, n(B) == n(A), B an n-gram, B != A by pattern number (an n-gram A is its own window: no rows); with a threshold,
//                   B's own count and the joint count reach it
//   gettemplates    i == t, n(B) == n(A) >= 3, B a skipgram, unless rel_masked_equals(window, mask(B), A) — the reference's comparison of the
//                   masked window with A byte by byte AT THE SAME INDEX, under which a skipgram whose gap covers a multi-byte token is its
//                   own template; with a threshold, A's own count and the joint count reach it (B's own count is not tested: the B list is
//                   built unfiltered for this kind)
// The test reads A's key bytes and the corpus bytes, nothing else. The pipeline is cooc's (cooc_api.inc: steps (a) and (b), the chunks, the
// carried runs) with the two kernels below in place of cooc_events_kernel / cooc_emit_kernel and its own ordering pass. gfx950 only.
#pragma once
#include "cooc.hpp"

namespace colibri {

enum RelKind : int { kRelSubchildren = 0, kRelSubparents = 1, kRelLeft = 2, kRelRight = 3, kRelInstances = 4, kRelTemplates = 5 };

// the bytes of token j of a key: [*b, *e)
__device__ __forceinline__ void rel_key_token(const uint8_t* __restrict__ k, uint32_t len, uint32_t j, uint32_t& b, uint32_t& e) {
    uint32_t n = 0, s = 0;
    for (uint32_t x = 0; x < len; ++x) {
        if (k[x] >= 128) continue;
        if (n == j) {
            b = s;
            e = x + 1;
            return;
        }
        ++n;
        s = x + 1;
    }
    b = e = len;
}
// corpus token at position q equals the key bytes [kb, ke)
__device__ __forceinline__ bool rel_token_eq(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ tokstart, uint32_t q, const uint8_t* __restrict__ k, uint32_t kb,
                                             uint32_t ke) {
    const uint32_t b = tokstart[q], e = tokstart[q + 1];
    if (e - b != ke - kb) return false;
    for (uint32_t x = 0; x < e - b; ++x)
        if (bytes[b + x] != k[kb + x]) return false;
    return true;
}

// the inputs of one relation pass
struct RelArgs {
    const uint32_t*           rs;
    const uint32_t*           aid;
    const uint16_t*           rt;
    const uint8_t*            ntok;
    const uint32_t*           pmask;
    const uint8_t*            kbytes;
    const unsigned long long* koff;
    const uint32_t*           delimpos;
    uint32_t                  ndelim, npos, nsent, first_sentence, maxn;
    const unsigned long long* boff;
    const uint32_t*           bpos;
    const uint8_t*            bn;
    const uint32_t*           bid;
    const uint8_t*            bytes;
    const uint32_t*           tokstart;
    const uint32_t*           cnt;  // occurrence counts of the patterns
    uint32_t                  thr;
};

// PatternPointer::operator==(const Pattern&) of the reference for the window of na tokens at p under `mask` against A's key (src/pattern.cpp:1009-1041,
// host/include/patternmodel.h masked_pointer_equals), byte for byte: a byte past A's key reads as 0
__device__ __forceinline__ bool rel_masked_equals(const RelArgs& r, uint32_t p, uint32_t na, uint32_t mask, uint32_t a) {
    const uint8_t* data   = r.bytes + r.tokstart[p];
    const uint32_t nbytes = r.tokstart[p + na] - r.tokstart[p];
    const uint8_t* k      = r.kbytes + r.koff[a];
    const uint32_t obytes = (uint32_t)(r.koff[a + 1] - r.koff[a]);
    auto           at     = [&](uint32_t i) -> uint32_t { return i < obytes ? k[i] : 0u; };
    if (nbytes == 0 || data[0] == 0) return obytes == 0;
    if (obytes == 0) return false;
    uint32_t tok = 0;
    for (uint32_t i = 0; i < nbytes; ++i) {
        if (i > 0 && at(i - 1) >= 128 && at(i) == 0) return false;
        if (mask != 0 && data[i] < 128) {
            if (tok <= 30 && (mask & (1u << tok))) {
                if (at(i) != 3u) return false;
            } else if (data[i] != at(i)) {
                return false;
            }
            ++tok;
        } else if (data[i] != at(i)) {
            return false;
        }
    }
    return at(nbytes) == 0;
}

// does the occurrence j of the B list (at position q, sentence start `start`) count for A = a at position p (token t = p - start)?
template <int K>
__device__ __forceinline__ bool rel_counts(const RelArgs& r, uint32_t a, uint32_t na, uint32_t ma, uint32_t start, uint32_t p, uint64_t j) {
    const uint32_t q = r.bpos[j], n = r.bn[j];
    if (K == kRelRight) return q == p + na;
    if (K == kRelLeft) return q + n == p;
    const uint32_t b = r.bid[j], mb = r.pmask[b];
    if (K == kRelInstances) return n == na && mb == 0 && b != a;  // (the span is the position p, and the window lies inside the sentence)
    if (K == kRelTemplates) {
        if (n != na || na < 3 || mb == 0 || (r.thr && r.cnt[a] < r.thr)) return false;
        return !rel_masked_equals(r, p, na, mb, a);
    }
    if (K == kRelSubchildren) {
        if (q < p || q >= p + na || n > na - (q - p)) return false;
    } else {
        if (q > p || n < na + (p - q)) return false;
    }
    if (b == a) {  // B != A as PatternPointer::operator== has it: a skipgram's gapped tokens must all be single bytes to be equal
        bool same = true;
        for (uint32_t k = 0; k < n && k < 32; ++k)
            if (((ma >> k) & 1u) && r.tokstart[q + k + 1] - r.tokstart[q + k] != 1u) same = false;
        if (same) return false;
    }
    if (ma == 0 && mb == 0) return true;
    if (K == kRelSubparents) return ma == 0 && n == na;
    if (ma == 0) return false;  // the slice of an n-gram A has no gap: a skipgram B is no instance of it
    const uint32_t i = q - start;  // the corpus token index the reference slices A at
    if (i + n > na) return false;
    const uint8_t* k   = r.kbytes + r.koff[a];
    const uint32_t len = (uint32_t)(r.koff[a + 1] - r.koff[a]);
    bool           gap = false;
    for (uint32_t x = 0; x < n; ++x) {
        if ((ma >> (i + x)) & 1u) {
            gap = true;
            continue;
        }
        uint32_t kb, ke;
        rel_key_token(k, len, i + x, kb, ke);
        if (!rel_token_eq(r.bytes, r.tokstart, q + x, k, kb, ke)) return false;
    }
    return gap || mb == 0;
}

// the range of the B list an occurrence of A at p (tokens na) can relate to: the positions [q0, q1] clipped to its sentence [start, end)
template <int K>
__device__ __forceinline__ void rel_span(const RelArgs& r, uint32_t p, uint32_t na, uint32_t start, uint32_t end, uint64_t& j0, uint64_t& j1) {
    uint32_t q0, q1;  // [q0, q1)
    if (K == kRelRight) {
        q0 = p + na;
        q1 = q0 + 1;
    } else if (K == kRelLeft) {
        q0 = p >= start + r.maxn ? p - r.maxn : start;
        q1 = p;
    } else if (K == kRelSubchildren) {
        q0 = p;
        q1 = p + na;
    } else if (K == kRelSubparents) {
        const uint32_t back = r.maxn > na ? r.maxn - na : 0u;
        q0                  = p >= start + back ? p - back : start;
        q1                  = p + 1;
    } else {  // instances, templates: the position p alone, and only when the window [p, p + na) lies inside the sentence
        q0 = p;
        q1 = (p <= end && na <= end - p) ? p + 1 : p;
    }
    q1 = q1 < end ? q1 : end;
    q0 = q0 < q1 ? q0 : q1;
    j0 = r.boff[q0];
    j1 = r.boff[q1];
}

// one lane per A occurrence k: its sentence, position, and the B-list range it relates to; false when its sentence lies outside the corpus
__device__ __forceinline__ bool rel_a(const RelArgs& r, uint64_t k, uint32_t& a, uint32_t& na, uint32_t& start, uint32_t& end, uint32_t& p) {
    const uint32_t sn = r.rs[k];
    if (sn < r.first_sentence || sn - r.first_sentence >= r.nsent) return false;
    sentence_span(r.delimpos, r.ndelim, r.npos, sn - r.first_sentence, start, end);
    a  = r.aid[k];
    na = r.ntok[a];
    p  = start + r.rt[k];
    return true;
}

// events[k] = the related occurrences of the A occurrence k; *maxev = the most one occurrence has
template <int K>
__global__ __launch_bounds__(kBlock) void rel_events_kernel(RelArgs r, uint64_t nrefs, uint32_t* __restrict__ events, uint32_t* __restrict__ maxev) {
    for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < nrefs; k += (uint64_t)gridDim.x * kBlock) {
        uint32_t a, na, start, end, p, e = 0;
        if (rel_a(r, k, a, na, start, end, p)) {
            const uint32_t ma = r.pmask[a];
            uint64_t       j0, j1;
            rel_span<K>(r, p, na, start, end, j0, j1);
            for (uint64_t j = j0; j < j1; ++j) e += rel_counts<K>(r, a, na, ma, start, p, j) ? 1u : 0u;
        }
        events[k] = e;
        if (e) atomicMax(maxev, e);
    }
}
// the related occurrences of the A occurrences [k0, k1) as (key = B, val = A) at evoff[k] - base
template <int K>
__global__ __launch_bounds__(kBlock) void rel_emit_kernel(RelArgs r, uint64_t k0, uint64_t k1, unsigned long long base, const unsigned long long* __restrict__ evoff,
                                                          uint32_t* __restrict__ kb, uint32_t* __restrict__ ka) {
    for (uint64_t k = k0 + blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < k1; k += (uint64_t)gridDim.x * kBlock) {
        uint32_t a, na, start, end, p;
        if (!rel_a(r, k, a, na, start, end, p)) continue;
        const uint32_t ma = r.pmask[a];
        uint64_t       j0, j1, w = evoff[k] - base;
        rel_span<K>(r, p, na, start, end, j0, j1);
        for (uint64_t j = j0; j < j1; ++j)
            if (rel_counts<K>(r, a, na, ma, start, p, j)) {
                kb[w] = r.bid[j];
                ka[w] = a;
                ++w;
            }
    }
}
// descending order of a count as a sort key (ascending sort)
__global__ __launch_bounds__(kBlock) void rel_countkey_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ perm, uint64_t n, uint32_t* __restrict__ key) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) key[i] = ~cnt[perm[i]];
}

}  // namespace colibri
