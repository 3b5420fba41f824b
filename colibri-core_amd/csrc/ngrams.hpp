// ngrams.hpp — n-gram extraction (colibri-extractngrams; reference src/extractngrams.cpp:62-73): every window of n tokens inside a line of the
// tokenised corpus as text, one per row, in corpus order.
//
// Specification: for each line of T tokens (a run of tokens ended by a 00 or by the end of the data) and i = 0 .. T - n, the text of the
// tokens i .. i + n - 1 and "\n". The text is print.hpp's (print_word: the id's word, {?} for an id without one, a space before a token only when the
// text so far is not empty). A line of fewer than n tokens prints nothing.
//
// The pipeline (ngrams_api.inc drives it), on what colibri_decode_upload leaves (cls per position, 0 = a 00; delimpos) and the table of
// colibri_print_classes:
//   ngrams_word_kernel    per position: wl = the bytes of its token's text (0 for a 00), and the flag "an n-gram starts here" (the tokens left in
//                         its line, from delimpos, are at least n)                         -> 64-bit exclusive scans P (of wl) and of the flags
//   ngrams_gather_kernel  the positions of the n-grams, in order (gpos), and the bytes of each: P[i + n] - P[i], the separators (i + n - 1 - f for the
//                         first token f of the window with wl > 0, none without one) and the newline -> 64-bit exclusive scan G
//   per output window [W0, W1): decode_range_kernel over G, then
//   ngrams_lane_kernel    one lane per n-gram: the part of its text that falls in the window, byte by byte (the shape of decode_write_kernel). Only
//                         positions that start an n-gram have a lane (that is what the gather is for: a run of empty lines has none), and the lanes
//                         of a wave write adjacent rows.
// A second write kernel, one lane per aligned 16-byte piece of the window with the n-grams' starts staged in LDS, wrote the same bytes but was slower
// where it was measured (DESIGN §5n has the two numbers) and is not part of this file.
// gfx950 only.
#pragma once
#include "decode.hpp"
#include "print.hpp"

namespace colibri {

constexpr uint64_t kNgramsWindowBytes = 64ull << 20;  // output window (environment: COLIBRI_NGRAMS_WINDOW_BYTES)
constexpr uint32_t kNgramsBadRow      = 1u;           // a word or an n-gram of kNgramsMaxRow bytes or more
constexpr uint32_t kNgramsMaxRow      = 1u << 22;     // scan_apply_kernel adds the kBlock * 4 = 1024 lengths of a tile in 32 bits: below 4 MiB each, no tile's sum reaches 2^32

__device__ __forceinline__ uint32_t ngrams_wordlen(uint32_t id, const PrintTable& tab) {
    return (id < tab.nids && tab.has[id]) ? tab.wordoff[id + 1] - tab.wordoff[id] : 3u;  // {?}
}

// wl[i], flag[i] for i < npos. The line of position i ends at the first 00 at or after i, or at npos. A word of kNgramsMaxRow bytes or more sets kNgramsBadRow.
__global__ __launch_bounds__(kBlock) void ngrams_word_kernel(const uint32_t* __restrict__ cls, const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos,
                                                              unsigned long long n, PrintTable tab, uint32_t* __restrict__ wl, uint32_t* __restrict__ flag,
                                                              uint32_t* __restrict__ bad) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < npos; i += gridDim.x * kBlock) {
        const uint32_t id = cls[i];
        if (id == 0) {
            wl[i] = flag[i] = 0;
            continue;
        }
        uint32_t lo = 0, hi = ndelim;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (delimpos[mid] >= i) hi = mid;
            else lo = mid + 1;
        }
        const unsigned long long rem = (lo < ndelim ? delimpos[lo] : npos) - i;
        const uint32_t           w   = ngrams_wordlen(id, tab);
        if (w >= kNgramsMaxRow) atomicOr(bad, kNgramsBadRow);
        wl[i]   = w;
        flag[i] = rem >= n ? 1u : 0u;
    }
}

// for every position with a flag: gpos[idx[i]] = i, glen[idx[i]] = the bytes of its n-gram
__global__ __launch_bounds__(kBlock) void ngrams_gather_kernel(const uint32_t* __restrict__ wl, const uint32_t* __restrict__ flag, const unsigned long long* __restrict__ idx,
                                                                const unsigned long long* __restrict__ P, uint32_t npos, uint32_t n, uint32_t* __restrict__ gpos,
                                                                uint32_t* __restrict__ glen, uint32_t* __restrict__ bad) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < npos; i += gridDim.x * kBlock) {
        if (!flag[i]) continue;  // (flag: i + n <= npos)
        uint32_t f = 0;
        while (f < n && wl[i + f] == 0) ++f;
        const unsigned long long len = P[i + n] - P[i] + (f < n ? n - 1 - f : 0u) + 1u;
        if (len >= kNgramsMaxRow) atomicOr(bad, kNgramsBadRow);
        const unsigned long long k = idx[i];
        gpos[k]                    = i;
        glen[k]                    = (uint32_t)len;
    }
}

// the text of the n-gram at position i: its tokens' words, then the newline
template <class Sink>
__device__ __forceinline__ void ngrams_text(const uint32_t* __restrict__ cls, uint32_t i, uint32_t n, const PrintTable& tab, Sink& sink) {
    bool any = false;  // the text so far is not empty
    for (uint32_t t = 0; t < n && !sink.done(); ++t) print_word(cls[i + t], any, tab, sink);
    const uint8_t nl = '\n';
    sink.put(&nl, 1);
}

struct NgramEmit : PrintEmit {  // PrintEmit that knows when nothing more can fall into [lo, hi)
    __device__ __forceinline__ bool done() const { return pos >= hi; }
};

// the window's text, one lane per n-gram of [range[0], range[1]): out[q - W0] for q in [W0, W1)
__global__ __launch_bounds__(kBlock) void ngrams_lane_kernel(const uint32_t* __restrict__ cls, const uint32_t* __restrict__ gpos, const unsigned long long* __restrict__ G,
                                                              uint32_t n, PrintTable tab, const uint32_t* __restrict__ range, unsigned long long W0, unsigned long long W1,
                                                              uint8_t* __restrict__ out) {
    const uint32_t k0 = range[0], k1 = range[1];
    for (uint32_t k = k0 + blockIdx.x * kBlock + threadIdx.x; k < k1; k += gridDim.x * kBlock) {
        const unsigned long long o = G[k], e = G[k + 1];
        NgramEmit                s;
        s.out = out, s.pos = o, s.lo = o > W0 ? o : W0, s.hi = e < W1 ? e : W1, s.W0 = W0;
        if (s.lo >= s.hi) continue;
        ngrams_text(cls, gpos[k], n, tab, s);
    }
}

}  // namespace colibri
