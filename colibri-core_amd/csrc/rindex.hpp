// rindex.hpp — the reverse index as a product of its own (colibri-patternmodeller -Z, PatternModel::getreverseindex / printreverseindex;
// reference include/patternmodel.h:1746-1862, :2325-2338).
//
// For every real token position (s, t) of the corpus: the patterns of the model that start there — the window of n tokens, MINLENGTH <= n <=
// MAXLENGTH, when the model has it, and (n >= 3) that window under every gap mask a skipgram of the model has at that length, when the model has
// that key — filtered by occurrence count (per pattern), category and size (per layer). The order is defined: positions ascending, n ascending,
// the n-gram before its skipgrams, masks ascending. The look-ups are co-occurrence's (cooc_api.inc: the key table and one probe layer per
// length / per (length, mask)); they run over position ranges of the corpus, so the layer array is bounded by a scratch budget.
//
// The pipeline (rindex_api.inc drives it), per chunk [p0, p0 + n) of positions (delimiters included):
//   constraint_probe_*      per position and layer: the pattern number of the window
//   rindex_hits_kernel      per position: the patterns that pass the count filter -> 64-bit scan
//   rindex_fill_kernel      per real position r (= position - sentences before it): pos_off[r], sentence[r], token[r], and its patterns in order
// The text (printreverseindex: "s:t" then "\t<pattern text>" per pattern, "\n"; one more "\n" after the last line):
//   rindex_textlen_kernel / rindex_arena_kernel   the text of every pattern, once (print_text of print.hpp), with an offset array
//   rindex_linelen_kernel   per position: digits(s) + 1 + digits(t) + sum(1 + textlen) + 1 -> 64-bit scan (entry nreal is the closing newline)
//   per output window [W0, W1):
//   rindex_range_kernel     the positions whose lines meet the window, and their range of row entries
//   rindex_head_kernel      one lane per position: "s:t" and the line's newline
//   rindex_entry_kernel     one lane per row entry (balanced by entry, not by position): the tab and the pattern's text from the arena; the
//                           lanes of a wave write adjacent runs. A window may cut a line, a number or a word anywhere. gfx950 only.
#pragma once
#include "cooc.hpp"
#include "print.hpp"

namespace colibri {

constexpr uint64_t kRindexBudgetBytes = 8ull << 30;   // scratch and result the calls may take (environment: COLIBRI_RINDEX_BUDGET)
constexpr uint64_t kRindexWindowBytes = 64ull << 20;  // output window of the text (environment: COLIBRI_RINDEX_WINDOW_BYTES)
constexpr uint32_t kRindexBadToken    = 1u;           // a token index above 65535
constexpr uint32_t kRindexBadLine     = 2u;           // a line of 4 GiB or more

// sentence (0-based, = delimiters before i) of position i and that sentence's first position
__device__ __forceinline__ void rindex_locate(const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t i, uint32_t& s, uint32_t& start) {
    uint32_t lo = 0, hi = ndelim;  // first delimiter position >= i
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (delimpos[mid] < i)
            lo = mid + 1;
        else
            hi = mid;
    }
    s     = lo;
    start = lo == 0 ? 0u : delimpos[lo - 1] + 1;
}

// hits[j] = patterns at position p0 + j that pass the count filter (a delimiter has none: every probe misses there); hits[n] = 0
__global__ __launch_bounds__(kBlock) void rindex_hits_kernel(const uint32_t* __restrict__ memb, size_t stride, uint32_t nlayers, uint32_t n, const uint32_t* __restrict__ cnt,
                                                             uint32_t thr, uint32_t* __restrict__ hits) {
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j <= n; j += gridDim.x * kBlock) {
        uint32_t h = 0;
        if (j < n)
            for (uint32_t l = 0; l < nlayers; ++l) h += cooc_hit(memb[(size_t)l * stride + j], cnt, thr) ? 1u : 0u;
        hits[j] = h;
    }
}
// the chunk's share of the result: for the real position r of p0 + j, pos_off[r] = base + boff[j], its sentence and token, and its patterns in
// the order of `order` (layer numbers by n, the n-gram before the skipgrams, masks ascending)
__global__ __launch_bounds__(kBlock) void rindex_fill_kernel(const uint32_t* __restrict__ memb, size_t stride, uint32_t nlayers, const uint32_t* __restrict__ order, uint32_t p0,
                                                             uint32_t n, const uint32_t* __restrict__ rem, const uint32_t* __restrict__ delimpos, uint32_t ndelim,
                                                             uint32_t first_sentence, const uint32_t* __restrict__ cnt, uint32_t thr, const unsigned long long* __restrict__ boff,
                                                             unsigned long long base, unsigned long long* __restrict__ pos_off, uint32_t* __restrict__ sentence,
                                                             uint16_t* __restrict__ token, uint32_t* __restrict__ pattern, uint32_t* __restrict__ bad) {
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
        const uint32_t i = p0 + j;
        if (rem[i] == 0) continue;  // a delimiter
        uint32_t s, start;
        rindex_locate(delimpos, ndelim, i, s, start);
        const uint32_t     r = i - s, t = i - start;
        unsigned long long o = base + boff[j];
        pos_off[r]  = o;
        sentence[r] = first_sentence + s;
        token[r]    = (uint16_t)t;
        if (t > 0xFFFFu) atomicOr(bad, kRindexBadToken);
        for (uint32_t q = 0; q < nlayers; ++q) {
            const uint32_t b = memb[(size_t)order[q] * stride + j];
            if (cooc_hit(b, cnt, thr)) pattern[o++] = b;
        }
    }
}

// ---- the text ----------------------------------------------------------------------------------------------------------------------------------
// tlen[p] = bytes of pattern p's text (print_text), tlen[np] = 0
__global__ __launch_bounds__(kBlock) void rindex_textlen_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, uint32_t np, PrintTable tab,
                                                                uint32_t* __restrict__ tlen, uint32_t* __restrict__ bad) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p <= np; p += gridDim.x * kBlock) {
        PrintCount text;
        if (p < np) print_text(kbytes + koff[p], (uint32_t)(koff[p + 1] - koff[p]), tab, text);
        if (text.n >= 0xFFFFFFF0ull) atomicOr(bad, kRindexBadLine);
        tlen[p] = (uint32_t)text.n;
    }
}
__global__ __launch_bounds__(kBlock) void rindex_arena_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, uint32_t np, PrintTable tab,
                                                              const unsigned long long* __restrict__ toff, uint8_t* __restrict__ arena) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < np; p += gridDim.x * kBlock) {
        PrintEmit e{arena, toff[p], 0ull, ~0ull, 0ull};
        print_text(kbytes + koff[p], (uint32_t)(koff[p + 1] - koff[p]), tab, e);
    }
}
__device__ __forceinline__ uint32_t rindex_headlen(uint32_t s, uint32_t t) { return print_digits(s) + 1u + print_digits(t); }
// linelen[r] for r < nreal; linelen[nreal] = 1 (the closing newline), linelen[nreal + 1] = 0 (the scan's last entry is the total)
__global__ __launch_bounds__(kBlock) void rindex_linelen_kernel(const unsigned long long* __restrict__ pos_off, const uint32_t* __restrict__ sentence,
                                                                const uint16_t* __restrict__ token, const uint32_t* __restrict__ pattern, const uint32_t* __restrict__ tlen,
                                                                uint32_t nreal, uint32_t* __restrict__ linelen, uint32_t* __restrict__ bad) {
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r <= (uint64_t)nreal + 1; r += (uint64_t)gridDim.x * kBlock) {
        if (r >= nreal) {
            linelen[r] = r == nreal ? 1u : 0u;
            continue;
        }
        unsigned long long len = rindex_headlen(sentence[r], token[r]) + 1u;
        for (unsigned long long k = pos_off[r]; k < pos_off[r + 1]; ++k) len += 1ull + tlen[pattern[k]];
        if (len > 0xFFFFFFFFull) atomicOr(bad, kRindexBadLine);
        linelen[r] = (uint32_t)len;
    }
}
// range[0] = the first line (0 .. nreal, nreal = the closing newline) that ends after W0, range[1] = the first that starts at or after W1;
// range[2] / range[3] = the row entries of the positions among them (one thread)
__global__ void rindex_range_kernel(const unsigned long long* __restrict__ linestart, const unsigned long long* __restrict__ pos_off, uint32_t nreal, unsigned long long W0,
                                    unsigned long long W1, unsigned long long* __restrict__ range) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long nlines = (unsigned long long)nreal + 1;
    unsigned long long       lo = 0, hi = nlines;
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (linestart[mid + 1] > W0) hi = mid;
        else lo = mid + 1;
    }
    const unsigned long long r0 = lo;
    hi = nlines;
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (linestart[mid] >= W1) hi = mid;
        else lo = mid + 1;
    }
    const unsigned long long r1 = lo;
    range[0] = r0;
    range[1] = r1;
    range[2] = pos_off[r0 < nreal ? r0 : nreal];
    range[3] = pos_off[r1 < nreal ? r1 : nreal];
}
// the window's share of the lines' heads ("s:t") and newlines: out[q - W0] for q in [W0, W1)
__global__ __launch_bounds__(kBlock) void rindex_head_kernel(const unsigned long long* __restrict__ linestart, const uint32_t* __restrict__ sentence, const uint16_t* __restrict__ token,
                                                             uint32_t nreal, const unsigned long long* __restrict__ range, unsigned long long W0, unsigned long long W1,
                                                             uint8_t* __restrict__ out) {
    const unsigned long long r0 = range[0], r1 = range[1];
    for (unsigned long long r = r0 + (unsigned long long)blockIdx.x * kBlock + threadIdx.x; r < r1; r += (unsigned long long)gridDim.x * kBlock) {
        const uint8_t nl = '\n';
        PrintEmit     e{out, linestart[r], W0, W1, W0};
        if (r < nreal) {
            uint8_t  buf[32];
            uint32_t k = print_number(sentence[r], buf);
            buf[k++]   = ':';
            k += print_number(token[r], buf + k);
            e.put(buf, k);
            e.pos = linestart[r + 1] - 1;
        }
        e.put(&nl, 1);
    }
}
// the window's share of the row entries [range[2], range[3]): entry k of position r is "\t" + the text of pattern[k], after the line's head and
// the entries before it
__global__ __launch_bounds__(kBlock) void rindex_entry_kernel(const unsigned long long* __restrict__ linestart, const unsigned long long* __restrict__ pos_off,
                                                              const uint32_t* __restrict__ sentence, const uint16_t* __restrict__ token, const uint32_t* __restrict__ pattern,
                                                              const uint32_t* __restrict__ tlen, const unsigned long long* __restrict__ toff, const uint8_t* __restrict__ arena,
                                                              uint32_t nreal, const unsigned long long* __restrict__ range, unsigned long long W0, unsigned long long W1,
                                                              uint8_t* __restrict__ out) {
    const unsigned long long r0 = range[0], r1 = range[1] < nreal ? range[1] : nreal, k0 = range[2], k1 = range[3];
    for (unsigned long long k = k0 + (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < k1; k += (unsigned long long)gridDim.x * kBlock) {
        unsigned long long lo = r0, hi = r1;  // the first position r with pos_off[r + 1] > k
        while (lo < hi) {
            const unsigned long long mid = lo + (hi - lo) / 2;
            if (pos_off[mid + 1] > k) hi = mid;
            else lo = mid + 1;
        }
        const unsigned long long r = lo;
        unsigned long long       o = linestart[r] + rindex_headlen(sentence[r], token[r]);
        for (unsigned long long j = pos_off[r]; j < k; ++j) o += 1ull + tlen[pattern[j]];
        const uint32_t p = pattern[k], n = tlen[p];
        if (o + 1 + n <= W0 || o >= W1) continue;
        const uint8_t tabc = '\t';
        PrintEmit     e{out, o, W0, W1, W0};
        e.put(&tabc, 1);
        e.put(arena + toff[p], n);
    }
}

}  // namespace colibri
