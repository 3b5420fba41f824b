// print.hpp — the text of a pattern model (colibri-patternmodeller -P) and its histogram (-H) from the flat export arrays (the host
// loops PatternModel::print / histogram of host/include/patternmodel.h are the specification).
//
// A row:  <text> \t <count> \t <count * n> \t %g(count * n / tokens) \t ngram|skipgram|flexgram \t <n> \t %g(count / (unsigned)grouptotal) [\t s:t s:t ...] \n
// text = the tokens' words joined by one space (the space only when the text so far is not empty: an empty word leaves none), {?} for an id
// without a word; n and the category as cov_info_kernel derives them; the group total from cov_group_kernel (a flexgram has no per-size group:
// its total is 0 and the quotient prints as inf); the two doubles by fmt_g6.hpp. Rows are in the order of the arrays.
//
// The pipeline (print_api.inc drives it):
//   print_reflen_kernel   per reference: digits(sentence) + 1 + digits(token) + 1 (the byte after it: a space, or the row's newline after the last)
//                         -> 64-bit exclusive scan R
//   print_row_kernel      per pattern: the text's length, the two doubles formatted once into a PrintRow, the bytes before the references
//                         (head) and the whole row (head + R[last] - R[first]) -> 64-bit exclusive scan rowstart
//   per output window [W0, W1):
//   print_range_kernel    the patterns whose rows meet the window and, inside the first and the last of them, the references that do
//   print_head_kernel     one lane per pattern: the part of its head that falls in the window
//   print_refs_kernel     one block per slice of the window's references, one lane per reference: balanced by reference, not by pattern, as
//                         coverage.hpp's per-reference kernels are (a pattern of millions of references spreads over thousands of blocks); the
//                         lanes of a wave write adjacent runs of at most 17 bytes
// With instances (colibri_print_instances; below, before the histogram) print_instlen_kernel and print_insts_kernel take the places of print_reflen_kernel and
// print_refs_kernel: the rest of the pipeline is the same.
// The histogram: hist_select_kernel / hist_gather_kernel compact the counts of the patterns of a (category, size) group, the context's radix
// sort orders them, hist_heads_kernel / hist_rows_kernel cut the runs. gfx950 only.
#pragma once
#include "cooc.hpp"
#include "coverage.hpp"
#include "fmt_g6.hpp"

namespace colibri {

constexpr uint32_t kPrintSlice       = 2048;         // references per block of print_refs_kernel (environment: COLIBRI_PRINT_SLICE)
constexpr uint64_t kPrintWindowBytes = 64ull << 20;  // output window (environment: COLIBRI_PRINT_WINDOW_BYTES)
constexpr uint64_t kPrintBudgetBytes = 8ull << 30;   // scratch the call may take (environment: COLIBRI_PRINT_BUDGET)
constexpr uint32_t kPrintBadRow      = 1u;           // PrintInfo.bad: a row of 4 GiB or more

struct PrintRow {  // the two doubles of a row, formatted once
    char    cov[kFmtG6Max], freq[kFmtG6Max];
    uint8_t covlen, freqlen;
};
struct PrintTable {  // the word table: id -> words[wordoff[id] .. wordoff[id + 1]) where has[id] != 0
    const uint32_t* wordoff;
    const uint8_t*  words;
    const uint8_t*  has;
    uint32_t        nids;
};

__device__ __forceinline__ uint32_t print_digits(unsigned long long v) {
    uint32_t           n = 1;
    unsigned long long p = 10;
    while (n < 20 && v >= p) {
        p *= 10u;
        ++n;
    }
    return n;
}
// the decimal digits of v into buf (at most 20); returns their number
__device__ __forceinline__ uint32_t print_number(unsigned long long v, uint8_t* buf) {
    const uint32_t n = print_digits(v);
    for (uint32_t i = n; i-- > 0;) {
        buf[i] = (uint8_t)('0' + (uint32_t)(v % 10u));
        v /= 10u;
    }
    return n;
}

struct PrintCount {  // a sink that only counts
    unsigned long long n = 0;
    __device__ __forceinline__ void put(const uint8_t*, uint32_t len) { n += len; }
};
struct PrintEmit {  // a sink that writes the bytes falling in [lo, hi) to out[q - W0]; pos = where the next byte belongs
    uint8_t*           out;
    unsigned long long pos, lo, hi, W0;
    __device__ __forceinline__ void put(const uint8_t* s, uint32_t len) {
        if (pos + len > lo && pos < hi)
            for (uint32_t i = 0; i < len; ++i) {
                const unsigned long long q = pos + i;
                if (q >= lo && q < hi) out[q - W0] = s[i];
            }
        pos += len;
    }
};

// one token of a text: a space when the text so far is not empty (any), then the id's word, or {?} for an id without one
template <class Sink>
__device__ __forceinline__ void print_word(unsigned long long id, bool& any, const PrintTable& tab, Sink& sink) {
    const uint8_t space = ' ';
    if (any) sink.put(&space, 1);
    if (id < tab.nids && tab.has[id]) {
        const uint32_t a = tab.wordoff[id], n = tab.wordoff[id + 1] - a;
        sink.put(tab.words + a, n);
        any = any || n != 0;
    } else {
        sink.put(reinterpret_cast<const uint8_t*>("{?}"), 3);
        any = true;
    }
}
// Pattern::tostring: the words of the key's tokens
template <class Sink>
__device__ __forceinline__ void print_text(const uint8_t* __restrict__ k, uint32_t len, const PrintTable& tab, Sink& sink) {
    unsigned long long id = 0;
    uint32_t           tb = 0;
    bool               any = false;  // the text so far is not empty
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t b = k[i];
        id |= (unsigned long long)(b & 127u) << (7 * tb);  // (a token of more than kCovMaxToken bytes was refused before)
        ++tb;
        if (b >= 128) continue;
        print_word(id, any, tab, sink);
        id = 0;
        tb = 0;
    }
}

__device__ __forceinline__ uint32_t print_count_of(const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ roff, uint32_t g) {
    return cnt ? cnt[g] : (roff ? (uint32_t)(roff[g + 1] - roff[g]) : 0u);
}
__device__ __forceinline__ uint32_t print_catlen(uint32_t c) { return c == 1 ? 5u : 8u; }  // ngram | skipgram, flexgram

// reflen[r] for r < nrefs, reflen[nrefs] = 0 (the scan's last entry is the total)
__global__ __launch_bounds__(kBlock) void print_reflen_kernel(const uint32_t* __restrict__ rs, const uint16_t* __restrict__ rt, uint64_t nrefs, uint32_t* __restrict__ reflen) {
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r <= nrefs; r += (uint64_t)gridDim.x * kBlock)
        reflen[r] = r < nrefs ? print_digits(rs[r]) + print_digits(rt[r]) + 2u : 0u;
}

// per pattern: its PrintRow, head[g], rowlen[g]; rowlen[np] = 0. gcounts = the counts part of cov_group_kernel's table (group c * G + n).
__global__ __launch_bounds__(kBlock) void print_row_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const uint32_t* __restrict__ cnt,
                                                            const unsigned long long* __restrict__ roff, const unsigned long long* __restrict__ R,
                                                            const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat, uint32_t np, uint32_t G,
                                                            const unsigned long long* __restrict__ gcounts, unsigned long long tokens, PrintTable tab,
                                                            PrintRow* __restrict__ row, uint32_t* __restrict__ head, uint32_t* __restrict__ rowlen, uint32_t* __restrict__ bad) {
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g <= np; g += gridDim.x * kBlock) {
        if (g == np) {
            rowlen[g] = 0;
            continue;
        }
        const uint32_t           count = print_count_of(cnt, roff, g), n = ntok[g], c = cat[g];
        const unsigned long long covc  = (unsigned long long)count * n;
        const uint32_t           gt    = c == 3 ? 0u : (uint32_t)gcounts[c * G + n];  // (unsigned int)totaloccurrencesingroup; a flexgram has no per-size group
        PrintRow                 pr;
        pr.covlen  = (uint8_t)fmt_g6(covc, tokens, pr.cov);
        pr.freqlen = (uint8_t)fmt_g6(count, gt, pr.freq);
        row[g]     = pr;
        PrintCount text;
        print_text(kbytes + koff[g], (uint32_t)(koff[g + 1] - koff[g]), tab, text);
        const unsigned long long refs = roff ? R[roff[g + 1]] - R[roff[g]] : 0ull;  // (the last reference's byte is the newline)
        const unsigned long long h    = text.n + 1 + print_digits(count) + 1 + print_digits(covc) + 1 + pr.covlen + 1 + print_catlen(c) + 1 + print_digits(n) + 1 + pr.freqlen +
                                     (roff ? 1u : 0u) + (refs ? 0u : 1u);
        if (h + refs > 0xFFFFFFFFull) atomicOr(bad, kPrintBadRow);
        head[g]   = (uint32_t)h;
        rowlen[g] = (uint32_t)(h + refs);
    }
}

// range[0] = the first pattern whose row ends after W0, range[1] = the first whose row starts at or after W1; range[2] / range[3] = the
// references [r0, r1) that can meet the window: from the first of pattern range[0] that ends after W0 to the first of pattern range[1] - 1
// that starts at or after W1 (one thread)
__global__ void print_range_kernel(const unsigned long long* __restrict__ rowstart, const uint32_t* __restrict__ head, const unsigned long long* __restrict__ roff,
                                   const unsigned long long* __restrict__ R, uint32_t np, unsigned long long W0, unsigned long long W1, uint32_t* __restrict__ range) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t lo = 0, hi = np;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rowstart[mid + 1] > W0) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t p0 = lo;
    lo = p0, hi = np;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rowstart[mid] >= W1) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t p1 = lo;
    range[0] = p0;
    range[1] = p1;
    range[2] = range[3] = 0;
    if (!roff || p0 >= p1) return;
    {
        const unsigned long long base = rowstart[p0] + head[p0] - R[roff[p0]];
        unsigned long long       a = roff[p0], b = roff[p0 + 1];
        while (a < b) {
            const unsigned long long mid = a + (b - a) / 2;
            if (base + R[mid + 1] > W0) b = mid;
            else a = mid + 1;
        }
        range[2] = (uint32_t)a;
    }
    {
        const uint32_t           pl   = p1 - 1;
        const unsigned long long base = rowstart[pl] + head[pl] - R[roff[pl]];
        unsigned long long       a = roff[pl], b = roff[pl + 1];
        while (a < b) {
            const unsigned long long mid = a + (b - a) / 2;
            if (base + R[mid] >= W1) b = mid;
            else a = mid + 1;
        }
        range[3] = (uint32_t)(a > range[2] ? a : range[2]);
    }
}

// the window's share of the rows' heads: out[q - W0] for q in [W0, W1)
__global__ __launch_bounds__(kBlock) void print_head_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const uint32_t* __restrict__ cnt,
                                                             const unsigned long long* __restrict__ roff, const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat,
                                                             PrintTable tab, const PrintRow* __restrict__ row, const uint32_t* __restrict__ head,
                                                             const unsigned long long* __restrict__ rowstart, const uint32_t* __restrict__ range, unsigned long long W0,
                                                             unsigned long long W1, uint8_t* __restrict__ out) {
    const uint32_t p0 = range[0], p1 = range[1];
    for (uint32_t g = p0 + blockIdx.x * kBlock + threadIdx.x; g < p1; g += gridDim.x * kBlock) {
        const unsigned long long o = rowstart[g], h = head[g];
        if (o + h <= W0 || o >= W1) continue;
        PrintEmit e{out, o, o > W0 ? o : W0, o + h < W1 ? o + h : W1, W0};
        print_text(kbytes + koff[g], (uint32_t)(koff[g + 1] - koff[g]), tab, e);
        const uint32_t count = print_count_of(cnt, roff, g), n = ntok[g], c = cat[g];
        const uint8_t  tabc = '\t', nl = '\n';
        uint8_t        buf[20];
        e.put(&tabc, 1);
        e.put(buf, print_number(count, buf));
        e.put(&tabc, 1);
        e.put(buf, print_number((unsigned long long)count * n, buf));
        e.put(&tabc, 1);
        const PrintRow pr = row[g];
        e.put(reinterpret_cast<const uint8_t*>(pr.cov), pr.covlen);
        e.put(&tabc, 1);
        e.put(reinterpret_cast<const uint8_t*>(c == 1 ? "ngram" : c == 2 ? "skipgram" : "flexgram"), print_catlen(c));
        e.put(&tabc, 1);
        e.put(buf, print_number(n, buf));
        e.put(&tabc, 1);
        e.put(reinterpret_cast<const uint8_t*>(pr.freq), pr.freqlen);
        if (roff) e.put(&tabc, 1);
        if (!roff || roff[g + 1] == roff[g]) e.put(&nl, 1);
    }
}

// the window's share of the references: block b takes the slices b, b + gridDim.x, ... of [range[2], range[3])
__global__ __launch_bounds__(kBlock) void print_refs_kernel(const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ rs, const uint16_t* __restrict__ rt,
                                                             const unsigned long long* __restrict__ R, const uint32_t* __restrict__ head,
                                                             const unsigned long long* __restrict__ rowstart, uint32_t np, uint32_t slice, const uint32_t* __restrict__ range,
                                                             unsigned long long W0, unsigned long long W1, uint8_t* __restrict__ out) {
    __shared__ uint32_t      sb[2];
    const unsigned long long first = range[2], last = range[3];
    for (unsigned long long r0 = first + (unsigned long long)blockIdx.x * slice; r0 < last; r0 += (unsigned long long)gridDim.x * slice) {
        const unsigned long long r1 = min(r0 + slice, last);
        cov_slice_bounds(roff, np, r0, r1, sb);
        const uint32_t plo = sb[0], phi = sb[1];
        for (unsigned long long r = r0 + threadIdx.x; r < r1; r += kBlock) {
            const uint32_t           p = cov_pattern_of(roff, plo, phi, r);
            const unsigned long long o = rowstart[p] + head[p] + (R[r] - R[roff[p]]), n = R[r + 1] - R[r];
            const unsigned long long lo = o > W0 ? o : W0, hi = o + n < W1 ? o + n : W1;
            if (lo >= hi) continue;
            uint8_t  buf[20];
            uint32_t k = print_number(rs[r], buf);
            buf[k++]   = ':';
            k += print_number(rt[r], buf + k);
            buf[k++] = r + 1 == roff[p + 1] ? '\n' : ' ';
            for (unsigned long long q = lo; q < hi; ++q) out[q - W0] = buf[q - o];
        }
        __syncthreads();  // (sb is written again by the next slice)
    }
}

// ---- instances: print(..., instantiate = true) ------------------------------------------------------------------------------------------------
// Behind every reference s:t of a skipgram row of n tokens: '[', the text of the n corpus tokens that start at (s, t), ']' (no byte between them; the
// separator follows as usual). The text is print_text's, read from the corpus' tokens instead of a key's: it does not matter what the skipgram's own tokens
// are. N-gram rows are unchanged; a flexgram in the model is refused before any of this runs (print_api.inc). Two kernels stand in for print_reflen_kernel
// and print_refs_kernel; both find a reference's pattern as print_refs_kernel does and walk its window token by token, one lane per reference.
struct PrintCorpus {  // the resident corpus: token p = bytes[tokstart[p] .. tokstart[p + 1]); the delimiters' positions; the first sentence's number
    const uint8_t*  bytes;
    const uint32_t* tokstart;
    const uint32_t* delimpos;
    uint32_t        ndelim, npos, nsent, first_sentence;
};
// the position of token t of sentence s when the n tokens from there lie inside that sentence; false: a sentence the corpus does not have, or one that ends before
__device__ __forceinline__ bool print_window(const PrintCorpus& C, uint32_t s, uint32_t t, uint32_t n, uint32_t& pos) {
    if (s < C.first_sentence || s - C.first_sentence >= C.nsent) return false;
    uint32_t start, end;
    sentence_span(C.delimpos, C.ndelim, C.npos, s - C.first_sentence, start, end);
    if ((unsigned long long)start + t + n > end) return false;
    pos = start + t;
    return true;
}
// PatternPointer::tostring of the plain window [pos, pos + n) (inside one sentence: print_window)
template <class Sink>
__device__ __forceinline__ void print_window_text(const PrintCorpus& C, uint32_t pos, uint32_t n, const PrintTable& tab, Sink& sink) {
    bool any = false;  // the text so far is not empty
    for (uint32_t p = pos; p < pos + n; ++p) {
        const uint32_t     a = C.tokstart[p], len = C.tokstart[p + 1] - a;
        unsigned long long id = 0;
        for (uint32_t i = 0; i < len; ++i) id = i < kCovMaxToken ? (id | ((unsigned long long)(C.bytes[a + i] & 127u) << (7 * i))) : ~0ull;
        print_word(id, any, tab, sink);
    }
}

constexpr uint32_t kPrintBadRef = 2u;  // PrintInfo.bad: a skipgram's reference whose window is not in the corpus

// reflen[r] for r < nrefs as print_reflen_kernel's, plus 2 + the instance's text for a reference of a skipgram; reflen[nrefs] = 0. Block b takes the slices b,
// b + gridDim.x, ... of the references. A window that does not fit sets kPrintBadRef (nothing of it is read), a reference of 4 GiB or more kPrintBadRow.
__global__ __launch_bounds__(kBlock) void print_instlen_kernel(const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ rs, const uint16_t* __restrict__ rt,
                                                                const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat, uint32_t np, uint64_t nrefs, uint32_t slice,
                                                                PrintCorpus C, PrintTable tab, uint32_t* __restrict__ reflen, uint32_t* __restrict__ bad) {
    __shared__ uint32_t sb[2];
    if (blockIdx.x == 0 && threadIdx.x == 0) reflen[nrefs] = 0;
    for (unsigned long long r0 = (unsigned long long)blockIdx.x * slice; r0 < nrefs; r0 += (unsigned long long)gridDim.x * slice) {
        const unsigned long long r1 = min(r0 + slice, (unsigned long long)nrefs);
        cov_slice_bounds(roff, np, r0, r1, sb);
        const uint32_t plo = sb[0], phi = sb[1];
        for (unsigned long long r = r0 + threadIdx.x; r < r1; r += kBlock) {
            const uint32_t     p   = cov_pattern_of(roff, plo, phi, r);
            unsigned long long len = print_digits(rs[r]) + print_digits(rt[r]) + 2u;
            if (cat[p] == 2) {
                uint32_t pos;
                if (print_window(C, rs[r], rt[r], ntok[p], pos)) {
                    PrintCount text;
                    print_window_text(C, pos, ntok[p], tab, text);
                    len += 2u + text.n;
                } else {
                    atomicOr(bad, kPrintBadRef);
                }
            }
            if (len > 0xFFFFFFFFull) atomicOr(bad, kPrintBadRow);
            reflen[r] = (uint32_t)len;
        }
        __syncthreads();  // (sb is written again by the next slice)
    }
}

// print_refs_kernel with instances: s:t, then for a skipgram's reference [ the window's words ], then the separator, all through the clipped sink: a window
// of the output may cut a reference at any byte. (print_instlen_kernel has seen every window fit; one that would not is left out, never read.)
__global__ __launch_bounds__(kBlock) void print_insts_kernel(const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ rs, const uint16_t* __restrict__ rt,
                                                              const unsigned long long* __restrict__ R, const uint32_t* __restrict__ head,
                                                              const unsigned long long* __restrict__ rowstart, const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat,
                                                              uint32_t np, uint32_t slice, const uint32_t* __restrict__ range, PrintCorpus C, PrintTable tab, unsigned long long W0,
                                                              unsigned long long W1, uint8_t* __restrict__ out) {
    __shared__ uint32_t      sb[2];
    const unsigned long long first = range[2], last = range[3];
    for (unsigned long long r0 = first + (unsigned long long)blockIdx.x * slice; r0 < last; r0 += (unsigned long long)gridDim.x * slice) {
        const unsigned long long r1 = min(r0 + slice, last);
        cov_slice_bounds(roff, np, r0, r1, sb);
        const uint32_t plo = sb[0], phi = sb[1];
        for (unsigned long long r = r0 + threadIdx.x; r < r1; r += kBlock) {
            const uint32_t           p = cov_pattern_of(roff, plo, phi, r);
            const unsigned long long o = rowstart[p] + head[p] + (R[r] - R[roff[p]]), n = R[r + 1] - R[r];
            const unsigned long long lo = o > W0 ? o : W0, hi = o + n < W1 ? o + n : W1;
            if (lo >= hi) continue;
            PrintEmit e{out, o, lo, hi, W0};
            uint8_t   buf[42];
            uint32_t  k = print_number(rs[r], buf);
            buf[k++]    = ':';
            k += print_number(rt[r], buf + k);
            e.put(buf, k);
            uint32_t pos;
            if (cat[p] == 2 && print_window(C, rs[r], rt[r], ntok[p], pos)) {
                const uint8_t open = '[', close = ']';
                e.put(&open, 1);
                print_window_text(C, pos, ntok[p], tab, e);
                e.put(&close, 1);
            }
            const uint8_t sep = r + 1 == roff[p + 1] ? '\n' : ' ';
            e.put(&sep, 1);
        }
        __syncthreads();  // (sb is written again by the next slice)
    }
}

// ---- histogram -------------------------------------------------------------------------------------------------------------------------------
// flag[g] = pattern g is of the group (category 0 = any, size 0 = any; ntok / cat may be NULL when both are 0)
__global__ __launch_bounds__(kBlock) void hist_select_kernel(const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat, uint32_t np, uint32_t category, uint32_t size,
                                                              uint32_t* __restrict__ flag) {
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < np; g += gridDim.x * kBlock)
        flag[g] = ((category == 0 || cat[g] == category) && (size == 0 || ntok[g] == size)) ? 1u : 0u;
}
__global__ __launch_bounds__(kBlock) void hist_gather_kernel(const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ flag,
                                                              const unsigned long long* __restrict__ pos, uint32_t np, uint32_t* __restrict__ key) {
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < np; g += gridDim.x * kBlock)
        if (flag[g]) key[pos[g]] = print_count_of(cnt, roff, g);
}
// flag[i] = key[i] opens a run of the sorted counts
__global__ __launch_bounds__(kBlock) void hist_heads_kernel(const uint32_t* __restrict__ key, uint32_t m, uint32_t* __restrict__ flag) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock) flag[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}
__global__ __launch_bounds__(kBlock) void hist_rows_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ flag, const unsigned long long* __restrict__ rank, uint32_t m,
                                                            uint32_t* __restrict__ value, uint32_t* __restrict__ start) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock)
        if (flag[i]) {
            value[rank[i]] = key[i];
            start[rank[i]] = i;
        }
}

}  // namespace colibri
