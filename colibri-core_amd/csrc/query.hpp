// query.hpp — a pattern model queried with new text (colibri-patternmodeller -q / --queryfile, PatternModel::getpatterns / query; reference
// src/patternmodeller.cpp:160-231, include/patternmodel.h:2272-2285).
//
// The text is a payload of its own (lines closed by the delimiter byte, empty lines kept); the context's corpus and trained model are not
// written. Per line s (number first_line + s) with pattern P of T tokens, in extensive mode: the row (s, 0, P) when the model has P, then for
// n = minlength .. min(maxlength, T) and i = 0 .. T - n the row (s, i, window) when the model has the window of n tokens at i. In exact mode
// (exact[s] != 0): one row (s, 0, P), with pattern number 0xFFFFFFFF when the model does not have P. The order of the rows is a function of the
// input alone: line-major, the whole-line row first, then length-major, then by token.
//
// The pipeline (query_api.inc drives it). A cell is a (line, k) pair, k = 0 the whole-line row, k = 1 + l the windows of layer l (n = n0 + l):
//   query_whole_kernel     per line: its whole-line look-up (at its own length, whatever minlength / maxlength; a line longer than the model's
//                          longest pattern misses without a probe) -> cell (s, 0)
//   per chunk [p0, p0 + n) of positions (delimiters included; a chunk may cut a line anywhere):
//   constraint_probe_*     per position and layer: the pattern number of the window (constrained.hpp)
//   query_posline_kernel   per position: its line
//   query_flags_kernel     per (layer, position): 1 where the window is a row -> one 64-bit scan over the layers' rows, laid end to end
//   query_count_kernel     per (layer, position): the position that opens a line's share of the chunk adds that share's hits, a difference
//                          of two scan entries, to its cell. One lane per cell and chunk, chunks in stream order: no atomics.
//   one 64-bit scan of the cells -> the first row of every cell; query_lineoff_kernel cuts line_off from it
//   query_wholefill_kernel per line: its whole-line row
//   per chunk again (a single chunk keeps its layers: no second probe):
//   query_fill_kernel      per (layer, position): a hit's row = its cell's first row + its rank in the cell = hits of the line's share of the
//                          chunk before it (scan difference) + the line's hits in earlier chunks (carry)
//   query_carry_kernel     per layer: the hits so far of the line that runs on into the next chunk
// Work is per position and layer throughout: a line of 65 536 tokens is spread like any other 65 536 positions.
//
// The text (a row of extensive mode: "L:i\t" + the pattern's print() row; exact mode: the print() row, or PATTERN "<line>" NOT FOUND IN MODEL):
//   query_mark_kernel / query_compact_kernel   the patterns hit at least once, compacted, with the number of references of each
//   query_reflen_kernel    the hit patterns' references, numbered by a scan of those numbers: the bytes of each ("s:t" + one byte)
//   query_row_kernel       per hit pattern: PrintRow, head and row length (print.hpp's pieces) -> scan -> arena offsets
//   query_head_kernel / query_refs_kernel      the arena: one lane per hit pattern / per compacted reference
//   query_miss_* kernels   the NOT FOUND lines of the exact-mode misses, into a second arena
//   query_rowlen_kernel    per result row: prefix + arena run -> 64-bit scan
//   query_emit_kernel      per output window: one lane per kQuerySeg bytes of the window (balanced by output byte: a row of millions of
//                          references spreads over as many lanes as it has segments). A window may cut a row anywhere.
// All of them are plain grid-stride kernels, built for gfx950 like the rest of the library: no LDS, no wave-level operation.
#pragma once
#include "rindex.hpp"

namespace colibri {

constexpr uint64_t kQueryBudgetBytes = 8ull << 30;   // scratch and result a call may take (environment: COLIBRI_QUERY_BUDGET)
constexpr uint64_t kQueryWindowBytes = 64ull << 20;  // output window of the text (environment: COLIBRI_QUERY_WINDOW_BYTES)
constexpr uint32_t kQueryMaxLine     = 65536u;       // tokens of a line: the reference prints (int) of a 16-bit token index
constexpr uint32_t kQueryBadLine     = 1u;           // a line of more than kQueryMaxLine tokens
constexpr uint32_t kQueryBadText     = 2u;           // a text line of 4 GiB or more
constexpr uint32_t kQuerySeg         = 32u;          // output bytes per lane of query_emit_kernel
constexpr uint32_t kQueryMissHead    = 9u;           // PATTERN "
constexpr uint32_t kQueryMissTail    = 21u;          // " NOT FOUND IN MODEL\n

// first position and number of tokens of line s (the positions between two delimiters; the last line may lack its delimiter)
__device__ __forceinline__ void query_line(const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos, uint32_t s, uint32_t& start, uint32_t& T) {
    start = s == 0 ? 0u : delimpos[s - 1] + 1;
    T     = (s < ndelim ? delimpos[s] : npos) - start;
}

// cells[s * K] = rows of the whole-line look-up of line s (exact: 1, hit or miss), whole[s] = its pattern number (kInvalid: none)
__global__ __launch_bounds__(kBlock) void query_whole_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ tokstart, const uint32_t* __restrict__ delimpos,
                                                             uint32_t ndelim, uint32_t npos, uint32_t nlines, const uint8_t* __restrict__ exact, const CSlot* __restrict__ table,
                                                             uint32_t cap, const uint8_t* __restrict__ jbytes, const unsigned long long* __restrict__ joff, uint32_t np,
                                                             uint32_t maxn /* tokens of the model's longest pattern */, uint32_t K, uint64_t hmask, uint32_t* __restrict__ cells,
                                                             uint32_t* __restrict__ whole, uint32_t* __restrict__ bad) {
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < nlines; s += gridDim.x * kBlock) {
        uint32_t start, T;
        query_line(delimpos, ndelim, npos, s, start, T);
        if (T > kQueryMaxLine) atomicOr(bad, kQueryBadLine);
        uint32_t found = kInvalid;
        if (np != 0 && T >= 1 && T <= maxn) {
            const uint32_t a0 = tokstart[start];
            uint64_t       h  = kConstraintSeed;
            uint32_t       a  = a0;
            for (uint32_t k = 0; k < T; ++k) {
                const uint32_t e = tokstart[start + k + 1];
                h                = fold_chunk(h, bytes + a, e - a);  // (a token of the text has at most 8 bytes: checked at its upload)
                a                = e;
            }
            h = (h == kEmptyKey ? h ^ 1ull : h) & hmask;
            const uint32_t sl = slot_of_hash(mix64(h), cap);
            found             = constraint_lookup(bytes + a0, a - a0, h, table[sl], sl, table, cap, jbytes, joff);
        }
        whole[s]                = found;
        cells[(size_t)s * K]    = (exact && exact[s]) ? 1u : (found != kInvalid ? 1u : 0u);
    }
}

// posline[j] = the line of position p0 + j (a delimiter belongs to the line it closes)
__global__ __launch_bounds__(kBlock) void query_posline_kernel(const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t p0, uint32_t n, uint32_t* __restrict__ posline) {
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
        uint32_t s, start;
        rindex_locate(delimpos, ndelim, p0 + j, s, start);
        posline[j] = s;
    }
}

// flags[l * stride + j] = the window of layer l at position p0 + j is a row (a hit in a line of extensive mode); 0 at j == n
__global__ __launch_bounds__(kBlock) void query_flags_kernel(const uint32_t* __restrict__ memb, size_t stride, uint32_t L, uint32_t n, const uint32_t* __restrict__ posline,
                                                             const uint8_t* __restrict__ exact, uint32_t* __restrict__ flags) {
    const uint64_t total = (uint64_t)L * stride;
    for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < total; x += (uint64_t)gridDim.x * kBlock) {
        const uint32_t j = (uint32_t)(x % stride);
        flags[x]         = (j < n && memb[x] != kInvalid && !(exact && exact[posline[j]])) ? 1u : 0u;
    }
}

// the share of the chunk that line `line`, which holds position p0 + j, has: [a, b) in chunk positions
__device__ __forceinline__ void query_share(const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos, uint32_t line, uint32_t p0, uint32_t n, uint32_t& start,
                                            uint32_t& a, uint32_t& b) {
    uint32_t T;
    query_line(delimpos, ndelim, npos, line, start, T);
    const uint32_t end = start + T;
    a                  = start > p0 ? start - p0 : 0u;
    b                  = end < p0 + n ? end - p0 : n;
}

// cells[line * K + 1 + l] += the hits of layer l in the line's share of the chunk: added by the lane of the share's first position
__global__ __launch_bounds__(kBlock) void query_count_kernel(const unsigned long long* __restrict__ pref, size_t stride, uint32_t L, uint32_t p0, uint32_t n,
                                                             const uint32_t* __restrict__ posline, const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos, uint32_t K,
                                                             uint32_t* __restrict__ cells) {
    const uint64_t total = (uint64_t)L * n;
    for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < total; x += (uint64_t)gridDim.x * kBlock) {
        const uint32_t l = (uint32_t)(x / n), j = (uint32_t)(x % n);
        const uint32_t line = posline[j];
        uint32_t       start, a, b;
        query_share(delimpos, ndelim, npos, line, p0, n, start, a, b);
        if (j != a || a >= b) continue;  // (a delimiter that opens the chunk: a == b)
        const unsigned long long* pl = pref + (size_t)l * stride;
        const uint32_t            h  = (uint32_t)(pl[b] - pl[a]);
        if (h) cells[(size_t)line * K + 1 + l] += h;
    }
}

__global__ __launch_bounds__(kBlock) void query_lineoff_kernel(const unsigned long long* __restrict__ celloff, uint32_t nlines, uint32_t K, unsigned long long nrows,
                                                               unsigned long long* __restrict__ line_off) {
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s <= nlines; s += gridDim.x * kBlock) line_off[s] = s < nlines ? celloff[(size_t)s * K] : nrows;
}

__global__ __launch_bounds__(kBlock) void query_wholefill_kernel(const uint32_t* __restrict__ cells, const unsigned long long* __restrict__ celloff, const uint32_t* __restrict__ whole,
                                                                 uint32_t nlines, uint32_t K, uint16_t* __restrict__ token, uint32_t* __restrict__ pattern,
                                                                 uint32_t* __restrict__ rowline) {
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < nlines; s += gridDim.x * kBlock) {
        if (!cells[(size_t)s * K]) continue;
        const unsigned long long o = celloff[(size_t)s * K];
        token[o]   = 0;
        pattern[o] = whole[s];
        rowline[o] = s;
    }
}

// the rows of the chunk's hits: row = the cell's first row + hits of the line's share before j + carry[l] (the line's hits in earlier chunks)
__global__ __launch_bounds__(kBlock) void query_fill_kernel(const uint32_t* __restrict__ memb, const uint32_t* __restrict__ flags, const unsigned long long* __restrict__ pref,
                                                            size_t stride, uint32_t L, uint32_t p0, uint32_t n, const uint32_t* __restrict__ posline,
                                                            const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos, uint32_t K,
                                                            const unsigned long long* __restrict__ celloff, const uint32_t* __restrict__ carry, uint16_t* __restrict__ token,
                                                            uint32_t* __restrict__ pattern, uint32_t* __restrict__ rowline) {
    const uint64_t total = (uint64_t)L * n;
    for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < total; x += (uint64_t)gridDim.x * kBlock) {
        const uint32_t l = (uint32_t)(x / n), j = (uint32_t)(x % n);
        const size_t   at = (size_t)l * stride + j;
        if (!flags[at]) continue;
        const uint32_t line = posline[j];
        uint32_t       start, a, b;
        query_share(delimpos, ndelim, npos, line, p0, n, start, a, b);
        const unsigned long long rank = pref[at] - pref[(size_t)l * stride + a] + (start < p0 ? carry[l] : 0u);
        const unsigned long long o    = celloff[(size_t)line * K + 1 + l] + rank;
        token[o]   = (uint16_t)(p0 + j - start);
        pattern[o] = memb[at];
        rowline[o] = line;
    }
}

// carry[l] for the next chunk: the hits so far of the line that the chunk's end cuts (0 when it cuts none)
__global__ __launch_bounds__(kBlock) void query_carry_kernel(const unsigned long long* __restrict__ pref, size_t stride, uint32_t L, uint32_t p0, uint32_t n,
                                                             const uint32_t* __restrict__ posline, const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos,
                                                             uint32_t* __restrict__ carry) {
    for (uint32_t l = blockIdx.x * kBlock + threadIdx.x; l < L; l += gridDim.x * kBlock) {
        const uint32_t line = posline[n - 1];
        uint32_t       start, T, a, b;
        query_line(delimpos, ndelim, npos, line, start, T);
        query_share(delimpos, ndelim, npos, line, p0, n, start, a, b);
        uint32_t v = 0;
        if (start + T > p0 + n) {  // the line has tokens beyond the chunk
            const unsigned long long* pl = pref + (size_t)l * stride;
            v                            = (start < p0 ? carry[l] : 0u) + (uint32_t)(pl[b] - pl[a]);
        }
        carry[l] = v;
    }
}

// ---- the text ----------------------------------------------------------------------------------------------------------------------------------
// flag[p] = 1 for every pattern some row names (every writer stores the same value); missflag[r] = row r is an exact-mode miss; [nrows] = 0
__global__ __launch_bounds__(kBlock) void query_mark_kernel(const uint32_t* __restrict__ pattern, unsigned long long nrows, uint32_t* __restrict__ flag,
                                                            uint32_t* __restrict__ missflag) {
    for (unsigned long long r = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; r <= nrows; r += (unsigned long long)gridDim.x * kBlock) {
        const uint32_t p = r < nrows ? pattern[r] : 0u;
        missflag[r]      = (r < nrows && p == kInvalid) ? 1u : 0u;
        if (r < nrows && p != kInvalid) flag[p] = 1u;
    }
}
// hitp[hidx[p]] = p for the flagged patterns; refcnt[k] = its references (refcnt[nh] = 0)
__global__ __launch_bounds__(kBlock) void query_compact_kernel(const uint32_t* __restrict__ flag, const unsigned long long* __restrict__ hidx, uint32_t np,
                                                               const unsigned long long* __restrict__ roff, uint32_t nh, uint32_t* __restrict__ hitp, uint32_t* __restrict__ refcnt,
                                                               uint32_t* __restrict__ bad) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p <= np; p += gridDim.x * kBlock) {
        if (p == np) {
            refcnt[nh] = 0;
            continue;
        }
        if (!flag[p]) continue;
        const uint32_t k = (uint32_t)hidx[p];
        hitp[k]          = p;
        const unsigned long long nr = roff ? roff[p + 1] - roff[p] : 0ull;
        if (nr >= 0xFFFFFFF0ull) atomicOr(bad, kQueryBadText);
        refcnt[k] = (uint32_t)nr;
    }
}
// the last k in [0, nh) with hroff[k] <= q
__device__ __forceinline__ uint32_t query_owner(const unsigned long long* __restrict__ hroff, uint32_t nh, unsigned long long q) {
    uint32_t lo = 0, hi = nh - 1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (hroff[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// creflen[q] = bytes of compacted reference q ("s:t" and the byte after it), creflen[nhrefs] = 0
__global__ __launch_bounds__(kBlock) void query_reflen_kernel(const unsigned long long* __restrict__ hroff, const uint32_t* __restrict__ hitp, uint32_t nh,
                                                              const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ rs, const uint16_t* __restrict__ rt,
                                                              unsigned long long nhrefs, uint32_t* __restrict__ creflen) {
    for (unsigned long long q = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; q <= nhrefs; q += (unsigned long long)gridDim.x * kBlock) {
        if (q == nhrefs) {
            creflen[q] = 0;
            continue;
        }
        const uint32_t           k = query_owner(hroff, nh, q);
        const unsigned long long r = roff[hitp[k]] + (q - hroff[k]);
        creflen[q]                 = print_digits(rs[r]) + print_digits(rt[r]) + 2u;
    }
}
// per hit pattern k: its PrintRow, head[k], arowlen[k] (the whole print() row); arowlen[nh] = 0
__global__ __launch_bounds__(kBlock) void query_row_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const uint32_t* __restrict__ cnt,
                                                           const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ hitp, uint32_t nh,
                                                           const unsigned long long* __restrict__ hroff, const unsigned long long* __restrict__ CR,
                                                           const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat, uint32_t G,
                                                           const unsigned long long* __restrict__ gcounts, unsigned long long tokens, PrintTable tab, PrintRow* __restrict__ row,
                                                           uint32_t* __restrict__ head, uint32_t* __restrict__ arowlen, uint32_t* __restrict__ bad) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k <= nh; k += gridDim.x * kBlock) {
        if (k == nh) {
            arowlen[k] = 0;
            continue;
        }
        const uint32_t           g = hitp[k];
        const uint32_t           count = print_count_of(cnt, roff, g), n = ntok[g], c = cat[g];
        const unsigned long long covc  = (unsigned long long)count * n;
        const uint32_t           gt    = c == 3 ? 0u : (uint32_t)gcounts[c * G + n];
        PrintRow                 pr;
        pr.covlen  = (uint8_t)fmt_g6(covc, tokens, pr.cov);
        pr.freqlen = (uint8_t)fmt_g6(count, gt, pr.freq);
        row[k]     = pr;
        PrintCount text;
        print_text(kbytes + koff[g], (uint32_t)(koff[g + 1] - koff[g]), tab, text);
        const unsigned long long refs = roff ? CR[hroff[k + 1]] - CR[hroff[k]] : 0ull;
        const unsigned long long h    = text.n + 1 + print_digits(count) + 1 + print_digits(covc) + 1 + pr.covlen + 1 + print_catlen(c) + 1 + print_digits(n) + 1 + pr.freqlen +
                                     (roff ? 1u : 0u) + (refs ? 0u : 1u);
        if (h + refs > 0xFFFFFFFFull) atomicOr(bad, kQueryBadText);
        head[k]    = (uint32_t)h;
        arowlen[k] = (uint32_t)(h + refs);
    }
}
// the heads of the hit patterns' rows into the arena (print_head_kernel's row, whole)
__global__ __launch_bounds__(kBlock) void query_head_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const uint32_t* __restrict__ cnt,
                                                            const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ hitp, uint32_t nh,
                                                            const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat, PrintTable tab, const PrintRow* __restrict__ row,
                                                            const unsigned long long* __restrict__ arow, uint8_t* __restrict__ arena) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < nh; k += gridDim.x * kBlock) {
        const uint32_t g = hitp[k];
        PrintEmit      e{arena, arow[k], 0ull, ~0ull, 0ull};
        print_text(kbytes + koff[g], (uint32_t)(koff[g + 1] - koff[g]), tab, e);
        const uint32_t count = print_count_of(cnt, roff, g), n = ntok[g], c = cat[g];
        const uint8_t  tabc = '\t', nl = '\n';
        uint8_t        buf[20];
        e.put(&tabc, 1);
        e.put(buf, print_number(count, buf));
        e.put(&tabc, 1);
        e.put(buf, print_number((unsigned long long)count * n, buf));
        e.put(&tabc, 1);
        const PrintRow pr = row[k];
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
// the references of the hit patterns' rows into the arena: one lane per compacted reference
__global__ __launch_bounds__(kBlock) void query_refs_kernel(const unsigned long long* __restrict__ hroff, const uint32_t* __restrict__ hitp, uint32_t nh,
                                                            const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ rs, const uint16_t* __restrict__ rt,
                                                            const unsigned long long* __restrict__ CR, unsigned long long nhrefs, const uint32_t* __restrict__ head,
                                                            const unsigned long long* __restrict__ arow, uint8_t* __restrict__ arena) {
    for (unsigned long long q = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; q < nhrefs; q += (unsigned long long)gridDim.x * kBlock) {
        const uint32_t           k = query_owner(hroff, nh, q);
        const unsigned long long r = roff[hitp[k]] + (q - hroff[k]);
        uint8_t*                 o = arena + arow[k] + head[k] + (CR[q] - CR[hroff[k]]);
        uint8_t                  buf[32];
        uint32_t                 m = print_number(rs[r], buf);
        buf[m++]                   = ':';
        m += print_number(rt[r], buf + m);
        buf[m++] = q + 1 == hroff[k + 1] ? '\n' : ' ';
        for (uint32_t i = 0; i < m; ++i) o[i] = buf[i];
    }
}
// missrow[midx[r]] = r for the exact-mode misses; misslen[m] = bytes of its NOT FOUND line (misslen[nmiss] = 0)
__global__ __launch_bounds__(kBlock) void query_miss_len_kernel(const uint32_t* __restrict__ missflag, const unsigned long long* __restrict__ midx, unsigned long long nrows,
                                                                const uint32_t* __restrict__ rowline, const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ tokstart,
                                                                const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos, PrintTable tab, uint32_t nmiss,
                                                                uint32_t* __restrict__ missrow, uint32_t* __restrict__ misslen, uint32_t* __restrict__ bad) {
    for (unsigned long long r = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; r <= nrows; r += (unsigned long long)gridDim.x * kBlock) {
        if (r == nrows) {
            misslen[nmiss] = 0;
            continue;
        }
        if (!missflag[r]) continue;
        const uint32_t m = (uint32_t)midx[r];
        uint32_t       start, T;
        query_line(delimpos, ndelim, npos, rowline[r], start, T);
        PrintCount text;
        const uint32_t a = tokstart[start];
        print_text(bytes + a, tokstart[start + T] - a, tab, text);
        const unsigned long long len = kQueryMissHead + text.n + kQueryMissTail;
        if (len > 0xFFFFFFFFull) atomicOr(bad, kQueryBadText);
        missrow[m] = (uint32_t)r;
        misslen[m] = (uint32_t)len;
    }
}
__global__ __launch_bounds__(kBlock) void query_miss_text_kernel(const uint32_t* __restrict__ missrow, const unsigned long long* __restrict__ moff, uint32_t nmiss,
                                                                 const uint32_t* __restrict__ rowline, const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ tokstart,
                                                                 const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos, PrintTable tab, uint8_t* __restrict__ marena) {
    for (uint32_t m = blockIdx.x * kBlock + threadIdx.x; m < nmiss; m += gridDim.x * kBlock) {
        uint32_t start, T;
        query_line(delimpos, ndelim, npos, rowline[missrow[m]], start, T);
        PrintEmit      e{marena, moff[m], 0ull, ~0ull, 0ull};
        const uint32_t a = tokstart[start];
        e.put(reinterpret_cast<const uint8_t*>("PATTERN \""), kQueryMissHead);
        print_text(bytes + a, tokstart[start + T] - a, tab, e);
        e.put(reinterpret_cast<const uint8_t*>("\" NOT FOUND IN MODEL\n"), kQueryMissTail);
    }
}
// "L:i\t" of a row of extensive mode into buf (at most 27 bytes); 0 for a row of exact mode
__device__ __forceinline__ uint32_t query_prefix(uint32_t first_line, uint32_t line, uint32_t token, bool isexact, uint8_t* buf) {
    if (isexact) return 0;
    uint32_t k = print_number((unsigned long long)first_line + line, buf);
    buf[k++]   = ':';
    k += print_number(token, buf + k);
    buf[k++] = '\t';
    return k;
}
// rlen[r] = bytes of result row r, rlen[nrows] = 0
__global__ __launch_bounds__(kBlock) void query_rowlen_kernel(const uint32_t* __restrict__ pattern, const uint16_t* __restrict__ token, const uint32_t* __restrict__ rowline,
                                                              unsigned long long nrows, const uint8_t* __restrict__ exact, uint32_t first_line,
                                                              const unsigned long long* __restrict__ hidx, const uint32_t* __restrict__ arowlen,
                                                              const unsigned long long* __restrict__ midx, const uint32_t* __restrict__ misslen, uint32_t* __restrict__ rlen,
                                                              uint32_t* __restrict__ bad) {
    for (unsigned long long r = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; r <= nrows; r += (unsigned long long)gridDim.x * kBlock) {
        if (r == nrows) {
            rlen[r] = 0;
            continue;
        }
        const uint32_t           p = pattern[r], line = rowline[r];
        uint8_t                  buf[32];
        const unsigned long long len = (unsigned long long)query_prefix(first_line, line, token[r], exact && exact[line], buf) + (p == kInvalid ? misslen[midx[r]] : arowlen[hidx[p]]);
        if (len > 0xFFFFFFFFull) atomicOr(bad, kQueryBadText);
        rlen[r] = (uint32_t)len;
    }
}
// the window [W0, W1) of the text: lane x writes the bytes [W0 + x * kQuerySeg, + kQuerySeg) from the rows that hold them
__global__ __launch_bounds__(kBlock) void query_emit_kernel(const unsigned long long* __restrict__ rstart, unsigned long long nrows, const uint32_t* __restrict__ pattern,
                                                            const uint16_t* __restrict__ token, const uint32_t* __restrict__ rowline, const uint8_t* __restrict__ exact,
                                                            uint32_t first_line, const unsigned long long* __restrict__ hidx, const unsigned long long* __restrict__ arow,
                                                            const uint8_t* __restrict__ arena, const unsigned long long* __restrict__ midx,
                                                            const unsigned long long* __restrict__ moff, const uint8_t* __restrict__ marena, unsigned long long W0,
                                                            unsigned long long W1, uint8_t* __restrict__ out) {
    const unsigned long long nseg = (W1 - W0 + kQuerySeg - 1) / kQuerySeg;
    for (unsigned long long x = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; x < nseg; x += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long q0 = W0 + x * kQuerySeg, q1 = q0 + kQuerySeg < W1 ? q0 + kQuerySeg : W1;
        unsigned long long       lo = 0, hi = nrows - 1;  // the last row that starts at or before q0 (every row has at least one byte)
        while (lo < hi) {
            const unsigned long long mid = lo + ((hi - lo + 1) >> 1);
            if (rstart[mid] <= q0) lo = mid;
            else hi = mid - 1;
        }
        unsigned long long r = lo;
        for (unsigned long long q = q0; q < q1;) {
            const unsigned long long rs0 = rstart[r], rs1 = rstart[r + 1];
            const uint32_t           p = pattern[r], line = rowline[r];
            uint8_t                  buf[32];
            const uint32_t           plen = query_prefix(first_line, line, token[r], exact && exact[line], buf);
            const uint8_t*           src  = p == kInvalid ? marena + moff[midx[r]] : arena + arow[hidx[p]];
            const unsigned long long end  = rs1 < q1 ? rs1 : q1;
            for (; q < end; ++q) {
                const unsigned long long d = q - rs0;
                out[q - W0]                = d < plen ? buf[d] : src[d - plen];
            }
            ++r;
        }
    }
}

}  // namespace colibri
