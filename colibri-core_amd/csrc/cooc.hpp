// cooc.hpp — sentence co-occurrence of an indexed model (IndexedPatternModel::getcooc summed over the model; reference
// include/patternmodel.h:3542-3576, :3700-3719 computecooc, :3671-3691 computenpmi, :3582-3587 npmi).
//
// For every reference (s, t) of a pattern A in A's own forward index and every occurrence (t2, B) the corpus scan finds in sentence s
// (getreverseindex_bysentence :1849-1862 over getreverseindex :1746-1824), the pair counts when t2 + n(B) < t or t2 > t + n(A): B lies
// wholly before A or after it with at least one token between them. B == A counts (ordersignificant is false). The B side is looked up in
// the corpus — every window of n tokens, MINLENGTH <= n <= MAXLENGTH of the model, and (n >= 3) that window under every gap mask a
// skipgram of the model has at that length — with the key table and window probes of constrained training (constrained.hpp). So a
// skipgram B is found also where its n-gram was pruned, while A's occurrences are its forward index: the reference's asymmetry.
//
// The pipeline (cooc_api.inc drives it):
//   cooc_info_kernel         per pattern: tokens, gap mask, category; the model's MINLENGTH / MAXLENGTH / longest key
//   constraint_probe_*       per position and layer (one layer per length, one per (length, mask)): the pattern number of the window
//   cooc_hits_kernel         per position: occurrences the reverse index holds there (B's count >= threshold) -> scan -> B list
//   cooc_bfill_kernel        the B list, by position: (position, n, pattern)
//   cooc_aocc_kernel         per reference: its pattern (binary search over the reference offsets)
//   cooc_events_kernel       per A occurrence (one wave each, its 64 lanes split the sentence's B list): the qualifying pairs
//   cooc_chunks_kernel       chunks of consecutive references whose pair events fit a fixed scratch budget (cut anywhere, also inside a pattern)
//   cooc_emit_kernel         the pairs of one chunk as (A, B) (one wave per A occurrence, ballot-compacted), radix-sorted by (A, B), run-length counted
//   cooc_bounds_kernel, cooc_mergeb_kernel   the runs of a pattern A cut by a chunk boundary: carried to the next chunk and merged there
// The pair events are counted exactly first. The references are in forward-index order (by A), so a chunk boundary cuts at most one pattern:
// the runs of that pattern are held back (not thresholded, not valued) and merged with the next chunk's runs of the same pattern; every other
// run of a chunk is final when the chunk ends, and only the kept rows accumulate. Scratch is bounded by the budget plus the events of one
// occurrence (at most its sentence's B list) plus the model's size (the carried runs of one pattern). gfx950 only.
#pragma once
#include "constrained.hpp"

namespace colibri {

constexpr uint64_t kCoocChunkEvents = 1ull << 26;  // pair events per chunk: about 76 bytes of scratch per event

// per pattern: tokens, gap mask (skipgrams; bit k = token k is {*}), category bits (1 n-gram, 2 skipgram, 4 flexgram); info[0..3] =
// min tokens, max tokens, longest key in bytes, categories present (atomics)
__global__ __launch_bounds__(kBlock) void cooc_info_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, uint32_t np,
                                                           uint8_t* __restrict__ ntok, uint32_t* __restrict__ mask, uint32_t* __restrict__ info) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < np; p += gridDim.x * kBlock) {
        const uint8_t* k   = kbytes + koff[p];
        const uint32_t len = (uint32_t)(koff[p + 1] - koff[p]);
        uint32_t       n = 0, m = 0, cat = 0, start = 0;
        for (uint32_t i = 0; i < len; ++i) {
            if (k[i] >= 128) continue;
            if (i == start && k[i] == 3) {
                if (n < 32) m |= 1u << n;
                cat |= 2;
            } else if (i == start && k[i] == 4) {
                cat |= 4;
            }
            ++n;
            start = i + 1;
        }
        if (cat == 0) cat = 1;
        ntok[p] = (uint8_t)(n > 255 ? 255 : n);
        mask[p] = (cat & 2) ? m : 0u;
        atomicMin(&info[0], n);
        atomicMax(&info[1], n);
        atomicMax(&info[2], len);
        atomicOr(&info[3], cat);
    }
}
__global__ __launch_bounds__(kBlock) void cooc_count_kernel(const unsigned long long* __restrict__ roff, uint32_t np, uint32_t* __restrict__ cnt) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < np; p += gridDim.x * kBlock) cnt[p] = (uint32_t)(roff[p + 1] - roff[p]);
}
// gate of a masked probe: a window of n tokens starts at i
__global__ __launch_bounds__(kBlock) void cooc_gate_kernel(const uint32_t* __restrict__ rem, uint32_t npos, uint32_t n, uint32_t* __restrict__ gate) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < npos; i += gridDim.x * kBlock) gate[i] = rem[i] >= n ? 0u : kInvalid;
}
// layer l of memb holds the pattern number of the window at every position (kInvalid: none); a hit counts iff B's count passes the threshold
__device__ __forceinline__ bool cooc_hit(uint32_t b, const uint32_t* __restrict__ cnt, uint32_t thr) { return b != kInvalid && (thr == 0 || cnt[b] >= thr); }
__global__ __launch_bounds__(kBlock) void cooc_hits_kernel(const uint32_t* __restrict__ memb, size_t stride, uint32_t nlayers, uint32_t npos, const uint32_t* __restrict__ cnt,
                                                           uint32_t thr, uint32_t* __restrict__ hits) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < npos; i += gridDim.x * kBlock) {
        uint32_t h = 0;
        for (uint32_t l = 0; l < nlayers; ++l) h += cooc_hit(memb[(size_t)l * stride + i], cnt, thr) ? 1u : 0u;
        hits[i] = h;
    }
}
__global__ __launch_bounds__(kBlock) void cooc_bfill_kernel(const uint32_t* __restrict__ memb, size_t stride, uint32_t nlayers, const uint8_t* __restrict__ layer_n, uint32_t npos,
                                                            const uint32_t* __restrict__ cnt, uint32_t thr, const unsigned long long* __restrict__ boff, uint32_t* __restrict__ bpos,
                                                            uint8_t* __restrict__ bn, uint32_t* __restrict__ bid) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < npos; i += gridDim.x * kBlock) {
        unsigned long long o = boff[i];
        for (uint32_t l = 0; l < nlayers; ++l) {
            const uint32_t b = memb[(size_t)l * stride + i];
            if (!cooc_hit(b, cnt, thr)) continue;
            bpos[o] = i;
            bn[o]   = layer_n[l];
            bid[o]  = b;
            ++o;
        }
    }
}
// per reference k: its pattern (the last p with roff[p] <= k)
__global__ __launch_bounds__(kBlock) void cooc_aocc_kernel(const unsigned long long* __restrict__ roff, uint32_t np, uint64_t nrefs, uint32_t* __restrict__ aid) {
    for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < nrefs; k += (uint64_t)gridDim.x * kBlock) {
        uint32_t lo = 0, hi = np;  // first p with roff[p + 1] > k
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (roff[mid + 1] <= k)
                lo = mid + 1;
            else
                hi = mid;
        }
        aid[k] = lo;
    }
}
// the positions of sentence s: [start, end)
__device__ __forceinline__ void sentence_span(const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos, uint32_t s, uint32_t& start, uint32_t& end) {
    start = s == 0 ? 0u : delimpos[s - 1] + 1;
    end   = s < ndelim ? delimpos[s] : npos;
}
// one A occurrence (reference k): its pattern, first position and tokens, and its sentence's range of the B list; false when its sentence
// lies outside the uploaded corpus
struct CoocA {
    uint32_t a, p, na;
    uint64_t b0, b1;
};
__device__ __forceinline__ bool cooc_a(uint64_t k, uint32_t nsent, uint32_t first_sentence, const uint32_t* __restrict__ rs, const uint32_t* __restrict__ aid,
                                       const uint16_t* __restrict__ rt, const uint8_t* __restrict__ ntok, const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t npos,
                                       const unsigned long long* __restrict__ boff, CoocA& o) {
    const uint32_t sn = rs[k];
    if (sn < first_sentence || sn - first_sentence >= nsent) return false;
    uint32_t start, end;
    sentence_span(delimpos, ndelim, npos, sn - first_sentence, start, end);
    o.a  = aid[k];
    o.p  = start + rt[k];
    o.na = ntok[o.a];
    o.b0 = boff[start];
    o.b1 = boff[end];
    return true;
}
__device__ __forceinline__ bool cooc_apart(uint32_t p, uint32_t na, uint32_t p2, uint32_t n2) { return p2 + n2 < p || p2 > p + na; }
// One wave per A occurrence: the lanes take the sentence's B list 64 entries at a time (consecutive, coalesced loads), so a long sentence
// is split across the lanes of every wave that holds one of its A occurrences, and no lane walks a whole list alone.
constexpr int kCoocWave = 64;
// events[k] = qualifying pairs of the A occurrence k; *maxev = the most one occurrence has
__global__ __launch_bounds__(kBlock) void cooc_events_kernel(uint64_t nrefs, uint32_t nsent, uint32_t first_sentence, const uint32_t* __restrict__ rs, const uint32_t* __restrict__ aid,
                                                             const uint16_t* __restrict__ rt, const uint8_t* __restrict__ ntok, const uint32_t* __restrict__ delimpos, uint32_t ndelim,
                                                             uint32_t npos, const unsigned long long* __restrict__ boff, const uint32_t* __restrict__ bpos, const uint8_t* __restrict__ bn,
                                                             uint32_t* __restrict__ events, uint32_t* __restrict__ maxev) {
    const uint32_t lane = threadIdx.x & (kCoocWave - 1);
    const uint64_t nw   = (uint64_t)gridDim.x * (kBlock / kCoocWave);
    for (uint64_t k = (uint64_t)blockIdx.x * (kBlock / kCoocWave) + threadIdx.x / kCoocWave; k < nrefs; k += nw) {
        CoocA    o;
        uint32_t e = 0;
        if (cooc_a(k, nsent, first_sentence, rs, aid, rt, ntok, delimpos, ndelim, npos, boff, o))
            for (uint64_t j = o.b0 + lane; j < o.b1; j += kCoocWave) e += cooc_apart(o.p, o.na, bpos[j], bn[j]) ? 1u : 0u;
        for (int off = kCoocWave / 2; off > 0; off >>= 1) e += __shfl_down(e, off, kCoocWave);
        if (lane == 0) {
            events[k] = e;
            if (e) atomicMax(maxev, e);
        }
    }
}
// chunk j starts at the first reference whose events begin at or after j * budget; with it: its first event, and whether the cut lies inside a
// pattern (mid[j]: the references on either side have the same pattern) and which patterns touch it (afirst: of the reference after, alast: before)
__global__ __launch_bounds__(kBlock) void cooc_chunks_kernel(const unsigned long long* __restrict__ evoff, uint64_t nrefs, const uint32_t* __restrict__ aid, uint64_t budget,
                                                             uint32_t nchunks, unsigned long long* __restrict__ cstart, unsigned long long* __restrict__ cbase, uint32_t* __restrict__ mid,
                                                             uint32_t* __restrict__ afirst, uint32_t* __restrict__ alast) {
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j <= nchunks; j += gridDim.x * kBlock) {
        const unsigned long long want = (unsigned long long)j * budget;
        uint64_t                 lo = 0, hi = nrefs;
        while (lo < hi) {
            const uint64_t m = (lo + hi) >> 1;
            if (evoff[m] < want)
                lo = m + 1;
            else
                hi = m;
        }
        const uint64_t k = j == nchunks ? nrefs : lo;
        cstart[j]        = k;
        cbase[j]         = evoff[k];
        afirst[j]        = k < nrefs ? aid[k] : kInvalid;
        alast[j]         = k > 0 ? aid[k - 1] : kInvalid;
        mid[j]           = (k > 0 && k < nrefs && aid[k - 1] == aid[k]) ? 1u : 0u;
    }
}
// the pairs of the A occurrences [k0, k1) as (key = B, val = A) at evoff[k] - base, in B-list order (ballot-compacted per 64 entries)
__global__ __launch_bounds__(kBlock) void cooc_emit_kernel(uint64_t k0, uint64_t k1, unsigned long long base, uint32_t nsent, uint32_t first_sentence,
                                                           const unsigned long long* __restrict__ evoff, const uint32_t* __restrict__ rs, const uint32_t* __restrict__ aid,
                                                           const uint16_t* __restrict__ rt, const uint8_t* __restrict__ ntok, const uint32_t* __restrict__ delimpos, uint32_t ndelim,
                                                           uint32_t npos, const unsigned long long* __restrict__ boff, const uint32_t* __restrict__ bpos, const uint8_t* __restrict__ bn,
                                                           const uint32_t* __restrict__ bid, uint32_t* __restrict__ kb, uint32_t* __restrict__ ka) {
    const uint32_t lane  = threadIdx.x & (kCoocWave - 1);
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t nw    = (uint64_t)gridDim.x * (kBlock / kCoocWave);
    for (uint64_t k = k0 + (uint64_t)blockIdx.x * (kBlock / kCoocWave) + threadIdx.x / kCoocWave; k < k1; k += nw) {
        CoocA o;
        if (!cooc_a(k, nsent, first_sentence, rs, aid, rt, ntok, delimpos, ndelim, npos, boff, o)) continue;  // (uniform across the wave)
        uint64_t w = evoff[k] - base;
        for (uint64_t j0 = o.b0; j0 < o.b1; j0 += kCoocWave) {
            const uint64_t j    = j0 + lane;
            const bool     q    = j < o.b1 && cooc_apart(o.p, o.na, bpos[j], bn[j]);
            const uint64_t mask = __ballot(q);
            if (q) {
                const uint64_t at = w + __popcll(mask & below);
                kb[at]            = bid[j];
                ka[at]            = o.a;
            }
            w += __popcll(mask);
        }
    }
}
// run heads of a (A, B)-sorted list
__global__ __launch_bounds__(kBlock) void cooc_heads_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t n, uint32_t* __restrict__ head) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
        head[i] = (i == 0 || a[i] != a[i - 1] || b[i] != b[i - 1]) ? 1u : 0u;
}
// one run per head (rid = exclusive scan of the heads): its (A, B) and first index; the count is the distance to the next run's first index
__global__ __launch_bounds__(kBlock) void cooc_runs_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ head,
                                                           const unsigned long long* __restrict__ rid, uint64_t n, uint32_t* __restrict__ ra, uint32_t* __restrict__ rb,
                                                           unsigned long long* __restrict__ rstart) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        if (!head[i]) continue;
        const uint64_t r = rid[i];
        ra[r]            = a[i];
        rb[r]            = b[i];
        rstart[r]        = i;
    }
}
__global__ __launch_bounds__(kBlock) void cooc_runlen_kernel(const unsigned long long* __restrict__ rstart, uint64_t nruns, uint64_t n, uint32_t* __restrict__ rc) {
    for (uint64_t r = blockIdx.x * (uint64_t)kBlock + threadIdx.x; r < nruns; r += (uint64_t)gridDim.x * kBlock) rc[r] = (uint32_t)((r + 1 < nruns ? rstart[r + 1] : n) - rstart[r]);
}
// within runs sorted by A: out[0] = the runs of pattern ahead end here (upper bound), out[1] = the runs of pattern atail start here (lower bound)
__global__ void cooc_bounds_kernel(const uint32_t* __restrict__ ra, uint64_t n, uint32_t ahead, uint32_t atail, unsigned long long* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if (ra[m] <= ahead)
            lo = m + 1;
        else
            hi = m;
    }
    out[0] = lo;
    lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if (ra[m] < atail)
            lo = m + 1;
        else
            hi = m;
    }
    out[1] = lo;
}
// the runs of one pattern A from two lists (the carried one, the chunk's), sorted together by B (perm = their index in the concatenation):
// one run per B with the sum of the counts (every B is at most once in each list: at most two adds into a run; rc zeroed first)
__global__ __launch_bounds__(kBlock) void cooc_mergeb_kernel(const uint32_t* __restrict__ b, const uint32_t* __restrict__ head, const unsigned long long* __restrict__ rid, uint64_t n,
                                                             const uint32_t* __restrict__ w, const uint32_t* __restrict__ perm, uint32_t a, uint32_t* __restrict__ ra,
                                                             uint32_t* __restrict__ rb, uint32_t* __restrict__ rc) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t r = rid[i] + head[i] - 1;
        if (head[i]) {
            ra[r] = a;
            rb[r] = b[i];
        }
        atomicAdd(&rc[r], w[perm[i]]);
    }
}
__global__ __launch_bounds__(kBlock) void cooc_iota_kernel(uint32_t* __restrict__ v, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) v[i] = (uint32_t)i;
}
__global__ __launch_bounds__(kBlock) void cooc_gather_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx, uint64_t n, uint32_t* __restrict__ dst) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) dst[i] = src[idx[i]];
}
// dst[i] = src[idx2[idx[i]]]: a per-pattern value of the row that is i-th in the current order
__global__ __launch_bounds__(kBlock) void cooc_gather2_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx2, const uint32_t* __restrict__ idx, uint64_t n,
                                                              uint32_t* __restrict__ dst) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) dst[i] = src[idx2[idx[i]]];
}
// rank of the patterns by key bytes: the sort key of pass `chunk` is the chunk-th group of four bytes of the key, zero-padded, big-endian
// (chunk = kInvalid: the key's length, the least significant pass). Zero-padded bytes, then length, is std::string's order.
__global__ __launch_bounds__(kBlock) void cooc_keychunk_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const uint32_t* __restrict__ perm,
                                                               uint32_t np, uint32_t chunk, uint32_t* __restrict__ key) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < np; i += gridDim.x * kBlock) {
        const uint32_t       p   = perm[i];
        const uint8_t*       k   = kbytes + koff[p];
        const uint32_t       len = (uint32_t)(koff[p + 1] - koff[p]);
        if (chunk == kInvalid) {
            key[i] = len;
            continue;
        }
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t at = chunk * 4 + b;
            v                 = (v << 8) | (at < len ? k[at] : 0u);
        }
        key[i] = v;
    }
}
__global__ __launch_bounds__(kBlock) void cooc_rank_kernel(const uint32_t* __restrict__ perm, uint32_t np, uint32_t* __restrict__ rank) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < np; i += gridDim.x * kBlock) rank[perm[i]] = i;
}
// the value of a row and whether it is kept: -C keeps count >= threshold (computecooc :3715-3717); -Y computes npmi (:3582-3587: the two
// occurrence counts multiply as unsigned int, wrapping past 2^32) and keeps it when >= x
__global__ __launch_bounds__(kBlock) void cooc_value_kernel(const uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb, const uint32_t* __restrict__ rc, uint64_t n,
                                                            const uint32_t* __restrict__ cnt, int npmi, uint32_t thr, double x, uint32_t total, double* __restrict__ val,
                                                            uint32_t* __restrict__ keep) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t j = rc[i];
        if (!npmi) {
            val[i]  = (double)j;
            keep[i] = j >= thr ? 1u : 0u;
            continue;
        }
        const uint64_t prod = (uint64_t)cnt[ra[i]] * cnt[rb[i]];  // (occurrencecount returns size_t, :1653-1669: the product does not wrap)
        const double   v    = log((double)j / (double)prod) / -log((double)j / (double)total);
        val[i]              = v;
        keep[i]             = v >= x ? 1u : 0u;
    }
}
// the kept rows, compacted: (A, B, count, value)
__global__ __launch_bounds__(kBlock) void cooc_compact_kernel(const uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb, const uint32_t* __restrict__ rc,
                                                              const double* __restrict__ val, const uint32_t* __restrict__ keep, const unsigned long long* __restrict__ kofs, uint64_t n,
                                                              uint32_t* __restrict__ oa, uint32_t* __restrict__ ob, uint32_t* __restrict__ oc, double* __restrict__ ov) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        if (!keep[i]) continue;
        const uint64_t o = kofs[i];
        oa[o]            = ra[i];
        ob[o]            = rb[i];
        oc[o]            = rc[i];
        ov[o]            = val[i];
    }
}
// descending order of the value as a 64-bit sort key (ascending sort): half = 0 the low, 1 the high 32 bits
__global__ __launch_bounds__(kBlock) void cooc_valkey_kernel(const double* __restrict__ val, const uint32_t* __restrict__ perm, uint64_t n, int half, uint32_t* __restrict__ key) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        uint64_t u = (uint64_t)__double_as_longlong(val[perm[i]]);
        u          = (u >> 63) ? ~u : (u | (1ull << 63));  // ascending as unsigned
        u          = ~u;                                    // descending
        key[i]     = half ? (uint32_t)(u >> 32) : (uint32_t)u;
    }
}
__global__ __launch_bounds__(kBlock) void cooc_permute_kernel(const uint32_t* __restrict__ perm, uint64_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                              const uint32_t* __restrict__ c, const double* __restrict__ v, uint32_t* __restrict__ oa, uint32_t* __restrict__ ob,
                                                              uint32_t* __restrict__ oc, double* __restrict__ ov) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t r = perm[i];
        oa[i]            = a[r];
        ob[i]            = b[r];
        oc[i]            = c[r];
        ov[i]            = v[r];
    }
}

}  // namespace colibri
