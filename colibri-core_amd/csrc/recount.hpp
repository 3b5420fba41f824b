// recount.hpp — the skipgrams of an in-place rebuild (colibri-patternmodeller -I -s, PatternModel::trainskipgrams_selfconstrained; reference
// include/patternmodel.h:1569-1604).
//
// Given skipgram keys (n >= 3 tokens, gap mask m != 0) and the uploaded corpus: skipgram p occurs at (s, t) iff the window of its n tokens fits
// the sentence (t + n <= sentencelength(s)) and every token outside m equals the key's. A gap takes any one token; a window never crosses a
// sentence end. counts[p] = its occurrences; for an indexed call its references, ascending by (sentence, token), for the patterns whose count
// reaches mintokens. MINSKIPTYPES, MINTOKENS_SKIPGRAMS and MAXSKIPS play no part.
//
// The pipeline (recount_api.inc drives it). The keys go into the constraint set's table (constrained.hpp) and are grouped by (n, mask): one
// probe layer per group, as the reverse index has them (cooc_api.inc: rev_table / rev_probe). Per chunk [p0, p0 + n) of positions:
//   pass 1   constraint_probe_masked_kernel   per position and group: the pattern number of the masked window, or none
//            recount_count_kernel             counts[p] += 1 per hit
//   between  recount_kept_kernel              the reference runs' lengths (0 below mintokens) -> 64-bit scan = ref_off
//   pass 2 (indexed), the probes again, then
//            rindex_hits_kernel               per position: hits whose pattern reaches mintokens -> 64-bit scan
//            recount_pairs_kernel             (pattern, position) per hit, positions ascending
//            radix_sort_pairs                 stable by pattern number: every pattern's positions of the chunk, still ascending
//            recount_refs_kernel              pair k of pattern p -> ref_off[p] + done[p] + (k - first pair of p): sentence and token
//            recount_done_kernel              done[p] += the pattern's pairs of the chunk (its own launch: recount_refs_kernel reads done)
// Chunks ascend, so a pattern's references ascend across them too. gfx950 only.
#pragma once
#include "rindex.hpp"

namespace colibri {

// counts[p] += 1 for every group whose masked window at position p0 + j is pattern p
__global__ __launch_bounds__(kBlock) void recount_count_kernel(const uint32_t* __restrict__ memb, size_t stride, uint32_t nlayers, uint32_t n, uint32_t* __restrict__ counts) {
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock)
        for (uint32_t l = 0; l < nlayers; ++l) {
            const uint32_t b = memb[(size_t)l * stride + j];
            if (b != kInvalid) atomicAdd(&counts[b], 1u);
        }
}
// kept[p] = counts[p] where it reaches mintokens, else 0 (kept[np] = 0: the scan's last entry is the total); nkept += the patterns that do
__global__ __launch_bounds__(kBlock) void recount_kept_kernel(const uint32_t* __restrict__ counts, uint32_t np, uint32_t mintokens, uint32_t* __restrict__ kept,
                                                              uint32_t* __restrict__ nkept) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p <= np; p += gridDim.x * kBlock) {
        const bool k = p < np && counts[p] >= mintokens;
        kept[p]      = k ? counts[p] : 0u;
        if (k) atomicAdd(nkept, 1u);
    }
}
// the chunk's hits as (pattern, position) pairs from boff[j] on, positions ascending (the groups of one position name different patterns)
__global__ __launch_bounds__(kBlock) void recount_pairs_kernel(const uint32_t* __restrict__ memb, size_t stride, uint32_t nlayers, uint32_t p0, uint32_t n,
                                                               const uint32_t* __restrict__ counts, uint32_t mintokens, const unsigned long long* __restrict__ boff,
                                                               uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
        unsigned long long o = boff[j];
        for (uint32_t l = 0; l < nlayers; ++l) {
            const uint32_t b = memb[(size_t)l * stride + j];
            if (cooc_hit(b, counts, mintokens)) {
                key[o] = b;
                val[o] = p0 + j;
                ++o;
            }
        }
    }
}
// the first pair of key[k]'s run in the sorted pairs [0, m)
__device__ __forceinline__ uint32_t recount_run_first(const uint32_t* __restrict__ key, uint32_t k) {
    const uint32_t p  = key[k];
    uint32_t       lo = 0, hi = k;  // first index whose key is >= p
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key[mid] < p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// pair k (sorted by pattern, positions ascending within one) into its pattern's reference run, after the references of the chunks before
__global__ __launch_bounds__(kBlock) void recount_refs_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, uint32_t m,
                                                              const unsigned long long* __restrict__ ref_off, const uint32_t* __restrict__ done,
                                                              const uint32_t* __restrict__ delimpos, uint32_t ndelim, uint32_t first_sentence, uint32_t* __restrict__ ref_sentence,
                                                              uint16_t* __restrict__ ref_token) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < m; k += gridDim.x * kBlock) {
        const uint32_t           p = key[k];
        const unsigned long long o = ref_off[p] + done[p] + (k - recount_run_first(key, k));
        uint32_t                 s, start;
        rindex_locate(delimpos, ndelim, val[k], s, start);
        ref_sentence[o] = first_sentence + s;
        ref_token[o]    = (uint16_t)(val[k] - start);
    }
}
// done[p] += the pairs of p in this chunk, by the first pair of each run
__global__ __launch_bounds__(kBlock) void recount_done_kernel(const uint32_t* __restrict__ key, uint32_t m, uint32_t* __restrict__ done) {
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < m; k += gridDim.x * kBlock) {
        const uint32_t p = key[k];
        if (k > 0 && key[k - 1] == p) continue;
        uint32_t lo = k + 1, hi = m;  // first index whose key is > p
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (key[mid] <= p)
                lo = mid + 1;
            else
                hi = mid;
        }
        done[p] += lo - k;
    }
}

}  // namespace colibri
