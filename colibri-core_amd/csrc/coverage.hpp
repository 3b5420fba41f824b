// coverage.hpp — the coverage report of a pattern model (colibri-patternmodeller -R / -r; reference computestats, include/patternmodel.h:1903-1935, and
// computecoveragestats, :1946-1995 and :3390-3450; the host face's restatement in host/include/patternmodel.h is the specification).
//
// Groups: (category c, size n), c in {0 = all, 1 = n-gram, 2 = skipgram, 3 = flexgram}, n in {0 = all, 1 .. maxn}; group number c * G + n with
// G = maxn + 1. A pattern of category pc and pn tokens (Pattern::n(): every byte under 128 closes a token, so a gap {*} or {**} is one token)
// belongs to (0, 0), (pc, 0), (0, pn) and (pc, pn). Per group, the plain values:
//   patterns   its patterns                       } a flexgram is counted in (0, 0) and (3, 0) only (computestats: no per-size rows)
//   counts     the sum of their counts            }
//   types      the distinct tokens of its patterns, identified by class id (gap markers are ids 3 and 4: a gap counts as one type)
//   tokens     the distinct corpus positions (sentence, (token + i) mod 65536), i < pn, over every reference of its patterns (the host face packs a
//              position as sentence << 16 | uint16_t(token + i)); 0 for a model without references
// What report() makes of them (per-size token rows print 0, unindexed groups print the sum of all counts) stays in the host face.
//
// The pipeline (coverage_api.inc drives it):
//   cov_info_kernel    per pattern: tokens, category; the most tokens and the largest class id of the model
//   cov_group_kernel   patterns / counts / members per group, summed in LDS and flushed once per block (members counts a flexgram in all four of
//                      its groups: two groups of equal members that contain one another are the same set and share their bitmaps)
//   cov_types_kernel   per pattern: the bit of each token's class id in the class bitmap of each of its groups (load first, atomicOr only a new bit)
//   cov_range_kernel   lowest / highest sentence over the references
//   cov_extent_kernel  per reference: extent[sentence - lowest] = max(token + pn), capped at 65 536; a 64-bit exclusive scan of the extents gives
//                      every sentence a base, so position (s, t) is bit base[s - lowest] + t
//   cov_mark_kernel    per reference: bits base + t .. base + t + pn - 1 in the position bitmap of each of its groups
//   cov_popc_kernel    set bits per bitmap, 64-bit sums
// The two per-reference kernels balance by reference, not by pattern: a block takes a contiguous slice of the reference array, two of its lanes
// find the first and the last pattern of the slice by binary search in ref_off, and each lane then finds its reference's pattern between those
// two. gfx950 only.
#pragma once
#include "kernels.hpp"

namespace colibri {

constexpr uint32_t kCovNoSlot   = 0xFFFFFFFFu;
constexpr uint32_t kCovExtent   = 65536u;  // token positions live in 16 bits
constexpr uint32_t kCovMaxToken = 9;       // bytes of a token whose class id still fits 63 bits
constexpr uint32_t kCovSlice    = 2048;    // references per block of the two per-reference kernels (environment: COLIBRI_COV_SLICE)
constexpr uint64_t kCovBudgetBytes = 8ull << 30;  // scratch the call may take for extents, bases and bitmaps (environment: COLIBRI_COV_BUDGET)

// info[0] = most tokens of a pattern, info[1] = largest class id (a token of more than kCovMaxToken bytes: ~0)
__global__ __launch_bounds__(kBlock) void cov_info_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, uint32_t np, uint16_t* __restrict__ ntok,
                                                          uint8_t* __restrict__ cat, unsigned long long* __restrict__ info) {
    unsigned long long mn = 0, mc = 0;
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < np; g += gridDim.x * kBlock) {
        const uint8_t* k   = kbytes + koff[g];
        const uint32_t len = (uint32_t)(koff[g + 1] - koff[g]);
        uint32_t       n = 0, c = 0, tb = 0;
        unsigned long long id = 0;
        for (uint32_t i = 0; i < len; ++i) {
            const uint32_t b = k[i];
            if (tb == 0 && c == 0 && b == 3) c = 2;
            if (tb == 0 && c == 0 && b == 4) c = 3;
            id = tb < kCovMaxToken ? (id | ((unsigned long long)(b & 127u) << (7 * tb))) : ~0ull;
            ++tb;
            if (b < 128) {
                mc = max(mc, id);
                id = 0;
                tb = 0;
                ++n;
            }
        }
        ntok[g] = (uint16_t)(n > 0xFFFFu ? 0xFFFFu : n);
        cat[g]  = (uint8_t)(c == 0 ? 1u : c);
        mn      = max(mn, (unsigned long long)n);
    }
    if (mn) atomicMax(&info[0], mn);
    if (mc) atomicMax(&info[1], mc);
}

// grp[0 .. 4G) patterns, [4G .. 8G) counts, [8G .. 12G) members. cnt == NULL: a pattern's count is its number of references. `lds`: the block
// sums in LDS first (12G u64 must fit), else every pattern adds to HBM directly.
__global__ __launch_bounds__(kBlock) void cov_group_kernel(const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat, const uint32_t* __restrict__ cnt,
                                                           const unsigned long long* __restrict__ roff, uint32_t np, uint32_t G, int lds, unsigned long long* __restrict__ grp) {
    extern __shared__ unsigned long long sgrp[];
    const uint32_t      nt  = 12u * G;
    unsigned long long* dst = lds ? sgrp : grp;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < nt; i += kBlock) sgrp[i] = 0;
        __syncthreads();
    }
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < np; g += gridDim.x * kBlock) {
        const uint32_t           c = cat[g], n = ntok[g];
        const unsigned long long v = cnt ? (unsigned long long)cnt[g] : (roff ? roff[g + 1] - roff[g] : 0ull);
        const uint32_t           gs[4] = {0u, c * G, n, c * G + n};
        for (int k = 0; k < 4; ++k) {
            if (n == 0 && (k & 2)) continue;  // (an empty key: its per-size groups are its all-sizes groups)
            atomicAdd(&dst[8u * G + gs[k]], 1ull);
            if (c == 3 && (k & 2)) continue;
            atomicAdd(&dst[gs[k]], 1ull);
            if (v) atomicAdd(&dst[4u * G + gs[k]], v);
        }
    }
    if (lds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nt; i += kBlock)
            if (sgrp[i]) atomicAdd(&grp[i], sgrp[i]);
    }
}

// the (at most four) distinct bitmaps of a pattern of category c and n tokens: slot[] maps a group to its bitmap (kCovNoSlot: none)
__device__ __forceinline__ int cov_slots(const uint32_t* __restrict__ slot, uint32_t G, uint32_t c, uint32_t n, uint32_t out[4]) {
    const uint32_t gs[4] = {0u, c * G, n, c * G + n};
    int            k     = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = slot[gs[i]];
        if (s == kCovNoSlot) continue;
        bool seen = false;
        for (int j = 0; j < k; ++j) seen = seen || out[j] == s;
        if (!seen) out[k++] = s;
    }
    return k;
}
// bits [lo, hi) of one bitmap: one non-returning atomicOr per touched word; TEST: the word is loaded first and left alone when it already has the bits
template <bool TEST>
__device__ __forceinline__ void cov_set_range(uint32_t* __restrict__ bits, unsigned long long lo, unsigned long long hi) {
    for (unsigned long long w = lo >> 5; w <= ((hi - 1) >> 5); ++w) {
        const unsigned long long wlo = w << 5;
        const uint32_t           a = lo > wlo ? (uint32_t)(lo - wlo) : 0u, b = hi < wlo + 32 ? (uint32_t)(hi - wlo) : 32u;  // bits [a, b) of word w
        const uint32_t           m = (b == 32 ? 0xFFFFFFFFu : ((1u << b) - 1u)) & ~((1u << a) - 1u);
        if (TEST && (bits[w] & m) == m) continue;  // (a stale word only costs the atomic it would have saved: bits are never cleared)
        atomicOr(&bits[w], m);
    }
}

// one lane per pattern: its tokens' class ids into the class bitmaps (CW words each) of its groups
__global__ __launch_bounds__(kBlock) void cov_types_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const uint16_t* __restrict__ ntok,
                                                           const uint8_t* __restrict__ cat, uint32_t np, uint32_t G, const uint32_t* __restrict__ slot, unsigned long long CW,
                                                           uint32_t* __restrict__ bits) {
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < np; g += gridDim.x * kBlock) {
        const uint8_t* k   = kbytes + koff[g];
        const uint32_t len = (uint32_t)(koff[g + 1] - koff[g]);
        uint32_t       ss[4];
        const int      ns = cov_slots(slot, G, cat[g], ntok[g], ss);
        unsigned long long id = 0;
        uint32_t           tb = 0;
        for (uint32_t i = 0; i < len; ++i) {
            const uint32_t b = k[i];
            id |= (unsigned long long)(b & 127u) << (7 * tb);  // (a longer token was refused before this kernel runs)
            ++tb;
            if (b >= 128) continue;
            const uint32_t m = 1u << (id & 31u);
            for (int s = 0; s < ns; ++s) {
                uint32_t* w = bits + ss[s] * CW + (id >> 5);
                if (!(*w & m)) atomicOr(w, m);
            }
            id = 0;
            tb = 0;
        }
    }
}

// info[0] = lowest, info[1] = highest sentence of the references (info starts as {~0, 0})
__global__ __launch_bounds__(kBlock) void cov_range_kernel(const uint32_t* __restrict__ rs, uint64_t nrefs, uint32_t* __restrict__ info) {
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < nrefs; r += (uint64_t)gridDim.x * kBlock) {
        const uint32_t s = rs[r];
        lo               = min(lo, s);
        hi               = max(hi, s);
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, (uint32_t)__shfl_down(lo, off, kWave));
        hi = max(hi, (uint32_t)__shfl_down(hi, off, kWave));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicMin(&info[0], lo);
        atomicMax(&info[1], hi);
    }
}

// the block's slice of the reference array is [r0, r1): the patterns its references belong to lie in [*plo, *phi] (the last pattern whose first
// reference is <= r0 resp. <= r1 - 1; patterns without references are never found). Both values come back through LDS.
__device__ __forceinline__ uint32_t cov_pattern_of(const unsigned long long* __restrict__ roff, uint32_t lo, uint32_t hi, unsigned long long r) {
    while (lo < hi) {  // the last p in [lo, hi] with roff[p] <= r
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (roff[mid] <= r)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ void cov_slice_bounds(const unsigned long long* __restrict__ roff, uint32_t np, unsigned long long r0, unsigned long long r1, uint32_t* sb) {
    if (threadIdx.x < 2) sb[threadIdx.x] = cov_pattern_of(roff, 0, np - 1, threadIdx.x ? r1 - 1 : r0);
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void cov_extent_kernel(const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ rs, const uint16_t* __restrict__ rt,
                                                            const uint16_t* __restrict__ ntok, uint32_t np, uint64_t nrefs, uint32_t slice, uint32_t mins,
                                                            uint32_t* __restrict__ extent) {
    __shared__ uint32_t      sb[2];
    const unsigned long long r0 = (unsigned long long)blockIdx.x * slice, r1 = min(r0 + slice, (unsigned long long)nrefs);
    if (r0 >= r1) return;
    cov_slice_bounds(roff, np, r0, r1, sb);
    const uint32_t plo = sb[0], phi = sb[1];
    for (unsigned long long r = r0 + threadIdx.x; r < r1; r += kBlock) {
        const uint32_t p = cov_pattern_of(roff, plo, phi, r);
        const uint32_t e = min((uint32_t)rt[r] + (uint32_t)ntok[p], kCovExtent);
        uint32_t*      x = extent + (rs[r] - mins);
        if (*x < e) atomicMax(x, e);
    }
}

template <bool TEST>
__global__ __launch_bounds__(kBlock) void cov_mark_kernel(const unsigned long long* __restrict__ roff, const uint32_t* __restrict__ rs, const uint16_t* __restrict__ rt,
                                                          const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat, uint32_t np, uint64_t nrefs, uint32_t slice,
                                                          uint32_t mins, const unsigned long long* __restrict__ base, uint32_t G, const uint32_t* __restrict__ slot,
                                                          unsigned long long W, uint32_t* __restrict__ bits) {
    __shared__ uint32_t      sb[2];
    const unsigned long long r0 = (unsigned long long)blockIdx.x * slice, r1 = min(r0 + slice, (unsigned long long)nrefs);
    if (r0 >= r1) return;
    cov_slice_bounds(roff, np, r0, r1, sb);
    const uint32_t plo = sb[0], phi = sb[1];
    for (unsigned long long r = r0 + threadIdx.x; r < r1; r += kBlock) {
        const uint32_t p = cov_pattern_of(roff, plo, phi, r);
        const uint32_t n = ntok[p], t = rt[r];
        if (n == 0) continue;
        uint32_t  ss[4];
        const int ns = cov_slots(slot, G, cat[p], n, ss);
        const unsigned long long b    = base[rs[r] - mins];
        const uint32_t           end  = min(t + n, kCovExtent);        // [t, end), and past 65 535 the 16-bit token index starts again at 0:
        const uint32_t           wrap = t + n > kCovExtent ? t + n - kCovExtent : 0u;  // [0, wrap)
        for (int s = 0; s < ns; ++s) {
            uint32_t* bm = bits + ss[s] * W;
            cov_set_range<TEST>(bm, b + t, b + end);
            if (wrap) cov_set_range<TEST>(bm, b, b + min(wrap, t));
        }
    }
}

// sums[blockIdx.y] += set bits of bitmap blockIdx.y (W words each)
__global__ __launch_bounds__(kBlock) void cov_popc_kernel(const uint32_t* __restrict__ bits, unsigned long long W, unsigned long long* __restrict__ sums) {
    const uint32_t*    bm = bits + blockIdx.y * W;
    unsigned long long s  = 0;
    for (unsigned long long w = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; w < W; w += (unsigned long long)gridDim.x * kBlock) s += (unsigned long long)__popc(bm[w]);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && s) atomicAdd(&sums[blockIdx.y], s);
}

}  // namespace colibri
