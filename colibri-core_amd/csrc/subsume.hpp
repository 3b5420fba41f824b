// subsume.hpp — the two subsumption prunes of a finished model (PatternModelOptions::PRUNENONSUBSUMED / PRUNESUBSUMED, colibri-patternmodeller
// -p / --prunesubsumed; reference include/patternmodel.h:1285-1336 with prunenotinset / pruneinset :2194-2242) as a mark and sweep over the
// model's own keys. The specification:
//
// A key is a sequence of tokens, a token ends at its first byte < 128, {*} is the one byte 03 and a token like any other. The two sub-patterns
// of a pattern of n tokens are its first n-1 and its last n-1 tokens, as byte strings. `alive` starts as the whole model.
//   pass 1 (PRUNENONSUBSUMED = p > 0), n = min(p, MAXLENGTH) down to 2: M = the alive patterns of n tokens. M empty: nothing happens at this
//          level. Otherwise every alive pattern of n-1 tokens that is no sub-pattern of a member of M dies. A cascade: level n-1 sees what
//          level n left.
//   pass 2 (PRUNESUBSUMED = S > 0), after pass 1 and on its survivors, n = 2 up to min(S, MAXLENGTH): every alive pattern of n-1 tokens that is a
//          sub-pattern of an alive pattern of n tokens dies. Level n kills (n-1)-grams and level n+1 marks with n+1-grams: the levels do not
//          see one another's work.
//
// The pipeline (subsume_api.inc drives it; the key table is the constraint set's, constrained.hpp, and the token counts are cooc_info_kernel's):
//   subsume_hist_kernel     patterns per length (tokens 0..255, LDS histogram) -> scan -> the start of every length's list
//   subsume_scatter_kernel  the pattern numbers, one list per length (a block reserves its share of every list with one atomic per length)
//   subsume_mark_kernel     one lane per pattern of the marking length n that is alive: the end of its first and the start of its last token,
//                           the two slices of its own key bytes hashed (fold_hash_key under the call's mask) and looked up (constraint_lookup);
//                           mark[found] = the level's tag. Nothing is copied. The alive markers are counted (one atomic per block).
//   subsume_sweep_kernel    one lane per pattern of the pruned length n-1 that is alive: it dies when unmarked (pass 1) or marked (pass 2).
//                           The dead are counted per wave with a ballot and added by one atomic per block, to the level's count and off the
//                           alive count of their length.
// The empty-M rule is the sweep's: it reads the alive count of the marking length, which the sweep of the level above left, and does nothing
// at 0. So the host enqueues the whole ladder from the length histogram alone (a level whose marking length the model never had costs no
// launch, a level walks only the lists of its two lengths) and reads the counts once, at the end.
// Marks are level TAGS, never cleared: pass 1's level n writes n, pass 2's level n writes kSubsumePass2 | n, and a sweep compares with its own
// level's tag, so a mark of pass 1 (or of any other level) is no mark to pass 2. Every writer of a launch stores the same value: plain stores.
// gfx950 only.
#pragma once
#include "constrained.hpp"

namespace colibri {

constexpr uint32_t kSubsumeLengths = 256;      // cooc_info_kernel's token counts are bytes: 255 stands for "255 or more"
constexpr uint32_t kSubsumePass2   = 0x10000;  // tag bit of pass 2's marks
static_assert(kBlock == (int)kSubsumeLengths, "the histogram kernels give every length one thread of a block");

// hist[t] = patterns of t tokens
__global__ __launch_bounds__(kBlock) void subsume_hist_kernel(const uint8_t* __restrict__ ntok, uint32_t np, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kSubsumeLengths];
    h[threadIdx.x] = 0;  // (kBlock == kSubsumeLengths)
    __syncthreads();
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < np; p += gridDim.x * kBlock) atomicAdd(&h[ntok[p]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
// list[start[t] ..] = the patterns of t tokens, in no particular order; cursor[t] = 0 on entry, hist[t] on return
__global__ __launch_bounds__(kBlock) void subsume_scatter_kernel(const uint8_t* __restrict__ ntok, uint32_t np, const unsigned long long* __restrict__ start,
                                                                 uint32_t* __restrict__ cursor, uint32_t* __restrict__ list) {
    __shared__ uint32_t h[kSubsumeLengths], base[kSubsumeLengths];
    for (uint32_t b0 = blockIdx.x * kBlock; b0 < np; b0 += gridDim.x * kBlock) {  // (b0 is the block's: every lane takes every barrier)
        h[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t p = b0 + threadIdx.x;
        uint32_t       t = 0, rank = 0;
        if (p < np) {
            t    = ntok[p];
            rank = atomicAdd(&h[t], 1u);
        }
        __syncthreads();
        if (h[threadIdx.x]) base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], h[threadIdx.x]);
        __syncthreads();
        if (p < np) list[start[t] + base[t] + rank] = p;
        __syncthreads();
    }
}

// a block's sum of its waves' counts (`v` is wave-uniform), handed to thread 0
__device__ __forceinline__ uint32_t subsume_block_sum(uint32_t v) {
    __shared__ uint32_t part[kBlock / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = v;
    __syncthreads();
    uint32_t s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kBlock / kWave; ++w) s += part[w];
    return s;
}

// members[0..n): the patterns of the marking length. *nmarkers += the alive ones (each makes two look-ups)
__global__ __launch_bounds__(kBlock) void subsume_mark_kernel(const uint32_t* __restrict__ members, uint32_t n, const uint8_t* __restrict__ alive, const uint8_t* __restrict__ kbytes,
                                                              const unsigned long long* __restrict__ koff, const CSlot* __restrict__ table, uint32_t cap, uint64_t hmask, uint32_t tag,
                                                              uint32_t* __restrict__ mark, uint32_t* __restrict__ nmarkers) {
    uint32_t cnt = 0;
    for (uint32_t b0 = blockIdx.x * kBlock; b0 < n; b0 += gridDim.x * kBlock) {
        const uint32_t i  = b0 + threadIdx.x;
        const uint32_t p  = i < n ? members[i] : 0u;
        const bool     on = i < n && alive[p] != 0;
        cnt += (uint32_t)__popcll(__ballot(on));
        if (on) {
            const uint8_t* key = kbytes + koff[p];
            const uint32_t len = (uint32_t)(koff[p + 1] - koff[p]);
            uint32_t       a = 0, cut = 0;  // end of the first token, start of the last
            for (uint32_t k = 0; k + 1 < len; ++k)
                if (key[k] < 128) {
                    if (a == 0) a = k + 1;
                    cut = k + 1;
                }
            if (cut != 0) {  // (0: one token, not a marking length)
                const uint64_t h0 = fold_hash_key(key, cut) & hmask, h1 = fold_hash_key(key + a, len - a) & hmask;
                const uint32_t s0 = slot_of_hash(mix64(h0), cap), s1 = slot_of_hash(mix64(h1), cap);
                const CSlot    c0 = table[s0], c1 = table[s1];  // both first probes in flight together
                const uint32_t f0 = constraint_lookup(key, cut, h0, c0, s0, table, cap, kbytes, koff);
                const uint32_t f1 = constraint_lookup(key + a, len - a, h1, c1, s1, table, cap, kbytes, koff);
                if (f0 != kInvalid) mark[f0] = tag;
                if (f1 != kInvalid) mark[f1] = tag;
            }
        }
    }
    const uint32_t s = subsume_block_sum(cnt);
    if (threadIdx.x == 0 && s) atomicAdd(nmarkers, s);
}

// members[0..n): the patterns of the pruned length. gate: the alive count of the marking length (pass 1: 0 = the level does nothing; NULL: no
// gate). The dead leave `alive`, *pruned += their number, *nalive -= it.
__global__ __launch_bounds__(kBlock) void subsume_sweep_kernel(const uint32_t* __restrict__ members, uint32_t n, uint8_t* __restrict__ alive, const uint32_t* __restrict__ mark,
                                                               uint32_t tag, int die_marked, const uint32_t* __restrict__ gate, uint32_t* __restrict__ nalive,
                                                               unsigned long long* __restrict__ pruned) {
    if (gate != nullptr && *gate == 0) return;  // (written by an earlier launch; uniform over the grid)
    uint32_t cnt = 0;
    for (uint32_t b0 = blockIdx.x * kBlock; b0 < n; b0 += gridDim.x * kBlock) {
        const uint32_t i   = b0 + threadIdx.x;
        const uint32_t p   = i < n ? members[i] : 0u;
        const bool     die = i < n && alive[p] != 0 && ((mark[p] == tag) == (die_marked != 0));
        if (die) alive[p] = 0;
        cnt += (uint32_t)__popcll(__ballot(die));
    }
    const uint32_t s = subsume_block_sum(cnt);
    if (threadIdx.x == 0 && s) {
        atomicAdd(pruned, (unsigned long long)s);
        atomicSub(nalive, s);
    }
}

}  // namespace colibri
