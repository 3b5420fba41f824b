// expand.hpp — expanding a loaded model on further corpus data: the reference's train() on a NON-EMPTY model with continued = false
// (include/patternmodel.h:880-1270, colibri-patternmodeller -i model -f corpus -e N). The loaded patterns are a SEED set: the constraint set's
// open-addressed table (constrained.hpp) plus one count per pattern. Every order counts its windows on the global table as an unseeded run does;
// between count and prune the SEED JOIN walks the table's occupied slots — one probe per DISTINCT key of the order, never one per corpus position —,
// adds the seed's count to the slot on a hit (so the prune compares new + loaded with MINTOKENS and the export carries the sum) and counts the misses:
// they are the keys the order CREATED, the reference's `found`. An order that creates nothing ends the run before its prune.
// The look-back of the next order asks "is the (n-1)-gram a key of the model as it stands": for a window the order counted that is its survivor id; a
// window the order did NOT count (its own look-back failed) can still be a loaded pattern that stays — only in a seed set that is not closed under
// sub-windows with non-increasing counts (seed_closed_kernel), and only then seed_fill_kernel probes those positions. gfx950 only.
#pragma once
#include "constrained.hpp"

namespace colibri {

struct SeedInfo {
    uint32_t created;  // occupied slots of the order's table that are no seed
    uint32_t filled;   // positions that got a seed's id from seed_fill_kernel
    uint32_t open;     // seed_closed_kernel: some seed of two or more tokens has a sub-window that is no seed, or one with a smaller count
    uint32_t erased;   // seed_rows_kernel: seeds of the order that never occurred in the corpus and go (their own count is below the threshold)
    uint32_t saturated;  // seed_join_kernel: a loaded count plus the corpus' does not fit 32 bits: the run is refused (COLIBRI_ERR_OVERFLOW)
    uint32_t pad[3];
};
constexpr uint32_t kSeedIdFlag  = 0x80000000u;  // survivor id of a window that is a loaded pattern the order did not count: kSeedIdFlag | seed number
constexpr uint64_t kMaxSeeds    = 0x7FFFFFF0ull;  // (so that such an id is never kInvalid)

// hash of the window of n tokens at position i, folded token by token as fold_hash_key folds a key's bytes (a corpus token has at most 8 bytes)
__device__ __forceinline__ uint64_t seed_window_hash(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ tokstart, uint32_t i, int n, uint32_t* a0, uint32_t* len) {
    uint64_t h = kConstraintSeed;
    uint32_t a = tokstart[i];
    *a0        = a;
    for (int k = 1; k <= n; ++k) {
        const uint32_t e = tokstart[i + k];
        h                = fold_chunk(h, bytes + a, e - a);
        a                = e;
    }
    *len = a - *a0;
    return h == kEmptyKey ? h ^ 1ull : h;
}

__device__ __forceinline__ void block_add(uint32_t* counter, uint32_t v) {  // (every lane of the block arrives)
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && v) atomicAdd(counter, v);
}

// the seed join: table = the order's counted table (Slot.rep = a position where the key's window starts), before the prune
__global__ __launch_bounds__(kBlock) void seed_join_kernel(Slot* __restrict__ table, const DevState* __restrict__ st, const uint8_t* __restrict__ bytes,
                                                            const uint32_t* __restrict__ tokstart, int n, const CSlot* __restrict__ stable, uint32_t scap,
                                                            const uint8_t* __restrict__ jbytes, const unsigned long long* __restrict__ joff,
                                                            const uint32_t* __restrict__ seed_count, uint32_t* __restrict__ seed_slot, SeedInfo* __restrict__ info) {
    if (st->done) return;
    const uint32_t cap = st->cap;
    uint32_t       ncreated = 0;
    for (uint32_t base = blockIdx.x * kBlock; base < cap; base += gridDim.x * kBlock) {
        const uint32_t s = base + threadIdx.x;
        if (s >= cap) continue;
        const Slot sl = table[s];
        if (sl.key == kEmptyKey) continue;
        uint32_t       a0, len;
        const uint64_t h   = seed_window_hash(bytes, tokstart, sl.rep, n, &a0, &len);
        const uint32_t cs  = slot_of_hash(mix64(h), scap);
        const uint32_t idx = constraint_lookup(bytes + a0, len, h, stable[cs], cs, stable, scap, jbytes, joff);
        if (idx == kInvalid) {
            ++ncreated;
            continue;
        }
        const uint64_t sum = (uint64_t)sl.count + seed_count[idx];
        if (sum > 0xFFFFFFFFull) info->saturated = 1;  // (the host ends the run: a count is 32 bits wide everywhere behind this point)
        table[s].count = (uint32_t)sum;
        seed_slot[idx]     = s;
    }
    block_add(&info->created, ncreated);
}

// after the order's prune: which result row carries each seed of n tokens, and whether the seed stays in the model. stop: the order was not pruned
__global__ __launch_bounds__(kBlock) void seed_rows_kernel(uint32_t npatterns, const uint8_t* __restrict__ seed_order, int n, const uint32_t* __restrict__ seed_slot,
                                                            const uint32_t* __restrict__ seed_count, const Slot* __restrict__ table, uint32_t thr, int stop,
                                                            uint32_t* __restrict__ row_of_seed, uint8_t* __restrict__ kept, SeedInfo* __restrict__ info) {
    uint32_t nerased = 0;
    for (uint32_t base = blockIdx.x * kBlock; base < npatterns; base += gridDim.x * kBlock) {
        const uint32_t p = base + threadIdx.x;
        if (p >= npatterns || seed_order[p] != (uint8_t)n) continue;
        const uint32_t s = seed_slot[p];
        if (s != kInvalid) {
            const uint32_t tag = table[s].count;
            const uint32_t row = (tag & kKeptFlag) ? (tag & ~kKeptFlag) : kInvalid;
            row_of_seed[p]     = row;
            kept[p]            = (row != kInvalid || stop) ? 1 : 0;
        } else {
            const bool stays = stop || seed_count[p] >= thr;
            kept[p]          = stays ? 1 : 0;
            nerased += stays ? 0u : 1u;
        }
    }
    block_add(&info->erased, nerased);
}

// an indexed run: references per result row = the row's summed count minus the loaded count of the seed it carries (refcnt starts as a copy of the counts)
__global__ __launch_bounds__(kBlock) void seed_refcnt_kernel(uint32_t npatterns, const uint32_t* __restrict__ row_of_seed, const uint32_t* __restrict__ seed_count, uint32_t nrows,
                                                              uint32_t* __restrict__ refcnt) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < npatterns; p += gridDim.x * kBlock) {
        const uint32_t r = row_of_seed[p];
        if (r < nrows) refcnt[r] -= seed_count[p];  // (one seed per row: keys are distinct)
    }
}

// a window of n tokens the order did not count, which is a loaded pattern that stays (count >= thr), is a key of the model for the next order's look-back.
// (A window the order counted and pruned has new + loaded < thr, so its seed fails the same test: ids[i] == kInvalid needs no second look.)
__global__ __launch_bounds__(kBlock) void seed_fill_kernel(uint32_t* __restrict__ ids, const uint32_t* __restrict__ rem, uint32_t npos, const uint8_t* __restrict__ bytes,
                                                            const uint32_t* __restrict__ tokstart, int n, const CSlot* __restrict__ stable, uint32_t scap,
                                                            const uint8_t* __restrict__ jbytes, const unsigned long long* __restrict__ joff,
                                                            const uint32_t* __restrict__ seed_count, uint32_t thr, SeedInfo* __restrict__ info) {
    uint32_t nfilled = 0;
    for (uint32_t base = blockIdx.x * kBlock; base < npos; base += gridDim.x * kBlock) {
        const uint32_t i = base + threadIdx.x;
        if (i >= npos || ids[i] != kInvalid || rem[i] < (uint32_t)n) continue;
        uint32_t       a0, len;
        const uint64_t h   = seed_window_hash(bytes, tokstart, i, n, &a0, &len);
        const uint32_t cs  = slot_of_hash(mix64(h), scap);
        const uint32_t idx = constraint_lookup(bytes + a0, len, h, stable[cs], cs, stable, scap, jbytes, joff);
        if (idx != kInvalid && seed_count[idx] >= thr) {
            ids[i] = kSeedIdFlag | idx;
            ++nfilled;
        }
    }
    block_add(&info->filled, nfilled);
}

// Is the seed set closed under sub-windows with non-increasing counts — has every seed of two or more tokens both its windows one token shorter
// as seeds, each with a count no smaller than its own? A model this training procedure built is. Then a loaded pattern that stays has sub-windows
// that stay, its windows pass the look-back and are counted, and seed_fill_kernel has nothing to find.
__global__ __launch_bounds__(kBlock) void seed_closed_kernel(const uint8_t* __restrict__ jbytes, const unsigned long long* __restrict__ joff, uint32_t npatterns,
                                                              const CSlot* __restrict__ stable, uint32_t scap, const uint32_t* __restrict__ seed_count, SeedInfo* __restrict__ info) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < npatterns; p += gridDim.x * kBlock) {
        const uint8_t* key = jbytes + joff[p];
        const uint32_t len = (uint32_t)(joff[p + 1] - joff[p]);
        uint32_t       first_end = 0, last_start = 0;  // end of the first token, start of the last
        for (uint32_t i = 0; i + 1 < len; ++i)
            if (key[i] < 128) {
                if (first_end == 0) first_end = i + 1;
                last_start = i + 1;
            }
        if (first_end == 0) continue;  // one token (or none)
        const uint32_t mine = seed_count[p];
        const uint8_t* sub[2]  = {key, key + first_end};
        const uint32_t slen[2] = {last_start, len - first_end};
        for (int k = 0; k < 2; ++k) {
            const uint64_t h   = fold_hash_key(sub[k], slen[k]);
            const uint32_t cs  = slot_of_hash(mix64(h), scap);
            const uint32_t idx = constraint_lookup(sub[k], slen[k], h, stable[cs], cs, stable, scap, jbytes, joff);
            if (idx == kInvalid || seed_count[idx] < mine) info->open = 1;
        }
    }
}

}  // namespace colibri
