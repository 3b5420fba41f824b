// chain_step.hpp — an entry of the chained orders' step tables, and which entries a block takes: plain C++, __host__ __device__, shared by chain.hpp and the
// host-side check tests/chain_step_check.cpp.
// A step is a piece of at most `kChStep` pairs of ONE (bucket, shard) list; its table entry is {index of its first pair in plist / pcode, pairs | bucket << 16}.
// The bucket travels in the entry because a reader cannot recover it from the index: the head windows' lists lie behind the shards', in another layout.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COLIBRI_STEP_HD __host__ __device__ __forceinline__
#else
#define COLIBRI_STEP_HD inline
#endif

namespace colibri {

constexpr uint32_t kChStepPairBits = 16;  // pairs of a step <= kChStep <= 65 535; the bucket (< kBi2Buckets <= 65 536) above them
COLIBRI_STEP_HD uint32_t chain_step_pack(uint32_t pairs, uint32_t bucket) { return pairs | (bucket << kChStepPairBits); }
COLIBRI_STEP_HD uint32_t chain_step_pairs(uint32_t y) { return y & ((1u << kChStepPairBits) - 1u); }
COLIBRI_STEP_HD uint32_t chain_step_bucket(uint32_t y) { return y >> kChStepPairBits; }

// Runs: block k of the `nper` blocks of an XCD takes the table entries (k + j nper) R .. (k + j nper) R + R - 1 for j = 0, 1, ... — R consecutive entries at a time,
// round-robin over the blocks in units of R (R = 1: entries k, k + nper, ...). Every entry belongs to exactly one block.
COLIBRI_STEP_HD uint32_t chain_run_first(uint32_t k, uint32_t run) { return k * run; }
COLIBRI_STEP_HD uint32_t chain_run_next(uint32_t s, uint32_t nper, uint32_t run) { return (s + 1u) % run != 0u ? s + 1u : s + 1u + (nper - 1u) * run; }

}  // namespace colibri
