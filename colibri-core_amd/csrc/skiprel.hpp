// skiprel.hpp — the skip content of an indexed model's skipgrams: IndexedPatternModel::getskipcontent (reference include/patternmodel.h:3029-3059)
// summed over the model. (getinstances / gettemplates are the relation kinds kRelInstances / kRelTemplates of relations.hpp.)
//
// For every reference (s, t) of a skipgram A (n tokens, head = index of its first gap, tail = tokens after its last gap) whose window
// [t, t + n) lies inside sentence s, the content is the corpus bytes of the tokens [t + head, t + n - tail): the mask is dropped, so the tokens
// between two gaps belong to it. One row per (A, distinct content) with its count. A content is no pattern of the model: it gets its identity
// here, from its bytes.
//
// Identity (skiprel_api.inc drives the rounds). `pend` holds the references not yet numbered. Per round:
//   skc_insert_kernel    hash of (A, content bytes), re-mixed with the round; one table slot per distinct hash (arrivals with a slot's hash
//                        merge into it: equal contents are the norm, a chain of equal hashes walked by each member would be quadratic);
//                        the slot's representative is its lowest reference (atomicMin, read first: a reference that cannot lower it adds nothing)
//   skc_resolve_kernel   byte check against the representative: equal -> rep[k] = representative; different (a true collision) -> carried
//   (scan + skc_carry_kernel) the carried references are the next round's `pend`
// A class of equal (A, content) has one hash, hence one slot and one verdict: it is resolved whole, to its lowest reference, or carried whole.
// The lowest reference of a slot resolves to itself, so every round numbers at least one class: the rounds end, at any hash width, and the
// result does not depend on the hash. With 64 bits it is one round.
//   skc_isrep_kernel, scan, skc_number_kernel   the representatives numbered in reference order: per distinct pair its A, its bytes' place in the
//                        corpus, its length, and the content's own pattern number in the model (the B-list entry at t + head of that length
//                        without a mask; kInvalid: the model does not hold it)
//   skc_bytes_kernel     the distinct contents as key bytes
// Counting is the relation pipeline's: one event (content number, A) per reference, sorted, run-length counted, carried across chunks; the
// order is by the contents' key-byte ranks. gfx950 only.
#pragma once
#include "flexgrams.hpp"  // FSlot, flex_clear_kernel
#include "relations.hpp"

namespace colibri {

// the content of reference k: its pattern, the position of its first token, its tokens; false when A has no gap or the window leaves its
// sentence (*leaves set then)
__device__ __forceinline__ bool skc_content(const RelArgs& r, uint64_t k, uint32_t& a, uint32_t& q, uint32_t& nc, bool& leaves) {
    uint32_t na, start, end, p;
    leaves = false;
    if (!rel_a(r, k, a, na, start, end, p)) {
        leaves = r.pmask[r.aid[k]] != 0;
        return false;
    }
    const uint32_t m = r.pmask[a];
    if (!m) return false;
    if (p > end || na > end - p) {
        leaves = true;
        return false;
    }
    const uint32_t head = (uint32_t)__ffs((int)m) - 1u, last = 31u - (uint32_t)__clz((int)m);
    q  = p + head;
    nc = last + 1u - head;  // (= na - head - tail)
    return true;
}
__device__ __forceinline__ uint64_t skc_hash(uint32_t a, const uint8_t* __restrict__ b, uint32_t len, uint32_t round, uint64_t hmask) {
    uint64_t h = mix64(((uint64_t)round << 32) ^ a ^ 0x9E3779B97F4A7C15ull);
    for (uint32_t i = 0; i < len; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    h = mix64(h ^ len) & hmask;
    return h == kEmptyKey ? h ^ 1ull : h;
}
// flag[k] = reference k has a content; *skipped += the references of skipgrams whose window leaves its sentence or the corpus (rare: a loaded model)
__global__ __launch_bounds__(kBlock) void skc_flag_kernel(RelArgs r, uint64_t nrefs, uint32_t* __restrict__ flag, uint32_t* __restrict__ rep, unsigned long long* __restrict__ skipped) {
    for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < nrefs; k += (uint64_t)gridDim.x * kBlock) {
        uint32_t a, q, nc;
        bool     leaves;
        const bool ok = skc_content(r, k, a, q, nc, leaves);
        flag[k]       = ok ? 1u : 0u;
        rep[k]        = kInvalid;
        if (leaves) atomicAdd(skipped, 1ull);
    }
}
// pend[at[k]] = k for the flagged references
__global__ __launch_bounds__(kBlock) void skc_pend_kernel(const uint32_t* __restrict__ flag, const unsigned long long* __restrict__ at, uint64_t nrefs, uint32_t* __restrict__ pend) {
    for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < nrefs; k += (uint64_t)gridDim.x * kBlock)
        if (flag[k]) pend[at[k]] = (uint32_t)k;
}
__global__ __launch_bounds__(kBlock) void skc_insert_kernel(RelArgs r, const uint32_t* __restrict__ pend, uint64_t npend, uint32_t round, uint64_t hmask, FSlot* __restrict__ table,
                                                            uint32_t cap, uint32_t* __restrict__ slot_of) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < npend; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t k = pend[i];
        uint32_t       a, q, nc;
        bool           leaves;
        skc_content(r, k, a, q, nc, leaves);
        const uint32_t b0 = r.tokstart[q], b1 = r.tokstart[q + nc];
        const uint64_t h  = skc_hash(a, r.bytes + b0, b1 - b0, round, hmask);
        uint32_t       s  = slot_of_hash(mix64(h), cap);
        for (;;) {
            uint64_t old = table[s].hash;
            if (old == kEmptyKey) old = atomicCAS(reinterpret_cast<unsigned long long*>(&table[s].hash), (unsigned long long)kEmptyKey, (unsigned long long)h);
            if (old == kEmptyKey || old == h) break;
            s = (s + 1 == cap) ? 0 : s + 1;
        }
        if (table[s].rep > k) atomicMin(&table[s].rep, k);
        slot_of[i] = s;
    }
}
// rep[k] = the slot's representative when (A, bytes) are its; else carry[i] = 1
__global__ __launch_bounds__(kBlock) void skc_resolve_kernel(RelArgs r, const uint32_t* __restrict__ pend, uint64_t npend, const FSlot* __restrict__ table,
                                                             const uint32_t* __restrict__ slot_of, uint32_t* __restrict__ rep, uint32_t* __restrict__ carry) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < npend; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t k = pend[i], g = table[slot_of[i]].rep;
        bool           same = true;
        if (g != k) {
            uint32_t a, q, nc, a2, q2, nc2;
            bool     leaves;
            skc_content(r, k, a, q, nc, leaves);
            skc_content(r, g, a2, q2, nc2, leaves);
            const uint32_t b0 = r.tokstart[q], len = r.tokstart[q + nc] - b0, c0 = r.tokstart[q2], len2 = r.tokstart[q2 + nc2] - c0;
            same = a == a2 && len == len2;
            for (uint32_t x = 0; same && x < len; ++x) same = r.bytes[b0 + x] == r.bytes[c0 + x];
        }
        if (same) rep[k] = g;
        carry[i] = same ? 0u : 1u;
    }
}
__global__ __launch_bounds__(kBlock) void skc_carry_kernel(const uint32_t* __restrict__ pend, const uint32_t* __restrict__ carry, const unsigned long long* __restrict__ at, uint64_t npend,
                                                           uint32_t* __restrict__ next) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < npend; i += (uint64_t)gridDim.x * kBlock)
        if (carry[i]) next[at[i]] = pend[i];
}
__global__ __launch_bounds__(kBlock) void skc_isrep_kernel(const uint32_t* __restrict__ rep, uint64_t nrefs, uint32_t* __restrict__ isrep) {
    for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < nrefs; k += (uint64_t)gridDim.x * kBlock) isrep[k] = rep[k] == (uint32_t)k ? 1u : 0u;
}
// cnum[k] = the number of reference k's (A, content) pair (kInvalid: none); per representative the pair's facts
__global__ __launch_bounds__(kBlock) void skc_number_kernel(RelArgs r, const uint32_t* __restrict__ rep, const unsigned long long* __restrict__ num, uint64_t nrefs,
                                                            uint32_t* __restrict__ cnum, uint32_t* __restrict__ da, uint32_t* __restrict__ dsrc, uint32_t* __restrict__ dlen,
                                                            uint32_t* __restrict__ dpb, uint32_t* __restrict__ maxlen) {
    for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < nrefs; k += (uint64_t)gridDim.x * kBlock) {
        const uint32_t g = rep[k];
        cnum[k]          = g == kInvalid ? kInvalid : (uint32_t)num[g];
        if (g != (uint32_t)k) continue;
        uint32_t a, q, nc;
        bool     leaves;
        skc_content(r, k, a, q, nc, leaves);
        const uint32_t d = (uint32_t)num[k], b0 = r.tokstart[q], len = r.tokstart[q + nc] - b0;
        uint32_t       pb = kInvalid;
        for (uint64_t j = r.boff[q]; j < r.boff[q + 1]; ++j)
            if (r.bn[j] == nc && r.pmask[r.bid[j]] == 0) pb = r.bid[j];
        da[d]   = a;
        dsrc[d] = b0;
        dlen[d] = len;
        dpb[d]  = pb;
        atomicMax(maxlen, len);
    }
}
__global__ __launch_bounds__(kBlock) void skc_bytes_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ src, const uint32_t* __restrict__ perm,
                                                           const unsigned long long* __restrict__ off, uint64_t n, uint8_t* __restrict__ out) {
    for (uint64_t d = blockIdx.x * (uint64_t)kBlock + threadIdx.x; d < n; d += (uint64_t)gridDim.x * kBlock) {
        const uint32_t           s   = src[perm ? perm[d] : d];
        const unsigned long long o   = off[d];
        const uint32_t           len = (uint32_t)(off[d + 1] - o);
        for (uint32_t x = 0; x < len; ++x) out[o + x] = bytes[s + x];
    }
}
// one event per reference with a content: (key = its pair's number, val = A)
__global__ __launch_bounds__(kBlock) void skc_events_kernel(const uint32_t* __restrict__ cnum, uint64_t nrefs, uint32_t* __restrict__ events, uint32_t* __restrict__ maxev) {
    for (uint64_t k = blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < nrefs; k += (uint64_t)gridDim.x * kBlock) {
        const uint32_t e = cnum[k] != kInvalid ? 1u : 0u;
        events[k]        = e;
        if (e && *maxev == 0) atomicMax(maxev, 1u);
    }
}
__global__ __launch_bounds__(kBlock) void skc_emit_kernel(const uint32_t* __restrict__ cnum, const uint32_t* __restrict__ aid, uint64_t k0, uint64_t k1, unsigned long long base,
                                                          const unsigned long long* __restrict__ evoff, uint32_t* __restrict__ kb, uint32_t* __restrict__ ka) {
    for (uint64_t k = k0 + blockIdx.x * (uint64_t)kBlock + threadIdx.x; k < k1; k += (uint64_t)gridDim.x * kBlock) {
        if (cnum[k] == kInvalid) continue;
        const uint64_t w = evoff[k] - base;
        kb[w]            = cnum[k];
        ka[w]            = aid[k];
    }
}
// the rows in output order: the content's pattern number in the model and its length, by the pair number the row carries
__global__ __launch_bounds__(kBlock) void skc_rows_kernel(const uint32_t* __restrict__ rowd, uint64_t n, const uint32_t* __restrict__ dpb, const uint32_t* __restrict__ dlen,
                                                          uint32_t* __restrict__ pb, uint32_t* __restrict__ len) {
    for (uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        pb[i]  = dpb[rowd[i]];
        len[i] = dlen[rowd[i]];
    }
}

}  // namespace colibri
