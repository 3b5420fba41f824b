// compare.hpp — log-likelihood comparison of N pattern models (colibri-comparemodels; reference src/comparemodels.cpp with
// comparemodels_loglikelihood, src/patternmodel.cpp:22-171, after Rayson & Garside 2000).
//
// Rows: the union of the models' patterns, each once (with `-a`: those with a non-zero count in every model). Per row and model i: o_i = its
// count there (int), n_i = tokens() of model i (int); o_sum, n_sum as unsigned long long; e_i = exp(log(n_i) + log(o_sum) - log(n_sum));
// ll = 2 * sum over o_i > 0 of o_i * log(o_i / e_i), NaN -> 0, in the reference's order of evaluation (FMA contraction off). Sorted output:
// ll descending, then key bytes ascending (Pattern::operator<, src/pattern.cpp:1114-1125: byte-lexicographic, a proper prefix first); -0.0
// sorts as 0.0.
//
// The pipeline (compare_api.inc drives it) over the N models' keys concatenated (global key index g, model m(g)):
//   cmp_info_kernel       per key: 64-bit hash (fold_hash_key, the constrained-training key hash), tokens, category; longest key, most tokens
//   cmp_insert_kernel     every key into one open-addressed table (first free slot of its probe sequence; equal hashes are not merged)
//   cmp_rep_kernel        per key: its representative, the lowest g among the byte-equal keys of its probe chain (identity = the bytes)
//   (scan of rep[g] == g) the distinct patterns, numbered in g order
//   cmp_scatter_kernel    observed[d][m] = count (race-free: a model holds a key once); per (model, category, tokens) the occurrence totals
//                         (LDS-privatised when the table fits)
//   cmp_ll_kernel         one lane per distinct pattern: ll in double; the -a filter
//   cmp_compact_kernel    the kept patterns
//   cmp_keychunk_kernel / cooc-style LSD radix passes: key bytes (length, then four-byte groups from the last), then ll (two 32-bit passes)
//   cmp_emit_kernel       the rows in output order: representative (model, index), ll, observed[N], group totals[N]
// gfx950 only.
#pragma once
#include "constrained.hpp"

namespace colibri {

// the model of global key g: the last m with mstart[m] <= g
__device__ __forceinline__ uint32_t cmp_model_of(const uint32_t* __restrict__ mstart, uint32_t nm, uint32_t g) {
    uint32_t lo = 0, hi = nm;  // first m with mstart[m + 1] > g
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (mstart[mid + 1] <= g)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// per key: hash (hmask < ~0: a test override that forces collisions, so the byte checks decide), tokens (bytes < 128), category
// (colibri_host::category_of: the first token that is the skip class 3 -> skipgram (2), the flex class 4 -> flexgram (3), else n-gram (1));
// info[0] = longest key in bytes, info[1] = most tokens
__global__ __launch_bounds__(kBlock) void cmp_info_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, uint32_t T, uint64_t hmask,
                                                          uint64_t* __restrict__ hash, uint16_t* __restrict__ ntok, uint8_t* __restrict__ cat, uint32_t* __restrict__ info) {
    uint32_t mlen = 0, mn = 0;
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < T; g += gridDim.x * kBlock) {
        const uint8_t* k   = kbytes + koff[g];
        const uint32_t len = (uint32_t)(koff[g + 1] - koff[g]);
        uint64_t       h   = fold_hash_key(k, len) & hmask;
        if (h == kEmptyKey) h ^= 1ull;
        uint32_t n = 0, c = 0;
        bool     start = true;
        for (uint32_t i = 0; i < len; ++i) {
            if (start && c == 0 && k[i] == 3) c = 2;
            if (start && c == 0 && k[i] == 4) c = 3;
            start = k[i] < 128;
            n += start ? 1u : 0u;
        }
        hash[g] = h;
        ntok[g] = (uint16_t)(n > 0xFFFFu ? 0xFFFFu : n);
        cat[g]  = (uint8_t)(c == 0 ? 1u : c);
        mlen    = max(mlen, len);
        mn      = max(mn, n);
    }
    if (mlen) atomicMax(&info[0], mlen);
    if (mn) atomicMax(&info[1], mn);
}
__global__ __launch_bounds__(kBlock) void cmp_insert_kernel(const uint64_t* __restrict__ hash, const unsigned long long* __restrict__ koff, uint32_t T, CSlot* __restrict__ table,
                                                            uint32_t cap) {
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < T; g += gridDim.x * kBlock) {
        const uint64_t h = hash[g];
        uint32_t       s = slot_of_hash(mix64(h), cap);
        for (;;) {
            const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(&table[s].hash), (unsigned long long)kEmptyKey, (unsigned long long)h);
            if (old == kEmptyKey) {
                table[s].idx = g;
                table[s].len = (uint32_t)(koff[g + 1] - koff[g]);
                break;
            }
            s = (s + 1 == cap) ? 0 : s + 1;
        }
    }
}
// rep[g] = the lowest key index whose bytes equal key g's. Every key of hash h sits between h's home slot and the first free slot after it
// (linear probing, nothing is ever removed), so the walk to that free slot sees all of them.
__global__ __launch_bounds__(kBlock) void cmp_rep_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const uint64_t* __restrict__ hash, uint32_t T,
                                                         const CSlot* __restrict__ table, uint32_t cap, uint32_t* __restrict__ rep) {
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < T; g += gridDim.x * kBlock) {
        const uint64_t h   = hash[g];
        const uint8_t* key = kbytes + koff[g];
        const uint32_t len = (uint32_t)(koff[g + 1] - koff[g]);
        uint32_t       best = g, s = slot_of_hash(mix64(h), cap);
        for (uint32_t probe = 0; probe < cap; ++probe) {
            const CSlot c = table[s];
            if (c.hash == kEmptyKey) break;
            if (c.hash == h && c.len == len && c.idx < best) {
                const uint8_t* q    = kbytes + koff[c.idx];
                bool           same = true;
                uint32_t       k    = 0;
                for (; same && k + 8 <= len; k += 8) same = ld64u(key + k) == ld64u(q + k);
                for (; same && k < len; ++k) same = key[k] == q[k];
                if (same) best = c.idx;
            }
            s = (s + 1 == cap) ? 0 : s + 1;
        }
        rep[g] = best;
    }
}
__global__ __launch_bounds__(kBlock) void cmp_head_kernel(const uint32_t* __restrict__ rep, uint32_t T, uint32_t* __restrict__ head) {
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < T; g += gridDim.x * kBlock) head[g] = rep[g] == g ? 1u : 0u;
}
// observed[d * nm + m(g)] = count[g] for d = the distinct number of g's representative; rowg[d] = the representative; tot[(m * 4 + cat) * G + n]
// += count over every n-gram and skipgram (colibri_host computestats: a flexgram adds nothing to its (category, size) group). `lds`: the block
// sums its share in LDS first (4 * nm * G u64 must fit), else every key adds to HBM directly.
__global__ __launch_bounds__(kBlock) void cmp_scatter_kernel(const uint32_t* __restrict__ rep, const unsigned long long* __restrict__ did, const uint32_t* __restrict__ cnt,
                                                             const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat, const uint32_t* __restrict__ mstart, uint32_t nm,
                                                             uint32_t T, uint32_t G, int lds, uint32_t* __restrict__ observed, uint32_t* __restrict__ rowg,
                                                             unsigned long long* __restrict__ tot) {
    extern __shared__ unsigned long long stot[];
    const uint32_t nt = 4u * nm * G;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < nt; i += kBlock) stot[i] = 0;
        __syncthreads();
    }
    for (uint32_t g = blockIdx.x * kBlock + threadIdx.x; g < T; g += gridDim.x * kBlock) {
        const uint32_t r = rep[g], m = cmp_model_of(mstart, nm, g), c = cnt[g];
        const uint64_t d = did[r];
        observed[d * nm + m] = c;
        if (r == g) rowg[d] = g;
        if (cat[g] == 3 || c == 0) continue;
        const uint32_t t = (m * 4u + cat[g]) * G + ntok[g];
        if (lds)
            atomicAdd(&stot[t], (unsigned long long)c);
        else
            atomicAdd(&tot[t], (unsigned long long)c);
    }
    if (lds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nt; i += kBlock)
            if (stot[i]) atomicAdd(&tot[i], stot[i]);
    }
}
// one lane per distinct pattern: ll as the reference computes it (patternmodel.h:114-150), keep = not -a, or a non-zero count in every model
__global__ __launch_bounds__(kBlock) void cmp_ll_kernel(const uint32_t* __restrict__ observed, const int* __restrict__ tokens, uint32_t nm, uint32_t D, int conj,
                                                        double* __restrict__ ll, uint32_t* __restrict__ keep) {
#pragma clang fp contract(off)
    for (uint32_t d = blockIdx.x * kBlock + threadIdx.x; d < D; d += gridDim.x * kBlock) {
        const uint32_t* o    = observed + (size_t)d * nm;
        unsigned long long n_sum = 0, o_sum = 0;
        bool           all   = true;
        for (uint32_t i = 0; i < nm; ++i) {
            const int oi = (int)o[i];
            all          = all && oi != 0;
            n_sum += tokens[i];
            o_sum += oi;
        }
        const double lo = log((double)o_sum), ln = log((double)n_sum);
        double       v  = 0;
        for (uint32_t i = 0; i < nm; ++i) {
            const int oi = (int)o[i];
            if (oi > 0) {
                const double e = exp((log((double)tokens[i]) + lo) - ln);
                v              = v + (oi * log(oi / e));
            }
        }
        v = v * 2;
        if (isnan(v)) v = 0;
        ll[d]   = v;
        keep[d] = (!conj || all) ? 1u : 0u;
    }
}
__global__ __launch_bounds__(kBlock) void cmp_compact_kernel(const uint32_t* __restrict__ keep, const unsigned long long* __restrict__ kofs, const uint32_t* __restrict__ rowg,
                                                             uint32_t D, uint32_t* __restrict__ kd, uint32_t* __restrict__ kg) {
    for (uint32_t d = blockIdx.x * kBlock + threadIdx.x; d < D; d += gridDim.x * kBlock) {
        if (!keep[d]) continue;
        const uint64_t k = kofs[d];
        kd[k]            = d;
        kg[k]            = rowg[d];
    }
}
// the sort key of pass `chunk` for the row at perm[i]: its key's chunk-th group of four bytes, zero-padded, big-endian; chunk = kInvalid: the
// key's length (the least significant pass). Key bytes are never 0, so this is Pattern::operator<.
__global__ __launch_bounds__(kBlock) void cmp_keychunk_kernel(const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const uint32_t* __restrict__ kg,
                                                              const uint32_t* __restrict__ perm, uint32_t K, uint32_t chunk, uint32_t* __restrict__ key) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < K; i += gridDim.x * kBlock) {
        const uint32_t g   = kg[perm[i]];
        const uint8_t* k   = kbytes + koff[g];
        const uint32_t len = (uint32_t)(koff[g + 1] - koff[g]);
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
// ll descending as an ascending 64-bit sort key (half 0: low, 1: high 32 bits); -0.0 is 0.0 (the reference's set compares them equal)
__global__ __launch_bounds__(kBlock) void cmp_valkey_kernel(const double* __restrict__ ll, const uint32_t* __restrict__ kd, const uint32_t* __restrict__ perm, uint32_t K, int half,
                                                            uint32_t* __restrict__ key) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < K; i += gridDim.x * kBlock) {
        double v = ll[kd[perm[i]]];
        if (v == 0.0) v = 0.0;
        uint64_t u = (uint64_t)__double_as_longlong(v);
        u          = (u >> 63) ? ~u : (u | (1ull << 63));
        u          = ~u;
        key[i]     = half ? (uint32_t)(u >> 32) : (uint32_t)u;
    }
}
// row r of the output (perm == NULL: the kept patterns in distinct order, i.e. by their representative's g)
__global__ __launch_bounds__(kBlock) void cmp_emit_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ kd, const uint32_t* __restrict__ kg,
                                                          const double* __restrict__ ll, const uint32_t* __restrict__ observed, const unsigned long long* __restrict__ tot,
                                                          const uint16_t* __restrict__ ntok, const uint8_t* __restrict__ cat, const uint32_t* __restrict__ mstart, uint32_t nm,
                                                          uint32_t G, uint32_t K, uint32_t* __restrict__ omodel, uint32_t* __restrict__ oindex, double* __restrict__ oll,
                                                          uint32_t* __restrict__ oobs, uint32_t* __restrict__ ogt) {
    for (uint32_t r = blockIdx.x * kBlock + threadIdx.x; r < K; r += gridDim.x * kBlock) {
        const uint32_t k = perm ? perm[r] : r, d = kd[k], g = kg[k], m = cmp_model_of(mstart, nm, g);
        omodel[r] = m;
        oindex[r] = g - mstart[m];
        oll[r]    = ll[d];
        const uint32_t c = cat[g], n = ntok[g];
        for (uint32_t i = 0; i < nm; ++i) {
            oobs[(size_t)r * nm + i] = observed[(size_t)d * nm + i];
            ogt[(size_t)r * nm + i]  = c == 3 ? 0u : (uint32_t)tot[(i * 4u + c) * G + n];  // (unsigned int, as totaloccurrencesingroup returns it)
        }
    }
}
// global key offsets: the model's own offsets shifted by where its bytes start
__global__ __launch_bounds__(kBlock) void cmp_shift_kernel(unsigned long long* __restrict__ koff, uint32_t n, unsigned long long base) {
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) koff[i] += base;
}

}  // namespace colibri
