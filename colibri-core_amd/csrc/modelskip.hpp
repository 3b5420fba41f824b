// modelskip.hpp — the skipgrams of an indexed model that already holds its n-grams: IndexedPatternModel::trainskipgrams (reference
// include/patternmodel.h:2969-3010 over computeskipgrams :1370-1537, prune :2107-2128 and the indexed pruneskipgrams :3362-3383), what
// colibri-patternmodeller -i model -s runs. No corpus is read: a skipgram's references are its source n-grams' references, and its skip-type
// count is the number of its sources. The specification, t = MINTOKENS, msk = max(MINTOKENS_SKIPGRAMS, t), T = MINSKIPTYPES:
//
//   for n = 3 .. MAXLENGTH, with the gap masks of compute_skip_configurations(n, MAXSKIPS):
//     every live n-gram G of n tokens is a source iff msk <= 1 or its first n-1 and its last n-1 tokens are both live patterns of the model;
//     every (source, mask) is a candidate: the key of G with every masked token replaced by the one byte 03;
//     the candidates of equal bytes are one skipgram: count = the sum of its sources' reference counts, types = its sources;
//     no skipgram at this order: the loop ends here and this order is NOT pruned;
//     otherwise every pattern of n tokens with count < t goes (n-grams too: that is what order n+1 sees), then every skipgram with types < T.
//
// The pipeline per order (modelskip_api.inc drives it; the key table is the constraint set's, constrained.hpp, and the token counts are
// cooc_info_kernel's):
//   mskip_valid_kernel    one lane per pattern: a live n-gram of n tokens whose two slices (byte ranges of its own key) are found live -> flag
//   mskip_sources_kernel  the flagged patterns, ascending, as the order's source list (ranks from a scan: the candidate order is deterministic)
//   mskip_len_kernel      one lane per candidate (source i, mask m) = i * nmasks + m: the masked key's length; the key is read in 8-byte words
//   mskip_write_kernel    the masked bytes behind the scan of the lengths: assembled in a register, stored 8 bytes at a time, the tail in 4 / 2 / 1
//   mskip_insert_kernel   open-addressed table on a seeded 64-bit hash of the masked bytes: a group's representative is its lowest candidate;
//                         its references and its members are summed by ONE 64-bit atomic per candidate (members in the high word)
//   mskip_verify_kernel   every member compares its bytes with the representative's, word-wise: a collision is seen and the caller retries
//                         under another seed (up to four), so groups are exact
//   mskip_groups_kernel   dense group numbers in representative order; count, types, key length; the verdict (below t / below T / kept), counted
//                         per wave with ballots and added by one atomic per wave
//   mskip_prune_kernel    the n-grams of n tokens below t leave `live` and `keep`
//   mskip_contrib_kernel  references each candidate hands to a KEPT group (0 for the others: their references are never touched)
//   mskip_ref_list_kernel one lane per kept reference: which input reference it is, its group; then the radix sort by (group, sentence, token)
//                         that flexgrams use, which leaves every kept group's list contiguous and ascending
//   mskip_keys_kernel     the kept groups' keys, copied word-wise from their representatives
// Candidates, groups and table slots reach 2^32 - 16: every loop over them counts in 64 bits (a 32-bit counter would wrap under the grid's stride and
// never end); the loops over patterns stay 32-bit, a model has fewer than 2^31 - 16. gfx950 only.
#pragma once
#include "constrained.hpp"
#include "flexgrams.hpp"  // kSkipByte
#include "textenc.hpp"    // text_hash

namespace colibri {

struct MSlot {
    uint64_t           hash;  // kEmptyKey = free
    uint32_t           rep;   // lowest candidate of the group
    uint32_t           pad;
    unsigned long long acc;   // members << 32 | references (a model's references are fewer than 2^32 and no two sources share one: no carry)
};
struct MskipInfo {
    uint32_t collision;
    uint32_t maxsentence;
    uint32_t pruned_ngrams;  // n-grams of the order below t
    uint32_t pruned_groups;  // skipgrams of the order below t
    uint32_t extra;          // surviving skipgrams below T
    uint32_t kept;
    uint32_t pad[2];
};
constexpr int kMskipMaxTokens = 31;  // a gap mask is 32 bits and the last token is never masked

// the masked form of a key, byte by byte into `sink`: token k (a token ends at its first byte < 128) becomes the one byte 03 iff bit k of mask.
// The key is fetched in 8-byte words (the model's bytes end in 16 bytes of slack).
template <class Sink>
__device__ __forceinline__ void mskip_masked(const uint8_t* __restrict__ key, uint32_t len, uint32_t mask, Sink& sink) {
    uint32_t tok = 0;
    for (uint32_t off = 0; off < len; off += 8) {
        uint64_t       w  = ld64u(key + off);
        const uint32_t nb = min(8u, len - off);
        for (uint32_t b = 0; b < nb; ++b, w >>= 8) {
            const uint32_t byte   = (uint32_t)(w & 0xFFu);
            const bool     last   = byte < 128;
            const bool     masked = (mask >> (tok & 31)) & 1u;
            if (!masked)
                sink.put(byte);
            else if (last)
                sink.put(kSkipByte);
            tok += last ? 1u : 0u;
        }
    }
}
struct MskipCount {
    uint32_t n = 0;
    __device__ __forceinline__ void put(uint32_t) { ++n; }
};
struct MskipStore {  // bytes gather in a register and leave 8 at a time; finish() stores the rest in 4 / 2 / 1 (the next candidate's bytes follow at once)
    uint8_t* out;
    uint64_t acc = 0;
    uint32_t n   = 0;
    __device__ __forceinline__ void put(uint32_t byte) {
        acc |= (uint64_t)byte << (8 * n);
        if (++n == 8) {
            __builtin_memcpy(out, &acc, 8);
            out += 8;
            acc = 0;
            n   = 0;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n & 4) {
            const uint32_t v = (uint32_t)acc;
            __builtin_memcpy(out, &v, 4);
            out += 4;
            acc >>= 32;
        }
        if (n & 2) {
            const uint16_t v = (uint16_t)acc;
            __builtin_memcpy(out, &v, 2);
            out += 2;
            acc >>= 16;
        }
        if (n & 1) *out = (uint8_t)acc;
    }
};

// flag[p] = 1 iff p is a live pattern of n tokens and (check == 0 or its first and its last n - 1 tokens are both live patterns)
__global__ __launch_bounds__(kBlock) void mskip_valid_kernel(const uint8_t* __restrict__ ntok, const uint8_t* __restrict__ live, uint32_t np, uint32_t n, int check,
                                                             const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const CSlot* __restrict__ table, uint32_t cap,
                                                             uint32_t* __restrict__ flag) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < np; p += gridDim.x * kBlock) {
        bool on = ntok[p] == n && live[p] != 0;
        if (on && check) {
            const uint8_t* key = kbytes + koff[p];
            const uint32_t len = (uint32_t)(koff[p + 1] - koff[p]);
            uint32_t       a = 0, cut = 0;  // end of the first token, start of the last
            for (uint32_t k = 0; k + 1 < len; ++k)
                if (key[k] < 128) {
                    if (a == 0) a = k + 1;
                    cut = k + 1;
                }
            const uint64_t h0 = fold_hash_key(key, cut), h1 = fold_hash_key(key + a, len - a);
            const uint32_t s0 = slot_of_hash(mix64(h0), cap), s1 = slot_of_hash(mix64(h1), cap);
            const CSlot    c0 = table[s0], c1 = table[s1];  // both first probes in flight together
            const uint32_t f0 = constraint_lookup(key, cut, h0, c0, s0, table, cap, kbytes, koff);
            const uint32_t f1 = constraint_lookup(key + a, len - a, h1, c1, s1, table, cap, kbytes, koff);
            on                = f0 != kInvalid && f1 != kInvalid && live[f0] != 0 && live[f1] != 0;
        }
        flag[p] = on ? 1u : 0u;
    }
}
__global__ __launch_bounds__(kBlock) void mskip_sources_kernel(const uint32_t* __restrict__ flag, const unsigned long long* __restrict__ rank, uint32_t np, uint32_t* __restrict__ src) {
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < np; p += gridDim.x * kBlock)
        if (flag[p]) src[rank[p]] = p;
}
// candidate c = source c / nmasks under mask c % nmasks
__global__ __launch_bounds__(kBlock) void mskip_len_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ masks, uint32_t nmasks, uint32_t ncand,
                                                           const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, uint32_t* __restrict__ clen) {
    for (uint64_t c64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c64 < ncand; c64 += (uint64_t)gridDim.x * kBlock) {
        const uint32_t c = (uint32_t)c64;
        const uint32_t p = src[c / nmasks];
        MskipCount     sink;
        mskip_masked(kbytes + koff[p], (uint32_t)(koff[p + 1] - koff[p]), masks[c % nmasks], sink);
        clen[c] = sink.n;
    }
}
__global__ __launch_bounds__(kBlock) void mskip_write_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ masks, uint32_t nmasks, uint32_t ncand,
                                                             const uint8_t* __restrict__ kbytes, const unsigned long long* __restrict__ koff, const unsigned long long* __restrict__ moff,
                                                             uint8_t* __restrict__ mbytes) {
    for (uint64_t c64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c64 < ncand; c64 += (uint64_t)gridDim.x * kBlock) {
        const uint32_t c = (uint32_t)c64;
        const uint32_t p = src[c / nmasks];
        MskipStore     sink{mbytes + moff[c]};
        mskip_masked(kbytes + koff[p], (uint32_t)(koff[p + 1] - koff[p]), masks[c % nmasks], sink);
        sink.finish();
    }
}
__global__ __launch_bounds__(kBlock) void mskip_clear_kernel(MSlot* __restrict__ table, uint32_t cap) {
    for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * kBlock) table[s] = MSlot{kEmptyKey, 0xFFFFFFFFu, 0u, 0ull};
}
// hmask: ~0, or the low bits COLIBRI_MSKIP_HASH_BITS keeps (a masked hash is never kEmptyKey)
__global__ __launch_bounds__(kBlock) void mskip_insert_kernel(const uint8_t* __restrict__ mbytes, const unsigned long long* __restrict__ moff, const uint32_t* __restrict__ clen,
                                                              const uint32_t* __restrict__ src, uint32_t nmasks, uint32_t ncand, const unsigned long long* __restrict__ roff, uint64_t seed,
                                                              uint64_t hmask, MSlot* __restrict__ table, uint32_t cap, uint32_t* __restrict__ slot_of) {
    for (uint64_t c64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c64 < ncand; c64 += (uint64_t)gridDim.x * kBlock) {
        const uint32_t c = (uint32_t)c64;
        const uint64_t h = text_hash(mbytes + moff[c], clen[c], seed) & hmask;
        uint32_t       s = slot_of_hash(mix64(h), cap);
        for (;;) {
            const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(&table[s].hash), (unsigned long long)kEmptyKey, (unsigned long long)h);
            if (old == kEmptyKey || old == h) break;
            s = (s + 1 == cap) ? 0 : s + 1;
        }
        const uint32_t p = src[c / nmasks];
        atomicMin(&table[s].rep, c);
        atomicAdd(&table[s].acc, (1ull << 32) | (unsigned long long)(roff[p + 1] - roff[p]));
        slot_of[c] = s;
    }
}
__global__ __launch_bounds__(kBlock) void mskip_verify_kernel(const uint8_t* __restrict__ mbytes, const unsigned long long* __restrict__ moff, const uint32_t* __restrict__ clen,
                                                              uint32_t ncand, const MSlot* __restrict__ table, const uint32_t* __restrict__ slot_of, uint32_t* __restrict__ isrep,
                                                              MskipInfo* __restrict__ info) {
    for (uint64_t c64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c64 < ncand; c64 += (uint64_t)gridDim.x * kBlock) {
        const uint32_t c = (uint32_t)c64;
        const uint32_t r   = table[slot_of[c]].rep;
        const uint32_t len = clen[c];
        if (r != c) {
            bool           same = clen[r] == len;
            const uint8_t *a = mbytes + moff[c], *b = mbytes + moff[r];
            uint32_t       k = 0;
            for (; same && k + 8 <= len; k += 8) same = ld64u(a + k) == ld64u(b + k);
            if (same && k < len) same = keep_bytes(ld64u(a + k), len - k) == keep_bytes(ld64u(b + k), len - k);  // (the bytes end in 16 bytes of slack)
            if (!same) info->collision = 1;
        }
        isrep[c] = r == c ? 1u : 0u;
    }
}
// group g = the rank of its representative among the representatives. kcnt / klen: the references and key bytes it keeps (0: erased)
__global__ __launch_bounds__(kBlock) void mskip_groups_kernel(const uint32_t* __restrict__ isrep, const unsigned long long* __restrict__ rank, const uint32_t* __restrict__ clen,
                                                              const MSlot* __restrict__ table, const uint32_t* __restrict__ slot_of, uint32_t ncand, uint32_t t, uint32_t mintypes,
                                                              uint32_t* __restrict__ gcnt, uint32_t* __restrict__ gtypes, uint32_t* __restrict__ grep, uint32_t* __restrict__ gkeep,
                                                              uint32_t* __restrict__ kcnt, uint32_t* __restrict__ klen, MskipInfo* __restrict__ info) {
    uint32_t low = 0, few = 0, kept = 0;
    for (uint64_t b0 = (uint64_t)blockIdx.x * kBlock; b0 < ncand; b0 += (uint64_t)gridDim.x * kBlock) {  // (b0 is the block's: every lane takes every ballot)
        const uint32_t c  = (uint32_t)(b0 + threadIdx.x);
        const bool     on = b0 + threadIdx.x < ncand && isrep[c] != 0;
        bool           is_low = false, is_few = false;
        if (on) {
            const uint32_t           g   = (uint32_t)rank[c];
            const unsigned long long acc = table[slot_of[c]].acc;
            const uint32_t           cnt = (uint32_t)acc, types = (uint32_t)(acc >> 32);
            is_low                       = cnt < t;
            is_few                       = !is_low && mintypes > 1 && types < mintypes;
            const bool keep              = !is_low && !is_few;
            gcnt[g]                      = cnt;
            gtypes[g]                    = types;
            grep[g]                      = c;
            gkeep[g]                     = keep ? 1u : 0u;
            kcnt[g]                      = keep ? cnt : 0u;
            klen[g]                      = keep ? clen[c] : 0u;
        }
        low += (uint32_t)__popcll(__ballot(is_low));
        few += (uint32_t)__popcll(__ballot(is_few));
        kept += (uint32_t)__popcll(__ballot(on && !is_low && !is_few));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {  // (the sums are wave-uniform)
        if (low) atomicAdd(&info->pruned_groups, low);
        if (few) atomicAdd(&info->extra, few);
        if (kept) atomicAdd(&info->kept, kept);
    }
}
// the n-grams of n tokens with fewer than t references go: out of `live` (what the next order's slices are looked up in) and out of `keep`
__global__ __launch_bounds__(kBlock) void mskip_prune_kernel(const uint8_t* __restrict__ ntok, uint32_t np, uint32_t n, const unsigned long long* __restrict__ roff, uint32_t t,
                                                             uint8_t* __restrict__ live, uint8_t* __restrict__ keep, MskipInfo* __restrict__ info) {
    uint32_t gone = 0;
    for (uint32_t b0 = blockIdx.x * kBlock; b0 < np; b0 += gridDim.x * kBlock) {
        const uint32_t p   = b0 + threadIdx.x;
        const bool     die = p < np && ntok[p] == n && live[p] != 0 && (roff[p + 1] - roff[p]) < (unsigned long long)t;
        if (die) live[p] = keep[p] = 0;
        gone += (uint32_t)__popcll(__ballot(die));
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && gone) atomicAdd(&info->pruned_ngrams, gone);
}
// references candidate c hands over: its source's, if its group is kept
__global__ __launch_bounds__(kBlock) void mskip_contrib_kernel(const uint32_t* __restrict__ src, uint32_t nmasks, uint32_t ncand, const unsigned long long* __restrict__ roff,
                                                               const MSlot* __restrict__ table, const uint32_t* __restrict__ slot_of, const unsigned long long* __restrict__ rank,
                                                               const uint32_t* __restrict__ gkeep, uint32_t* __restrict__ contrib) {
    for (uint64_t c64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c64 < ncand; c64 += (uint64_t)gridDim.x * kBlock) {
        const uint32_t c = (uint32_t)c64;
        const uint32_t p = src[c / nmasks];
        const uint32_t g = (uint32_t)rank[table[slot_of[c]].rep];
        contrib[c]       = gkeep[g] ? (uint32_t)(roff[p + 1] - roff[p]) : 0u;
    }
}
// kept reference j (soff = the scan of contrib, nk its total): its candidate by binary search, the input reference it copies (iref), its kept
// group's number (gref) and its token (the first sort key); the sorts carry j (an input reference may serve several groups)
__global__ __launch_bounds__(kBlock) void mskip_ref_list_kernel(const unsigned long long* __restrict__ soff, const uint32_t* __restrict__ contrib, uint32_t ncand, uint64_t nk,
                                                                const uint32_t* __restrict__ src, uint32_t nmasks, const unsigned long long* __restrict__ roff,
                                                                const MSlot* __restrict__ table, const uint32_t* __restrict__ slot_of, const unsigned long long* __restrict__ rank,
                                                                const unsigned long long* __restrict__ krank, const uint32_t* __restrict__ ref_sentence,
                                                                const uint16_t* __restrict__ ref_token, uint32_t* __restrict__ iref, uint32_t* __restrict__ gref, uint32_t* __restrict__ key,
                                                                uint32_t* __restrict__ val, MskipInfo* __restrict__ info) {
    uint32_t maxs = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nk; j += (uint64_t)gridDim.x * kBlock) {
        uint32_t lo = 0, hi = ncand;  // last candidate whose soff <= j (candidates that hand nothing over share an offset: take the one that owns j)
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (soff[mid] <= j)
                lo = mid;
            else
                hi = mid;
        }
        const uint32_t c = lo;
        const uint32_t p = src[c / nmasks];
        const uint32_t i = (uint32_t)(roff[p] + (j - soff[c]));
        iref[j]          = i;
        gref[j]          = (uint32_t)krank[(uint32_t)rank[table[slot_of[c]].rep]];
        key[j]           = ref_token[i];
        val[j]           = (uint32_t)j;
        maxs             = max(maxs, ref_sentence[i]);
    }
    for (int off = 32; off > 0; off >>= 1) maxs = max(maxs, (uint32_t)__shfl_down(maxs, off, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0 && maxs) atomicMax(&info->maxsentence, maxs);
}
// key[j] = field[index[val[j]]] (index == NULL: field[val[j]]): the next sort key of the entries where they stand
__global__ __launch_bounds__(kBlock) void mskip_gather_kernel(const uint32_t* __restrict__ field, const uint32_t* __restrict__ index, const uint32_t* __restrict__ val, uint64_t n,
                                                              uint32_t* __restrict__ key) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) key[j] = field[index ? index[val[j]] : val[j]];
}
__global__ __launch_bounds__(kBlock) void mskip_refs_out_kernel(const uint32_t* __restrict__ val, const uint32_t* __restrict__ iref, uint64_t n, const uint32_t* __restrict__ ref_sentence,
                                                                const uint16_t* __restrict__ ref_token, uint32_t* __restrict__ out_sentence, uint16_t* __restrict__ out_token) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
        const uint32_t i = iref[val[j]];
        out_sentence[j]  = ref_sentence[i];
        out_token[j]     = ref_token[i];
    }
}
// the kept groups' rows (kkoff / kroff: the scans of klen / kcnt over all groups): key (from the representative, word-wise; `out` ends in 16 bytes of slack but a key's last word is stored exactly), count, types
__global__ __launch_bounds__(kBlock) void mskip_keys_kernel(const uint8_t* __restrict__ mbytes, const unsigned long long* __restrict__ moff, const uint32_t* __restrict__ clen,
                                                            const uint32_t* __restrict__ grep, const uint32_t* __restrict__ gkeep, const uint32_t* __restrict__ gcnt,
                                                            const uint32_t* __restrict__ gtypes, const unsigned long long* __restrict__ krank, const unsigned long long* __restrict__ kkoff,
                                                            const unsigned long long* __restrict__ kroff, uint32_t ngroups, uint8_t* __restrict__ out,
                                                            unsigned long long* __restrict__ out_keyoff, unsigned long long* __restrict__ out_refoff, uint32_t* __restrict__ out_cnt,
                                                            uint32_t* __restrict__ out_types) {
    for (uint64_t g64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g64 < ngroups; g64 += (uint64_t)gridDim.x * kBlock) {
        const uint32_t g = (uint32_t)g64;
        if (!gkeep[g]) continue;
        const uint32_t c   = grep[g];
        const uint32_t len = clen[c];
        const uint8_t* a   = mbytes + moff[c];
        MskipStore     sink{out + kkoff[g]};
        uint32_t       k = 0;
        for (; k + 8 <= len; k += 8) {
            const uint64_t w = ld64u(a + k);
            __builtin_memcpy(sink.out, &w, 8);
            sink.out += 8;
        }
        sink.acc = keep_bytes(ld64u(a + k), len - k);
        sink.n   = len - k;
        sink.finish();
        const uint32_t r = (uint32_t)krank[g];
        out_keyoff[r]    = kkoff[g];
        out_refoff[r]    = kroff[g];
        out_cnt[r]       = gcnt[g];
        out_types[r]     = gtypes[g];
    }
}

}  // namespace colibri
