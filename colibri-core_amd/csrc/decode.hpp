// decode.hpp — corpus decoding (colibri-classdecode; reference src/classdecoder.cpp:166-238): class ids back to text, on the tokenised corpus.
//
// Specification: a 00 ends a line and prints "\n"; every other token prints its word (the empty string for an id without one),
// preceded by one space unless it is the first item of its line. Line L (from 1) is printed iff (start == 0 && end == 0) || L >= start ||
// L <= end, so the hidden lines are one run, end < L < start; a hidden line prints neither its tokens nor its newline. v1 files only: the
// markers {*} / {**} (v1 bytes 128 / 129) are printed in hidden lines too, with a space before them when an earlier marker of the same
// line was printed.
//
// Layout. The host converts v1 data to varints (colibri_decode_upload), writing the markers as tokens no encoder writes — 80 80 80 80 80 80 00
// ({*}) and 80 80 80 80 80 80 80 00 ({**}) — so that a genuine class 3 / 4 token keeps its own word. The tokeniser of the trainer
// (tokenise(): tokstart, delimpos, cls per position) then holds everything a position needs. Three passes over the positions:
//   decode_classify_kernel  highest id, tokens no v2 encoder writes (refused)
//   decode_len_kernel       output bytes of each position -> a 64-bit exclusive scan (scan_reduce / scan_sums / scan_apply of kernels.hpp)
//   decode_write_kernel     per output window [W0, W1): every position writes the part of its text that falls in the window, one lane per
//                           position (the writes of a wave are adjacent in the output; what they cost beside the device-to-host copy: §5d)
#pragma once
#include "kernels.hpp"

namespace colibri {

constexpr uint32_t kDecodeMaxIds  = 1u << 26;  // the word table holds ids 0 .. 2^26 - 1 at most (256 MiB of offsets)
constexpr uint32_t kDecodeBadLong = 1u;        // (v2) a token of more than 5 bytes: its id is beyond 32 bits
constexpr uint32_t kDecodeBadZero = 2u;        // (v2) a multi-byte token whose id is 0: the reference would end the line there
constexpr uint32_t kDecodeSkipLen = 7u;        // (v1) token lengths of the converted markers
constexpr uint32_t kDecodeFlexLen = 8u;
constexpr uint64_t kDecodeWindowBytes = 64ull << 20;  // output window: two of them are staged on the device and two in pinned host memory

struct DecodeInfo {
    uint32_t maxclass;  // highest id of a word token (markers and delimiters excluded)
    uint32_t bad;       // kDecodeBad*
};

__device__ __forceinline__ bool dec_is_delim(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ tokstart, uint32_t i) {
    const uint32_t a = tokstart[i];
    return tokstart[i + 1] - a == 1u && bytes[a] == 0;
}

__global__ __launch_bounds__(kBlock) void decode_classify_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ tokstart, const uint32_t* __restrict__ cls,
                                                                  uint32_t npos, int v1, DecodeInfo* __restrict__ info) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t       c = 0, bad = 0;
    if (i < npos) {
        const uint32_t len = tokstart[i + 1] - tokstart[i];
        if (len == 1 && bytes[tokstart[i]] == 0) {
            // delimiter
        } else if (v1 && len >= kDecodeSkipLen) {
            // marker
        } else if (len > 5) {
            bad = kDecodeBadLong;
        } else {
            c = cls[i];
            if (c == 0 && !v1) bad = kDecodeBadZero;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        bad |= __shfl_down(bad, off, kWave);
        c = max(c, __shfl_down(c, off, kWave));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (bad) atomicOr(&info->bad, bad);
        if (c > __hip_atomic_load(&info->maxclass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&info->maxclass, c);
    }
}

// output bytes of position i; positions [h0, h1) are the hidden lines' (their delimiters included)
__global__ __launch_bounds__(kBlock) void decode_len_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ tokstart, const uint32_t* __restrict__ cls,
                                                             uint32_t npos, int v1, const uint32_t* __restrict__ wordoff, uint32_t nids, uint32_t h0, uint32_t h1,
                                                             uint32_t* __restrict__ len_out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= npos) return;
    const uint32_t a = tokstart[i], len = tokstart[i + 1] - a;
    const bool     hidden = i >= h0 && i < h1;
    uint32_t       out    = 0;
    if (len == 1 && bytes[a] == 0) {
        out = hidden ? 0u : 1u;
    } else {
        const bool first = i == 0 || dec_is_delim(bytes, tokstart, i - 1);
        if (v1 && len >= kDecodeSkipLen) {
            uint32_t sep = first ? 0u : 1u;
            if (hidden) {  // only markers print in a hidden line: was one printed before this one in the line? (each walks back to the previous one)
                sep = 0;
                for (uint32_t j = i; j-- > 0;) {
                    const uint32_t lj = tokstart[j + 1] - tokstart[j];
                    if (lj == 1 && bytes[tokstart[j]] == 0) break;
                    if (lj >= kDecodeSkipLen) {
                        sep = 1;
                        break;
                    }
                }
            }
            out = sep + (len == kDecodeSkipLen ? 3u : 4u);
        } else if (!hidden) {
            const uint32_t c = cls[i];
            out              = (first ? 0u : 1u) + (c < nids ? wordoff[c + 1] - wordoff[c] : 0u);
        }
    }
    len_out[i] = out;
}

// range[0] = the first position whose text ends after W0, range[1] = the first position whose text starts at or after W1 (one thread each)
__global__ void decode_range_kernel(const unsigned long long* __restrict__ off, uint32_t npos, unsigned long long W0, unsigned long long W1, uint32_t* __restrict__ range) {
    const int t = threadIdx.x;
    if (t > 1) return;
    uint32_t lo = 0, hi = npos;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t == 0 ? off[mid + 1] > W0 : off[mid] >= W1) hi = mid;
        else lo = mid + 1;
    }
    range[t] = lo;
}

// the window's text: out[q - W0] for q in [W0, W1)
__global__ __launch_bounds__(kBlock) void decode_write_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ tokstart, const uint32_t* __restrict__ cls,
                                                               const unsigned long long* __restrict__ off, int v1, const uint32_t* __restrict__ wordoff,
                                                               const uint8_t* __restrict__ words, const uint32_t* __restrict__ range, unsigned long long W0,
                                                               unsigned long long W1, uint8_t* __restrict__ out) {
    const uint32_t p0 = range[0], p1 = range[1];
    for (uint32_t i = p0 + blockIdx.x * kBlock + threadIdx.x; i < p1; i += gridDim.x * kBlock) {
        const unsigned long long o = off[i], n = off[i + 1] - o;
        const unsigned long long lo = o > W0 ? o : W0, hi = o + n < W1 ? o + n : W1;
        if (lo >= hi) continue;
        const uint32_t a = tokstart[i], len = tokstart[i + 1] - a;
        if (len == 1 && bytes[a] == 0) {  // (printed: n == 1)
            out[lo - W0] = '\n';
            continue;
        }
        const uint8_t* src;
        uint32_t       sep;
        if (v1 && len >= kDecodeSkipLen) {
            src = reinterpret_cast<const uint8_t*>(len == kDecodeSkipLen ? "{*}" : "{**}");
            sep = (uint32_t)n - (len == kDecodeSkipLen ? 3u : 4u);
        } else {
            sep = (i == 0 || dec_is_delim(bytes, tokstart, i - 1)) ? 0u : 1u;
            src = words + ((uint32_t)n > sep ? wordoff[cls[i]] : 0u);  // a token with a word: cls[i] < nids
        }
        uint8_t* dst = out + (lo - W0);
        for (unsigned long long q = lo; q < hi; ++q) {
            const uint32_t k = (uint32_t)(q - o);
            *dst++           = k < sep ? (uint8_t)' ' : src[k - sep];
        }
    }
}

}  // namespace colibri
