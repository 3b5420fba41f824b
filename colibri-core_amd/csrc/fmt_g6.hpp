// fmt_g6.hpp — what an ostream in its default float state (printf's "%.6g") writes for the double a / (double)b, without printf, log10 or any
// other float routine beside the one IEEE division: plain C++, __host__ __device__, shared by print.hpp and the host-side tests.
//
// The quotient d = a / (double)b is the correctly rounded double (a, b < 2^53 are exact doubles; the division of gfx950 is IEEE). "%.6g" rounds
// the exact binary value of d, m * 2^x, to six significant digits, half to even. With e the decimal exponent of d that is
//   q = floor(d * 10^(5 - e)), 10^5 <= q < 10^6, and the rest of d * 10^(5 - e) against one half:
//   e <= 5   d * 10^k = (m * 10^k) >> s with s = -x: a 128-bit product (m < 2^53, k <= 21 -> under 2^123) and a shift; the rest is the low s bits
//   e >  5   d < 2^54 has an integer part I that fits 64 bits and a fraction that only matters as "non-zero": q = I / 10^j, the rest I % 10^j
// Then the form: exponent form d.ddddde-XX below 10^-4 and from 10^6 (the exponent of the ROUNDED value), fixed otherwise; trailing zeros and a
// bare point dropped. b == 0 gives what the division gives: inf, or the default NaN of x86-64, which prints as -nan.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COLIBRI_FMT_HD __host__ __device__
#else
#define COLIBRI_FMT_HD
#endif

namespace colibri {

constexpr int kFmtG6Max = 12;  // the longest text: 1.23457e-16 (11 bytes); -nan / inf are shorter

COLIBRI_FMT_HD inline uint64_t fmt_pow10(int k) {  // 10^k, k <= 19
    uint64_t v = 1;
    for (int i = 0; i < k; ++i) v *= 10u;
    return v;
}

// q (six digits) and the decimal exponent e of the finite double d > 0, rounded as "%.6g" rounds
COLIBRI_FMT_HD inline void fmt_g6_digits(double d, uint32_t* q_out, int* e_out) {
    union {
        double   f;
        uint64_t u;
    } v;
    v.f              = d;
    const int      x = (int)((v.u >> 52) & 0x7FFu) - 1075;          // d = m * 2^x (normal numbers only: d >= 2^-53)
    const uint64_t m = (v.u & 0xFFFFFFFFFFFFFull) | (1ull << 52);
    int            e = ((x + 52) * 1233) >> 12;                      // floor((x + 52) * log10(2)) within one; settled below
    uint64_t       q = 0;
    int            dir = 0;  // the rest against one half: -1 below, 0 a tie, +1 above
    for (int tries = 0; tries < 4; ++tries) {
        const int k = 5 - e;
        if (k >= 0) {
            const int         s   = -x;  // (e <= 5: d < 10^6 < 2^52, so x < 0; d >= 2^-53: s <= 105)
            unsigned __int128 num = (unsigned __int128)m * fmt_pow10(k > 10 ? 10 : k);
            if (k > 10) num *= fmt_pow10(k - 10);
            const unsigned __int128 hi = num >> s;
            if (hi >= 1000000u) {
                ++e;
                continue;
            }
            if (hi < 100000u) {
                --e;
                continue;
            }
            q                            = (uint64_t)hi;
            const unsigned __int128 rest = num - (hi << s), half = (unsigned __int128)1 << (s - 1);
            dir                          = rest < half ? -1 : rest == half ? 0 : 1;
        } else {
            const uint64_t I    = x >= 0 ? m << x : m >> -x;  // (d < 2^54)
            const bool     frac = x < 0 && (m & ((1ull << -x) - 1u)) != 0;
            const uint64_t p    = fmt_pow10(-k);
            const uint64_t hi   = I / p, rest = I % p;
            if (hi >= 1000000u) {
                ++e;
                continue;
            }
            if (hi < 100000u) {
                --e;
                continue;
            }
            q   = hi;
            dir = 2 * rest > p ? 1 : 2 * rest < p ? -1 : (frac ? 1 : 0);  // (p is even: below one half stays below with any fraction)
        }
        break;
    }
    if (dir > 0 || (dir == 0 && (q & 1u))) ++q;
    if (q == 1000000u) {
        q = 100000u;
        ++e;
    }
    *q_out = (uint32_t)q;
    *e_out = e;
}

// the text of a / (double)b into out (at most kFmtG6Max bytes, no terminator); returns its length
COLIBRI_FMT_HD inline int fmt_g6(uint64_t a, uint64_t b, char* out) {
    int n = 0;
    if (b == 0) {
        const char* s = a ? "inf" : "-nan";
        while (*s) out[n++] = *s++;
        return n;
    }
    if (a == 0) {
        out[0] = '0';
        return 1;
    }
    uint32_t q;
    int      e;
    fmt_g6_digits((double)a / (double)b, &q, &e);
    char dg[6];
    for (int i = 5; i >= 0; --i) {
        dg[i] = (char)('0' + q % 10u);
        q /= 10u;
    }
    int nd = 6;  // significant digits without the trailing zeros
    while (nd > 1 && dg[nd - 1] == '0') --nd;
    if (e < -4 || e >= 6) {
        out[n++] = dg[0];
        if (nd > 1) {
            out[n++] = '.';
            for (int i = 1; i < nd; ++i) out[n++] = dg[i];
        }
        out[n++]       = 'e';
        out[n++]       = e < 0 ? '-' : '+';
        const int ae   = e < 0 ? -e : e;
        if (ae >= 100) out[n++] = (char)('0' + ae / 100);
        out[n++] = (char)('0' + (ae / 10) % 10);
        out[n++] = (char)('0' + ae % 10);
        return n;
    }
    if (e < 0) {
        out[n++] = '0';
        out[n++] = '.';
        for (int i = 0; i < -e - 1; ++i) out[n++] = '0';
        for (int i = 0; i < nd; ++i) out[n++] = dg[i];
        return n;
    }
    for (int i = 0; i <= e; ++i) out[n++] = dg[i];  // (zeros inside the integer part stay)
    if (nd > e + 1) {
        out[n++] = '.';
        for (int i = e + 1; i < nd; ++i) out[n++] = dg[i];
    }
    return n;
}

}  // namespace colibri
