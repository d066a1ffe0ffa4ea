// vtx_f64_text.h — Rust's `{}` text of an f64 by ONE LANE: the per-value logic of mtx_len_kernel<true> / mtx_text_kernel<true>
// (vtx_ingest.hip), the values of `vartrix -s alt_frac` (sprs::io::write_matrix_market, src/main.rs:381-389, values from :1131-1145).
//
// The text: the SHORTEST digit string inside the rounding interval of v (the reals that round to v; its ends belong to it when the
// mantissa is even), the closest to v among those of that length (an exact tie goes to the even digit), positional, no exponent, no
// trailing ".0" — 0.3333333333333333, 0.000033333333333333335, NaN.  What Ryu, Grisu + Dragon and std::to_chars(fixed) produce; the
// yardstick is vtxh_format_f64 (host/vtx_host.cpp), tests/test_f64_text.py compares byte for byte.
//
// Domain (everything alt_frac can produce — a / (r + a + k) of three u32 counters is NaN, 0 or in [1 / (3 * 2^32), 1] — with room):
//   NaN -> "NaN" (any payload, either sign);  +-0 -> "0" / "-0";  finite v with 2^MIN_EXP2 <= |v| < 2^53, either sign.
// Outside (infinities, subnormals, |v| >= 2^53, |v| < 2^MIN_EXP2): f64_len returns 0 and the caller declines (VTX_E_UNSUPPORTED).
// MIN_EXP2 = -40: no text of the domain is longer than MAX_LEN = 31 bytes, what vtxh_format_f64 keeps.  A value in [10^-12, 2^-39) is
// "-0." + 11 zeros + at most 17 digits; one in [2^-40, 10^-12) has 12 zeros but its neighbours are 2^-92 = 2.02e-28 apart, more than
// the 10^-28 between numbers of 16 digits there, so 16 digits always suffice.  (From 2^-42 down 32-byte texts exist.)
//
// Method: exact digit generation in fixed point (Steele & White's free-format algorithm), no tables, no division.
//   * Every integer below 2^53 is a double, and no double other than v lies in v's rounding interval: the integer part of the text
//     is floor(|v|), printed as it is, and a text with a fraction never rounds into the integer.
//   * The fraction f, the half-gaps to the neighbours below and above (M-, M+; M- is a quarter of the gap above when v is a power
//     of two) are multiples of 2^-94 in the domain: three 128-bit words with the binary point at bit FP.  Per digit: all three
//     times ten, the digit is what crossed the point; stop as soon as the digits so far (remainder <= M-) or the digits so far plus
//     one unit of the last place (remainder + M+ >= 1) are inside the interval.  The first such length is the shortest.
//   At most 28 trips (11 zeros + 17 digits, 12 + 16); a lane spends a few hundred integer instructions per value, three orders of magnitude
//   below what the text's bytes cost to store and to copy.
// Digits go straight to the output pointer, nothing is indexed in private memory: no scratch.
//
// Compiles for the host too (tests/f64text/: CPU suite, no GPU needed).
#ifndef VTX_F64_TEXT_H
#define VTX_F64_TEXT_H

#include <stdint.h>

#ifdef __HIPCC__
#define VTXT_FN __device__ __forceinline__
#else
#define VTXT_FN static inline
#endif

namespace vtxt {

typedef unsigned __int128 u128;

constexpr int MIN_EXP2 = -40;          // lower edge of the domain: 2^MIN_EXP2 <= |v|
constexpr int MAX_EXP2 = 52;           // upper edge: |v| < 2^(MAX_EXP2 + 1)
constexpr uint32_t MAX_LEN = 31;       // longest text of the domain ("-0." + 11 zeros + 17 digits, "-0." + 12 zeros + 16 digits)
constexpr int FP = 96;                 // binary point of the fixed-point words (>= 52 - MIN_EXP2 + 2 fractional bits, <= 124)
static_assert(FP >= 52 - MIN_EXP2 + 2 && FP <= 124, "fixed point: room for a quarter ulp below and for * 10 above");

VTXT_FN uint32_t ndigits64(uint64_t v) {          // v < 2^53
    uint32_t n = 1;
    if (v >= 100000000ull) { v /= 100000000ull; n += 8; }      // (constant divisors: multiply-high, no library call)
    const uint32_t w = (uint32_t)v;                            // < 10^8 (2^53 < 10^16)
    return n + (w < 10u ? 0u : w < 100u ? 1u : w < 1000u ? 2u : w < 10000u ? 3u : w < 100000u ? 4u : w < 1000000u ? 5u : w < 10000000u ? 6u : 7u);
}

// the text of v at p (PUT) or only its length: number of bytes, 0 = outside the domain (nothing written)
template <bool PUT>
VTXT_FN uint32_t f64_core(uint8_t* p, double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    const uint32_t neg = (uint32_t)(b >> 63);
    const uint32_t be = (uint32_t)(b >> 52) & 0x7ffu;
    const uint64_t mant = b & ((1ull << 52) - 1);
    if (be == 0x7ffu) {
        if (!mant) return 0;                                   // +-inf
        if (PUT) { p[0] = 'N'; p[1] = 'a'; p[2] = 'N'; }
        return 3;
    }
    if (be == 0) {
        if (mant) return 0;                                    // subnormal
        if (PUT) { if (neg) p[0] = '-'; p[neg] = '0'; }
        return 1 + neg;
    }
    const int e2 = (int)be - 1023;                             // floor(log2 |v|)
    if (e2 < MIN_EXP2 || e2 > MAX_EXP2) return 0;
    const uint64_t m = mant | (1ull << 52);                    // |v| = m * 2^-fb
    const uint32_t fb = (uint32_t)(52 - e2);                   // 0 .. 52 - MIN_EXP2
    uint32_t n = neg;
    if (PUT && neg) p[0] = '-';
    {
        uint64_t ip = fb >= 53 ? 0ull : m >> fb;
        const uint32_t nd = ndigits64(ip);
        if (PUT) for (uint32_t i = nd; i-- > 0;) { p[n + i] = (uint8_t)('0' + (uint32_t)(ip % 10u)); ip /= 10u; }
        n += nd;
    }
    const uint64_t fm = fb >= 53 ? m : m & ((1ull << fb) - 1);
    if (!fm) return n;                                         // an integer
    if (PUT) p[n] = '.';
    ++n;
    const u128 one = (u128)1 << FP;
    u128 r = (u128)fm << (FP - fb);                            // the fraction, < 1
    u128 mhi = (u128)1 << (FP - 1 - fb);                       // half the gap to the double above
    u128 mlo = mant ? mhi : mhi >> 1;                          // ... below: the doubles under a power of two are twice as dense
    const bool even = !(m & 1);                                // round-to-nearest-even: the interval's ends round to v
    for (;;) {
        r *= 10u; mlo *= 10u; mhi *= 10u;
        uint32_t d = (uint32_t)(r >> FP);
        r &= one - 1;
        const bool low = even ? r <= mlo : r < mlo;            // the digits so far are inside the interval
        const bool high = even ? r + mhi >= one : r + mhi > one;   // the digits so far + 1 in the last place are
        if (low || high) {
            // (d + 1 <= 9: a carry would mean that a shorter text was inside the interval one trip earlier)
            if (high && (!low || 2 * r > one || (2 * r == one && (d & 1u)))) ++d;
            if (PUT) p[n] = (uint8_t)('0' + d);
            return n + 1;
        }
        if (PUT) p[n] = (uint8_t)('0' + d);
        ++n;
    }
}

// number of bytes of Rust's `{}` text of v; 0 = outside the domain
VTXT_FN uint32_t f64_len(double v) { return f64_core<false>(nullptr, v); }
// writes exactly f64_len(v) bytes, returns the end
VTXT_FN uint8_t* f64_put(uint8_t* p, double v) { return p + f64_core<true>(p, v); }

}  // namespace vtxt

#endif
