// product_rule.h -- the product stage's rule (include/xritdemod_amd.h, "Image products"; tests/product_spec.py states the
// same) as plain integer functions for the device (product.hip) and the host (product_host_check.cpp replays a table
// recorded from the specification through them): the clamp of a sample, the percentile test, the choice between the
// tone asked for and the fallback, the tone table's entry and the thumbnail's byte.
#pragma once

#include <cstdint>

#include "../../include/xritdemod_amd.h"

#if defined(__HIPCC__)
#define XRIT_HD __host__ __device__
#else
#define XRIT_HD
#endif

namespace xrit {

// what the scan of the bins found, and what the table is made from
struct ProductTone {
    uint32_t tone;                  // the tone in effect: XRIT_TONE_LINEAR where the one asked for fell back
    uint32_t fallback;
    uint32_t bits;
    uint32_t min_nz, max_nz;        // 0 if no v >= 1 has a count
    uint32_t lo, hi;                // STRETCH in effect; else 0
    uint64_t n;                     // N = c[2^bits - 1]
    uint64_t cmin;                  // c[min_nz]
};

XRIT_HD inline uint32_t product_width(uint32_t bits) { return bits <= 8 ? 1u : 2u; }
XRIT_HD inline uint32_t product_max(uint32_t bits) { return (1u << bits) - 1u; }
// the stage's one out-of-bounds hazard: the bin and the table's entry of a sample above 2^bits - 1 are the last
XRIT_HD inline uint32_t product_clamp(uint32_t v, uint32_t maxv) { return v > maxv ? maxv : v; }

XRIT_HD inline uint32_t product_linear(uint32_t bits, uint32_t v) { return bits >= 8 ? v >> (bits - 8) : v << (8 - bits); }

// 10000 * c >= p * N (c, N <= 2^31, p <= 10000: 64 bits hold both sides)
XRIT_HD inline bool product_reaches(uint64_t c, uint32_t p, uint64_t n) { return 10000ull * c >= (uint64_t)p * n; }
// v (with c = c[v]) is a candidate for lo; the smallest one is lo
XRIT_HD inline bool product_is_lo(uint64_t c, uint32_t p_lo, uint64_t n) { return c > 0 && product_reaches(c, p_lo, n); }

// the tone in effect, from the tone asked for and what the scan found (lo, hi: STRETCH's, as found; 0 otherwise)
XRIT_HD inline ProductTone product_decide(uint32_t tone, uint32_t bits, uint64_t n, uint32_t min_nz, uint32_t max_nz, uint64_t cmin, uint32_t lo,
                                          uint32_t hi)
{
    ProductTone t{tone, 0, bits, min_nz, max_nz, 0, 0, n, cmin};
    if (tone == XRIT_TONE_EQUALISE && n - cmin == 0) t.fallback = 1;
    if (tone == XRIT_TONE_STRETCH) {
        if (n == 0 || hi <= lo) t.fallback = 1;
        else { t.lo = lo; t.hi = hi; }
    }
    if (t.fallback) t.tone = XRIT_TONE_LINEAR;
    return t;
}

// lut[v] for v <= 2^bits - 1, c = c[v]; table: TABLE's entry for v (not read otherwise)
XRIT_HD inline uint8_t product_lut_entry(const ProductTone &t, uint32_t v, uint64_t c, uint8_t table)
{
    switch (t.tone) {
    case XRIT_TONE_TABLE:
        return table;
    case XRIT_TONE_EQUALISE: {
        if (v == 0) return 0;
        if (v < t.min_nz) return 1;
        const uint64_t d = t.n - t.cmin;
        return (uint8_t)(1u + (254ull * (c - t.cmin) + d / 2) / d);
    }
    case XRIT_TONE_STRETCH: {
        if (v == 0) return 0;
        if (v <= t.lo) return 1;
        if (v >= t.hi) return 255;
        const uint32_t d = t.hi - t.lo;
        return (uint8_t)(1u + (254u * (v - t.lo) + d / 2) / d);
    }
    default:
        return (uint8_t)product_linear(t.bits, v);
    }
}

// a thumbnail's byte from its block: cnt pixels with data (<= 4096), the sum of their table entries (<= 4096 * 255)
XRIT_HD inline uint8_t product_small_byte(uint32_t sum, uint32_t cnt) { return cnt ? (uint8_t)((2u * sum + cnt) / (2u * cnt)) : (uint8_t)0; }

XRIT_HD inline uint32_t product_small_dim(uint32_t n, uint32_t f) { return f ? (n + f - 1) / f : 0u; }

}  // namespace xrit
