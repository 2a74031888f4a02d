// rs_core.h -- CCSDS RS(255,223) arithmetic shared by the device decoder (rs.hip) and host code: GF(2^8) with
// p(x) = x^8 + x^7 + x^2 + x + 1, generator roots alpha^(11 (112 + i)), i = 0 .. 31, Berlekamp's dual basis on the
// wire, the CCSDS pseudo-random sequence.  The tables are built at compile time.
#pragma once

#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace xrit {

constexpr int RS_NN = 255, RS_NROOTS = 32, RS_FCR = 112, RS_PRIM = 11, RS_T = 16;

struct RsTables {
    uint8_t exp[512];      // alpha^i, i = 0 .. 509 (two periods: exp[log a + log b] needs no modulo)
    uint8_t log[256];      // log[0] unused
    uint8_t to_dual[256];  // conventional -> Berlekamp dual basis
    uint8_t to_conv[256];  // dual -> conventional
    uint8_t pn[256];       // one period (255 bytes) of the PN sequence, h(x) = x^8 + x^7 + x^5 + x^3 + 1, all ones
};

constexpr RsTables rs_make_tables()
{
    RsTables t{};
    unsigned x = 1;
    for (int i = 0; i < 255; ++i) {
        t.exp[i] = (uint8_t)x;
        t.exp[i + 255] = (uint8_t)x;
        t.log[x] = (uint8_t)i;
        x <<= 1;
        if (x & 0x100) x ^= 0x187;
    }
    const uint8_t tal[8] = {0x8d, 0xef, 0xec, 0x86, 0xfa, 0x99, 0xaf, 0x7b};
    for (int i = 0; i < 256; ++i) {
        unsigned v = 0;
        for (int k = 0; k < 8; ++k)
            if ((i >> k) & 1) v ^= tal[7 - k];
        t.to_dual[i] = (uint8_t)v;
    }
    for (int i = 0; i < 256; ++i) t.to_conv[t.to_dual[i]] = (uint8_t)i;
    // a[n + 8] = a[n + 7] ^ a[n + 5] ^ a[n + 3] ^ a[n], a[0 .. 7] = 1, MSB first
    unsigned sr = 0xFF;                      // a[n .. n + 7], a[n] in bit 7
    for (int byte = 0; byte < 255; ++byte) {
        unsigned b = 0;
        for (int k = 0; k < 8; ++k) {
            const unsigned a0 = (sr >> 7) & 1;
            b = (b << 1) | a0;
            const unsigned nxt = ((sr >> 0) ^ (sr >> 2) ^ (sr >> 4) ^ (sr >> 7)) & 1;   // a[n+7], a[n+5], a[n+3], a[n]
            sr = ((sr << 1) | nxt) & 0xFF;
        }
        t.pn[byte] = (uint8_t)b;
    }
    return t;
}

__host__ __device__ inline unsigned rs_mul(unsigned a, unsigned b, const uint8_t *ex, const uint8_t *lg)
{
    return (a && b) ? ex[lg[a] + lg[b]] : 0u;
}

// Errors-only decoding of one codeword from its 32 syndromes (S[i] = c(alpha^(11 (112 + i))), conventional basis):
// Berlekamp-Massey, Chien search, Forney.  Returns the number of errors (1 .. 16) with their byte indices (0 = the
// highest-degree symbol, the first on the wire) and conventional-basis magnitudes, or -1 when the locator's degree is
// not its number of roots or a magnitude is zero.  The caller takes the all-zero syndrome case (0 errors) itself.
__host__ __device__ inline int rs_solve(const uint8_t *S, const uint8_t *ex, const uint8_t *lg, int *where, uint8_t *mag)
{
    uint8_t lam[RS_NROOTS + 1], B[RS_NROOTS + 1], tmp[RS_NROOTS + 1];
    for (int i = 0; i <= RS_NROOTS; ++i) lam[i] = B[i] = 0;
    lam[0] = B[0] = 1;
    int L = 0, m = 1;
    unsigned b = 1;
    for (int r = 0; r < RS_NROOTS; ++r) {
        unsigned d = S[r];
        for (int i = 1; i <= L; ++i) d ^= rs_mul(lam[i], S[r - i], ex, lg);
        if (d == 0) { ++m; continue; }
        const unsigned coef = ex[lg[d] + 255 - lg[b]];          // d / b
        if (2 * L <= r) {
            for (int i = 0; i <= RS_NROOTS; ++i) tmp[i] = lam[i];
            for (int i = m; i <= RS_NROOTS; ++i) lam[i] ^= (uint8_t)rs_mul(coef, B[i - m], ex, lg);
            L = r + 1 - L;
            for (int i = 0; i <= RS_NROOTS; ++i) B[i] = tmp[i];
            b = d;
            m = 1;
        } else {
            for (int i = m; i <= RS_NROOTS; ++i) lam[i] ^= (uint8_t)rs_mul(coef, B[i - m], ex, lg);
            ++m;
        }
    }
    int deg = 0;
    for (int i = 1; i <= RS_NROOTS; ++i)
        if (lam[i]) deg = i;
    if (deg == 0 || deg > RS_T) return -1;
    // Chien search: symbol of degree k is in error when lambda(beta^-k) = 0, beta = alpha^11
    int n = 0;
    uint8_t xinv[RS_T];
    for (int k = 0; k < RS_NN; ++k) {
        const unsigned lx = (unsigned)((RS_NN - (RS_PRIM * k) % RS_NN) % RS_NN);   // log of beta^-k
        unsigned v = lam[0];
        for (int i = 1; i <= deg; ++i)
            if (lam[i]) v ^= ex[(lg[lam[i]] + lx * i) % RS_NN];
        if (v == 0) {
            if (n == RS_T) return -1;
            where[n] = k;
            xinv[n] = ex[lx];
            ++n;
        }
    }
    if (n != deg) return -1;
    // Forney: Y = X^(1 - FCR) omega(X^-1) / lambda'(X^-1), omega = S lambda mod x^32
    uint8_t om[RS_NROOTS];
    for (int i = 0; i < RS_NROOTS; ++i) {
        unsigned v = 0;
        for (int j = 0; j <= deg && j <= i; ++j) v ^= rs_mul(S[i - j], lam[j], ex, lg);
        om[i] = (uint8_t)v;
    }
    for (int e = 0; e < n; ++e) {
        const unsigned lxi = lg[xinv[e]];
        unsigned num = 0, den = 0, pw = 0;                       // pw = log of xinv^i
        for (int i = 0; i < RS_NROOTS; ++i, pw = (pw + lxi) % RS_NN) {
            if (om[i]) num ^= ex[(lg[om[i]] + pw) % RS_NN];
            if ((i & 1) && i <= deg && lam[i]) den ^= ex[(lg[lam[i]] + pw + RS_NN - lxi) % RS_NN];   // lambda_i x^(i-1)
        }
        if (num == 0 || den == 0) return -1;
        // X^(1 - FCR) = beta^(k (1 - FCR))
        const unsigned lX = (unsigned)((RS_PRIM * where[e]) % RS_NN);
        const unsigned lfac = (unsigned)((lX * (unsigned)(RS_NN - (RS_FCR - 1) % RS_NN)) % RS_NN);
        mag[e] = (uint8_t)ex[(lg[num] + RS_NN - lg[den] + lfac) % RS_NN];
        where[e] = RS_NN - 1 - where[e];                          // degree k -> byte index
    }
    return n;
}

}  // namespace xrit
