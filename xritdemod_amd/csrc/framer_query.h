// framer_query.h -- one chunk's correlation as a range query over the hard bits and the per-64 maxima that
// framer_bits_kernel leaves (framer.hip), shared by the stream frame synchroniser's walkers and joints and by the frame
// lock's (lock.hip), which also asks for the first frame / 16 positions alone.  Device code.
#pragma once

#include "kernels.h"
#include "sync_core.h"

namespace xrit {

struct FrHit { unsigned word, pos, corr; };

// One chunk's correlation, by a whole wave: positions c .. c + span - 65 of V, every lane returns the answer.
// Keys order (count desc, position asc) per word; the first word with the strictly greatest count wins (sync.hip).
__device__ __forceinline__ FrHit fr_query_span(const FramerPar &par, const unsigned *__restrict__ bits,
                                               const unsigned *__restrict__ bmax, unsigned c, unsigned span, unsigned lane)
{
    const unsigned first = c, last = c + span - 65u;
    const unsigned bf = first >> 6, bl = last >> 6;
    unsigned k0 = 0, k1 = 0;
    auto point = [&](unsigned p) {
        const unsigned j = p >> 5, r = p & 31u;
        unsigned hi, lo;
        sync_window(bits[j], bits[j + 1], bits[j + 2], r, hi, lo);
        const unsigned rel = 0xFFFFFu - (p - c);
        k0 = max(k0, (sync_agree(hi, lo, par.whi[0], par.wlo[0]) << 20) | rel);
        k1 = max(k1, (sync_agree(hi, lo, par.whi[1], par.wlo[1]) << 20) | rel);
    };
    const unsigned ph = (bf << 6) + lane;
    if (ph >= first && ph <= last) point(ph);
    if (bl != bf) {
        const unsigned pt = (bl << 6) + lane;
        if (pt <= last) point(pt);
        for (unsigned b = bf + 1 + lane; b < bl; b += 64) {
            const unsigned u = bmax[b], u0 = u & 0xFFFFu, u1 = u >> 16;
            const unsigned base = (b << 6) - c;
            k0 = max(k0, ((u0 >> 6) << 20) | (0xFFFFFu - (base + 63u - (u0 & 63u))));
            k1 = max(k1, ((u1 >> 6) << 20) | (0xFFFFFu - (base + 63u - (u1 & 63u))));
        }
    }
    // (the two words' maxima stay in one written-out butterfly: as a wave maximum each, one behind the other, the frame
    // lock's 134 rounds over a damaged stream measured 473.8 ms against 472.9 ms)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        k0 = max(k0, (unsigned)__shfl_xor((int)k0, off, 64));
        k1 = max(k1, (unsigned)__shfl_xor((int)k1, off, 64));
    }
    // every word starts at correlation 0 / position 0 and is replaced on '>': no agreeing bit at all reports position 0
    FrHit h{0, 0, 0};
    const unsigned c0 = k0 >> 20, c1 = k1 >> 20;
    if (c0 > 0) { h.corr = c0; h.pos = 0xFFFFFu - (k0 & 0xFFFFFu); h.word = 0; }
    if (c1 > h.corr) { h.corr = c1; h.pos = 0xFFFFFu - (k1 & 0xFFFFFu); h.word = 1; }
    return h;
}

// the whole chunk: positions c .. c + frame - 65
__device__ inline FrHit fr_query(const FramerPar &par, const unsigned *__restrict__ bits, const unsigned *__restrict__ bmax, unsigned c,
                                 unsigned lane)
{
    return fr_query_span(par, bits, bmax, c, par.frame, lane);
}

}  // namespace xrit
