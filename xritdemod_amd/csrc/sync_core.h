// sync_core.h -- what the correlator (sync.hip) and the stream frame synchroniser (framer.hip) share on the device: the
// hard decision of four soft bytes at a time and the agreement of a 64-bit window with a sync word.
#pragma once

namespace xrit {

// hard bits of four soft bytes (lowest address first -> most significant bit of the nibble)
__device__ __forceinline__ unsigned sync_nibble(unsigned x)
{
    // unsigned byte >= 127  <=>  bit 7 set, or the low seven bits are all ones
    const unsigned ge = (x | ((x & 0x7f7f7f7fu) + 0x01010101u)) & 0x80808080u;
    const unsigned one = (~ge & 0x80808080u) >> 7;        // 1 at bit 0 / 8 / 16 / 24
    return ((one * 0x08040201u) >> 24) & 0xFu;            // byte 0 -> bit 3 ... byte 3 -> bit 0, no carries
}

// The window of 64 hard bits at bit offset r (0..31) of three consecutive MSB-first words a, b, c.
__device__ __forceinline__ void sync_window(unsigned a, unsigned b, unsigned c, unsigned r, unsigned &hi, unsigned &lo)
{
    hi = __funnelshift_l(b, a, r);                        // r = 0: a, b
    lo = __funnelshift_l(c, b, r);
}

// agreeing bits of the window with the word (whi:wlo)
__device__ __forceinline__ unsigned sync_agree(unsigned hi, unsigned lo, unsigned whi, unsigned wlo)
{
    return 64u - (unsigned)__popc(hi ^ whi) - (unsigned)__popc(lo ^ wlo);
}

}  // namespace xrit
