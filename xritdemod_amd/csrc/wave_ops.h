// wave_ops.h -- the sums and prefix sums over the 64 lanes of a wave and over the waves of a workgroup that the back-end
// stages compact their output with (a count per item, its exclusive prefix inside a tile, the
// tile's sums, a prefix over the tiles).  Device only.  Every function is called by all 64 lanes of a wave.
// The order of the additions is part of the contract (acquire_finish_kernel's double sums keep their bits by it):
// wave_sum is the xor butterfly at offsets 32, 16, .. 1, in which both lanes of a pair add the same two numbers, so every
// lane ends with the same bits; wave_incl_scan steps up by 1, 2, .. 32.  (The wave maxima of viterbi.hip and
// framer_query.h stay written out where they stand: see there.)
#pragma once

#include <hip/hip_runtime.h>

namespace xrit {

template <typename T> __device__ __forceinline__ T wave_sum(T x)
{
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

template <typename T> __device__ __forceinline__ T wave_incl_scan(T x, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

// the wave's sum from the inclusive scan x: lane 63's value, in every lane
template <typename T> __device__ __forceinline__ T wave_total(T x) { return __shfl(x, 63, 64); }

// one step of a scan that a single wave carries over rows of 64 values: the exclusive prefix of v along the rows so far
// (carry: the sum of the rows in front, the same in every lane; the row's sum is added to it)
template <typename T> __device__ __forceinline__ T wave_excl_scan_step(T v, int lane, T &carry)
{
    const T x = wave_incl_scan(v, lane), before = carry + x - v;
    carry += wave_total(x);
    return before;
}

// The waves' parts of a workgroup of NW waves: part is wave w's own sum (lane 63's value is the one taken).  Returns the sum
// of the parts of the waves in front of w, and total: the sum of all NW parts.  All threads of the workgroup call it; it
// contains exactly one barrier, after lane 63's store to s_part[w].  s_part is the caller's __shared__ array of NW
// elements: a caller that uses it again (a loop, a second call on the same array) puts a barrier of its own in between.
template <unsigned NW, typename T> __device__ __forceinline__ T block_parts_before(T part, unsigned lane, unsigned w, T *s_part, T &total)
{
    if (lane == 63) s_part[w] = part;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma nounroll                // (unrolled, the NW parts in registers cost the tile kernels occupancy)
    for (unsigned i = 0; i < NW; ++i) {
        const T p = s_part[i];
        if (i < w) before += p;
        total += p;
    }
    return before;
}

// The workgroup inclusive scan for NW waves, thread order: the wave scan with the parts of the waves in front added, and
// total as above.  The contract is block_parts_before's (all threads, one barrier, the caller's s_part[NW]).  A caller
// that wants the exclusive value subtracts its own element.
template <unsigned NW, typename T> __device__ __forceinline__ T block_incl_scan(T x, unsigned lane, unsigned w, T *s_part, T &total)
{
    x = wave_incl_scan(x, (int)lane);
    return x + block_parts_before<NW>(x, lane, w, s_part, total);
}

}  // namespace xrit
