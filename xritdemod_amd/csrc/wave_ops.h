// wave_ops.h -- sums over the 64 lanes of a wave, as the demux and the packet assembler use them.  Device only.
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

}  // namespace xrit
