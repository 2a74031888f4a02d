// framer.hip -- the stream view of the stream frame synchroniser and the frame lock (include/xritdemod_amd.h, "Stream
// frame synchroniser").  A call sees V = carry ++ new symbols; V[0] is the cursor.  Of a call's
// launches the first and the last are here; the chain between them (walkers, joints) is lock.hip's.
//
//  (a) framer_bits_kernel: the hard bits of V (sync_core.h) and, for every run of 64 positions and each word on its
//      own, the best agreement count and the first offset that reaches it.
//  (d) framer_gather_kernel: the rows' frames with inversion, dword-wide across the carry / new-symbols seam, the zero
//      rows, the small per-row outputs and the next call's carry.
#include "kernels.h"
#include "sync_core.h"

namespace xrit {

namespace {

constexpr unsigned FR_THREADS = 256;
constexpr unsigned FR_TILE_WORDS = FR_THREADS;          // bit words per workgroup of (a): 8192 positions

struct FrView {
    const int8_t *carry;      // 4-byte aligned, the handle's own buffer
    const int8_t *fresh;      // the call's symbols, any alignment
    unsigned L, T;            // bytes of carry, bytes of V
};

__device__ __forceinline__ unsigned fr_byte(const FrView &v, unsigned p)
{
    if (p < v.L) return (unsigned char)v.carry[p];
    if (p < v.T) return (unsigned char)v.fresh[p - v.L];
    return 0u;
}

// V[p .. p + 4), lowest address in the low byte; zeros past the end.  Only aligned dwords that hold at least one byte
// of the buffer they belong to are loaded.
__device__ __forceinline__ unsigned fr_dword(const FrView &v, unsigned p)
{
    if (p + 4 <= v.L) {
        const unsigned *q = reinterpret_cast<const unsigned *>(v.carry) + (p >> 2);
        const unsigned sh = p & 3u, lo = q[0];
        return sh ? __funnelshift_r(lo, q[1], sh * 8u) : lo;
    }
    if (p >= v.L && p + 4 <= v.T) {
        const size_t a = reinterpret_cast<size_t>(v.fresh) + (p - v.L);
        const unsigned *q = reinterpret_cast<const unsigned *>(a & ~(size_t)3);
        const unsigned sh = (unsigned)(a & 3), lo = q[0];
        return sh ? __funnelshift_r(lo, q[1], sh * 8u) : lo;
    }
    return fr_byte(v, p) | (fr_byte(v, p + 1) << 8) | (fr_byte(v, p + 2) << 16) | (fr_byte(v, p + 3) << 24);
}

// hard bits of V[32 j .. 32 j + 32), MSB = first byte
__device__ __forceinline__ unsigned fr_bits_word(const FrView &v, unsigned j)
{
    const unsigned p0 = j * 32u;
    if (p0 >= v.T) return 0u;
    unsigned w = 0;
#pragma unroll
    for (unsigned k = 0; k < 8; ++k) w = (w << 4) | sync_nibble(fr_dword(v, p0 + 4u * k));
    return w;
}

// (a) one bit word per thread; then the thread's 32 positions one after another, two threads to a run of 64
__global__ void __launch_bounds__(FR_THREADS) framer_bits_kernel(FramerPar par, const FramerState *__restrict__ state,
                                                                 const int8_t *__restrict__ carry, const int8_t *__restrict__ fresh,
                                                                 unsigned *__restrict__ bits, unsigned *__restrict__ bmax)
{
    __shared__ unsigned w[FR_TILE_WORDS + 2];
    const unsigned tid = threadIdx.x, j = blockIdx.x * FR_TILE_WORDS + tid;
    FrView v{carry, fresh, state->carry, state->carry + par.n};
    const unsigned mine = fr_bits_word(v, j);
    w[tid] = mine;
    if (tid < 2) w[FR_TILE_WORDS + tid] = fr_bits_word(v, blockIdx.x * FR_TILE_WORDS + FR_TILE_WORDS + tid);
    bits[j] = mine;
    __syncthreads();
    const unsigned a = w[tid], b = w[tid + 1], c = w[tid + 2];
    unsigned k0 = 0, k1 = 0;
    const unsigned off0 = 63u - 32u * (tid & 1u);
#pragma unroll 8
    for (unsigned r = 0; r < 32; ++r) {
        unsigned hi, lo;
        sync_window(a, b, c, r, hi, lo);
        k0 = max(k0, (sync_agree(hi, lo, par.whi[0], par.wlo[0]) << 6) | (off0 - r));
        k1 = max(k1, (sync_agree(hi, lo, par.whi[1], par.wlo[1]) << 6) | (off0 - r));
    }
    unsigned u = k0 | (k1 << 16);
    const unsigned o = (unsigned)__shfl_xor((int)u, 1, 64);
    if (!(tid & 1u)) bmax[j >> 1] = max(u & 0xFFFFu, o & 0xFFFFu) | (max(u >> 16, o >> 16) << 16);
}

// (d) blockIdx.x: the row (par.cap: the next call's carry); blockIdx.y: a share of its bytes
__global__ void __launch_bounds__(FR_THREADS) framer_gather_kernel(FramerPar par, const FramerCall *__restrict__ call,
                                                                   const int8_t *__restrict__ carry, const int8_t *__restrict__ fresh,
                                                                   const uint4 *__restrict__ rows, int8_t *__restrict__ carry_out,
                                                                   int8_t *__restrict__ frames, unsigned char *__restrict__ valid,
                                                                   xrit_sync_hit *__restrict__ hits, unsigned long long *__restrict__ start)
{
    const FramerCall cr = *call;
    const FrView v{carry, fresh, cr.carry, cr.total};
    const unsigned r = blockIdx.x;
    const unsigned i0 = (blockIdx.y * FR_THREADS + threadIdx.x) * 4u, step = gridDim.y * FR_THREADS * 4u;
    if (r == par.cap) {
        unsigned left = cr.total - cr.cursor;
        if (left > 2u * par.frame) left = 2u * par.frame;
        unsigned *dst = reinterpret_cast<unsigned *>(carry_out);
        for (unsigned i = i0; i < left; i += step) dst[i >> 2] = fr_dword(v, cr.cursor + i);
        return;
    }
    const bool have = r < cr.count;
    const uint4 row = have ? rows[r] : make_uint4(0, 0, 0, 0);
    const bool good = have && row.w >= par.min_corr;
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        valid[r] = good ? 1 : 0;
        xrit_sync_hit h;
        h.word = row.y;
        h.position = row.z;
        h.correlation = row.w;
        h.reserved = 0;
        hits[r] = h;
        start[r] = have ? cr.base + row.x + (good ? row.z : 0u) : 0ull;
    }
    const unsigned src0 = row.x + row.z;
    const unsigned inv = (good && row.y != 0 && par.invert) ? 0xFFFFFFFFu : 0u;
    int8_t *dst = frames + (size_t)r * par.frame;
    const bool words_ok = (reinterpret_cast<size_t>(dst) & 3) == 0;
    for (unsigned i = i0; i < par.frame; i += step) {
        if (words_ok && i + 4 <= par.frame) {
            *reinterpret_cast<unsigned *>(dst + i) = good ? (fr_dword(v, src0 + i) ^ inv) : 0u;
        } else {
            for (unsigned k = 0; k < 4 && i + k < par.frame; ++k)
                dst[i + k] = good ? (int8_t)(fr_byte(v, src0 + i + k) ^ (inv & 0xFFu)) : (int8_t)0;
        }
    }
}

unsigned bit_tiles(size_t n, unsigned frame)
{
    // the last word a query reads is two behind the one that holds its last position
    const size_t words = framer_host::span_max(n, frame) / 32 + 3;
    return (unsigned)((words + FR_TILE_WORDS - 1) / FR_TILE_WORDS);
}

}  // namespace

size_t framer_scratch_carve(void *p, size_t n, unsigned frame, unsigned seg_chunks, FramerScratch &sc)
{
    const size_t tiles = bit_tiles(n, frame), segs = framer_host::segments(n, frame, seg_chunks);
    const size_t cap = framer_host::rows_cap(n, frame);
    Carver c{static_cast<char *>(p)};
    sc.bits = c.take<unsigned>(tiles * FR_TILE_WORDS + 4, 16);
    sc.bmax = c.take<unsigned>(tiles * (FR_TILE_WORDS / 2), 16);
    sc.rec = c.take<uint4>(segs * seg_chunks, 16);
    sc.nrec = c.take<unsigned>(segs, 16);
    sc.wout = c.take<uint2>(segs, 16);
    sc.rows = c.take<uint4>(cap + 1, 16);
    sc.flags = c.take<unsigned char>(cap + 1, 16);
    sc.call = c.take<FramerCall>(1, 16);
    return c.used();
}

int launch_framer_bits(const FramerPar &par, const FramerState *state, const int8_t *carry_in, const int8_t *symbols,
                       FramerScratch &sc, hipStream_t s)
{
    const unsigned tiles = bit_tiles(par.n, par.frame);
    hipLaunchKernelGGL(framer_bits_kernel, dim3(tiles), dim3(FR_THREADS), 0, s, par, state, carry_in, symbols, sc.bits, sc.bmax);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_framer_gather(const FramerPar &par, const FramerCall *call, const int8_t *carry_in, const int8_t *symbols,
                         const uint4 *rows, int8_t *carry_out, int8_t *frames, unsigned char *valid, xrit_sync_hit *hits,
                         unsigned long long *start, hipStream_t s)
{
    const unsigned per = (par.frame / 4 + FR_THREADS - 1) / FR_THREADS;
    hipLaunchKernelGGL(framer_gather_kernel, dim3(par.cap + 1, per > 16 ? 16 : (per ? per : 1)), dim3(FR_THREADS), 0, s, par, call,
                       carry_in, symbols, rows, carry_out, frames, valid, hits, start);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
