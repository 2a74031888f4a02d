// framer.hip -- stream frame synchroniser (include/xritdemod_amd.h, "Stream frame synchroniser"):
// the reference decoder's walk over a stream of soft symbols, chunk by chunk (decoder/src/newdecoder.cpp:212-270 with
// flywheelRecheck = 1), as four launches per call.  The call sees V = carry ++ new symbols; V[0] is the cursor.
//
//  (a) framer_bits_kernel: the hard bits of V (sync_core.h) and, for every run of 64 positions and each word on its
//      own, the best agreement count and the first offset that reaches it.
//  (b) framer_walk_kernel: V is cut into segments of S chunks; one wave per segment walks the recurrence
//      c -> c + F | c + pos + F from the segment's nominal start and records its steps.  A step is one range query over
//      positions c .. c + F - 65: the two partial runs at its ends from the bits, the whole runs between from (a),
//      reduced across the lanes.
//  (c) framer_joints_kernel: one wave follows the true chain from cursor 0.  Where its cursor is a cursor the segment's
//      walker recorded, the rest of that record is the chain (the walk is a function of the cursor alone); elsewhere it
//      takes real steps until it meets the record or leaves the segment.  It writes the rows, the count, the call record
//      and the handle's state.
//  (d) framer_gather_kernel: the rows' frames with inversion, dword-wide across the carry / new-symbols seam, the zero
//      rows, the small per-row outputs and the next call's carry.
#include "kernels.h"
#include "framer_query.h"
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

// (b) one wave per segment
__global__ void __launch_bounds__(64) framer_walk_kernel(FramerPar par, const FramerState *__restrict__ state,
                                                         const unsigned *__restrict__ bits, const unsigned *__restrict__ bmax,
                                                         uint4 *__restrict__ rec, unsigned *__restrict__ nrec, uint2 *__restrict__ wout)
{
    const unsigned k = blockIdx.x, lane = threadIdx.x;
    const unsigned long long T = (unsigned long long)state->carry + par.n;
    const unsigned long long seg1 = (unsigned long long)(k + 1) * par.seg_bytes;
    unsigned long long x = (unsigned long long)k * par.seg_bytes;
    unsigned i = 0, stop = 0;
    uint4 *mine = rec + (size_t)k * par.seg_chunks;
    while (x < seg1 && i < par.seg_chunks) {
        if (x + par.frame > T) { stop = 1; break; }
        const FrHit h = fr_query(par, bits, bmax, (unsigned)x, lane);
        const bool good = h.corr >= par.min_corr;
        if (good && x + h.pos + par.frame > T) { stop = 1; break; }
        if (lane == 0) mine[i] = make_uint4((unsigned)x, h.word, h.pos, h.corr);
        ++i;
        x += good ? (unsigned long long)h.pos + par.frame : par.frame;
    }
    if (lane == 0) {
        nrec[k] = i;
        wout[k] = make_uint2((unsigned)x, stop);
    }
}

__device__ __forceinline__ unsigned long long fr_wave_sum(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off, 64);
    return v;
}

// (c) one wave: the true chain through the walkers' records
__global__ void __launch_bounds__(64) framer_joints_kernel(FramerPar par, FramerState *__restrict__ state,
                                                           const unsigned *__restrict__ bits, const unsigned *__restrict__ bmax,
                                                           const uint4 *__restrict__ rec, const unsigned *__restrict__ nrec,
                                                           const uint2 *__restrict__ wout, uint4 *__restrict__ rows,
                                                           FramerCall *__restrict__ call, unsigned *__restrict__ d_count)
{
    const unsigned lane = threadIdx.x;
    const unsigned L = state->carry;
    const unsigned long long T = (unsigned long long)L + par.n;
    unsigned long long x = 0;
    unsigned count = 0, rewalked = 0, adopted = 0;
    unsigned frames = 0, dropped = 0, resyncs = 0;          // per lane, summed at the end
    while (x + par.frame <= T && count < par.cap) {
        const unsigned k = (unsigned)(x / par.seg_bytes);
        if (k >= par.segs) break;
        const uint4 *theirs = rec + (size_t)k * par.seg_chunks;
        const unsigned nr = nrec[k];
        int found = -1;
        for (unsigned base = 0; base < nr && found < 0; base += 64) {
            const unsigned idx = base + lane;
            const unsigned long long m = __ballot(idx < nr && theirs[idx].x == (unsigned)x);
            if (m) found = (int)(base + (unsigned)__ffsll((long long)m) - 1u);
        }
        if (found >= 0) {
            const unsigned have = nr - (unsigned)found, room = par.cap - count, m = have < room ? have : room;
            for (unsigned base = 0; base < m; base += 64) {
                const unsigned idx = base + lane;
                if (idx < m) {
                    const uint4 r = theirs[(unsigned)found + idx];
                    rows[count + idx] = r;
                    const bool good = r.w >= par.min_corr;
                    frames += good ? 1u : 0u;
                    dropped += good ? 0u : 1u;
                    resyncs += (good && r.z != 0) ? 1u : 0u;
                }
            }
            count += m;
            adopted += m;
            if (m < have) { x = theirs[(unsigned)found + m].x; break; }     // (the row bound makes this unreachable)
            const uint2 o = wout[k];
            x = o.x;
            if (o.y) break;
            continue;
        }
        const FrHit h = fr_query(par, bits, bmax, (unsigned)x, lane);
        ++rewalked;
        const bool good = h.corr >= par.min_corr;
        if (good && x + h.pos + par.frame > T) break;
        if (lane == 0) {
            rows[count] = make_uint4((unsigned)x, h.word, h.pos, h.corr);
            frames += good ? 1u : 0u;
            dropped += good ? 0u : 1u;
            resyncs += (good && h.pos != 0) ? 1u : 0u;
        }
        ++count;
        x += good ? (unsigned long long)h.pos + par.frame : par.frame;
    }
    const unsigned long long f = fr_wave_sum(frames), d = fr_wave_sum(dropped), rs = fr_wave_sum(resyncs);
    if (lane == 0) {
        unsigned long long left = T - x;                                   // at most 2 * frame - 66
        if (left > 2ull * par.frame) left = 2ull * par.frame;
        FramerCall cr;
        cr.base = state->cursor;
        cr.carry = L;
        cr.total = (unsigned)T;
        cr.cursor = (unsigned)x;
        cr.count = count;
        *call = cr;
        *d_count = count;
        state->symbols += par.n;
        state->cursor += x;
        state->rows += count;
        state->frames += f;
        state->dropped += d;
        state->resyncs += rs;
        state->rewalked += rewalked;
        state->adopted += adopted;
        state->calls += 1;
        state->carry = (unsigned)left;
    }
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

unsigned framer_segments(size_t n, unsigned frame, unsigned seg_chunks)
{
    const size_t seg = (size_t)seg_chunks * frame;
    return (unsigned)((framer_host::span_max(n, frame) + seg - 1) / seg);
}

size_t framer_scratch_carve(void *p, size_t n, unsigned frame, unsigned seg_chunks, FramerScratch &sc)
{
    const size_t tiles = bit_tiles(n, frame), segs = framer_segments(n, frame, seg_chunks);
    const size_t cap = framer_host::rows_cap(n, frame);
    Carver c{static_cast<char *>(p)};
    sc.bits = c.take<unsigned>(tiles * FR_TILE_WORDS + 4, 16);
    sc.bmax = c.take<unsigned>(tiles * (FR_TILE_WORDS / 2), 16);
    sc.rec = c.take<uint4>(segs * seg_chunks, 16);
    sc.nrec = c.take<unsigned>(segs, 16);
    sc.wout = c.take<uint2>(segs, 16);
    sc.rows = c.take<uint4>(cap + 1, 16);
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

int launch_framer(const FramerPar &par, FramerState *state, const int8_t *carry_in, int8_t *carry_out, const int8_t *symbols,
                  FramerScratch &sc, int8_t *frames, unsigned char *valid, xrit_sync_hit *hits, unsigned long long *start,
                  unsigned *count, hipStream_t s)
{
    XR_TRY(launch_framer_bits(par, state, carry_in, symbols, sc, s));
    hipLaunchKernelGGL(framer_walk_kernel, dim3(par.segs), dim3(64), 0, s, par, state, sc.bits, sc.bmax, sc.rec, sc.nrec, sc.wout);
    hipLaunchKernelGGL(framer_joints_kernel, dim3(1), dim3(64), 0, s, par, state, sc.bits, sc.bmax, sc.rec, sc.nrec, sc.wout, sc.rows,
                       sc.call, count);
    XR_HIP(hipGetLastError());
    return launch_framer_gather(par, sc.call, carry_in, symbols, sc.rows, carry_out, frames, valid, hits, start, s);
}

}  // namespace xrit
