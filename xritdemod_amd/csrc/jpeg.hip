// jpeg.hip -- the JPEG stage's kernels (jpeg_rule.h has the rules per value, tests/jpeg_spec.py is the
// specification).  One call is
//   transform   8 MCUs per wave: colour conversion, edge replication, both DCT passes with the transpose in LDS, the
//               quantiser; int16 coefficients in zigzag order to scratch, block after block in scan order
//   lengths     one wave per block, lane k holds zigzag coefficient k: the block's code length in bits
//   scan        block lengths -> 64-bit bit offsets (P); per restart interval the bytes it fills -> byte offsets (U) in an
//               unstuffed stream in which every interval begins on a byte
//   zero, pack  one wave per block: its words to their bit positions through LDS, then one atomic OR per dword
//   scan        0xFF bytes per 16 bytes of the unstuffed stream -> their exclusive prefix
//   emit        header, stuffed bytes with RSTm between the intervals, EOI, the result record
// The sizes of the unstuffed stream are only known on the device: the kernels behind the first scan stride over them with
// grids that the host sizes from the bound.
#include "common.h"
#include "jpeg_rule.h"
#include "kernels.h"
#include "scan.h"
#include "wave_ops.h"

namespace xrit {

namespace {

__device__ const JpegCodeTables d_codes = jpeg_make_code_tables();

struct Unzig {
    uint8_t at[64];                 // natural index -> zigzag position
};
constexpr Unzig make_unzig()
{
    Unzig u{};
    for (int k = 0; k < 64; ++k) u.at[JPEG_ZIGZAG[k]] = (uint8_t)k;
    return u;
}
__device__ const Unzig d_unzig = make_unzig();

constexpr int WAVES = 4;            // per workgroup, everywhere below
constexpr int WS_ROW = 9, WS_BLOCK = 8 * WS_ROW + 1;

// the first block of interval k (k = n_int: the number of blocks)
__device__ __forceinline__ uint32_t interval_first(const JpegPar &p, uint32_t k)
{
    const unsigned long long m = (unsigned long long)k * p.ri;
    return (uint32_t)(m < p.mcus ? m : p.mcus) * p.comps;
}

// ---- transform --------------------------------------------------------------------------------------------------------
// Lane (b, r) of a wave loads row r of MCU m0 + b and makes its row pass; lane (b, c) then makes column c's pass.
__global__ void __launch_bounds__(64 * WAVES) jpeg_transform_kernel(JpegPar p, int16_t *__restrict__ coef)
{
    __shared__ int32_t s_ws[WAVES][8 * WS_BLOCK];
    __shared__ int16_t s_zz[WAVES][8 * 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = lane >> 3, r = lane & 7;
    const uint32_t m0 = (blockIdx.x * WAVES + w) * 8;
    const uint32_t m = m0 + b < p.mcus ? m0 + b : p.mcus - 1;             // a lane past the end repeats the last MCU, and stores nothing
    const uint32_t by = m / p.bw, bx = m - by * p.bw;
    const uint32_t y = by * 8 + r < p.rows ? by * 8 + r : p.rows - 1;
    const uint8_t *row = p.pix + (size_t)y * p.pitch;
    int32_t px[3][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t x = bx * 8 + i < p.columns ? bx * 8 + i : p.columns - 1;
        if (p.comps == 1) {
            px[0][i] = row[x];
            px[1][i] = px[2][i] = 0;
        } else {
            jpeg_colour(row[(size_t)x * 3], row[(size_t)x * 3 + 1], row[(size_t)x * 3 + 2], px[0][i], px[1][i], px[2][i]);
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        if (c >= p.comps) break;                        // uniform
        int32_t d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = px[c][i] - 128;
        jpeg_dct_pass(d, false);
#pragma unroll
        for (int i = 0; i < 8; ++i) s_ws[w][b * WS_BLOCK + r * WS_ROW + i] = d[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s_ws[w][b * WS_BLOCK + i * WS_ROW + r];          // column r
        jpeg_dct_pass(d, true);
#pragma unroll
        for (int i = 0; i < 8; ++i) s_zz[w][b * 64 + d_unzig.at[i * 8 + r]] = (int16_t)jpeg_quantise(d[i], p.q[c ? 1 : 0][i * 8 + r]);
        __syncthreads();
        for (uint32_t bb = 0; bb < 8; ++bb)
            if (m0 + bb < p.mcus) coef[((size_t)(m0 + bb) * p.comps + c) * 64 + lane] = s_zz[w][bb * 64 + lane];
        __syncthreads();
    }
}

// ---- a block's words --------------------------------------------------------------------------------------------------
// Lane k's word of block blk: lane 0 the DC difference, a lane with a non-zero AC coefficient the ZRL codes in front of
// it, its code and its magnitude bits (at most 3 * 11 + 16 + 10 = 59 bits), lane 63 the EOB when coefficient 63 is zero.
__device__ __forceinline__ void jpeg_block_words(const JpegPar &p, const int16_t *__restrict__ coef, uint32_t blk, uint32_t lane,
                                                 unsigned long long &word, uint32_t &len)
{
    const uint32_t m = blk / p.comps, c = blk - m * p.comps, tab = c ? 2 : 0;
    int32_t v = coef[(size_t)blk * 64 + lane];
    if (lane == 0 && m % p.ri != 0) v -= coef[(size_t)(blk - p.comps) * 64];
    const unsigned long long nz = __ballot(v != 0) & ~1ull;
    uint32_t bits;
    const uint32_t cat = jpeg_category(v, bits);
    word = 0;
    len = 0;
    if (lane == 0) {
        const uint32_t e = d_codes.t[tab].e[cat];
        word = (unsigned long long)(e >> 8) << cat | bits;
        len = (e & 255) + cat;
    } else if (v != 0) {
        const unsigned long long below = nz & ((1ull << lane) - 1);
        const uint32_t before = below ? 63 - (uint32_t)__clzll((long long)below) : 0, run = lane - before - 1;
        const uint32_t e = d_codes.t[tab + 1].e[(run & 15) << 4 | cat], z = d_codes.t[tab + 1].e[0xF0];
        for (uint32_t i = 0; i < run >> 4; ++i) {
            word = word << (z & 255) | (z >> 8);
            len += z & 255;
        }
        word = (word << (e & 255) | (e >> 8)) << cat | bits;
        len += (e & 255) + cat;
    } else if (lane == 63) {
        const uint32_t e = d_codes.t[tab + 1].e[0];
        word = e >> 8;
        len = e & 255;
    }
}

__global__ void __launch_bounds__(64 * WAVES) jpeg_lengths_kernel(JpegPar p, const int16_t *__restrict__ coef, uint32_t *__restrict__ blen)
{
    const uint32_t lane = threadIdx.x & 63, blk = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (blk >= p.blocks) return;
    unsigned long long word;
    uint32_t len;
    jpeg_block_words(p, coef, blk, lane, word, len);
    const uint32_t total = wave_sum(len);
    if (lane == 0) blen[blk] = total;
}

// ---- the scans (scan.h) -----------------------------------------------------------------------------------------------
// P[i], i = 0 .. blocks: the bits of the blocks in front of block i
struct BitsF {
    typedef unsigned long long T;
    const uint32_t *blen;
    unsigned long long *P;
    long long n;
    __device__ T identity() const { return 0; }
    __device__ T combine(const T &lo, const T &hi) const { return lo + hi; }
    __device__ T reduce_run(long long i0, int cnt) const
    {
        T v = 0;
        for (int k = 0; k < cnt; ++k)
            if (i0 + k < n) v += blen[i0 + k];
        return v;
    }
    __device__ void apply_run(long long i0, int cnt, const T &pre) const
    {
        T v = pre;
        for (int k = 0; k < cnt; ++k) {
            P[i0 + k] = v;
            if (i0 + k < n) v += blen[i0 + k];
        }
    }
};

// U[k], k = 0 .. n_int: the bytes of the intervals in front of interval k, each interval's bits rounded up to a byte
struct BytesF {
    typedef uint32_t T;
    JpegPar p;
    const unsigned long long *P;
    uint32_t *U;
    __device__ T value(long long k) const
    {
        if (k >= p.n_int) return 0;
        return (uint32_t)((P[interval_first(p, (uint32_t)k + 1)] - P[interval_first(p, (uint32_t)k)] + 7) >> 3);
    }
    __device__ T identity() const { return 0; }
    __device__ T combine(const T &lo, const T &hi) const { return lo + hi; }
    __device__ T reduce_run(long long i0, int cnt) const
    {
        T v = 0;
        for (int k = 0; k < cnt; ++k) v += value(i0 + k);
        return v;
    }
    __device__ void apply_run(long long i0, int cnt, const T &pre) const
    {
        T v = pre;
        for (int k = 0; k < cnt; ++k) {
            U[i0 + k] = v;
            v += value(i0 + k);
        }
    }
};

__device__ __forceinline__ uint32_t count_ff(uint32_t x)
{
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) n += ((x >> (8 * i)) & 255) == 255;
    return n;
}

// F[g], g = 0 .. ceil(T / 16): the 0xFF bytes in front of group g of 16 bytes of the unstuffed stream (T = U[n_int] bytes)
struct StuffF {
    typedef uint32_t T;
    const uint32_t *raw;
    const uint32_t *total;          // &U[n_int]
    uint32_t *F;
    __device__ T value(long long g) const
    {
        const uint32_t t = *total;
        if ((unsigned long long)g * 16 >= t) return 0;
        const uint4 q = reinterpret_cast<const uint4 *>(raw)[g];
        const uint32_t x[4] = {q.x, q.y, q.z, q.w};
        uint32_t n = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long at = g * 16 + i * 4;        // bytes behind the stream's end are zero (jpeg_zero_kernel)
            if (at < t) n += count_ff(x[i]);
        }
        return n;
    }
    __device__ T identity() const { return 0; }
    __device__ T combine(const T &lo, const T &hi) const { return lo + hi; }
    __device__ T reduce_run(long long i0, int cnt) const
    {
        T v = 0;
        for (int k = 0; k < cnt; ++k) v += value(i0 + k);
        return v;
    }
    __device__ void apply_run(long long i0, int cnt, const T &pre) const
    {
        const long long groups = ((long long)*total + 15) >> 4;
        T v = pre;
        for (int k = 0; k < cnt; ++k) {
            if (i0 + k <= groups) F[i0 + k] = v;
            v += value(i0 + k);
        }
    }
};

template <typename F> int run_scan(const F &f, long long n, typename F::T *aggs, hipStream_t s)
{
    const int nb = scan_blocks(n);
    hipLaunchKernelGGL(scan_reduce_kernel<F>, dim3(nb), dim3(SCAN_BLOCK), 0, s, f, n, aggs);
    XR_HIP(hipGetLastError());
    scan_aggs_launch(f, aggs, nb, s);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(scan_apply_kernel<F>, dim3(nb), dim3(SCAN_BLOCK), 0, s, f, n, aggs);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}
size_t scan_aggs_count(long long n)
{
    const size_t nb = scan_blocks(n);
    return nb + scan_blocks((long long)nb) + 2;
}

// ---- zero and pack ----------------------------------------------------------------------------------------------------
// the unstuffed stream's dwords, whole groups of 16 bytes
__global__ void __launch_bounds__(256) jpeg_zero_kernel(const uint32_t *__restrict__ total, uint4 *__restrict__ raw)
{
    const size_t groups = ((size_t)*total + 15) >> 4;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) raw[g] = make_uint4(0, 0, 0, 0);
}

// `len` bits (1 .. 59) of `word` at bit `at` of a buffer of big-endian dwords in LDS
__device__ __forceinline__ void put_bits(uint32_t *buf, uint32_t at, unsigned long long word, uint32_t len)
{
    const unsigned long long top = word << (64 - len);             // the word's first bit at bit 63
    const uint32_t d = at >> 5, o = at & 31;
    const unsigned long long a = top >> o;
    const uint32_t x0 = (uint32_t)(a >> 32), x1 = (uint32_t)a, x2 = o ? (uint32_t)((top << (64 - o)) >> 32) : 0;
    if (x0) atomicOr(&buf[d], x0);
    if (x1) atomicOr(&buf[d + 1], x1);
    if (x2) atomicOr(&buf[d + 2], x2);
}

constexpr int PACK_DWORDS = 64;     // (31 + 1660 + 7) / 32 + 3 = 56 are reached

__global__ void __launch_bounds__(64 * WAVES) jpeg_pack_kernel(JpegPar p, const int16_t *__restrict__ coef, const unsigned long long *__restrict__ P,
                                                               const uint32_t *__restrict__ U, uint32_t *__restrict__ raw)
{
    __shared__ uint32_t s_buf[WAVES][PACK_DWORDS];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, blk = blockIdx.x * WAVES + w;
    const bool valid = blk < p.blocks;
    s_buf[w][lane] = 0;
    __syncthreads();
    uint32_t n_dwords = 0;
    size_t base = 0;
    if (valid) {
        unsigned long long word;
        uint32_t len;
        jpeg_block_words(p, coef, blk, lane, word, len);
        const uint32_t incl = wave_incl_scan(len, (int)lane), total = wave_total(incl);
        const uint32_t k = blk / p.comps / p.ri, first = interval_first(p, k);
        const unsigned long long in_interval = P[blk] - P[first], at = 8ull * U[k] + in_interval;
        const uint32_t off = (uint32_t)(at & 31);
        base = (size_t)(at >> 5);
        if (len) put_bits(s_buf[w], off + incl - len, word, len);
        // the interval's last block fills the last byte with 1-bits
        uint32_t fill = 0;
        if (blk + 1 == interval_first(p, k + 1)) fill = (uint32_t)(-(long long)(in_interval + total)) & 7;
        if (lane == 0 && fill) put_bits(s_buf[w], off + total, (1u << fill) - 1, fill);
        n_dwords = (off + total + fill + 31) >> 5;
    }
    __syncthreads();
    if (lane < n_dwords) {
        const uint32_t v = s_buf[w][lane];
        if (v) atomicOr(&raw[base + lane], __builtin_bswap32(v));
    }
}

// ---- emit ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_byte(uint8_t *out, unsigned long long cap, unsigned long long at, uint32_t v)
{
    if (at < cap) out[at] = (uint8_t)v;
}

__global__ void __launch_bounds__(256) jpeg_emit_kernel(JpegPar p, JpegHeader h, const uint32_t *__restrict__ U, const uint32_t *__restrict__ raw,
                                                        const uint32_t *__restrict__ F, uint8_t *__restrict__ out, unsigned long long cap,
                                                        xrit_jpeg_result *__restrict__ result)
{
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t total = U[p.n_int];
    const size_t groups = ((size_t)total + 15) >> 4;
    if (tid < h.n) put_byte(out, cap, tid, h.b[tid]);
    if (tid == 0) {
        const unsigned long long size = (unsigned long long)h.n + total + F[groups] + 2ull * (p.n_int - 1) + 2;
        put_byte(out, cap, size - 2, 0xFF);
        put_byte(out, cap, size - 1, 0xD9);
        xrit_jpeg_result r;
        r.size = size;
        r.status = size > cap ? 1u : 0u;
        r.restarts = p.n_int - 1;
        *result = r;
    }
    for (size_t g = tid; g < groups; g += (size_t)gridDim.x * 256) {
        const uint32_t j0 = (uint32_t)(g * 16);
        // the interval of byte j0: the last k with U[k] <= j0
        uint32_t lo = 0, hi = p.n_int;
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (U[mid] <= j0) lo = mid;
            else hi = mid;
        }
        uint32_t k = lo, begin = U[k], next = U[k + 1], ff = F[g];
        const uint4 q = reinterpret_cast<const uint4 *>(raw)[g];
        for (uint32_t i = 0; i < 16; ++i) {
            const uint32_t j = j0 + i;
            if (j >= total) break;
            if (j >= next) {                            // an interval holds at least one byte: one step
                ++k;
                begin = next;
                next = U[k + 1];
            }
            const uint32_t x = i < 4 ? q.x : i < 8 ? q.y : i < 12 ? q.z : q.w, v = (x >> (8 * (i & 3))) & 255;
            const unsigned long long at = (unsigned long long)h.n + j + ff + 2ull * k;
            if (j == begin && k > 0) {
                put_byte(out, cap, at - 2, 0xFF);
                put_byte(out, cap, at - 1, 0xD0 + ((k - 1) & 7));
            }
            put_byte(out, cap, at, v);
            if (v == 255) {
                put_byte(out, cap, at + 1, 0);
                ++ff;
            }
        }
    }
}

}  // namespace

size_t jpeg_stream_bound(uint32_t blocks, uint32_t n_int) { return ((size_t)blocks * JPEG_BLOCK_BITS + 7) / 8 + n_int; }

size_t jpeg_scratch_carve(void *base, uint32_t blocks, uint32_t n_int, JpegScratch &sc)
{
    const size_t stream = jpeg_stream_bound(blocks, n_int), groups = (stream + 15) / 16;
    Carver c{static_cast<char *>(base)};
    sc.P = c.take<unsigned long long>((size_t)blocks + 1, 16);
    sc.P_aggs = c.take<unsigned long long>(scan_aggs_count((long long)blocks + 1), 16);
    sc.raw = c.take<uint32_t>(groups * 4 + 4, 16);
    sc.coef = c.take<int16_t>((size_t)blocks * 64, 16);
    sc.blen = c.take<uint32_t>(blocks, 16);
    sc.U = c.take<uint32_t>((size_t)n_int + 1, 16);
    sc.U_aggs = c.take<uint32_t>(scan_aggs_count((long long)n_int + 1), 16);
    sc.F = c.take<uint32_t>(groups + 1, 16);
    sc.F_aggs = c.take<uint32_t>(scan_aggs_count((long long)groups + 1), 16);
    return c.used();
}

int launch_jpeg(const JpegPar &p, const JpegHeader &h, const JpegScratch &sc, unsigned char *out, size_t cap, xrit_jpeg_result *result,
                hipStream_t s)
{
    const size_t groups = (jpeg_stream_bound(p.blocks, p.n_int) + 15) / 16;
    const unsigned g_stream = div_up(groups, 256);
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3(div_up(p.mcus, 8 * WAVES)), dim3(64 * WAVES), 0, s, p, sc.coef);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpeg_lengths_kernel, dim3(div_up(p.blocks, WAVES)), dim3(64 * WAVES), 0, s, p, sc.coef, sc.blen);
    XR_HIP(hipGetLastError());
    XR_TRY(run_scan(BitsF{sc.blen, sc.P, (long long)p.blocks}, (long long)p.blocks + 1, sc.P_aggs, s));
    XR_TRY(run_scan(BytesF{p, sc.P, sc.U}, (long long)p.n_int + 1, sc.U_aggs, s));
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(g_stream < 2048u ? g_stream : 2048u), dim3(256), 0, s, sc.U + p.n_int, reinterpret_cast<uint4 *>(sc.raw));
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(div_up(p.blocks, WAVES)), dim3(64 * WAVES), 0, s, p, sc.coef, sc.P, sc.U, sc.raw);
    XR_HIP(hipGetLastError());
    XR_TRY(run_scan(StuffF{sc.raw, sc.U + p.n_int, sc.F}, (long long)groups + 1, sc.F_aggs, s));
    const unsigned g_emit = g_stream < 4u ? 4u : g_stream < 4096u ? g_stream : 4096u;       // at least JPEG_MAX_HEADER threads
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3(g_emit), dim3(256), 0, s, p, h, sc.U, sc.raw, sc.F, out, (unsigned long long)cap, result);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
