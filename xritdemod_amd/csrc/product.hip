// product.hip -- the kernels of the product stage (include/xritdemod_amd.h, "Image products"):
//   (a) product_hist_kernel       the histogram: a wave per row, the grid striding over the rows; up to 12 bits the bins are
//                                 the workgroup's in LDS (a copy per wave where they fit), flushed with one global atomic
//                                 per non-empty bin; above, global atomics on the table
//   (b) product_lut_kernel        one workgroup: the bins scanned, min_nz / max_nz / lo / hi found, the tone table and the
//                                 summary written; the entry is product_rule.h's
//   (c) product_tone_kernel       the toned image and the thumbnail from one read of the source: a workgroup per band of
//                                 `factor` rows and tile of columns, a wave per row, the blocks' sums in LDS
//   (d) product_composite_kernel  the false-colour lookup: four pixels a lane, twelve bytes stored as three dwords
// Rows are walked by walk_row: sixteen bytes per lane between a row segment's first and last 16-byte boundary, single
// samples in front and behind; nothing outside the segment is read.
#include "common.h"
#include "kernels.h"
#include "product_rule.h"
#include "wave_ops.h"

namespace xrit {
namespace {

constexpr unsigned WAVES = 4;
constexpr unsigned THREADS = 64 * WAVES;
constexpr unsigned LDS_BITS = 12;                   // up to here the bins and the tone table are held in LDS
constexpr unsigned LDS_BINS = 1u << LDS_BITS;
constexpr unsigned CELLS = 256;                     // thumbnail bytes per row of a tone tile
constexpr unsigned PLAIN_TILE = 4096;               // columns of a tone tile without a thumbnail

// The samples p[0 .. n) of W bytes each, by the 64 lanes of a wave: f(i, v) with v an array of the 16 / W samples from i
// on for every whole 16-byte unit between the first and the last 16-byte boundary, and of one sample for those in front
// and behind (at most 15 bytes each: one lane per sample, one trip).  For W = 2, p is even.
template <unsigned W, class F> __device__ __forceinline__ void walk_row(const unsigned char *p, uint32_t n, unsigned lane, F &&f)
{
    constexpr unsigned K = 16 / W;
    const uint32_t in_front = (uint32_t)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / W;
    const uint32_t head = in_front < n ? in_front : n;
    const uint32_t units = (n - head) / K;
    const uint32_t tail0 = head + units * K, tail = n - tail0;
    if (lane < head + tail) {
        const uint32_t i = lane < head ? lane : tail0 + (lane - head);
        uint32_t v[1];
        if (W == 1) v[0] = p[i];
        else v[0] = reinterpret_cast<const uint16_t *>(p)[i];
        f(i, v);
    }
    const uint4 *body = reinterpret_cast<const uint4 *>(p + (size_t)head * W);
    for (uint32_t u = lane; u < units; u += 64) {
        const uint4 q = body[u];
        const uint32_t d[4] = {q.x, q.y, q.z, q.w};
        uint32_t v[K];
#pragma unroll
        for (unsigned k = 0; k < K; ++k) v[k] = W == 1 ? (d[k >> 2] >> (8 * (k & 3))) & 0xFFu : (d[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
        f(head + u * K, v);
    }
}

// (a) ------------------------------------------------------------------------------------------------------------------
template <unsigned W>
__global__ void __launch_bounds__(THREADS) product_hist_kernel(const unsigned char *__restrict__ pixels, uint32_t columns, uint32_t rows,
                                                               uint32_t pitch, uint32_t bits, uint32_t *hist, unsigned long long *over_count)
{
    __shared__ uint32_t s_bins[LDS_BINS];
    const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t maxv = product_max(bits);
    const bool local = bits <= LDS_BITS;
    // as many copies of the bins as fit (a power of two, at most one per wave): fewer lanes meet on one LDS word
    const unsigned fit = LDS_BINS >> (local ? bits : LDS_BITS), copies = fit < WAVES ? fit : WAVES;
    const unsigned mine = (w & (copies - 1)) << bits;
    if (local) {
        for (unsigned i = tid; i < LDS_BINS; i += THREADS) s_bins[i] = 0;
        __syncthreads();
    }
    uint32_t over = 0;
    for (unsigned long long r = (unsigned long long)blockIdx.x * WAVES + w; r < rows; r += (unsigned long long)gridDim.x * WAVES) {
        walk_row<W>(pixels + r * pitch, columns, lane, [&](uint32_t, const auto &v) {
            constexpr unsigned C = sizeof(v) / sizeof(uint32_t);
#pragma unroll
            for (unsigned k = 0; k < C; ++k) {
                over += v[k] > maxv;
                const uint32_t x = product_clamp(v[k], maxv);
                if (local) atomicAdd(&s_bins[mine + x], 1u);
                else atomicAdd(&hist[x], 1u);
            }
        });
    }
    if (local) {
        __syncthreads();
        const uint32_t bins = 1u << bits;
        for (uint32_t b = tid; b < bins; b += THREADS) {
            uint32_t sum = 0;
            for (unsigned c = 0; c < copies; ++c) sum += s_bins[(c << bits) + b];
            if (sum) atomicAdd(&hist[b], sum);
        }
    }
    over = wave_sum(over);
    if (lane == 0 && over) atomicAdd(over_count, (unsigned long long)over);
}

// (b) ------------------------------------------------------------------------------------------------------------------
// Thread t holds the bins [t * per, (t + 1) * per): c[v] is the workgroup scan's prefix in front of the run plus the run's
// own counts up to v.  (N <= 2^31: the counts fit 32 bits.)
__global__ void __launch_bounds__(THREADS) product_lut_kernel(const uint32_t *__restrict__ hist, const unsigned long long *__restrict__ over_count,
                                                              const unsigned char *__restrict__ table_in, xrit_product_params pp, uint32_t bits,
                                                              uint32_t columns, uint32_t rows, unsigned char *lut,
                                                              xrit_product_summary *summary)
{
    __shared__ uint32_t s_part[WAVES];
    __shared__ uint32_t s_min, s_max, s_lo, s_hi;
    const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t bins = 1u << bits, per = (bins + THREADS - 1) / THREADS;
    const uint32_t b0 = tid * per < bins ? tid * per : bins, b1 = b0 + per < bins ? b0 + per : bins;
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    if (tid == 0) {
        s_min = s_lo = s_hi = NONE;
        s_max = 0;
    }
    uint32_t part = 0, mn = NONE, mx = 0;
    for (uint32_t v = b0; v < b1; ++v) {
        const uint32_t h = v ? hist[v] : 0u;
        part += h;
        if (h) {
            mn = mn < v ? mn : v;
            mx = v;
        }
    }
    __syncthreads();
    if (mn != NONE) {
        atomicMin(&s_min, mn);
        atomicMax(&s_max, mx);
    }
    uint32_t total;
    const uint32_t before = block_incl_scan<WAVES>(part, lane, w, s_part, total) - part;
    const uint64_t n = total;
    const uint32_t min_nz = s_min == NONE ? 0u : s_min, max_nz = s_max;
    if (pp.tone == XRIT_TONE_STRETCH && n) {
        uint32_t c = before, lo = NONE, hi = NONE;
        for (uint32_t v = b0; v < b1; ++v) {
            if (!v) continue;
            c += hist[v];
            if (lo == NONE && product_is_lo(c, pp.p_lo, n)) lo = v;
            if (hi == NONE && product_reaches(c, pp.p_hi, n)) hi = v;
        }
        if (lo != NONE) atomicMin(&s_lo, lo);
        if (hi != NONE) atomicMin(&s_hi, hi);
    }
    __syncthreads();
    const uint32_t lo = s_lo == NONE ? 0u : s_lo, hi = s_hi == NONE ? 0u : s_hi;
    const ProductTone t = product_decide(pp.tone, bits, n, min_nz, max_nz, min_nz ? hist[min_nz] : 0u, lo, hi);
    uint32_t c = before;
    for (uint32_t v = b0; v < b1; ++v) {
        if (v) c += hist[v];
        lut[v] = product_lut_entry(t, v, c, t.tone == XRIT_TONE_TABLE ? table_in[v] : (unsigned char)0);
    }
    if (tid == 0) {
        xrit_product_summary o{};
        o.total = (uint64_t)columns * rows;
        o.zeros = hist[0];
        o.out_of_range = *over_count;
        o.min_nz = min_nz;
        o.max_nz = max_nz;
        o.lo = t.lo;
        o.hi = t.hi;
        o.fallback = t.fallback;
        o.tone = pp.tone;
        o.tone_columns = columns;
        o.tone_rows = rows;
        o.small_columns = product_small_dim(columns, pp.factor);
        o.small_rows = product_small_dim(rows, pp.factor);
        *summary = o;
    }
}

// (c) ------------------------------------------------------------------------------------------------------------------
// An item is a band of band_rows rows by a tile of tile_cols columns.  With a thumbnail band_rows is the factor and
// tile_cols the factor times CELLS, so a tile's blocks are its own: their (count << 32 | sum) are added up in LDS (one
// 64-bit add per run of a lane's samples inside one block; samples without data add nothing), then the workgroup writes the
// tile's bytes of the thumbnail's row.  The sum of a block is at most 4096 * 255: exact in its 32 bits.
template <unsigned W>
__global__ void __launch_bounds__(THREADS) product_tone_kernel(const unsigned char *__restrict__ pixels, uint32_t columns, uint32_t rows,
                                                               uint32_t pitch, uint32_t bits, uint32_t factor,
                                                               const unsigned char *__restrict__ lut, unsigned char *tone, unsigned char *small,
                                                               uint32_t band_rows, uint32_t tile_cols, uint32_t n_tiles,
                                                               unsigned long long items)
{
    __shared__ unsigned char s_lut[LDS_BINS];
    __shared__ unsigned long long s_acc[CELLS];
    const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t maxv = product_max(bits);
    const bool local = bits <= LDS_BITS;
    if (local)
        for (uint32_t i = tid; i <= maxv; i += THREADS) s_lut[i] = lut[i];
    if (small)
        for (unsigned i = tid; i < CELLS; i += THREADS) s_acc[i] = 0;
    __syncthreads();
    const uint32_t small_cols = product_small_dim(columns, factor);
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned long long band = item / n_tiles;
        const uint32_t tile = (uint32_t)(item % n_tiles);
        const unsigned long long r0 = band * band_rows, r1 = r0 + band_rows < rows ? r0 + band_rows : rows;
        const uint32_t c0 = tile * tile_cols, n = columns - c0 < tile_cols ? columns - c0 : tile_cols;
        for (unsigned long long r = r0 + w; r < r1; r += WAVES) {
            unsigned char *out = tone ? tone + r * columns + c0 : nullptr;
            walk_row<W>(pixels + r * pitch + (size_t)c0 * W, n, lane, [&](uint32_t i, const auto &v) {
                constexpr unsigned C = sizeof(v) / sizeof(uint32_t);
                uint32_t t[C];
#pragma unroll
                for (unsigned k = 0; k < C; ++k) {
                    const uint32_t x = product_clamp(v[k], maxv);
                    t[k] = local ? s_lut[x] : lut[x];
                }
                if (out) {
                    unsigned char *o = out + i;
                    if (C == 16 && ((uintptr_t)o & 15u) == 0) {
                        uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
                        for (unsigned k = 0; k < C; ++k) d[(k >> 2) & 3] |= t[k] << (8 * (k & 3));
                        *reinterpret_cast<uint4 *>(o) = make_uint4(d[0], d[1], d[2], d[3]);
                    } else if (C == 8 && ((uintptr_t)o & 7u) == 0) {
                        uint32_t d[2] = {0, 0};
#pragma unroll
                        for (unsigned k = 0; k < C; ++k) d[(k >> 2) & 1] |= t[k] << (8 * (k & 3));
                        *reinterpret_cast<uint2 *>(o) = make_uint2(d[0], d[1]);
                    } else {
#pragma unroll
                        for (unsigned k = 0; k < C; ++k) o[k] = (unsigned char)t[k];
                    }
                }
                if (small) {
                    uint32_t cell = i / factor, rem = i - cell * factor;
                    unsigned long long acc = 0;
#pragma unroll
                    for (unsigned k = 0; k < C; ++k) {
                        if (v[k]) acc += (1ull << 32) | t[k];
                        if (++rem == factor) {
                            if (acc) atomicAdd(&s_acc[cell], acc);
                            acc = 0;
                            rem = 0;
                            ++cell;
                        }
                    }
                    if (acc) atomicAdd(&s_acc[cell], acc);
                }
            });
        }
        if (small) {
            __syncthreads();
            const uint32_t cells = (n + factor - 1) / factor;
            unsigned char *row = small + band * small_cols + c0 / factor;
            for (uint32_t c = tid; c < cells; c += THREADS) {
                const unsigned long long acc = s_acc[c];
                row[c] = product_small_byte((uint32_t)acc, (uint32_t)(acc >> 32));
                s_acc[c] = 0;
            }
            __syncthreads();
        }
    }
}

// (d) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS) product_composite_kernel(const unsigned char *__restrict__ a, uint32_t pitch_a,
                                                                    const unsigned char *__restrict__ b, uint32_t pitch_b, uint32_t columns,
                                                                    uint32_t rows, const unsigned char *__restrict__ table, unsigned char *rgb)
{
    const uint32_t groups = (columns + 3) / 4;
    for (unsigned long long r = blockIdx.y; r < rows; r += gridDim.y) {
        const unsigned char *pa = a + r * pitch_a, *pb = b + r * pitch_b;
        unsigned char *o = rgb + r * columns * 3;
        for (uint32_t g = blockIdx.x * THREADS + threadIdx.x; g < groups; g += gridDim.x * THREADS) {
            const uint32_t x = g * 4, m = columns - x < 4 ? columns - x : 4;
            unsigned char *dst = o + (size_t)x * 3;
            if (m == 4) {
                uint32_t av, bv;
                if ((((uintptr_t)(pa + x) | (uintptr_t)(pb + x)) & 3u) == 0) {
                    av = *reinterpret_cast<const uint32_t *>(pa + x);
                    bv = *reinterpret_cast<const uint32_t *>(pb + x);
                } else {
                    av = pa[x] | pa[x + 1] << 8 | pa[x + 2] << 16 | (uint32_t)pa[x + 3] << 24;
                    bv = pb[x] | pb[x + 1] << 8 | pb[x + 2] << 16 | (uint32_t)pb[x + 3] << 24;
                }
                uint32_t d[3] = {0, 0, 0};
#pragma unroll
                for (unsigned k = 0; k < 4; ++k) {
                    const unsigned char *e = table + (size_t)((((av >> (8 * k)) & 255u) << 8) | ((bv >> (8 * k)) & 255u)) * 3;
#pragma unroll
                    for (unsigned j = 0; j < 3; ++j) {
                        const unsigned at = 3 * k + j;
                        d[at >> 2] |= (uint32_t)e[j] << (8 * (at & 3));
                    }
                }
                if (((uintptr_t)dst & 3u) == 0) {
                    uint32_t *q = reinterpret_cast<uint32_t *>(dst);
                    q[0] = d[0];
                    q[1] = d[1];
                    q[2] = d[2];
                } else {
#pragma unroll
                    for (unsigned at = 0; at < 12; ++at) dst[at] = (unsigned char)(d[at >> 2] >> (8 * (at & 3)));
                }
            } else {
                for (uint32_t k = 0; k < m; ++k) {
                    const unsigned char *e = table + (size_t)(((uint32_t)pa[x + k] << 8) | pb[x + k]) * 3;
                    dst[3 * k] = e[0];
                    dst[3 * k + 1] = e[1];
                    dst[3 * k + 2] = e[2];
                }
            }
        }
    }
}

}  // namespace

int launch_product(const xrit_product_image &im, const xrit_product_params &pp, const unsigned char *table_in, uint32_t *hist,
                   unsigned long long *over_count, unsigned char *lut, unsigned char *tone, unsigned char *small,
                   xrit_product_summary *summary, hipStream_t s)
{
    const bool wide = product_width(im.bits) == 2;
    XR_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) << im.bits, s));
    XR_HIP(hipMemsetAsync(over_count, 0, sizeof *over_count, s));
    // (grids no larger than fill the chip a few times over, striding)
    const unsigned g_hist = div_up(im.rows, WAVES);
    const dim3 grid_hist(g_hist < 1024u ? g_hist : 1024u), block(THREADS);
    if (wide)
        hipLaunchKernelGGL(product_hist_kernel<2>, grid_hist, block, 0, s, im.d_pixels, im.columns, im.rows, im.pitch, im.bits, hist,
                           over_count);
    else
        hipLaunchKernelGGL(product_hist_kernel<1>, grid_hist, block, 0, s, im.d_pixels, im.columns, im.rows, im.pitch, im.bits, hist,
                           over_count);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(product_lut_kernel, dim3(1), block, 0, s, hist, over_count, table_in, pp, im.bits, im.columns, im.rows, lut, summary);
    XR_HIP(hipGetLastError());
    if (!pp.factor) small = nullptr;
    if (!tone && !small) return XRIT_OK;
    const uint32_t band_rows = small ? pp.factor : 2 * WAVES, tile_cols = small ? pp.factor * CELLS : PLAIN_TILE;
    const uint32_t n_tiles = div_up(im.columns, tile_cols);
    const unsigned long long items = (unsigned long long)div_up(im.rows, band_rows) * n_tiles;
    const dim3 grid_tone((unsigned)(items < 8192ull ? items : 8192ull));
    if (wide)
        hipLaunchKernelGGL(product_tone_kernel<2>, grid_tone, block, 0, s, im.d_pixels, im.columns, im.rows, im.pitch, im.bits, pp.factor, lut,
                           tone, small, band_rows, tile_cols, n_tiles, items);
    else
        hipLaunchKernelGGL(product_tone_kernel<1>, grid_tone, block, 0, s, im.d_pixels, im.columns, im.rows, im.pitch, im.bits, pp.factor, lut,
                           tone, small, band_rows, tile_cols, n_tiles, items);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_product_composite(const unsigned char *a, uint32_t pitch_a, const unsigned char *b, uint32_t pitch_b, uint32_t columns,
                             uint32_t rows, const unsigned char *table, unsigned char *rgb, hipStream_t s)
{
    const unsigned gx = div_up(div_up(columns, 4), THREADS);
    hipLaunchKernelGGL(product_composite_kernel, dim3(gx < 64u ? gx : 64u, rows < 4096u ? rows : 4096u), dim3(THREADS), 0, s, a, pitch_a, b,
                       pitch_b, columns, rows, table, rgb);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
