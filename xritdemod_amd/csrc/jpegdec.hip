// jpegdec.hip -- the JPEG decoder stage's kernels (jpegdec_rule.h has the rules per value,
// tests/jpegdec_spec.py is the specification).  One call is
//   header      one wave per item: lane 0 walks the marker chain, the lanes build the Huffman and quantiser tables
//   scan        items -> the blocks, MCUs, intervals, scan bytes and pixel bytes in front of each; the item that brings the
//               blocks or the scan bytes above the scratch's room, and every one behind it, becomes TOO_LARGE
//   zero        the coefficients of the blocks the call takes
//   terminator  byte-parallel over the scan bytes of all items: the first FF xx that is neither stuffing nor RSTm
//   scan        byte-parallel: FF 00 -> FF, FF Dm dropped; the unstuffed stream of all items, per RSTm its place and its m
//   entropy     form 0: a lane per restart interval walks it; form 1: a wave per interval, 64 subsequences at a time
//   resolve     one wave per item: the first fault in the serial walk's order is the status
//   scan        the DC differences -> coefficients: a segmented sum per component per interval
//   pixels      8 MCUs per wave: dequantise, both inverse-DCT passes with the transpose in LDS, range limit, colour
//   finish      the records, the padding, the summary
// All sizes are only known on the device: every kernel strides over them with a grid the host sizes from the bounds.
#include "common.h"
#include "jpegdec_rule.h"
#include "kernels.h"
#include "scan.h"
#include "wave_ops.h"

namespace xrit {

struct JpegDecItem {
    unsigned long long src;         // the stream's offset in the bytes
    uint32_t length, status;
    uint32_t columns, rows, comps, restart;
    uint32_t scan;                  // the first scan byte, from src
    uint32_t blocks, mcus, n_int, ri;
    uint32_t found;                 // intervals found
    uint32_t tend;                  // where the scan ends, from src: the first marker that is not RSTm, or length
    uint32_t fits;                  // offset + padded length <= cap
};
static_assert(sizeof(JpegDecItem) == 64, "JpegDecItem layout");

struct JpegDecSum {
    unsigned long long b, m, i, s, o;       // blocks, MCUs, intervals + 1, scan bytes, padded pixel bytes
};

namespace {

constexpr int WAVES = 4;            // per workgroup, everywhere below
constexpr int WS_ROW = 9, WS_BLOCK = 8 * WS_ROW + 1;
enum { TOT_B = 0, TOT_M = 1, TOT_I = 2, TOT_S = 3, TOT_O = 4 };

struct Orders {
    uint8_t zig[64];                // zigzag position -> natural index
    uint8_t unzig[64];              // natural index -> zigzag position
};
constexpr Orders make_orders()
{
    Orders o{};
    for (int k = 0; k < 64; ++k) {
        o.zig[k] = JPEG_ZIGZAG[k];
        o.unzig[JPEG_ZIGZAG[k]] = (uint8_t)k;
    }
    return o;
}
__device__ const Orders d_orders = make_orders();

// the last i in [0, n) with base[i] <= x; base[0] = 0
__device__ __forceinline__ uint32_t locate(const uint32_t *__restrict__ base, uint32_t n, uint32_t x)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (base[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t clamp32(unsigned long long v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// ---- header ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * WAVES) jpegdec_header_kernel(JpegDecPar P, JpegDecScratch sc)
{
    __shared__ JpegDecHeader s_h[WAVES];
    __shared__ unsigned long long s_src[WAVES];
    __shared__ uint32_t s_len[WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, it = blockIdx.x * WAVES + w;
    const bool valid = it < P.n_items;
    if (blockIdx.x == 0 && threadIdx.x == 0) *sc.rounds = 0;
    if (valid && lane == 0) {
        const unsigned char *r = P.items + (size_t)it * P.stride;
        unsigned long long off = 0;
        uint32_t len = 0;
        for (int i = 7; i >= 0; --i) off = off << 8 | r[i];
        for (int i = 11; i >= 8; --i) len = len << 8 | r[i];
        JpegDecHeader h;
        if (off > P.n_bytes || len > P.n_bytes - off) {
            h = jpegdec_fail(JPEGDEC_DAMAGED);
            off = 0;
            len = 0;
        } else {
            h = jpegdec_parse_header(P.bytes + off, len);
        }
        s_h[w] = h;
        s_src[w] = off;
        s_len[w] = len;
    }
    __syncthreads();
    if (!valid) return;
    const JpegDecHeader h = s_h[w];
    const unsigned char *src = P.bytes + s_src[w];
    if (h.status == JPEGDEC_OK) {
        if (lane < 2 * h.comps) jpegdec_build_huff(src + ((lane & 1) ? h.ac_at[lane >> 1] : h.dc_at[lane >> 1]), sc.huff[(size_t)it * 6 + lane]);
        for (uint32_t c = 0; c < h.comps; ++c) sc.q[(size_t)it * 192 + c * 64 + d_orders.zig[lane]] = src[h.q_at[c] + lane];
    }
    if (lane == 0) {
        JpegDecItem I;
        I.src = s_src[w];
        I.length = s_len[w];
        I.status = h.status;
        I.columns = h.columns;
        I.rows = h.rows;
        I.comps = h.comps;
        I.restart = h.restart;
        I.scan = h.scan;
        I.blocks = h.blocks;
        I.mcus = h.comps ? h.blocks / h.comps : 0;
        I.n_int = h.intervals;
        I.ri = h.restart ? h.restart : I.mcus;
        I.found = 0;
        I.tend = I.length;
        I.fits = 0;
        sc.item[it] = I;
    }
}

// ---- the scans (scan.h) -----------------------------------------------------------------------------------------------------
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

__device__ __forceinline__ unsigned long long padded_pixels(const JpegDecItem &I)
{
    return ((unsigned long long)I.columns * I.rows * I.comps + 3) & ~3ull;
}

// Elements 0 .. n_items: what lies in front of item i (element n_items: the totals).  The sums run over every item whose
// header is sound; once the blocks or the scan bytes pass the scratch's room, that item and all behind it are TOO_LARGE and
// the totals are those in front of it.
struct ItemF {
    typedef JpegDecSum T;
    JpegDecPar P;
    JpegDecScratch sc;
    __device__ T value(long long i) const
    {
        T v{0, 0, 0, 0, 0};
        if (i >= P.n_items) return v;
        const JpegDecItem I = sc.item[i];
        if (I.status != JPEGDEC_OK && !(I.status == JPEGDEC_TOO_LARGE && I.blocks)) return v;
        v.b = I.blocks;
        v.m = I.mcus;
        v.i = I.n_int + 1;
        v.s = I.length - I.scan;
        v.o = padded_pixels(I);
        return v;
    }
    __device__ T identity() const { return T{0, 0, 0, 0, 0}; }
    __device__ T combine(const T &lo, const T &hi) const { return T{lo.b + hi.b, lo.m + hi.m, lo.i + hi.i, lo.s + hi.s, lo.o + hi.o}; }
    __device__ bool room(const T &v) const { return v.b <= P.max_blocks && v.s <= P.max_scan; }
    __device__ T reduce_run(long long i0, int cnt) const
    {
        T v = identity();
        for (int k = 0; k < cnt; ++k) v = combine(v, value(i0 + k));
        return v;
    }
    __device__ void totals(const T &v) const
    {
        sc.tot[TOT_B] = v.b;
        sc.tot[TOT_M] = v.m;
        sc.tot[TOT_I] = v.i;
        sc.tot[TOT_S] = v.s;
        sc.tot[TOT_O] = v.o;
    }
    __device__ void apply_run(long long i0, int cnt, const T &pre) const
    {
        T v = pre;
        for (int k = 0; k < cnt; ++k) {
            const long long i = i0 + k;
            sc.bbase[i] = clamp32(v.b);
            sc.mbase[i] = clamp32(v.m);
            sc.ibase[i] = clamp32(v.i);
            sc.sbase[i] = clamp32(v.s);
            sc.obase[i] = v.o;
            if (i == P.n_items) {
                if (room(v)) totals(v);
                continue;
            }
            const T next = combine(v, value(i));
            if (sc.item[i].status == JPEGDEC_OK && !room(next)) {
                sc.item[i].status = JPEGDEC_TOO_LARGE;       // (its blocks stay: value() goes on counting it)
                if (room(v)) totals(v);
            }
            v = next;
        }
    }
};

// 0: dropped (stuffing, a marker's second byte), 1: kept, 2: the FF of an RSTm.  p in front of the item's tend.
__device__ __forceinline__ uint32_t scan_kind(const unsigned char *__restrict__ s, const JpegDecItem &I, uint32_t p, uint32_t &b)
{
    b = s[p];
    if (b == 0xFF) return (p + 1 < I.length ? s[p + 1] : 1u) == 0 ? 1u : 2u;
    if (p > I.scan && s[p - 1] == 0xFF && (b == 0 || (b >= 0xD0 && b <= 0xD7))) return 0;
    return 1;
}

__global__ void __launch_bounds__(256) jpegdec_terminator_kernel(JpegDecPar P, JpegDecScratch sc)
{
    const unsigned long long total = sc.tot[TOT_S];
    for (unsigned long long j0 = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * 16; j0 < total; j0 += (unsigned long long)gridDim.x * 256 * 16) {
        uint32_t it = locate(sc.sbase, P.n_items, (uint32_t)j0);
        for (uint32_t k = 0; k < 16 && j0 + k < total; ++k) {
            const uint32_t j = (uint32_t)j0 + k;
            while (it + 1 < P.n_items && sc.sbase[it + 1] <= j) ++it;
            const JpegDecItem &I = sc.item[it];
            const unsigned char *s = P.bytes + I.src;
            const uint32_t p = I.scan + (j - sc.sbase[it]);
            if (s[p] != 0xFF) continue;
            const uint32_t n = p + 1 < I.length ? s[p + 1] : 1u;
            if (n != 0 && !(n >= 0xD0 && n <= 0xD7)) atomicMin(&sc.item[it].tend, p);
        }
    }
}

// Elements 0 .. total scan bytes (the host's bound: max_scan + 1 of them): kept bytes and RSTm markers in front of each.
// The element at an item's first scan byte leaves them as kbase / rbase of that item and of the empty ones in front of it;
// the element behind the last byte does so for the items there.
struct UnstuffF {
    struct T {
        uint32_t kept, rst;
    };
    JpegDecPar P;
    JpegDecScratch sc;
    __device__ T identity() const { return T{0, 0}; }
    __device__ T combine(const T &lo, const T &hi) const { return T{lo.kept + hi.kept, lo.rst + hi.rst}; }
    __device__ T reduce_run(long long i0, int cnt) const
    {
        T v{0, 0};
        const unsigned long long total = sc.tot[TOT_S];
        if ((unsigned long long)i0 >= total) return v;
        uint32_t it = locate(sc.sbase, P.n_items, (uint32_t)i0);
        for (int k = 0; k < cnt && (unsigned long long)(i0 + k) < total; ++k) {
            const uint32_t j = (uint32_t)(i0 + k);
            while (it + 1 < P.n_items && sc.sbase[it + 1] <= j) ++it;
            const JpegDecItem &I = sc.item[it];
            const uint32_t p = I.scan + (j - sc.sbase[it]);
            if (p >= I.tend) continue;
            uint32_t b;
            const uint32_t kind = scan_kind(P.bytes + I.src, I, p, b);
            v.kept += kind == 1;
            v.rst += kind == 2;
        }
        return v;
    }
    __device__ void apply_run(long long i0, int cnt, const T &pre) const
    {
        T v = pre;
        const unsigned long long total = sc.tot[TOT_S];
        if ((unsigned long long)i0 > total) return;
        uint32_t it = locate(sc.sbase, P.n_items + 1, (uint32_t)i0);
        for (int k = 0; k < cnt && (unsigned long long)(i0 + k) <= total; ++k) {
            const uint32_t j = (uint32_t)(i0 + k);
            while (it + 1 <= P.n_items && sc.sbase[it + 1] <= j) ++it;
            if (sc.sbase[it] == j)
                for (uint32_t e = it;; --e) {
                    sc.kbase[e] = v.kept;
                    sc.rbase[e] = v.rst;
                    if (e == 0 || sc.sbase[e - 1] != j) break;
                }
            if (j == total) break;
            const JpegDecItem &I = sc.item[it];
            const uint32_t p = I.scan + (j - sc.sbase[it]);
            if (p >= I.tend) continue;
            uint32_t b;
            const uint32_t kind = scan_kind(P.bytes + I.src, I, p, b);
            if (kind == 1) {
                sc.un[v.kept++] = (unsigned char)b;
            } else if (kind == 2) {
                sc.rst_pos[v.rst] = v.kept;
                sc.rst_m[v.rst] = (unsigned char)(P.bytes[I.src + p + 1] & 7);
                ++v.rst;
            }
        }
    }
};

// ---- zero -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) jpegdec_zero_kernel(JpegDecScratch sc)
{
    const size_t groups = (size_t)sc.tot[TOT_B] * 8;               // 64 coefficients of 2 bytes: 8 groups of 16 bytes
    uint4 *c = reinterpret_cast<uint4 *>(sc.coef);
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) c[g] = make_uint4(0, 0, 0, 0);
}

// ---- entropy ----------------------------------------------------------------------------------------------------------------
struct Interval {
    const unsigned char *src;       // its unstuffed bytes
    uint32_t nbytes;
    const JpegDecHuff *tabs;
    uint32_t comps, blocks;
    size_t first;                   // its first block
};
// interval slot g of the call (every item has n_int + 1 slots; the last is none)
__device__ __forceinline__ bool interval_of(const JpegDecPar &P, const JpegDecScratch &sc, uint32_t g, Interval &iv)
{
    const uint32_t it = locate(sc.ibase, P.n_items, g), k = g - sc.ibase[it];
    const JpegDecItem &I = sc.item[it];
    if (I.status != JPEGDEC_OK || k >= I.n_int) return false;
    const uint32_t r0 = sc.rbase[it], nr = sc.rbase[it + 1] - r0, kb = sc.kbase[it], ke = sc.kbase[it + 1];
    const uint32_t begin = k == 0 ? kb : (k - 1 < nr ? sc.rst_pos[r0 + k - 1] : ke), end = k < nr ? sc.rst_pos[r0 + k] : ke;
    const unsigned long long m0 = (unsigned long long)k * I.ri, m1 = m0 + I.ri < I.mcus ? m0 + I.ri : I.mcus;
    iv.src = sc.un + begin;
    iv.nbytes = end - begin;
    iv.tabs = sc.huff + (size_t)it * 6;
    iv.comps = I.comps;
    iv.blocks = (uint32_t)(m1 - m0) * I.comps;
    iv.first = (size_t)sc.bbase[it] + (size_t)m0 * I.comps;
    return true;
}

struct CoefSink {
    int16_t *at;                    // the interval's first block
    uint32_t first;                 // the walk's first block in the interval
    __device__ void operator()(uint32_t block, uint32_t z, int32_t v) const { at[(size_t)(first + block) * 64 + z] = (int16_t)v; }
};
struct NoSink {
    __device__ void operator()(uint32_t, uint32_t, int32_t) const {}
};

// form 0: one lane per restart interval
__global__ void __launch_bounds__(256) jpegdec_entropy_lane_kernel(JpegDecPar P, JpegDecScratch sc)
{
    const uint32_t total = (uint32_t)sc.tot[TOT_I];
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < total; g += gridDim.x * 256) {
        Interval iv;
        if (!interval_of(P, sc, g, iv)) continue;
        JpegDecState st{0, 0, 0};
        uint32_t done;
        uint32_t fault = jpegdec_walk(iv.src, iv.nbytes, iv.tabs, iv.comps, st, iv.nbytes * 8, iv.blocks, done, CoefSink{sc.coef + iv.first * 64, 0});
        if (!fault && done < iv.blocks) fault = JPEGDEC_SHORT;
        sc.ifault[g] = fault;
    }
}

// form 1: one wave per restart interval, tiles of 64 subsequences of S bits.  In a round every lane whose entry state changed
// walks its subsequence again, then lane i + 1 takes lane i's exit state; a round that changes no entry ends the tile.  Lane
// 0's entry is the carried, settled state, so after round r lanes 0 .. r - 1 hold the serial walk's states: at most 64
// rounds.  Then every lane walks once more from its settled entry, with its block index, and stores.
__global__ void __launch_bounds__(64 * WAVES) jpegdec_entropy_wave_kernel(JpegDecPar P, JpegDecScratch sc)
{
    const uint32_t lane = threadIdx.x & 63, total = (uint32_t)sc.tot[TOT_I];
    uint32_t most = 0;
    for (uint32_t g = blockIdx.x * WAVES + (threadIdx.x >> 6); g < total; g += gridDim.x * WAVES) {
        Interval iv;
        if (!interval_of(P, sc, g, iv)) continue;                       // uniform in the wave
        const unsigned long long nbits = (unsigned long long)iv.nbytes * 8, nsub = (nbits + P.S - 1) / P.S;
        JpegDecState carry{0, 0, 0};
        uint32_t index = 0, fault = JPEGDEC_OK;
        for (unsigned long long t0 = 0; t0 < nsub; t0 += 64) {
            const unsigned long long sub = t0 + lane;
            const bool active = sub < nsub;
            const unsigned long long e64 = (sub + 1) * P.S;
            const uint32_t end = (uint32_t)(e64 < nbits ? e64 : nbits);
            JpegDecState entry = carry, out{0, 0, 0};
            if (lane) entry = JpegDecState{(uint32_t)(sub * P.S), 0, 0};
            uint32_t n_out = 0, rounds = 0;
            bool dirty = active;
            while (__ballot(dirty)) {
                ++rounds;
                if (dirty) {
                    out = entry;
                    (void)jpegdec_walk(iv.src, iv.nbytes, iv.tabs, iv.comps, out, end, 0xFFFFFFFFu, n_out, NoSink{});
                }
                const uint32_t up_p = __shfl_up(out.p, 1, 64), up_c = __shfl_up(out.c, 1, 64), up_z = __shfl_up(out.z, 1, 64);
                dirty = false;
                if (active && lane && (up_p != entry.p || up_c != entry.c || up_z != entry.z)) {
                    entry = JpegDecState{up_p, up_c, up_z};
                    dirty = true;
                }
            }
            most = rounds > most ? rounds : most;
            if (!active) n_out = 0;
            const uint32_t incl = wave_incl_scan(n_out, (int)lane), first = index + incl - n_out;
            uint32_t mine = JPEGDEC_OK;
            if (active && entry.p != JPEGDEC_DEAD && first < iv.blocks) {
                JpegDecState st = entry;
                uint32_t done;
                mine = jpegdec_walk(iv.src, iv.nbytes, iv.tabs, iv.comps, st, end, iv.blocks - first, done, CoefSink{sc.coef + iv.first * 64, first});
            }
            const unsigned long long faulted = __ballot(mine != JPEGDEC_OK);
            if (faulted) {
                fault = __shfl(mine, __ffsll((long long)faulted) - 1, 64);
                break;
            }
            index += wave_total(incl);
            carry = JpegDecState{__shfl(out.p, 63, 64), __shfl(out.c, 63, 64), __shfl(out.z, 63, 64)};
            if (index >= iv.blocks || carry.p == JPEGDEC_DEAD) break;
        }
        if (!fault && index < iv.blocks) fault = JPEGDEC_SHORT;
        if (lane == 0) sc.ifault[g] = fault;
    }
    if (lane == 0 && most) atomicMax(sc.rounds, most);
}

// ---- resolve ----------------------------------------------------------------------------------------------------------------
// The serial walk's order: interval 0's bits, the marker behind it, interval 1's bits, ...; the first fault is the status.
__global__ void __launch_bounds__(64 * WAVES) jpegdec_resolve_kernel(JpegDecPar P, JpegDecScratch sc)
{
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t it = blockIdx.x * WAVES + (threadIdx.x >> 6); it < P.n_items; it += gridDim.x * WAVES) {
        const JpegDecItem I = sc.item[it];
        if (I.status != JPEGDEC_OK) continue;
        const unsigned char *s = P.bytes + I.src;
        const bool other = I.tend + 1 < I.length && s[I.tend + 1] != 0xD9;          // the scan ends at a marker that is not EOI
        const uint32_t r0 = sc.rbase[it], nr = sc.rbase[it + 1] - r0, g0 = sc.ibase[it];
        uint32_t best = 0xFFFFFFFFu;
        for (uint32_t k = lane; k < I.n_int; k += 64) {
            uint32_t f = sc.ifault[g0 + k];
            if (!f) {
                if (k + 1 < I.n_int) {
                    if (k >= nr) f = other ? JPEGDEC_MARKER : JPEGDEC_INTERVALS;
                    else if (sc.rst_m[r0 + k] != (k & 7)) f = JPEGDEC_RST_ORDER;
                } else if (nr + 1 > I.n_int) {
                    f = JPEGDEC_INTERVALS;
                } else if (other) {
                    f = JPEGDEC_MARKER;
                }
            }
            if (f) {
                best = k << 4 | f;
                break;                                  // this lane's first
            }
        }
        for (int off = 32; off; off >>= 1) {
            const uint32_t o = __shfl_xor(best, off, 64);
            best = o < best ? o : best;
        }
        if (lane == 0) {
            sc.item[it].status = best == 0xFFFFFFFFu ? JPEGDEC_OK : (best & 15);
            sc.item[it].found = nr + 1;
            sc.item[it].fits = sc.obase[it] + padded_pixels(I) <= P.cap;
        }
    }
}

// ---- DC prediction ------------------------------------------------------------------------------------------------------------
// Over the blocks of the call: per component the sum of the differences since the interval's first MCU, kept in 16 bits
struct DcF {
    typedef uint4 T;                // x: a reset lies in the run; y, z, w: the sums per component since then
    JpegDecPar P;
    JpegDecScratch sc;
    __device__ T identity() const { return make_uint4(0, 0, 0, 0); }
    __device__ T combine(const T &lo, const T &hi) const { return hi.x ? hi : make_uint4(lo.x, lo.y + hi.y, lo.z + hi.z, lo.w + hi.w); }
    __device__ T element(uint32_t blk, uint32_t &it, uint32_t &c) const
    {
        while (it + 1 < P.n_items && sc.bbase[it + 1] <= blk) ++it;
        const JpegDecItem &I = sc.item[it];
        const uint32_t local = blk - sc.bbase[it], m = local / I.comps;
        c = local - m * I.comps;
        const uint32_t d = (uint32_t)(int32_t)sc.coef[(size_t)blk * 64];
        return make_uint4(c == 0 && m % I.ri == 0, c == 0 ? d : 0, c == 1 ? d : 0, c == 2 ? d : 0);
    }
    __device__ T reduce_run(long long i0, int cnt) const
    {
        T v = identity();
        const unsigned long long total = sc.tot[TOT_B];
        if ((unsigned long long)i0 >= total) return v;
        uint32_t it = locate(sc.bbase, P.n_items, (uint32_t)i0), c;
        for (int k = 0; k < cnt && (unsigned long long)(i0 + k) < total; ++k) v = combine(v, element((uint32_t)(i0 + k), it, c));
        return v;
    }
    __device__ void apply_run(long long i0, int cnt, const T &pre) const
    {
        T v = pre;
        const unsigned long long total = sc.tot[TOT_B];
        if ((unsigned long long)i0 >= total) return;
        uint32_t it = locate(sc.bbase, P.n_items, (uint32_t)i0), c;
        for (int k = 0; k < cnt && (unsigned long long)(i0 + k) < total; ++k) {
            v = combine(v, element((uint32_t)(i0 + k), it, c));
            sc.coef[(size_t)(i0 + k) * 64] = (int16_t)(uint16_t)(c == 0 ? v.y : c == 1 ? v.z : v.w);
        }
    }
};

// ---- pixels -------------------------------------------------------------------------------------------------------------------
// Lane (b, r) of a wave makes column r's pass of MCU m0 + b, then row r's; the transpose goes through LDS.
__global__ void __launch_bounds__(64 * WAVES) jpegdec_pixels_kernel(JpegDecPar P, JpegDecScratch sc)
{
    __shared__ int32_t s_ws[WAVES][8 * WS_BLOCK];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = lane >> 3, r = lane & 7;
    const unsigned long long total = sc.tot[TOT_M], groups = (total + 7) / 8;
    for (unsigned long long g0 = (unsigned long long)blockIdx.x * WAVES; g0 < groups; g0 += (unsigned long long)gridDim.x * WAVES) {
        const unsigned long long mcu = (g0 + w) * 8 + b;
        const bool valid = mcu < total;
        const uint32_t it = locate(sc.mbase, P.n_items, valid ? (uint32_t)mcu : 0u);
        const JpegDecItem &I = sc.item[it];
        const uint32_t comps = valid ? I.comps : 0, local = valid ? (uint32_t)mcu - sc.mbase[it] : 0;
        const uint32_t bw = (I.columns + 7) / 8, by = bw ? local / bw : 0, bx = local - by * bw;
        const bool decode = valid && I.status == JPEGDEC_OK;
        uint32_t px[3][8];
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            int32_t d[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = 0;
            if (decode && c < comps) {
                const int16_t *co = sc.coef + ((size_t)sc.bbase[it] + (size_t)local * comps + c) * 64;
                const unsigned char *q = sc.q + (size_t)it * 192 + c * 64;
#pragma unroll
                for (int i = 0; i < 8; ++i) d[i] = (int32_t)((uint32_t)(int32_t)co[d_orders.unzig[i * 8 + r]] * (uint32_t)q[i * 8 + r]);
                jpegdec_idct_pass(d, 11);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) s_ws[w][b * WS_BLOCK + i * WS_ROW + r] = d[i];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = s_ws[w][b * WS_BLOCK + r * WS_ROW + i];          // row r
            jpegdec_idct_pass(d, 18);
#pragma unroll
            for (int i = 0; i < 8; ++i) px[c][i] = jpegdec_range_limit(d[i]);
            __syncthreads();
        }
        const uint32_t y = by * 8 + r;
        if (!valid || !I.fits || y >= I.rows) continue;
        unsigned char *row = P.pixels + sc.obase[it] + (size_t)y * I.columns * comps;
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t x = bx * 8 + i;
            if (x >= I.columns) break;
            if (comps == 1) {
                row[x] = decode ? (unsigned char)px[0][i] : 0;
            } else {
                uint32_t cr = 0, cg = 0, cb = 0;
                if (decode) jpegdec_colour((int32_t)px[0][i], (int32_t)px[1][i], (int32_t)px[2][i], cr, cg, cb);
                row[(size_t)x * 3] = (unsigned char)cr;
                row[(size_t)x * 3 + 1] = (unsigned char)cg;
                row[(size_t)x * 3 + 2] = (unsigned char)cb;
            }
        }
    }
}

// ---- finish -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) jpegdec_finish_kernel(JpegDecPar P, JpegDecScratch sc)
{
    __shared__ uint32_t s_count[JPEGDEC_N_STATUS + 1];
    if (threadIdx.x <= JPEGDEC_N_STATUS) s_count[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t it = threadIdx.x; it < P.n_items; it += 256) {
        const JpegDecItem I = sc.item[it];
        const bool pixels = I.status == JPEGDEC_OK || I.status >= JPEGDEC_BAD_CODE;
        xrit_jpegdec_record rec{};
        rec.columns = I.columns;
        rec.rows = I.rows;
        rec.components = I.comps;
        rec.restart = I.restart;
        rec.status = I.status;
        if (pixels) {
            rec.offset = sc.obase[it];
            rec.length = (unsigned long long)I.columns * I.rows * I.comps;
            rec.intervals = I.found;
            if (I.fits)
                for (unsigned long long at = rec.offset + rec.length; at < rec.offset + padded_pixels(I); ++at) P.pixels[at] = 0;
            else
                atomicOr(&s_count[JPEGDEC_N_STATUS], 1u);
        }
        P.records[it] = rec;
        atomicAdd(&s_count[I.status], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        xrit_jpegdec_summary sum{};
        sum.images = s_count[0];
        sum.bytes = sc.tot[TOT_O];
        for (uint32_t i = 0; i < JPEGDEC_N_STATUS; ++i) sum.by_status[i] = s_count[i];
        sum.overflow = s_count[JPEGDEC_N_STATUS];
        *P.summary = sum;
    }
}

}  // namespace

size_t jpegdec_scratch_carve(void *base, uint32_t n_items, uint32_t max_scan, uint32_t max_blocks, JpegDecScratch &sc)
{
    Carver c{static_cast<char *>(base)};
    const size_t n1 = (size_t)n_items + 1;
    sc.coef = c.take<int16_t>((size_t)max_blocks * 64 + 8, 16);
    sc.item = c.take<JpegDecItem>(n1, 16);
    sc.obase = c.take<unsigned long long>(n1, 16);
    sc.tot = c.take<unsigned long long>(8, 16);
    sc.item_aggs = c.take<JpegDecSum>(scan_aggs_count((long long)n1), 16);
    sc.un_aggs = c.take<unsigned long long>(scan_aggs_count((long long)max_scan + 1), 16);
    sc.dc_aggs = c.take<uint4>(scan_aggs_count((long long)max_blocks), 16);
    sc.huff = c.take<JpegDecHuff>((size_t)n_items * 6 + 1, 16);
    sc.bbase = c.take<uint32_t>(n1, 16);
    sc.mbase = c.take<uint32_t>(n1, 16);
    sc.ibase = c.take<uint32_t>(n1, 16);
    sc.sbase = c.take<uint32_t>(n1, 16);
    sc.kbase = c.take<uint32_t>(n1, 16);
    sc.rbase = c.take<uint32_t>(n1, 16);
    sc.rst_pos = c.take<uint32_t>((size_t)max_scan / 2 + 2, 16);
    sc.ifault = c.take<uint32_t>((size_t)max_blocks + n1, 16);
    sc.rounds = c.take<uint32_t>(4, 16);
    sc.q = c.take<unsigned char>((size_t)n_items * 192 + 16, 16);
    sc.un = c.take<unsigned char>((size_t)max_scan + 16, 16);
    sc.rst_m = c.take<unsigned char>((size_t)max_scan / 2 + 2, 16);
    return c.used();
}

int launch_jpegdec(const JpegDecPar &p, const JpegDecScratch &sc, hipStream_t s)
{
    const auto grid = [](size_t work, size_t per, unsigned most) {
        const size_t g = (work + per - 1) / per;
        return dim3((unsigned)(g < 1 ? 1 : g < most ? g : most));
    };
    if (p.n_items) {
        hipLaunchKernelGGL(jpegdec_header_kernel, dim3(div_up(p.n_items, WAVES)), dim3(64 * WAVES), 0, s, p, sc);
        XR_HIP(hipGetLastError());
    } else {
        XR_HIP(hipMemsetAsync(sc.rounds, 0, sizeof(uint32_t), s));
    }
    XR_TRY(run_scan(ItemF{p, sc}, (long long)p.n_items + 1, sc.item_aggs, s));
    hipLaunchKernelGGL(jpegdec_zero_kernel, grid((size_t)p.max_blocks * 8, 256, 4096), dim3(256), 0, s, sc);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_terminator_kernel, grid(p.max_scan, 256 * 16, 4096), dim3(256), 0, s, p, sc);
    XR_HIP(hipGetLastError());
    XR_TRY(run_scan(UnstuffF{p, sc}, (long long)p.max_scan + 1, reinterpret_cast<UnstuffF::T *>(sc.un_aggs), s));
    const size_t slots = (size_t)p.max_blocks + p.n_items;
    if (p.form == 0) hipLaunchKernelGGL(jpegdec_entropy_lane_kernel, grid(slots, 256, 4096), dim3(256), 0, s, p, sc);
    else hipLaunchKernelGGL(jpegdec_entropy_wave_kernel, grid(slots, WAVES, 4096), dim3(64 * WAVES), 0, s, p, sc);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_resolve_kernel, grid(p.n_items, WAVES, 1024), dim3(64 * WAVES), 0, s, p, sc);
    XR_HIP(hipGetLastError());
    XR_TRY(run_scan(DcF{p, sc}, (long long)p.max_blocks, sc.dc_aggs, s));
    hipLaunchKernelGGL(jpegdec_pixels_kernel, grid(p.max_blocks, 8 * WAVES, 4096), dim3(64 * WAVES), 0, s, p, sc);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_finish_kernel, dim3(1), dim3(256), 0, s, p, sc);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
