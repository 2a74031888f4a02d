// overlay.hip -- the kernels of the map overlay stage (include/xritdemod_amd.h, "Map overlay"), all
// on overlay_rule.h's functions:
//   overlay_map_kernel     a lane per vertex: the quad {A, B, C, S} through geo_rule.h's geo_point
//   overlay_walk_kernel    form 0: a lane per pair of vertices, which sets the segment up, tallies it and walks its steps
//   overlay_count_kernel   form 1: a lane per pair, which sets the segment up, tallies it and leaves its step count; scan.h
//                          turns the counts into the steps in front of every pair (8 bytes per pair, nothing per step)
//   overlay_step_kernel    form 1: a lane per step, the grid striding over them; the step's pair by binary search in the
//                          prefix, the segment set up again from its two vertices (16 bytes, mostly shared with the
//                          neighbouring lanes), the one stamp
//   overlay_blend_kernel   a wave per row: 16 pixels a lane as 16-byte loads and stores where the row's three addresses
//                          are 16-byte aligned, single pixels otherwise and behind the last whole group; the covered
//                          pixels are counted per lane in registers and committed once per wave
// A stamp is at most 8 x 8 pixels: per row of it one atomic OR for each of the at most three dwords it meets, carrying only
// the bits of the pixels inside the stamp and the image, and none where the dword already holds them.  OR is idempotent and
// commutative: the mask does not depend on how the steps were dealt out.  The summaries are integer sums: registers, a
// wave sum, LDS, one global atomic per workgroup and field.
#include "common.h"
#include "geo_rule.h"
#include "kernels.h"
#include "overlay_rule.h"
#include "scan.h"
#include "wave_ops.h"

namespace xrit {
namespace {

constexpr unsigned WAVES = 4;
constexpr unsigned THREADS = 64 * WAVES;
constexpr unsigned MAX_GROUPS = 2048;               // 8 workgroups of 4 waves on each of 256 CUs

// ---- map ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS) overlay_map_kernel(GeoNav nav, const double *__restrict__ quads, uint32_t n,
                                                              xrit_geo_point *__restrict__ points)
{
    for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < n; i += gridDim.x * THREADS) {
        const double *q = quads + (size_t)i * 4;
        points[i] = geo_point(q[0], q[1], q[2], q[3], nav);
    }
}

// ---- draw --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void stamp_or(const OverlayDraw &d, const OverlayStamp &st)
{
    const uint32_t bits = 0x01010101u << d.layer;
    for (uint32_t y = st.y0; y <= st.y1; ++y) {
        uint32_t *row = reinterpret_cast<uint32_t *>(d.mask + (size_t)y * d.pitch);
        for (uint32_t w = st.x0 >> 2; w <= st.x1 >> 2; ++w) {
            const uint32_t lo = st.x0 > 4 * w ? st.x0 - 4 * w : 0u, hi = st.x1 < 4 * w + 3 ? st.x1 - 4 * w : 3u;
            const uint32_t v = bits & (0xFFFFFFFFu << (8 * lo)) & (0xFFFFFFFFu >> (8 * (3 - hi)));
            if ((__hip_atomic_load(&row[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & v) != v) atomicOr(&row[w], v);
        }
    }
}

// a pair's part of the summary, kept in registers over a lane's pairs
struct Tally {
    uint32_t segments = 0, hidden = 0, jumps = 0, outside = 0, drawn = 0;
    unsigned long long steps = 0;
    __device__ void add(const OverlaySeg &s, bool touched)
    {
        hidden += s.kind == OVERLAY_HIDDEN;
        segments += s.kind != OVERLAY_HIDDEN;
        jumps += s.kind == OVERLAY_JUMP;
        if (s.kind != OVERLAY_DRAWN) return;
        ++drawn;
        outside += !touched;
        steps += s.steps;
    }
};

// all threads of the workgroup: the tallies into the summary (zeroed in front of the launch), its other fields by one thread
__device__ void tally_commit(const Tally &t, const OverlayDraw &d, xrit_overlay_draw_summary *summary)
{
    __shared__ unsigned long long s_sum[6];
    const unsigned tid = threadIdx.x, lane = tid & 63;
    if (tid < 6) s_sum[tid] = 0;
    __syncthreads();
    const unsigned long long v[6] = {wave_sum((unsigned long long)t.segments), wave_sum((unsigned long long)t.hidden),
                                     wave_sum((unsigned long long)t.jumps),    wave_sum((unsigned long long)t.outside),
                                     wave_sum((unsigned long long)t.drawn),    wave_sum(t.steps)};
    if (lane == 0) {
#pragma unroll
        for (unsigned k = 0; k < 6; ++k)
            if (v[k]) atomicAdd(&s_sum[k], v[k]);
    }
    __syncthreads();
    if (tid < 6 && s_sum[tid]) atomicAdd(reinterpret_cast<unsigned long long *>(&summary->segments) + tid, s_sum[tid]);
    if (blockIdx.x == 0 && tid == 0) {
        summary->vertices = d.n;
        summary->layer = d.layer;
        summary->width = d.width;
    }
}

__global__ void __launch_bounds__(THREADS) overlay_walk_kernel(OverlayDraw d, uint32_t pairs, xrit_overlay_draw_summary *summary)
{
    Tally t;
    for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < pairs; i += gridDim.x * THREADS) {
        const OverlaySeg s = overlay_setup(d.points[i], d.points[i + 1], d.width, d.max_jump, d.columns, d.rows);
        bool touched = false;
        if (s.kind == OVERLAY_DRAWN) {
            for (uint32_t k = 0; k < s.steps; ++k) {
                int64_t px, py;
                overlay_step_pixel(s, k, px, py);
                OverlayStamp st;
                if (overlay_stamp(px, py, d.width, d.columns, d.rows, st)) {
                    touched = true;
                    stamp_or(d, st);
                }
            }
        }
        t.add(s, touched);
    }
    tally_commit(t, d, summary);
}

// steps[i] for i < pairs; steps[pairs] = 0, so that the exclusive scan leaves the total there
__global__ void __launch_bounds__(THREADS) overlay_count_kernel(OverlayDraw d, uint32_t pairs, unsigned long long *steps,
                                                                xrit_overlay_draw_summary *summary)
{
    Tally t;
    for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i <= pairs; i += gridDim.x * THREADS) {
        if (i == pairs) {
            steps[i] = 0;
            continue;
        }
        const OverlaySeg s = overlay_setup(d.points[i], d.points[i + 1], d.width, d.max_jump, d.columns, d.rows);
        steps[i] = s.kind == OVERLAY_DRAWN ? s.steps : 0u;
        t.add(s, s.kind == OVERLAY_DRAWN && overlay_touches(s, d.width, d.columns, d.rows));
    }
    tally_commit(t, d, summary);
}

struct StepsF {
    typedef unsigned long long T;
    unsigned long long *a;
    __device__ T identity() const { return 0; }
    __device__ T combine(const T &lo, const T &hi) const { return lo + hi; }
    __device__ T reduce_run(long long i0, int cnt) const
    {
        T m = 0;
        for (int k = 0; k < cnt; ++k) m += a[i0 + k];
        return m;
    }
    __device__ void apply_run(long long i0, int cnt, const T &pre) const
    {
        T p = pre;
        for (int k = 0; k < cnt; ++k) {
            const T e = a[i0 + k];
            a[i0 + k] = p;
            p += e;
        }
    }
};

// prefix[i]: the steps in front of pair i, prefix[pairs]: all.  Step t belongs to the last pair whose prefix is <= t (the
// pairs without steps in front of it share that prefix and are passed over).
__global__ void __launch_bounds__(THREADS) overlay_step_kernel(OverlayDraw d, uint32_t pairs, const unsigned long long *__restrict__ prefix)
{
    const unsigned long long total = prefix[pairs];
    for (unsigned long long t = (unsigned long long)blockIdx.x * THREADS + threadIdx.x; t < total; t += (unsigned long long)gridDim.x * THREADS) {
        uint32_t lo = 0, hi = pairs;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (prefix[mid] <= t) lo = mid;
            else hi = mid;
        }
        const OverlaySeg s = overlay_setup(d.points[lo], d.points[lo + 1], d.width, d.max_jump, d.columns, d.rows);
        const unsigned long long k = t - prefix[lo];
        if (s.kind != OVERLAY_DRAWN || k >= s.steps) continue;      // (cannot happen: the prefix was made from the same set-up)
        int64_t px, py;
        overlay_step_pixel(s, (uint32_t)k, px, py);
        OverlayStamp st;
        if (overlay_stamp(px, py, d.width, d.columns, d.rows, st)) stamp_or(d, st);
    }
}

size_t scan_aggs_count(long long n)
{
    const size_t nb = scan_blocks(n);
    return nb + scan_blocks((long long)nb) + 2;
}

// ---- blend -------------------------------------------------------------------------------------------------------------
template <unsigned CIN, unsigned COUT>
__global__ void __launch_bounds__(THREADS) overlay_blend_kernel(OverlayBlend b, xrit_overlay_blend_summary *summary)
{
    __shared__ uint32_t s_layer[8];
    const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 8) s_layer[tid] = 0;
    __syncthreads();
    uint32_t count[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // this lane's covered pixels by top layer, over all its rows (at most 2^31 pixels a call)
    for (unsigned long long r = (unsigned long long)blockIdx.x * WAVES + w; r < b.rows; r += (unsigned long long)gridDim.x * WAVES) {
        const unsigned char *src = b.pixels + r * b.pitch, *msk = b.mask + r * b.mask_pitch;
        unsigned char *out = b.out + r * b.out_pitch;
        const bool aligned = (((uintptr_t)src | (uintptr_t)msk | (uintptr_t)out) & 15u) == 0;
        const uint32_t groups = aligned ? b.columns / 16 : 0;
        for (uint32_t g = lane; g < groups; g += 64) {
            const uint4 mq = reinterpret_cast<const uint4 *>(msk)[g];
            const uint32_t mw[4] = {mq.x, mq.y, mq.z, mq.w};
            uint32_t sw[4 * CIN], ow[4 * COUT];
            unsigned long long packed = 0;          // the group's covered pixels by top layer, a byte each (at most 16)
#pragma unroll
            for (unsigned k = 0; k < CIN; ++k) {
                const uint4 q = reinterpret_cast<const uint4 *>(src)[(size_t)g * CIN + k];
                sw[4 * k] = q.x, sw[4 * k + 1] = q.y, sw[4 * k + 2] = q.z, sw[4 * k + 3] = q.w;
            }
#pragma unroll
            for (unsigned k = 0; k < 4 * COUT; ++k) ow[k] = CIN == COUT ? sw[k % (4 * CIN)] : 0u;
            // Lines are thin: most groups have no mask bit, and their output is the source (overlay_blend_pixel's m == 0) --
            // the words as they are, or the grey bytes three times -- without the per-pixel arithmetic.
            if ((mw[0] | mw[1] | mw[2] | mw[3]) == 0) {
                if (CIN != COUT) {
#pragma unroll
                    for (unsigned p = 0; p < 16; ++p) {
                        const uint32_t v = (sw[p >> 2] >> (8 * (p & 3))) & 255u;
#pragma unroll
                        for (unsigned c = 0; c < COUT; ++c) ow[(p * COUT + c) >> 2] |= v << (8 * ((p * COUT + c) & 3));
                    }
                }
            } else {
#pragma unroll
                for (unsigned k = 0; k < 4 * COUT; ++k) ow[k] = 0;
#pragma unroll
                for (unsigned p = 0; p < 16; ++p) {
                    const uint32_t m = (mw[p >> 2] >> (8 * (p & 3))) & 255u;
                    uint32_t s[CIN], o[COUT];
#pragma unroll
                    for (unsigned c = 0; c < CIN; ++c) s[c] = (sw[(p * CIN + c) >> 2] >> (8 * ((p * CIN + c) & 3))) & 255u;
                    overlay_blend_pixel(s, CIN, m, b.styles, o, COUT);
                    packed += (unsigned long long)(m != 0) << (8 * (31 - __clz(m | 1u)));
#pragma unroll
                    for (unsigned c = 0; c < COUT; ++c) ow[(p * COUT + c) >> 2] |= o[c] << (8 * ((p * COUT + c) & 3));
                }
            }
#pragma unroll
            for (unsigned k = 0; k < 8; ++k) count[k] += (uint32_t)(packed >> (8 * k)) & 255u;
#pragma unroll
            for (unsigned k = 0; k < COUT; ++k)
                reinterpret_cast<uint4 *>(out)[(size_t)g * COUT + k] = make_uint4(ow[4 * k], ow[4 * k + 1], ow[4 * k + 2], ow[4 * k + 3]);
        }
        for (uint32_t x = groups * 16 + lane; x < b.columns; x += 64) {
            const uint32_t m = msk[x];
            uint32_t s[CIN], o[COUT];
#pragma unroll
            for (unsigned c = 0; c < CIN; ++c) s[c] = src[(size_t)x * CIN + c];
            overlay_blend_pixel(s, CIN, m, b.styles, o, COUT);
#pragma unroll
            for (unsigned k = 0; k < 8; ++k) count[k] += m != 0 && overlay_top(m) == k;
#pragma unroll
            for (unsigned c = 0; c < COUT; ++c) out[(size_t)x * COUT + c] = (unsigned char)o[c];
        }
    }
#pragma unroll
    for (unsigned k = 0; k < 8; ++k) {
        const uint32_t n = wave_sum(count[k]);
        if (lane == 0 && n) atomicAdd(&s_layer[k], n);
    }
    __syncthreads();
    if (tid < 8 && s_layer[tid]) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&summary->by_layer[tid]), (unsigned long long)s_layer[tid]);
        atomicAdd(reinterpret_cast<unsigned long long *>(&summary->covered), (unsigned long long)s_layer[tid]);
    }
    if (blockIdx.x == 0 && tid == 0) {
        summary->pixels = (uint64_t)b.columns * b.rows;
        summary->columns = b.columns;
        summary->rows = b.rows;
        summary->components_in = CIN;
        summary->components_out = COUT;
    }
}

unsigned groups_for(unsigned long long items)
{
    const unsigned long long g = (items + THREADS - 1) / THREADS;
    return (unsigned)(g < 1 ? 1 : g < MAX_GROUPS ? g : MAX_GROUPS);
}

}  // namespace

size_t overlay_scratch_carve(void *p, size_t n, OverlayScratch &sc)
{
    Carver c{static_cast<char *>(p)};
    sc.prefix = c.take<unsigned long long>(n ? n : 1, 256);
    sc.aggs = c.take<unsigned long long>(scan_aggs_count((long long)(n ? n : 1)), 256);
    return c.used();
}

int launch_overlay_map(const xrit_geo_nav &nav, const double *quads, size_t n, xrit_geo_point *points, hipStream_t s)
{
    if (!n) return XRIT_OK;
    hipLaunchKernelGGL(overlay_map_kernel, dim3(groups_for(n)), dim3(THREADS), 0, s, geo_nav_of(nav), quads, (uint32_t)n, points);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_overlay_draw(const OverlayDraw &d, uint32_t form, uint32_t clear, const OverlayScratch &sc, xrit_overlay_draw_summary *summary,
                        hipStream_t s)
{
    XR_HIP(hipMemsetAsync(summary, 0, sizeof *summary, s));
    if (clear) XR_HIP(hipMemsetAsync(d.mask, 0, (size_t)d.rows * d.pitch, s));
    const uint32_t pairs = d.n ? d.n - 1 : 0;       // (none: the kernels still write the summary)
    if (form == 0) {
        hipLaunchKernelGGL(overlay_walk_kernel, dim3(groups_for(pairs)), dim3(THREADS), 0, s, d, pairs, summary);
        XR_HIP(hipGetLastError());
        return XRIT_OK;
    }
    hipLaunchKernelGGL(overlay_count_kernel, dim3(groups_for((unsigned long long)pairs + 1)), dim3(THREADS), 0, s, d, pairs, sc.prefix, summary);
    XR_HIP(hipGetLastError());
    if (!pairs) return XRIT_OK;
    const StepsF f{sc.prefix};
    const long long m = (long long)pairs + 1;
    const int nb = scan_blocks(m);
    hipLaunchKernelGGL(scan_reduce_kernel<StepsF>, dim3(nb), dim3(SCAN_BLOCK), 0, s, f, m, sc.aggs);
    XR_HIP(hipGetLastError());
    scan_aggs_launch(f, sc.aggs, nb, s);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(scan_apply_kernel<StepsF>, dim3(nb), dim3(SCAN_BLOCK), 0, s, f, m, sc.aggs);
    XR_HIP(hipGetLastError());
    // the grid for what the steps can be at most; it strides over what they are
    const unsigned long long most = (unsigned long long)pairs * ((d.columns > d.rows ? d.columns : d.rows) + d.width + 1);
    hipLaunchKernelGGL(overlay_step_kernel, dim3(groups_for(most)), dim3(THREADS), 0, s, d, pairs, sc.prefix);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_overlay_blend(const OverlayBlend &b, xrit_overlay_blend_summary *summary, hipStream_t s)
{
    XR_HIP(hipMemsetAsync(summary, 0, sizeof *summary, s));
    const dim3 grid(groups_for((unsigned long long)b.rows * 64)), block(THREADS);
    if (b.cin == 1 && b.cout == 1) hipLaunchKernelGGL((overlay_blend_kernel<1, 1>), grid, block, 0, s, b, summary);
    else if (b.cin == 1) hipLaunchKernelGGL((overlay_blend_kernel<1, 3>), grid, block, 0, s, b, summary);
    else hipLaunchKernelGGL((overlay_blend_kernel<3, 3>), grid, block, 0, s, b, summary);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
