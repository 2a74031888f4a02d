// geo.hip -- the kernels of the projection stage (include/xritdemod_amd.h, "Image projection"), all
// three one template over geo_rule.h's functions:
//   GEO_MAP       the map of the grid: a map entry per output pixel
//   GEO_RESAMPLE  a stored map applied to an image
//   GEO_FUSED     the entry computed and applied at once, never stored
// A wave covers a run of 256 columns of one output row, so the row's A and B are the same in every lane; a lane takes four
// adjacent columns: C and S as 32-byte runs, its four map entries as two 16-byte stores, its four one-byte outputs as one
// dword (two-byte: one 8-byte store) where the address allows.  The gather is not staged: neighbouring output pixels read
// neighbouring source pixels along a slowly curving line.  The grid is at most MAX_GROUPS workgroups striding over the
// runs: the summary's counts are kept in registers over a wave's runs, summed per workgroup in LDS and added with at most
// four global atomics per workgroup (one set per run made the kernels wait on those four addresses: the resample of
// 5424 x 5424 outputs took 0.38 ms, and takes 0.14 ms this way); integer sums do not depend on the order.
#include "common.h"
#include "geo_rule.h"
#include "kernels.h"
#include "wave_ops.h"

namespace xrit {
namespace {

constexpr unsigned WAVES = 4;
constexpr unsigned THREADS = 64 * WAVES;
constexpr unsigned PER_LANE = 4;
constexpr unsigned RUN = 64 * PER_LANE;             // columns of a wave
constexpr unsigned MAX_GROUPS = 2048;               // 8 workgroups of 4 waves on each of 256 CUs

enum GeoKind { GEO_MAP, GEO_RESAMPLE, GEO_FUSED };

struct GeoSource {
    const unsigned char *pixels;
    uint32_t columns, rows, pitch;
};

template <unsigned W> __device__ __forceinline__ uint32_t geo_fetch(const GeoSource &src, uint32_t x, uint32_t y)
{
    const unsigned char *p = src.pixels + (size_t)y * src.pitch + (size_t)x * W;
    if (W == 1) return *p;
    return *reinterpret_cast<const uint16_t *>(p);
}

template <unsigned W, int KIND>
__global__ void __launch_bounds__(THREADS) geo_kernel(GeoTables t, GeoNav nav, GeoSource src, const xrit_geo_point *__restrict__ map_in,
                                                       xrit_geo_point *__restrict__ map_out, uint32_t mode, unsigned char *__restrict__ out,
                                                       uint32_t out_pitch, xrit_geo_summary *summary, uint32_t runs, uint32_t items)
{
    __shared__ uint32_t s_count[4];
    const unsigned tid = threadIdx.x, lane = tid & 63;
    if (KIND != GEO_MAP) {
        if (tid < 4) s_count[tid] = 0;
        __syncthreads();
    }
    // a wave's items, the grid striding over them: the same in every lane, so the row's A and B are scalar loads
    const uint32_t first = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES + (tid >> 6));
    uint32_t count[4] = {0, 0, 0, 0};
    for (uint32_t item = first; item < items; item += gridDim.x * WAVES) {
        const uint32_t i = item / runs, j0 = (item - i * runs) * RUN + lane * PER_LANE;
        if (j0 < t.columns) {
            const uint32_t m = t.columns - j0 < PER_LANE ? t.columns - j0 : PER_LANE;
            const size_t at = (size_t)i * t.columns + j0;
            xrit_geo_point p[PER_LANE];
            if (KIND == GEO_RESAMPLE) {
                const xrit_geo_point *q = map_in + at;
                if (m == PER_LANE && ((uintptr_t)q & 15u) == 0) {
                    const int4 a = reinterpret_cast<const int4 *>(q)[0], b = reinterpret_cast<const int4 *>(q)[1];
                    p[0] = {a.x, a.y};
                    p[1] = {a.z, a.w};
                    p[2] = {b.x, b.y};
                    p[3] = {b.z, b.w};
                } else {
#pragma unroll
                    for (unsigned k = 0; k < PER_LANE; ++k) p[k] = k < m ? q[k] : xrit_geo_point{GEO_OFF, GEO_OFF};
                }
            } else {
                const double A = t.A[i], B = t.B[i];
                double C[PER_LANE], S[PER_LANE];
                if (m == PER_LANE) {                // the tables are the handle's: 32-byte aligned at j0, a multiple of 4
                    const double4 c = *reinterpret_cast<const double4 *>(t.C + j0), s = *reinterpret_cast<const double4 *>(t.S + j0);
                    C[0] = c.x, C[1] = c.y, C[2] = c.z, C[3] = c.w;
                    S[0] = s.x, S[1] = s.y, S[2] = s.z, S[3] = s.w;
                } else {
#pragma unroll
                    for (unsigned k = 0; k < PER_LANE; ++k) {
                        C[k] = k < m ? t.C[j0 + k] : 0.0;
                        S[k] = k < m ? t.S[j0 + k] : 0.0;
                    }
                }
#pragma unroll
                for (unsigned k = 0; k < PER_LANE; ++k) p[k] = geo_point(A, B, C[k], S[k], nav);
            }
            if (KIND == GEO_MAP) {
                xrit_geo_point *q = map_out + at;
                if (m == PER_LANE && ((uintptr_t)q & 15u) == 0) {
                    reinterpret_cast<int4 *>(q)[0] = make_int4(p[0].qx, p[0].qy, p[1].qx, p[1].qy);
                    reinterpret_cast<int4 *>(q)[1] = make_int4(p[2].qx, p[2].qy, p[3].qx, p[3].qy);
                } else {
#pragma unroll
                    for (unsigned k = 0; k < PER_LANE; ++k)
                        if (k < m) q[k] = p[k];
                }
            } else {
                uint32_t v[PER_LANE];
#pragma unroll
                for (unsigned k = 0; k < PER_LANE; ++k) {
                    GeoClass cls = GEO_OFF_DISC;
                    v[k] = geo_sample(p[k], mode, src.columns, src.rows, [&](uint32_t x, uint32_t y) { return geo_fetch<W>(src, x, y); }, cls);
                    if (k < m) {
#pragma unroll
                        for (unsigned c = 0; c < 4; ++c) count[c] += cls == c;
                    }
                }
                unsigned char *o = out + (size_t)i * out_pitch + (size_t)j0 * W;
                if (W == 1 && m == PER_LANE && ((uintptr_t)o & 3u) == 0) {
                    *reinterpret_cast<uint32_t *>(o) = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
                } else if (W == 2 && m == PER_LANE && ((uintptr_t)o & 7u) == 0) {
                    *reinterpret_cast<uint2 *>(o) = make_uint2(v[0] | v[1] << 16, v[2] | v[3] << 16);
                } else {
#pragma unroll
                    for (unsigned k = 0; k < PER_LANE; ++k) {
                        if (k >= m) continue;
                        if (W == 1) o[k] = (unsigned char)v[k];
                        else reinterpret_cast<uint16_t *>(o)[k] = (uint16_t)v[k];
                    }
                }
            }
        }
    }
    if (KIND != GEO_MAP) {
#pragma unroll
        for (unsigned c = 0; c < 4; ++c) {
            const uint32_t n = wave_sum(count[c]);
            if (lane == 0 && n) atomicAdd(&s_count[c], n);
        }
        __syncthreads();
        if (tid < 4 && s_count[tid]) {
            unsigned long long *dst = reinterpret_cast<unsigned long long *>(&summary->off_disc) + tid;
            atomicAdd(dst, (unsigned long long)s_count[tid]);
        }
        if (blockIdx.x == 0 && tid == 0) {          // the fields that are not sums (zeroed in front of the launch like the rest)
            summary->total = (uint64_t)t.columns * t.rows;
            summary->columns = t.columns;
            summary->rows = t.rows;
            summary->width = W;
            summary->mode = mode;
        }
    }
}

template <int KIND>
int geo_launch(const GeoTables &t, const GeoNav &nav, const xrit_product_image *im, const xrit_geo_point *map_in, xrit_geo_point *map_out,
               uint32_t mode, unsigned char *out, uint32_t out_pitch, xrit_geo_summary *summary, hipStream_t s)
{
    const uint32_t runs = div_up(t.columns, RUN), items = runs * t.rows;          // at most 64 * 16384
    const unsigned groups = div_up(items, WAVES);
    const dim3 grid(groups < MAX_GROUPS ? groups : MAX_GROUPS), block(THREADS);
    GeoSource src{};
    if (im) src = GeoSource{im->d_pixels, im->columns, im->rows, im->pitch};
    if (KIND != GEO_MAP) XR_HIP(hipMemsetAsync(summary, 0, sizeof *summary, s));
    if (im && geo_width(im->bits) == 2)
        hipLaunchKernelGGL((geo_kernel<2, KIND>), grid, block, 0, s, t, nav, src, map_in, map_out, mode, out, out_pitch, summary, runs, items);
    else
        hipLaunchKernelGGL((geo_kernel<1, KIND>), grid, block, 0, s, t, nav, src, map_in, map_out, mode, out, out_pitch, summary, runs, items);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace

int launch_geo_map(const GeoTables &t, const xrit_geo_nav &nav, xrit_geo_point *map, hipStream_t s)
{
    return geo_launch<GEO_MAP>(t, geo_nav_of(nav), nullptr, nullptr, map, 0, nullptr, 0, nullptr, s);
}

int launch_geo_resample(const GeoTables &t, const xrit_product_image &im, const xrit_geo_point *map, uint32_t mode, unsigned char *out,
                        uint32_t out_pitch, xrit_geo_summary *summary, hipStream_t s)
{
    return geo_launch<GEO_RESAMPLE>(t, GeoNav{}, &im, map, nullptr, mode, out, out_pitch, summary, s);
}

int launch_geo_project(const GeoTables &t, const xrit_geo_nav &nav, const xrit_product_image &im, uint32_t mode, unsigned char *out,
                       uint32_t out_pitch, xrit_geo_summary *summary, hipStream_t s)
{
    return geo_launch<GEO_FUSED>(t, geo_nav_of(nav), &im, nullptr, nullptr, mode, out, out_pitch, summary, s);
}

}  // namespace xrit
