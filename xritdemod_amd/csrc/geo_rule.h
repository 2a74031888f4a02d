// geo_rule.h -- the projection stage's rule per output pixel (include/xritdemod_amd.h, "Image projection"; DESIGN.md
// section 24; tests/geo_spec.py states the same in NumPy) as one set of functions for the device (geo.hip: the map, the
// resample and the fused kernel all call these, so the fused kernel cannot drift from the pair) and for the host
// (geo_host_check.cpp replays a table recorded from the specification through them).
// Everything is + - * / sqrt and floor in IEEE double in the order written; the build has -ffp-contract=off, so no
// multiply and add meet in an FMA, and / and sqrt on double are correctly rounded.  The arctangents are geo_atan_small: a
// fixed polynomial, no library call.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/xritdemod_amd.h"

#if defined(__HIPCC__)
#define XRIT_HD __host__ __device__
#else
#define XRIT_HD
#endif

namespace xrit {

// CGMS LRIT/HRIT Global Specification 4.4.3.2
constexpr double GEO_H = 42164.0;                   // km, the satellite from the earth's centre
constexpr double GEO_RPOL = 6356.5838;              // km
constexpr double GEO_FLAT = 0.993243;               // (rpol / req)^2, in front of tan(lat)
constexpr double GEO_E2 = 0.00675701;               // (req^2 - rpol^2) / req^2
constexpr double GEO_K = 1.006803;                  // (req / rpol)^2
constexpr double GEO_R2D = 57.29577951308232;
constexpr double GEO_LIMIT = 1073741824.0;          // 2^30: a source position in 1/256 pixel stays below it in magnitude
constexpr int32_t GEO_OFF = INT32_MIN;              // both members of a map entry off the disc

// what a call needs of xrit_geo_nav: fc = c0 + x * cs, fl = l0 + y * ls
struct GeoNav {
    double c0, cs, l0, ls;
};

XRIT_HD inline GeoNav geo_nav_of(const xrit_geo_nav &n)
{
    return GeoNav{(double)((int64_t)n.coff - n.origin), (double)n.cfac / 65536.0, (double)((int64_t)n.loff - n.origin), (double)n.lfac / 65536.0};
}

// atan(t) for |t| <= 0.2 (a visible point has |t| < 0.154): t * P(t^2), P the Horner form of the series' first ten terms
// from k = 9 down.  Within 1.2e-16 of atan there.
XRIT_HD inline double geo_atan_small(double t)
{
    const double z = t * t;
    double p = -(1.0 / 19.0);
    p = 1.0 / 17.0 + z * p;
    p = -(1.0 / 15.0) + z * p;
    p = 1.0 / 13.0 + z * p;
    p = -(1.0 / 11.0) + z * p;
    p = 1.0 / 9.0 + z * p;
    p = -(1.0 / 7.0) + z * p;
    p = 1.0 / 5.0 + z * p;
    p = -(1.0 / 3.0) + z * p;
    p = 1.0 + z * p;
    return t * p;
}

// fc (or fl) -> the position in 1/256 pixel; false where fc * 256 is not below 2^30 in magnitude (NaN included).  This
// test stands in front of every index the stage forms: its one out-of-bounds hazard.
XRIT_HD inline bool geo_quantise(double f, int32_t &q)
{
    const double s = f * 256.0;
    if (!(s < GEO_LIMIT && s > -GEO_LIMIT)) return false;
    q = (int32_t)::floor(s + 0.5);
    return true;
}

// the map entry of output pixel (i, j) from its row's A, B and its column's C, S
XRIT_HD inline xrit_geo_point geo_point(double A, double B, double C, double S, const GeoNav &nav)
{
    const xrit_geo_point off{GEO_OFF, GEO_OFF};
    const double ac = A * C;
    const double r1 = GEO_H - ac;
    const double r2 = -(A * S);
    const double r3 = B;
    const double r22 = r2 * r2;
    // (r1 > 0 holds for every real table, ac <= 6378.2: it keeps +inf or 1e300 in C from landing on the sub-satellite pixel)
    if (!(r1 > 0.0 && GEO_H * ac >= r22 + GEO_K * (r3 * r3))) return off;
    const double u = -r2 / r1;
    const double v = -r3 / ::sqrt(r1 * r1 + r22);
    const double x = geo_atan_small(u) * GEO_R2D;
    const double y = geo_atan_small(v) * GEO_R2D;
    xrit_geo_point p;
    if (!geo_quantise(nav.c0 + x * nav.cs, p.qx) || !geo_quantise(nav.l0 + y * nav.ls, p.qy)) return off;
    return p;
}

XRIT_HD inline bool geo_is_off(const xrit_geo_point &p) { return p.qx == GEO_OFF || p.qy == GEO_OFF; }

// what became of an output pixel: the summary's four counts
enum GeoClass : uint32_t { GEO_OFF_DISC = 0, GEO_OUTSIDE = 1, GEO_NO_DATA = 2, GEO_WRITTEN = 3 };

// The output sample of a map entry.  fetch(x, y) is the source sample at column x, line y, asked for only with
// 0 <= x < columns and 0 <= y < rows: a tap's coordinates are clamped into the image before the fetch and its value is
// dropped afterwards if the tap was outside, so that no branch stands between the taps' loads (on the device they are all
// in flight together).  A map entry handed in by a caller (xrit_geo_resample_device) may hold anything: the taps are
// formed in 64 bits.
template <class Fetch>
XRIT_HD inline uint32_t geo_sample(const xrit_geo_point &p, uint32_t mode, uint32_t columns, uint32_t rows, Fetch &&fetch, GeoClass &cls)
{
    const bool off = geo_is_off(p);
    const int64_t qx = p.qx, qy = p.qy, mx = (int64_t)columns - 1, my = (int64_t)rows - 1;
    auto tap = [&](int64_t x, int64_t y, bool &inside) -> uint32_t {
        inside = !off && x >= 0 && y >= 0 && x <= mx && y <= my;
        const uint32_t v = fetch((uint32_t)(x < 0 ? 0 : x > mx ? mx : x), (uint32_t)(y < 0 ? 0 : y > my ? my : y));
        return inside ? v : 0u;
    };
    if (mode == XRIT_GEO_NEAREST) {
        bool inside;
        const uint32_t v = tap((qx + 128) >> 8, (qy + 128) >> 8, inside);
        cls = off ? GEO_OFF_DISC : !inside ? GEO_OUTSIDE : v ? GEO_WRITTEN : GEO_NO_DATA;
        return v;
    }
    const int64_t x0 = qx >> 8, y0 = qy >> 8;
    const uint32_t fx = (uint32_t)(qx & 255), fy = (uint32_t)(qy & 255);
    bool in00, in10, in01, in11;
    const uint32_t v00 = tap(x0, y0, in00), v10 = tap(x0 + 1, y0, in10), v01 = tap(x0, y0 + 1, in01), v11 = tap(x0 + 1, y0 + 1, in11);
    // a tap of value 0 (no data, or outside) is left out of both sums
    const uint32_t w00 = v00 ? (256u - fx) * (256u - fy) : 0u, w10 = v10 ? fx * (256u - fy) : 0u;
    const uint32_t w01 = v01 ? (256u - fx) * fy : 0u, w11 = v11 ? fx * fy : 0u;
    const uint64_t W = (uint64_t)w00 + w10 + w01 + w11;
    const uint64_t V = (uint64_t)w00 * v00 + (uint64_t)w10 * v10 + (uint64_t)w01 * v01 + (uint64_t)w11 * v11;
    cls = off ? GEO_OFF_DISC : !(in00 || in10 || in01 || in11) ? GEO_OUTSIDE : W ? GEO_WRITTEN : GEO_NO_DATA;
    if (!W) return 0;
    if (W == 65536u) return (uint32_t)((2u * V + W) >> 17);    // all four taps kept: the same quotient without a 64-bit division
    return (uint32_t)((2u * V + W) / (2u * W));
}

XRIT_HD inline uint32_t geo_width(uint32_t bits) { return bits <= 8 ? 1u : 2u; }

}  // namespace xrit
