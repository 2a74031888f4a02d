// overlay_rule.h -- the map overlay stage's rules per value (include/xritdemod_amd.h, "Map overlay"; DESIGN.md section 28;
// tests/overlay_spec.py states the same in Python integers) as one set of functions for the device (overlay.hip: the
// count, draw and blend kernels all call these, so the two forms of the draw cannot drift apart) and for the host
// (overlay_host_check.cpp replays a table recorded from the specification through them).
// Everything is integer arithmetic.  A vertex is kept only with |qx|, |qy| < 2^29 (overlay_is_break), so that every
// difference is below 2^30 and every product formed here below 2^61: that test stands in front of every index.
#pragma once

#include <cstdint>

#include "../../include/xritdemod_amd.h"

#if defined(__HIPCC__)
#define XRIT_HD __host__ __device__
#else
#define XRIT_HD
#endif

namespace xrit {

constexpr int32_t OVERLAY_BREAK = INT32_MIN;        // both members of a break
constexpr int32_t OVERLAY_LIMIT = 1 << 29;          // a vertex at or above it in magnitude counts as a break
constexpr uint32_t OVERLAY_MAX_DIM = 16384;
constexpr uint32_t OVERLAY_MAX_WIDTH = 8;

XRIT_HD inline bool overlay_is_break(const xrit_geo_point &p)
{
    return !(p.qx > -OVERLAY_LIMIT && p.qx < OVERLAY_LIMIT && p.qy > -OVERLAY_LIMIT && p.qy < OVERLAY_LIMIT);
}

// floor(n / d) for d > 0
XRIT_HD inline int64_t overlay_floor_div(int64_t n, int64_t d)
{
    const int64_t q = n / d;
    return (n % d < 0) ? q - 1 : q;
}

// the pixel of a position in 1/256 pixel: centres at multiples of 256, ties upwards
XRIT_HD inline int64_t overlay_pixel(int64_t q) { return (q + 128) >> 8; }

// a stamp of width w reaches from -before to +behind of its pixel, in both directions
XRIT_HD inline int64_t overlay_before(uint32_t w) { return (int64_t)((w - 1) / 2); }
XRIT_HD inline int64_t overlay_behind(uint32_t w) { return (int64_t)(w / 2); }

enum OverlayKind : uint32_t { OVERLAY_HIDDEN = 0, OVERLAY_JUMP = 1, OVERLAY_DRAWN = 2 };

// What a pair of vertices comes to.  For OVERLAY_DRAWN: the ends in (major, minor) coordinates ordered by the major one,
// the walk's m = m0 .. m0 + line - 1 (already cut to what a stamp can reach inside the image along the major axis) and
// steps = 2 + line: step 0 and 1 are the stamps of the two ends as given, step k >= 2 the walk's m = m0 + k - 2.
struct OverlaySeg {
    uint32_t kind;
    uint32_t xmajor;
    int64_t a0, b0, da, db;                         // da = a1 - a0 >= 0, db = b1 - b0
    int64_t m0;
    uint32_t line;
    uint32_t steps;
    int64_t ex0, ey0, ex1, ey1;                     // the end pixels (scalars: an index would put them in scratch memory)
};

XRIT_HD inline OverlaySeg overlay_setup(const xrit_geo_point &p0, const xrit_geo_point &p1, uint32_t width, uint32_t max_jump, uint32_t columns,
                                        uint32_t rows)
{
    OverlaySeg s{};
    if (overlay_is_break(p0) || overlay_is_break(p1)) return s;
    const int64_t x0 = p0.qx, y0 = p0.qy, x1 = p1.qx, y1 = p1.qy;
    const int64_t dx = x1 - x0, dy = y1 - y0;
    const int64_t adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    if (max_jump && (adx > (int64_t)max_jump || ady > (int64_t)max_jump)) {
        s.kind = OVERLAY_JUMP;
        return s;
    }
    s.kind = OVERLAY_DRAWN;
    s.ex0 = overlay_pixel(x0), s.ey0 = overlay_pixel(y0);
    s.ex1 = overlay_pixel(x1), s.ey1 = overlay_pixel(y1);
    s.xmajor = adx >= ady;
    int64_t a0 = s.xmajor ? x0 : y0, b0 = s.xmajor ? y0 : x0, a1 = s.xmajor ? x1 : y1, b1 = s.xmajor ? y1 : x1;
    if (a0 > a1) {
        int64_t t = a0; a0 = a1; a1 = t;
        t = b0; b0 = b1; b1 = t;
    }
    s.a0 = a0, s.b0 = b0, s.da = a1 - a0, s.db = b1 - b0;
    s.steps = 2;
    if (s.da == 0) return s;
    // 256 m in a0 .. a1, and a stamp at m reaches pixels m - before .. m + behind: inside 0 .. dim - 1 for some of them
    const int64_t dim = s.xmajor ? columns : rows;
    int64_t lo = -overlay_floor_div(-a0, 256), hi = overlay_floor_div(a1, 256);
    const int64_t first = -overlay_behind(width), last = dim - 1 + overlay_before(width);
    if (lo < first) lo = first;
    if (hi > last) hi = last;
    if (hi >= lo) {
        s.m0 = lo;
        s.line = (uint32_t)(hi - lo + 1);
        s.steps += s.line;
    }
    return s;
}

// the minor coordinate (1/256 pixel) of the walk at m
XRIT_HD inline int64_t overlay_minor(const OverlaySeg &s, int64_t m)
{
    return s.b0 + overlay_floor_div(2 * (256 * m - s.a0) * s.db + s.da, 2 * s.da);
}

// the pixel that step k of a drawn segment stamps
XRIT_HD inline void overlay_step_pixel(const OverlaySeg &s, uint32_t k, int64_t &px, int64_t &py)
{
    if (k < 2) {
        px = k ? s.ex1 : s.ex0, py = k ? s.ey1 : s.ey0;
        return;
    }
    const int64_t m = s.m0 + (int64_t)(k - 2), p = overlay_pixel(overlay_minor(s, m));
    px = s.xmajor ? m : p;
    py = s.xmajor ? p : m;
}

// the part of a stamp inside the image: columns x0 .. x1 of rows y0 .. y1; false when there is none
struct OverlayStamp {
    uint32_t x0, x1, y0, y1;
};

XRIT_HD inline bool overlay_stamp(int64_t px, int64_t py, uint32_t width, uint32_t columns, uint32_t rows, OverlayStamp &st)
{
    int64_t x0 = px - overlay_before(width), x1 = px + overlay_behind(width), y0 = py - overlay_before(width), y1 = py + overlay_behind(width);
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > (int64_t)columns - 1) x1 = (int64_t)columns - 1;
    if (y1 > (int64_t)rows - 1) y1 = (int64_t)rows - 1;
    if (x1 < x0 || y1 < y0) return false;
    st = OverlayStamp{(uint32_t)x0, (uint32_t)x1, (uint32_t)y0, (uint32_t)y1};
    return true;
}

// Whether any stamp of a drawn segment touches the image, without the walk.  The walk is already cut along the major
// axis, so a stamp of it touches iff its minor pixel lies in -behind .. dim_minor - 1 + before.  The minor pixel is
// monotone in m and moves by at most one pixel per step (|db| <= da), and that band is at least one pixel wide: the walk
// misses it only when its first and last pixel lie on the same side of it.
XRIT_HD inline bool overlay_touches(const OverlaySeg &s, uint32_t width, uint32_t columns, uint32_t rows)
{
    OverlayStamp st;
    if (overlay_stamp(s.ex0, s.ey0, width, columns, rows, st) || overlay_stamp(s.ex1, s.ey1, width, columns, rows, st)) return true;
    if (!s.line) return false;
    const int64_t dim = s.xmajor ? rows : columns;
    const int64_t first = -overlay_behind(width), last = dim - 1 + overlay_before(width);
    const int64_t pa = overlay_pixel(overlay_minor(s, s.m0)), pb = overlay_pixel(overlay_minor(s, s.m0 + (int64_t)s.line - 1));
    const int64_t mn = pa < pb ? pa : pb, mx = pa < pb ? pb : pa;
    return mn <= last && mx >= first;
}

// ---- blend ------------------------------------------------------------------------------------------------------------
XRIT_HD inline uint32_t overlay_luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }
XRIT_HD inline uint32_t overlay_mix(uint32_t src, uint32_t c, uint32_t alpha) { return (src * (255u - alpha) + c * alpha + 127u) / 255u; }

// the top layer of a mask byte != 0
XRIT_HD inline uint32_t overlay_top(uint32_t m)
{
    uint32_t k = 0;
    while (m >>= 1) ++k;
    return k;
}

// One pixel: src[0 .. cin) -> out[0 .. cout) under mask byte m.  style_k: r | g << 8 | b << 16 | alpha << 24.
XRIT_HD inline void overlay_blend_pixel(const uint32_t *src, uint32_t cin, uint32_t m, const uint32_t *styles, uint32_t *out, uint32_t cout)
{
    uint32_t s3[3];
    s3[0] = src[0], s3[1] = cin == 3 ? src[1] : src[0], s3[2] = cin == 3 ? src[2] : src[0];
    if (!m) {
        for (uint32_t c = 0; c < cout; ++c) out[c] = s3[c];
        return;
    }
    const uint32_t st = styles[overlay_top(m)];
    const uint32_t r = st & 255u, g = (st >> 8) & 255u, b = (st >> 16) & 255u, alpha = st >> 24;
    if (cout == 1) {
        out[0] = overlay_mix(s3[0], overlay_luma(r, g, b), alpha);
        return;
    }
    out[0] = overlay_mix(s3[0], r, alpha);
    out[1] = overlay_mix(s3[1], g, alpha);
    out[2] = overlay_mix(s3[2], b, alpha);
}

}  // namespace xrit
