// overlay.cpp -- C ABI of the map overlay stage (include/xritdemod_amd.h, "Map overlay"): the handle owns the form, the
// scratch of form 1 and the host-buffer forms' staging; the host helpers (the quads and grid positions of longitudes and
// latitudes, densify, the graticule) are plain C++ on the C library; the kernels are in overlay.hip.
#include <cmath>
#include <cstddef>
#include <limits>

#include "common.h"
#include "geo_rule.h"
#include "kernels.h"
#include "overlay_rule.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_overlay_style) == 4, "xrit_overlay_style layout");
static_assert(sizeof(xrit_overlay_draw_summary) == 64 && offsetof(xrit_overlay_draw_summary, segments) == 8 &&
                  offsetof(xrit_overlay_draw_summary, steps) == 48 && offsetof(xrit_overlay_draw_summary, layer) == 56,
              "xrit_overlay_draw_summary layout (OVERLAY_DRAW_SUMMARY_DTYPE mirrors it; the kernels add to the six counts as one array)");
static_assert(sizeof(xrit_overlay_blend_summary) == 96 && offsetof(xrit_overlay_blend_summary, by_layer) == 16 &&
                  offsetof(xrit_overlay_blend_summary, columns) == 80,
              "xrit_overlay_blend_summary layout");
static_assert(XRIT_OVERLAY_MAX_DIM == OVERLAY_MAX_DIM && XRIT_OVERLAY_MAX_WIDTH == OVERLAY_MAX_WIDTH, "the header's bounds are the rule's");

namespace {
constexpr uint64_t MAX_PIXELS = (uint64_t)1 << 31;
constexpr double DEG = 3.141592653589793 / 180.0;
constexpr size_t STAGE_ALIGN = 256;
size_t padded(size_t bytes) { return (bytes + STAGE_ALIGN - 1) & ~(STAGE_ALIGN - 1); }
}  // namespace

struct xrit_overlay : StageHandle {
    DevBuf scratch;                                 // form 1: overlay_scratch_carve
    DevBuf h_in, h_out;                             // the host-buffer forms'
    DevBuf h_mask;                                  // the host-buffer draw's mask: kept for xrit_overlay_mask_device
    bool mask_drawn = false;
    uint32_t form = 1;
    void close_all() { close({&scratch, &h_in, &h_out, &h_mask}); }
};

int xrit_overlay_create(xrit_overlay **out, int device)
{
    return stage_create(out, device, [&](xrit_overlay &) { return XRIT_OK; });
}

int xrit_overlay_destroy(xrit_overlay *ov) { return stage_destroy(ov); }

int xrit_overlay_reset(xrit_overlay *ov)
{
    if (!ov) { set_error("null argument"); return XRIT_E_INVALID; }
    return ov->wait_last();
}

int xrit_overlay_set_form(xrit_overlay *ov, uint32_t form)
{
    if (!ov) { set_error("null argument"); return XRIT_E_INVALID; }
    if (form > 1) { set_error("overlay: form 0 (a lane per segment) or 1 (a lane per step)"); return XRIT_E_INVALID; }
    ov->form = form;
    return XRIT_OK;
}

// ---- the checks: pointers wherever they lie ------------------------------------------------------------------------------
static int check_map(const xrit_overlay *ov, const xrit_geo_nav *nav, const void *quads, size_t n, const void *points)
{
    if (!ov || !nav || (n && (!quads || !points))) { set_error("null argument"); return XRIT_E_INVALID; }
    if (n > XRIT_OVERLAY_MAX_VERTICES) { set_error("overlay: at most 2^26 vertices a call"); return XRIT_E_INVALID; }
    if (((size_t)quads | (size_t)points) & 7) { set_error("overlay: quads and points must be 8-byte aligned"); return XRIT_E_INVALID; }
    return XRIT_OK;
}

static int check_draw(const xrit_overlay *ov, const void *points, size_t n, uint32_t layer, uint32_t width, const void *mask, uint32_t columns,
                      uint32_t rows, uint32_t mask_pitch, const void *summary)
{
    if (!ov || (n && !points) || !mask || !summary) { set_error("null argument"); return XRIT_E_INVALID; }
    if (n > XRIT_OVERLAY_MAX_VERTICES) { set_error("overlay: at most 2^26 vertices a call"); return XRIT_E_INVALID; }
    if (layer >= XRIT_OVERLAY_LAYERS || width < 1 || width > XRIT_OVERLAY_MAX_WIDTH) {
        set_error("overlay: layer 0 .. 7, width 1 .. 8");
        return XRIT_E_INVALID;
    }
    if (columns < 1 || rows < 1 || columns > XRIT_OVERLAY_MAX_DIM || rows > XRIT_OVERLAY_MAX_DIM) {
        set_error("overlay: columns and rows 1 .. %d", XRIT_OVERLAY_MAX_DIM);
        return XRIT_E_INVALID;
    }
    if (mask_pitch < columns || (mask_pitch & 3) || ((size_t)mask & 3)) {
        set_error("overlay: mask_pitch >= columns and a multiple of 4, the mask 4-byte aligned");
        return XRIT_E_INVALID;
    }
    if (((size_t)points | (size_t)summary) & 7) { set_error("overlay: points and the summary must be 8-byte aligned"); return XRIT_E_INVALID; }
    return XRIT_OK;
}

static int check_blend(const xrit_overlay *ov, const xrit_product_image *im, uint32_t cin, const void *mask, uint32_t mask_pitch,
                       const xrit_overlay_style *styles, const void *out, uint32_t out_pitch, uint32_t cout, const void *summary)
{
    if (!ov || !im || !im->d_pixels || !mask || !styles || !out || !summary) { set_error("null argument"); return XRIT_E_INVALID; }
    if (im->bits != 8 || im->columns < 1 || im->rows < 1 || (uint64_t)im->columns * im->rows > MAX_PIXELS) {
        set_error("overlay: an image of 8 bits, columns, rows >= 1, columns * rows <= 2^31");
        return XRIT_E_INVALID;
    }
    if ((cin != 1 && cin != 3) || (cout != 1 && cout != 3) || cin > cout) {
        set_error("overlay: components 1 or 3, three in needs three out");
        return XRIT_E_INVALID;
    }
    if ((uint64_t)im->pitch < (uint64_t)im->columns * cin || (uint64_t)out_pitch < (uint64_t)im->columns * cout || mask_pitch < im->columns) {
        set_error("overlay: pitch >= columns * components_in, out_pitch >= columns * components_out, mask_pitch >= columns");
        return XRIT_E_INVALID;
    }
    if (out == im->d_pixels && (cin != cout || out_pitch != im->pitch)) {
        set_error("overlay: in place needs equal components and pitches");
        return XRIT_E_INVALID;
    }
    if ((size_t)summary & 7) { set_error("overlay: the summary must be 8-byte aligned"); return XRIT_E_INVALID; }
    return XRIT_OK;
}

static OverlayBlend blend_of(const xrit_product_image &im, uint32_t cin, const uint8_t *mask, uint32_t mask_pitch, const xrit_overlay_style *styles,
                             uint8_t *out, uint32_t out_pitch, uint32_t cout)
{
    OverlayBlend b{im.d_pixels, mask, out, im.columns, im.rows, im.pitch, mask_pitch, out_pitch, cin, cout, {}};
    for (int k = 0; k < XRIT_OVERLAY_LAYERS; ++k)
        b.styles[k] = (uint32_t)styles[k].r | (uint32_t)styles[k].g << 8 | (uint32_t)styles[k].b << 16 | (uint32_t)styles[k].alpha << 24;
    return b;
}

// the scratch of form 1 for n vertices: grown (with a wait for the call that may still use the old one) only when it is too small
static int scratch_for(xrit_overlay *ov, size_t n, OverlayScratch &sc)
{
    sc = OverlayScratch{};
    if (ov->form == 0) return XRIT_OK;
    const size_t need = overlay_scratch_carve(nullptr, n, sc);
    if (need > ov->scratch.bytes) {
        XR_TRY(ov->wait_last());
        XR_TRY(ov->scratch.reserve(need));
    }
    overlay_scratch_carve(ov->scratch.p, n, sc);
    return XRIT_OK;
}

// ---- device pointers -----------------------------------------------------------------------------------------------------
int xrit_overlay_map_device(xrit_overlay *ov, const xrit_geo_nav *nav, const double *d_quads, size_t n, xrit_geo_point *d_points, void *stream)
{
    XR_TRY(check_map(ov, nav, d_quads, n, d_points));
    XR_HIP(hipSetDevice(ov->device));
    XR_TRY(launch_overlay_map(*nav, d_quads, n, d_points, (hipStream_t)stream));
    ov->ran_on((hipStream_t)stream);
    return XRIT_OK;
}

int xrit_overlay_draw_device(xrit_overlay *ov, const xrit_geo_point *d_points, size_t n, uint32_t layer, uint32_t width, uint32_t max_jump,
                             uint8_t *d_mask, uint32_t columns, uint32_t rows, uint32_t mask_pitch, uint32_t clear,
                             xrit_overlay_draw_summary *d_summary, void *stream)
{
    XR_TRY(check_draw(ov, d_points, n, layer, width, d_mask, columns, rows, mask_pitch, d_summary));
    XR_HIP(hipSetDevice(ov->device));
    OverlayScratch sc;
    XR_TRY(scratch_for(ov, n, sc));
    const OverlayDraw d{d_points, (uint32_t)n, layer, width, max_jump, d_mask, columns, rows, mask_pitch};
    XR_TRY(launch_overlay_draw(d, ov->form, clear, sc, d_summary, (hipStream_t)stream));
    ov->ran_on((hipStream_t)stream);
    return XRIT_OK;
}

int xrit_overlay_blend_device(xrit_overlay *ov, const xrit_product_image *image, uint32_t components_in, const uint8_t *d_mask,
                              uint32_t mask_pitch, const xrit_overlay_style *styles, uint8_t *d_out, uint32_t out_pitch,
                              uint32_t components_out, xrit_overlay_blend_summary *d_summary, void *stream)
{
    XR_TRY(check_blend(ov, image, components_in, d_mask, mask_pitch, styles, d_out, out_pitch, components_out, d_summary));
    XR_HIP(hipSetDevice(ov->device));
    XR_TRY(launch_overlay_blend(blend_of(*image, components_in, d_mask, mask_pitch, styles, d_out, out_pitch, components_out), d_summary,
                                (hipStream_t)stream));
    ov->ran_on((hipStream_t)stream);
    return XRIT_OK;
}

// ---- host buffers ----------------------------------------------------------------------------------------------------------
int xrit_overlay_map(xrit_overlay *ov, const xrit_geo_nav *nav, const double *quads, size_t n, xrit_geo_point *points)
{
    XR_TRY(check_map(ov, nav, quads, n, points));
    if (!n) return XRIT_OK;
    hipStream_t s;
    XR_TRY(ov->adopt_own_stream(s));
    XR_TRY(ov->h_in.reserve(n * 4 * sizeof(double)));
    XR_TRY(ov->h_out.reserve(n * sizeof(xrit_geo_point)));
    XR_HIP(hipMemcpyAsync(ov->h_in.p, quads, n * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    XR_TRY(launch_overlay_map(*nav, ov->h_in.as<double>(), n, ov->h_out.as<xrit_geo_point>(), s));
    ov->ran_on(s);
    XR_HIP(hipMemcpyAsync(points, ov->h_out.p, n * sizeof(xrit_geo_point), hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}

int xrit_overlay_draw(xrit_overlay *ov, const xrit_geo_point *points, size_t n, uint32_t layer, uint32_t width, uint32_t max_jump, uint8_t *mask,
                      uint32_t columns, uint32_t rows, uint32_t mask_pitch, uint32_t clear, xrit_overlay_draw_summary *summary)
{
    XR_TRY(check_draw(ov, points, n, layer, width, mask, columns, rows, mask_pitch, summary));
    hipStream_t s;
    XR_TRY(ov->adopt_own_stream(s));
    OverlayScratch sc;
    XR_TRY(scratch_for(ov, n, sc));
    const size_t point_bytes = n * sizeof(xrit_geo_point), mask_bytes = (size_t)rows * mask_pitch;
    XR_TRY(ov->h_in.reserve(point_bytes ? point_bytes : 8));
    XR_TRY(ov->h_out.reserve(sizeof *summary));
    ov->mask_drawn = false;
    XR_TRY(ov->h_mask.reserve(mask_bytes));
    uint8_t *d_mask = ov->h_mask.as<uint8_t>();
    xrit_overlay_draw_summary *d_summary = ov->h_out.as<xrit_overlay_draw_summary>();
    if (point_bytes) XR_HIP(hipMemcpyAsync(ov->h_in.p, points, point_bytes, hipMemcpyHostToDevice, s));
    if (!clear) XR_HIP(hipMemcpyAsync(d_mask, mask, mask_bytes, hipMemcpyHostToDevice, s));
    const OverlayDraw dr{ov->h_in.as<xrit_geo_point>(), (uint32_t)n, layer, width, max_jump, d_mask, columns, rows, mask_pitch};
    XR_TRY(launch_overlay_draw(dr, ov->form, clear, sc, d_summary, s));
    ov->ran_on(s);
    XR_HIP(hipMemcpyAsync(summary, d_summary, sizeof *summary, hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpyAsync(mask, d_mask, mask_bytes, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    ov->mask_drawn = true;
    return XRIT_OK;
}

int xrit_overlay_mask_device(xrit_overlay *ov, const uint8_t **d_mask)
{
    if (!ov || !d_mask) { set_error("null argument"); return XRIT_E_INVALID; }
    *d_mask = ov->mask_drawn ? ov->h_mask.as<uint8_t>() : nullptr;
    return XRIT_OK;
}

// the blend of an image and a mask in device memory; the output (tight on the device, out_pitch on the host) and the summary
// to host memory behind it, then the wait
static int blend_to_host(xrit_overlay *ov, const xrit_product_image &im, uint32_t cin, const uint8_t *d_mask, uint32_t mask_pitch,
                         const xrit_overlay_style *styles, uint8_t *out, uint32_t out_pitch, uint32_t cout, xrit_overlay_blend_summary *summary,
                         hipStream_t s)
{
    const size_t row_bytes = (size_t)im.columns * cout, at_out = 256;
    XR_TRY(ov->h_out.reserve(at_out + row_bytes * im.rows));
    uint8_t *d = ov->h_out.as<uint8_t>();
    XR_TRY(launch_overlay_blend(blend_of(im, cin, d_mask, mask_pitch, styles, d + at_out, (uint32_t)row_bytes, cout),
                                reinterpret_cast<xrit_overlay_blend_summary *>(d), s));
    ov->ran_on(s);
    XR_HIP(hipMemcpyAsync(summary, d, sizeof *summary, hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpy2DAsync(out, out_pitch, d + at_out, row_bytes, row_bytes, im.rows, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}

int xrit_overlay_blend(xrit_overlay *ov, const xrit_product_image *image, uint32_t components_in, const uint8_t *mask, uint32_t mask_pitch,
                       const xrit_overlay_style *styles, uint8_t *out, uint32_t out_pitch, uint32_t components_out,
                       xrit_overlay_blend_summary *summary)
{
    XR_TRY(check_blend(ov, image, components_in, mask, mask_pitch, styles, out, out_pitch, components_out, summary));
    hipStream_t s;
    XR_TRY(ov->adopt_own_stream(s));
    const size_t in_bytes = (size_t)image->pitch * (image->rows - 1) + (size_t)image->columns * components_in;
    const size_t mask_bytes = (size_t)mask_pitch * (image->rows - 1) + image->columns, at_mask = padded(in_bytes);
    XR_TRY(ov->h_in.reserve(at_mask + mask_bytes));
    uint8_t *d = ov->h_in.as<uint8_t>();
    XR_HIP(hipMemcpyAsync(d, image->d_pixels, in_bytes, hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(d + at_mask, mask, mask_bytes, hipMemcpyHostToDevice, s));
    xrit_product_image im = *image;
    im.d_pixels = d;
    return blend_to_host(ov, im, components_in, d + at_mask, mask_pitch, styles, out, out_pitch, components_out, summary, s);
}

int xrit_overlay_blend_resident(xrit_overlay *ov, const xrit_product_image *image, uint32_t components_in, const uint8_t *d_mask,
                                uint32_t mask_pitch, const xrit_overlay_style *styles, uint8_t *out, uint32_t out_pitch,
                                uint32_t components_out, xrit_overlay_blend_summary *summary)
{
    XR_TRY(check_blend(ov, image, components_in, d_mask, mask_pitch, styles, out, out_pitch, components_out, summary));
    hipStream_t s;
    XR_TRY(ov->adopt_own_stream(s));
    return blend_to_host(ov, *image, components_in, d_mask, mask_pitch, styles, out, out_pitch, components_out, summary, s);
}

// ---- host helpers: no device -----------------------------------------------------------------------------------------------
int xrit_overlay_quads(const double *lon_deg, const double *lat_deg, size_t n, double sub_lon_deg, double *quads)
{
    if (n && (!lon_deg || !lat_deg || !quads)) { set_error("null argument"); return XRIT_E_INVALID; }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t i = 0; i < n; ++i) {
        double *q = quads + 4 * i;
        if (std::isnan(lon_deg[i]) || std::isnan(lat_deg[i])) {
            q[0] = q[1] = q[2] = q[3] = nan;
            continue;
        }
        // (xrit_geo_grid_tables' formulas, of a row for the latitude and of a column for the longitude)
        const double c_lat = std::atan(GEO_FLAT * std::tan(lat_deg[i] * DEG));
        const double cl = std::cos(c_lat);
        const double rl = GEO_RPOL / std::sqrt(1.0 - GEO_E2 * (cl * cl));
        const double dl = (lon_deg[i] - sub_lon_deg) * DEG;
        q[0] = rl * cl;
        q[1] = rl * std::sin(c_lat);
        q[2] = std::cos(dl);
        q[3] = std::sin(dl);
    }
    return XRIT_OK;
}

// v (pixels) -> 1/256 pixel; false where it is not below 2^29 in magnitude (NaN included)
static bool overlay_quantise(double v, int32_t &q)
{
    const double s = v * 256.0;
    if (!(s < (double)OVERLAY_LIMIT && s > -(double)OVERLAY_LIMIT)) return false;
    const double r = std::floor(s + 0.5);
    if (!(r < (double)OVERLAY_LIMIT && r > -(double)OVERLAY_LIMIT)) return false;
    q = (int32_t)r;
    return true;
}

int xrit_overlay_grid_points(const xrit_geo_grid *grid, const double *lon_deg, const double *lat_deg, size_t n, xrit_geo_point *points)
{
    if (!grid || (n && (!lon_deg || !lat_deg || !points))) { set_error("null argument"); return XRIT_E_INVALID; }
    if (grid->kind > XRIT_GEO_MERCATOR || !(grid->step_lon_deg != 0.0) || !(grid->step_lat_deg != 0.0)) {
        set_error("overlay: kind 0 .. 1, steps other than 0");
        return XRIT_E_INVALID;
    }
    for (size_t i = 0; i < n; ++i) {
        points[i] = xrit_geo_point{OVERLAY_BREAK, OVERLAY_BREAK};
        double d = lon_deg[i] - grid->lon0_deg;
        d -= 360.0 * std::floor((d + 180.0) / 360.0);
        const double y = grid->kind == XRIT_GEO_MERCATOR ? std::asinh(std::tan(lat_deg[i] * DEG)) : lat_deg[i];
        xrit_geo_point p;
        if (overlay_quantise(d / grid->step_lon_deg, p.qx) && overlay_quantise((grid->lat0_deg - y) / grid->step_lat_deg, p.qy)) points[i] = p;
    }
    return XRIT_OK;
}

int xrit_overlay_densify(const double *lon_deg, const double *lat_deg, size_t n, double max_step_deg, double *out_lon, double *out_lat, size_t cap,
                         size_t *n_out)
{
    if (!n_out || (n && (!lon_deg || !lat_deg)) || (cap && (!out_lon || !out_lat))) { set_error("null argument"); return XRIT_E_INVALID; }
    if (!(max_step_deg > 0.0) || n > XRIT_OVERLAY_MAX_VERTICES) { set_error("overlay: max_step_deg above 0, at most 2^26 vertices"); return XRIT_E_INVALID; }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    uint64_t m = 0;
    auto put = [&](double lon, double lat) {
        if (m < cap) out_lon[m] = lon, out_lat[m] = lat;
        ++m;
    };
    for (size_t i = 0; i < n; ++i) {
        const bool brk = std::isnan(lon_deg[i]) || std::isnan(lat_deg[i]);
        if (i && !brk && !std::isnan(lon_deg[i - 1]) && !std::isnan(lat_deg[i - 1])) {
            const double dlon = lon_deg[i] - lon_deg[i - 1], dlat = lat_deg[i] - lat_deg[i - 1];
            const double parts = std::ceil(std::fmax(std::fabs(dlon), std::fabs(dlat)) / max_step_deg);
            if (!(parts <= (double)XRIT_OVERLAY_MAX_VERTICES)) { set_error("overlay: a segment of more than 2^26 parts"); return XRIT_E_INVALID; }
            const uint32_t k = parts < 1.0 ? 1u : (uint32_t)parts;
            for (uint32_t j = 1; j < k; ++j) put(lon_deg[i - 1] + dlon * (double)j / (double)k, lat_deg[i - 1] + dlat * (double)j / (double)k);
            if (m > XRIT_OVERLAY_MAX_VERTICES) { set_error("overlay: more than 2^26 vertices"); return XRIT_E_INVALID; }
        }
        if (brk) put(nan, nan);
        else put(lon_deg[i], lat_deg[i]);
    }
    if (m > XRIT_OVERLAY_MAX_VERTICES) { set_error("overlay: more than 2^26 vertices"); return XRIT_E_INVALID; }
    *n_out = (size_t)m;
    if (m > cap) { set_error("overlay: %llu vertices: the output arrays are too small", (unsigned long long)m); return XRIT_E_CAPACITY; }
    return XRIT_OK;
}

int xrit_overlay_graticule(double step_deg, double vertex_step_deg, double *lon_deg, double *lat_deg, size_t cap, size_t *n_out)
{
    if (!n_out || (cap && (!lon_deg || !lat_deg))) { set_error("null argument"); return XRIT_E_INVALID; }
    if (!(step_deg >= 0.1 && step_deg <= 90.0 && vertex_step_deg >= 0.001 && vertex_step_deg <= step_deg)) {
        set_error("overlay: step_deg 0.1 .. 90, vertex_step_deg 0.001 .. step_deg");
        return XRIT_E_INVALID;
    }
    // at most 360 / step lines of 180 / vertex_step + 3 vertices and 180 / step of 360 / vertex_step + 3: refused before the walk
    if ((360.0 / step_deg + 1.0) * (180.0 / vertex_step_deg + 3.0) + (180.0 / step_deg + 1.0) * (360.0 / vertex_step_deg + 3.0) >
        (double)XRIT_OVERLAY_MAX_VERTICES) {
        set_error("overlay: these steps make more than 2^26 vertices");
        return XRIT_E_INVALID;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    size_t m = 0;
    auto put = [&](double lon, double lat) {
        if (m < cap) lon_deg[m] = lon, lat_deg[m] = lat;
        ++m;
    };
    // a line from `from` to `to` along one coordinate: a vertex every vertex_step_deg, the last one on `to`, then a break
    auto line = [&](double from, double to, auto &&at) {
        for (uint32_t j = 0;; ++j) {
            const double v = from + (double)j * vertex_step_deg;
            if (!(v < to)) break;
            at(v);
        }
        at(to);
        put(nan, nan);
    };
    for (uint32_t i = 0;; ++i) {
        const double lon = -180.0 + (double)i * step_deg;
        if (!(lon < 180.0)) break;
        line(-90.0, 90.0, [&](double lat) { put(lon, lat); });
    }
    for (uint32_t i = 1;; ++i) {
        const double lat = -90.0 + (double)i * step_deg;
        if (!(lat < 90.0)) break;
        line(-180.0, 180.0, [&](double lon) { put(lon, lat); });
    }
    *n_out = m;
    if (m > cap) { set_error("overlay: %zu vertices: the output arrays are too small", m); return XRIT_E_CAPACITY; }
    return XRIT_OK;
}
