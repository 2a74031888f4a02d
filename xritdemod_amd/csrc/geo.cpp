// geo.cpp -- C ABI of the projection stage (include/xritdemod_amd.h, "Image projection"): the handle owns the grid's four
// tables in device memory and the host-buffer forms' staging; the host helpers (the tables of a grid, the navigation
// record, the inverse of the map) are plain C++ on the C library; the kernels are in geo.hip.
#include <cmath>
#include <cstddef>
#include <vector>

#include "common.h"
#include "geo_rule.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_geo_nav) == 32 && offsetof(xrit_geo_nav, origin) == 16 && offsetof(xrit_geo_nav, sub_lon_deg) == 24,
              "xrit_geo_nav layout (the ctypes mirror follows it)");
static_assert(sizeof(xrit_geo_grid) == 48 && offsetof(xrit_geo_grid, lon0_deg) == 16, "xrit_geo_grid layout");
static_assert(sizeof(xrit_geo_point) == 8, "xrit_geo_point layout");
static_assert(sizeof(xrit_geo_summary) == 56 && offsetof(xrit_geo_summary, off_disc) == 8 && offsetof(xrit_geo_summary, written) == 32 &&
                  offsetof(xrit_geo_summary, columns) == 40,
              "xrit_geo_summary layout (GEO_SUMMARY_DTYPE mirrors it; the kernel adds to the four counts as one array)");

namespace {
constexpr uint64_t MAX_PIXELS = (uint64_t)1 << 31;
constexpr double DEG = 3.141592653589793 / 180.0;
constexpr size_t TABLE_ALIGN = 256;
size_t table_stride(uint32_t n) { return ((size_t)n * sizeof(double) + TABLE_ALIGN - 1) & ~(TABLE_ALIGN - 1); }
bool dims_ok(uint32_t columns, uint32_t rows) { return columns >= 1 && rows >= 1 && columns <= XRIT_GEO_MAX_DIM && rows <= XRIT_GEO_MAX_DIM; }
}  // namespace

struct xrit_geo : StageHandle {
    DevBuf tables;                                  // A, B (rows doubles each), C, S (columns), each on a 256-byte boundary
    DevBuf h_in, h_out;                             // the host-buffer forms'
    uint32_t columns = 0, rows = 0;                 // 0: no tables set
    GeoTables view() const
    {
        const size_t r = table_stride(rows), c = table_stride(columns);
        const char *p = tables.as<char>();
        return GeoTables{reinterpret_cast<const double *>(p), reinterpret_cast<const double *>(p + r), reinterpret_cast<const double *>(p + 2 * r),
                         reinterpret_cast<const double *>(p + 2 * r + c), columns, rows};
    }
    void close_all() { close({&tables, &h_in, &h_out}); }
};

int xrit_geo_create(xrit_geo **out, int device)
{
    return stage_create(out, device, [&](xrit_geo &) { return XRIT_OK; });
}

int xrit_geo_destroy(xrit_geo *g) { return stage_destroy(g); }

int xrit_geo_reset(xrit_geo *g)
{
    if (!g) { set_error("null argument"); return XRIT_E_INVALID; }
    return g->wait_last();
}

int xrit_geo_grid_tables(const xrit_geo_grid *grid, double sub_lon_deg, double *A, double *B, double *C, double *S)
{
    if (!grid || !A || !B || !C || !S) { set_error("null argument"); return XRIT_E_INVALID; }
    if (grid->kind > XRIT_GEO_MERCATOR || !dims_ok(grid->columns, grid->rows)) {
        set_error("geo: kind 0 .. 1, columns and rows 1 .. %d", XRIT_GEO_MAX_DIM);
        return XRIT_E_INVALID;
    }
    for (uint32_t i = 0; i < grid->rows; ++i) {
        const double lat = grid->kind == XRIT_GEO_MERCATOR ? std::atan(std::sinh(grid->lat0_deg - (double)i * grid->step_lat_deg))
                                                           : (grid->lat0_deg - (double)i * grid->step_lat_deg) * DEG;
        const double c_lat = std::atan(GEO_FLAT * std::tan(lat));
        const double cl = std::cos(c_lat);
        const double rl = GEO_RPOL / std::sqrt(1.0 - GEO_E2 * (cl * cl));
        A[i] = rl * cl;
        B[i] = rl * std::sin(c_lat);
    }
    for (uint32_t j = 0; j < grid->columns; ++j) {
        const double dl = (grid->lon0_deg + (double)j * grid->step_lon_deg - sub_lon_deg) * DEG;
        C[j] = std::cos(dl);
        S[j] = std::sin(dl);
    }
    return XRIT_OK;
}

int xrit_geo_set_tables(xrit_geo *g, uint32_t columns, uint32_t rows, const double *A, const double *B, const double *C, const double *S)
{
    if (!g || !A || !B || !C || !S) { set_error("null argument"); return XRIT_E_INVALID; }
    if (!dims_ok(columns, rows)) {
        set_error("geo: columns and rows 1 .. %d", XRIT_GEO_MAX_DIM);
        return XRIT_E_INVALID;
    }
    XR_TRY(g->wait_last());                         // a call that reads the tables in effect may still run
    const size_t r = table_stride(rows), c = table_stride(columns);
    g->columns = g->rows = 0;
    XR_TRY(g->tables.reserve(2 * r + 2 * c));
    char *p = g->tables.as<char>();
    XR_HIP(hipMemcpyAsync(p, A, (size_t)rows * sizeof(double), hipMemcpyHostToDevice, g->stream));
    XR_HIP(hipMemcpyAsync(p + r, B, (size_t)rows * sizeof(double), hipMemcpyHostToDevice, g->stream));
    XR_HIP(hipMemcpyAsync(p + 2 * r, C, (size_t)columns * sizeof(double), hipMemcpyHostToDevice, g->stream));
    XR_HIP(hipMemcpyAsync(p + 2 * r + c, S, (size_t)columns * sizeof(double), hipMemcpyHostToDevice, g->stream));
    XR_HIP(hipStreamSynchronize(g->stream));
    g->ran_on(g->stream);
    g->columns = columns;
    g->rows = rows;
    return XRIT_OK;
}

int xrit_geo_set_grid(xrit_geo *g, const xrit_geo_grid *grid, double sub_lon_deg)
{
    if (!g || !grid) { set_error("null argument"); return XRIT_E_INVALID; }
    if (!dims_ok(grid->columns, grid->rows)) {
        set_error("geo: columns and rows 1 .. %d", XRIT_GEO_MAX_DIM);
        return XRIT_E_INVALID;
    }
    std::vector<double> t(2 * (size_t)grid->rows + 2 * (size_t)grid->columns);
    double *A = t.data(), *B = A + grid->rows, *C = B + grid->rows, *S = C + grid->columns;
    XR_TRY(xrit_geo_grid_tables(grid, sub_lon_deg, A, B, C, S));
    return xrit_geo_set_tables(g, grid->columns, grid->rows, A, B, C, S);
}

static int need_tables(const xrit_geo *g)
{
    if (!g) { set_error("null argument"); return XRIT_E_INVALID; }
    if (!g->columns) { set_error("geo: no tables set (xrit_geo_set_grid, xrit_geo_set_tables)"); return XRIT_E_INVALID; }
    return XRIT_OK;
}

int xrit_geo_tables(xrit_geo *g, uint32_t *columns, uint32_t *rows, double *A, double *B, double *C, double *S)
{
    XR_TRY(need_tables(g));
    const GeoTables t = g->view();
    if (columns) *columns = t.columns;
    if (rows) *rows = t.rows;
    if (A) XR_TRY(g->read_back(A, t.A, (size_t)t.rows * sizeof(double)));
    if (B) XR_TRY(g->read_back(B, t.B, (size_t)t.rows * sizeof(double)));
    if (C) XR_TRY(g->read_back(C, t.C, (size_t)t.columns * sizeof(double)));
    if (S) XR_TRY(g->read_back(S, t.S, (size_t)t.columns * sizeof(double)));
    return XRIT_OK;
}

// the product stage's bounds on an image, and the output's; pixels and out: wherever they lie
static int check_call(const xrit_geo *g, const xrit_product_image *im, uint32_t mode, const void *out, uint32_t out_pitch, const void *summary)
{
    XR_TRY(need_tables(g));
    if (!im || !im->d_pixels || !out || !summary) { set_error("null argument"); return XRIT_E_INVALID; }
    if (mode > XRIT_GEO_BILINEAR) { set_error("geo: mode 0 (nearest) or 1 (bilinear)"); return XRIT_E_INVALID; }
    if (im->bits < 1 || im->bits > 16 || im->columns < 1 || im->rows < 1 || (uint64_t)im->columns * im->rows > MAX_PIXELS) {
        set_error("geo: 1 .. 16 bits, columns, rows >= 1, columns * rows <= 2^31");
        return XRIT_E_INVALID;
    }
    const uint32_t width = geo_width(im->bits);
    if ((uint64_t)im->pitch < (uint64_t)im->columns * width || (width == 2 && ((im->pitch | (size_t)im->d_pixels) & 1))) {
        set_error("geo: pitch >= columns * width; samples of two bytes on even addresses");
        return XRIT_E_INVALID;
    }
    if ((uint64_t)out_pitch < (uint64_t)g->columns * width || (width == 2 && ((out_pitch | (size_t)out) & 1))) {
        set_error("geo: out_pitch >= the grid's columns * width; samples of two bytes on even addresses");
        return XRIT_E_INVALID;
    }
    return XRIT_OK;
}

int xrit_geo_map_device(xrit_geo *g, const xrit_geo_nav *nav, xrit_geo_point *d_map, void *stream)
{
    XR_TRY(need_tables(g));
    if (!nav || !d_map) { set_error("null argument"); return XRIT_E_INVALID; }
    if ((size_t)d_map & 7) { set_error("geo: the map must be 8-byte aligned"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(g->device));
    XR_TRY(launch_geo_map(g->view(), *nav, d_map, (hipStream_t)stream));
    g->ran_on((hipStream_t)stream);
    return XRIT_OK;
}

int xrit_geo_resample_device(xrit_geo *g, const xrit_product_image *image, const xrit_geo_point *d_map, uint32_t mode, uint8_t *d_out,
                             uint32_t out_pitch, xrit_geo_summary *d_summary, void *stream)
{
    XR_TRY(check_call(g, image, mode, d_out, out_pitch, d_summary));
    if (!d_map) { set_error("null argument"); return XRIT_E_INVALID; }
    if (((size_t)d_map | (size_t)d_summary) & 7) { set_error("geo: the map and the summary must be 8-byte aligned"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(g->device));
    XR_TRY(launch_geo_resample(g->view(), *image, d_map, mode, d_out, out_pitch, d_summary, (hipStream_t)stream));
    g->ran_on((hipStream_t)stream);
    return XRIT_OK;
}

int xrit_geo_project_device(xrit_geo *g, const xrit_geo_nav *nav, const xrit_product_image *image, uint32_t mode, uint8_t *d_out,
                            uint32_t out_pitch, xrit_geo_summary *d_summary, void *stream)
{
    XR_TRY(check_call(g, image, mode, d_out, out_pitch, d_summary));
    if (!nav) { set_error("null argument"); return XRIT_E_INVALID; }
    if ((size_t)d_summary & 7) { set_error("geo: the summary must be 8-byte aligned"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(g->device));
    XR_TRY(launch_geo_project(g->view(), *nav, *image, mode, d_out, out_pitch, d_summary, (hipStream_t)stream));
    g->ran_on((hipStream_t)stream);
    return XRIT_OK;
}

// the fused call on an image in device memory, the output (tight on the device, out_pitch on the host) and the summary
// to host memory behind it, then the wait
static int project_to_host(xrit_geo *g, const xrit_geo_nav &nav, const xrit_product_image &im, uint32_t mode, uint8_t *out, uint32_t out_pitch,
                           xrit_geo_summary *summary, hipStream_t s)
{
    const size_t row_bytes = (size_t)g->columns * geo_width(im.bits), at_out = 64;
    XR_TRY(g->h_out.reserve(at_out + row_bytes * g->rows));
    uint8_t *d = g->h_out.as<uint8_t>();
    XR_TRY(launch_geo_project(g->view(), nav, im, mode, d + at_out, (uint32_t)row_bytes, reinterpret_cast<xrit_geo_summary *>(d), s));
    g->ran_on(s);
    XR_HIP(hipMemcpyAsync(summary, d, sizeof *summary, hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpy2DAsync(out, out_pitch, d + at_out, row_bytes, row_bytes, g->rows, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}

int xrit_geo_project(xrit_geo *g, const xrit_geo_nav *nav, const xrit_product_image *image, uint32_t mode, uint8_t *out, uint32_t out_pitch,
                     xrit_geo_summary *summary)
{
    XR_TRY(check_call(g, image, mode, out, out_pitch, summary));
    if (!nav) { set_error("null argument"); return XRIT_E_INVALID; }
    hipStream_t s;
    XR_TRY(g->adopt_own_stream(s));
    const size_t in_bytes = (size_t)image->pitch * (image->rows - 1) + (size_t)image->columns * geo_width(image->bits);
    XR_TRY(g->h_in.reserve(in_bytes));
    XR_HIP(hipMemcpyAsync(g->h_in.p, image->d_pixels, in_bytes, hipMemcpyHostToDevice, s));
    xrit_product_image im = *image;
    im.d_pixels = g->h_in.as<uint8_t>();
    return project_to_host(g, *nav, im, mode, out, out_pitch, summary, s);
}

int xrit_geo_project_resident(xrit_geo *g, const xrit_geo_nav *nav, const xrit_product_image *image, uint32_t mode, uint8_t *out,
                              uint32_t out_pitch, xrit_geo_summary *summary)
{
    XR_TRY(check_call(g, image, mode, out, out_pitch, summary));
    if (!nav) { set_error("null argument"); return XRIT_E_INVALID; }
    hipStream_t s;
    XR_TRY(g->adopt_own_stream(s));
    return project_to_host(g, *nav, *image, mode, out, out_pitch, summary, s);
}

// ---- host helpers: no device ---------------------------------------------------------------------------------------------
static uint32_t be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }
static int32_t be32(const uint8_t *p) { return (int32_t)((uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]); }

int xrit_geo_parse_navigation(const uint8_t *b, size_t n, xrit_geo_nav *nav)
{
    if (!b || !nav) { set_error("null argument"); return XRIT_E_INVALID; }
    // the primary header (type 0, length 16) says how long the header records are together
    if (n < 16 || b[0] != 0 || be16(b + 1) != 16) { set_error("geo: no primary header"); return XRIT_E_INVALID; }
    const size_t H = (size_t)be16(b + 4) << 16 | be16(b + 6);
    if (H > n) { set_error("geo: the header is truncated (%zu of %zu bytes)", n, H); return XRIT_E_INVALID; }
    size_t q = 16;
    while (q + 3 <= H) {
        const uint32_t t = b[q], l = be16(b + q + 1);
        if (l < 3 || q + l > H) break;
        if (t == 2 && l == 51) {
            const uint8_t *name = b + q + 3;
            if (!((name[0] == 'G' && name[1] == 'E' && name[2] == 'O' && name[3] == 'S') ||
                  (name[0] == 'g' && name[1] == 'e' && name[2] == 'o' && name[3] == 's')) || name[4] != '(') {
                set_error("geo: the projection is not GEOS(<sub_lon>)");
                return XRIT_E_INVALID;
            }
            char text[32] = {0};
            size_t k = 0;
            while (5 + k < 32 && name[5 + k] != ')' && name[5 + k] != 0) { text[k] = (char)name[5 + k]; ++k; }
            char *end = nullptr;
            const double lon = std::strtod(text, &end);
            if (5 + k >= 32 || name[5 + k] != ')' || end == text || *end != 0 || !(lon >= -360.0 && lon <= 360.0)) {
                set_error("geo: no sub-satellite longitude in the projection name");
                return XRIT_E_INVALID;
            }
            *nav = xrit_geo_nav{be32(name + 32), be32(name + 36), be32(name + 40), be32(name + 44), 1, 0, lon};
            return XRIT_OK;
        }
        q += l;
    }
    set_error("geo: no image navigation record (type 2, length 51)");
    return XRIT_E_INVALID;
}

int xrit_geo_pixel_to_lonlat(const xrit_geo_nav *nav, double column, double line, double *lon_deg, double *lat_deg)
{
    if (!nav || !lon_deg || !lat_deg || nav->cfac == 0 || nav->lfac == 0) { set_error("geo: null argument or a factor of 0"); return XRIT_E_INVALID; }
    const GeoNav g = geo_nav_of(*nav);
    // column and line count from origin: fc = column - origin, and fc = c0 + x * cs with c0 = coff - origin
    const double x = (column - (double)nav->coff) / g.cs * DEG, y = (line - (double)nav->loff) / g.ls * DEG;
    const double cx = std::cos(x), sx = std::sin(x), cy = std::cos(y), sy = std::sin(y);
    const double k = cy * cy + GEO_K * (sy * sy);
    const double d = (GEO_H * cx * cy) * (GEO_H * cx * cy) - k * 1737121856.0;     // 42164^2 - 6378.1690^2, as CGMS prints it
    if (!(d >= 0.0)) return 1;
    const double sn = (GEO_H * cx * cy - std::sqrt(d)) / k;
    const double s1 = GEO_H - sn * cx * cy, s2 = sn * sx * cy, s3 = -sn * sy;
    const double sxy = std::sqrt(s1 * s1 + s2 * s2);
    *lon_deg = std::atan(s2 / s1) / DEG + nav->sub_lon_deg;
    *lat_deg = std::atan(GEO_K * s3 / sxy) / DEG;
    return 0;
}
