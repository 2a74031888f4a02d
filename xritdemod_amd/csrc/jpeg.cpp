// jpeg.cpp -- C ABI of the JPEG stage (include/xritdemod_amd.h, "JPEG"): the handle owns the parameters (two quantisation
// tables, the restart interval), the scratch in device memory and the host-buffer forms' staging; the header and the bound
// are plain host code; the kernels are in jpeg.hip.
#include <cstddef>

#include "common.h"
#include "jpeg_rule.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_jpeg_result) == 16 && offsetof(xrit_jpeg_result, status) == 8 && offsetof(xrit_jpeg_result, restarts) == 12,
              "xrit_jpeg_result layout (JPEG_RESULT_DTYPE mirrors it)");
static_assert(XRIT_JPEG_MAX_BLOCKS == JPEG_MAX_BLOCKS, "the header's bound is the rule's");

struct xrit_jpeg : StageHandle {
    uint8_t tables[2][64];                          // natural order
    uint32_t restart = 0;
    DevBuf scratch;                                 // jpeg_scratch_carve's
    DevBuf h_in, h_out;                             // the host-buffer forms': the pixels; the result record, then the file
    void close_all() { close({&scratch, &h_in, &h_out}); }
};

namespace {

// what a shape comes to; false for a shape the stage does not take
struct Shape {
    uint32_t bw, mcus, blocks, ri, n_int;
};
bool shape_of(uint32_t components, uint32_t columns, uint32_t rows, uint32_t restart, Shape &sh)
{
    if ((components != 1 && components != 3) || columns < 1 || rows < 1 || columns > JPEG_MAX_DIM || rows > JPEG_MAX_DIM || restart > 65535)
        return false;
    const uint64_t bw = (columns + 7) / 8, mcus = bw * ((rows + 7) / 8);
    if (mcus * components > JPEG_MAX_BLOCKS) return false;
    sh.bw = (uint32_t)bw;
    sh.mcus = (uint32_t)mcus;
    sh.blocks = (uint32_t)mcus * components;
    sh.ri = restart ? restart : (uint32_t)mcus;
    sh.n_int = (sh.mcus + sh.ri - 1) / sh.ri;
    return true;
}

void quality_tables(uint32_t quality, uint8_t tables[2][64])
{
    for (int i = 0; i < 64; ++i) {
        tables[0][i] = (uint8_t)jpeg_quality_entry(JPEG_STD_LUMINANCE[i], quality);
        tables[1][i] = (uint8_t)jpeg_quality_entry(JPEG_STD_CHROMINANCE[i], quality);
    }
}

// SOI .. SOS as libjpeg writes them
struct HeaderWriter {
    JpegHeader h{};
    void u8(uint32_t v) { h.b[h.n++] = (uint8_t)v; }
    void u16(uint32_t v) { u8(v >> 8); u8(v & 255); }
    void marker(uint32_t m) { u8(0xFF); u8(m); }
};
JpegHeader make_header(const uint8_t tables[2][64], uint32_t restart, uint32_t components, uint32_t columns, uint32_t rows)
{
    HeaderWriter w;
    w.marker(0xD8);
    w.marker(0xE0);
    w.u16(16);
    for (uint8_t c : {0x4A, 0x46, 0x49, 0x46, 0x00}) w.u8(c);      // "JFIF"
    w.u16(0x0101);
    w.u8(0);                                                        // no density unit: the aspect ratio 1 : 1
    w.u16(1);
    w.u16(1);
    w.u16(0);                                                       // no thumbnail
    for (uint32_t t = 0; t < (components == 3 ? 2u : 1u); ++t) {
        w.marker(0xDB);
        w.u16(67);
        w.u8(t);
        for (int k = 0; k < 64; ++k) w.u8(tables[t][JPEG_ZIGZAG[k]]);
    }
    w.marker(0xC0);
    w.u16(8 + 3 * components);
    w.u8(8);
    w.u16(rows);
    w.u16(columns);
    w.u8(components);
    for (uint32_t c = 0; c < components; ++c) {
        w.u8(c + 1);
        w.u8(0x11);
        w.u8(c ? 1 : 0);
    }
    for (uint32_t t = 0; t < (components == 3 ? 4u : 2u); ++t) {
        const JpegHuffSpec &s = JPEG_HUFF_SPEC[t];
        w.marker(0xC4);
        w.u16(19 + s.count);
        w.u8(s.cls << 4 | s.index);
        for (int i = 0; i < 16; ++i) w.u8(s.bits[i]);
        for (uint32_t i = 0; i < s.count; ++i) w.u8(s.vals[i]);
    }
    if (restart) {
        w.marker(0xDD);
        w.u16(4);
        w.u16(restart);
    }
    w.marker(0xDA);
    w.u16(6 + 2 * components);
    w.u8(components);
    for (uint32_t c = 0; c < components; ++c) {
        w.u8(c + 1);
        w.u8(c ? 0x11 : 0x00);
    }
    w.u8(0);
    w.u8(63);
    w.u8(0);
    return w.h;
}
static_assert(sizeof(JpegHeader::b) >= JPEG_MAX_HEADER, "room for the longest header");

bool tables_ok(const uint8_t *t)
{
    for (int i = 0; i < 128; ++i)
        if (!t[i]) return false;
    return true;
}

int copy_header(const uint8_t *tables128, uint32_t restart, uint32_t components, uint32_t columns, uint32_t rows, uint8_t *out, size_t cap,
                size_t *n)
{
    Shape sh;
    if (!n || !tables128 || (!out && cap)) { set_error("null argument"); return XRIT_E_INVALID; }
    if (!shape_of(components, columns, rows, restart, sh) || !tables_ok(tables128)) {
        set_error("jpeg: components 1 or 3, columns, rows 1 .. 65535, at most 2^22 blocks, restart 0 .. 65535, table entries 1 .. 255");
        return XRIT_E_INVALID;
    }
    const JpegHeader h = make_header(reinterpret_cast<const uint8_t(*)[64]>(tables128), restart, components, columns, rows);
    *n = h.n;
    if (h.n <= cap) memcpy(out, h.b, h.n);
    return XRIT_OK;
}

}  // namespace

int xrit_jpeg_create(xrit_jpeg **out, int device)
{
    return stage_create(out, device, [&](xrit_jpeg &j) {
        quality_tables(90, j.tables);
        return XRIT_OK;
    });
}

int xrit_jpeg_destroy(xrit_jpeg *j) { return stage_destroy(j); }

int xrit_jpeg_reset(xrit_jpeg *j)
{
    if (!j) { set_error("null argument"); return XRIT_E_INVALID; }
    return j->wait_last();
}

int xrit_jpeg_set_quality(xrit_jpeg *j, uint32_t quality, uint32_t restart)
{
    if (!j) { set_error("null argument"); return XRIT_E_INVALID; }
    if (quality < 1 || quality > 100 || restart > 65535) { set_error("jpeg: quality 1 .. 100, restart 0 .. 65535"); return XRIT_E_INVALID; }
    quality_tables(quality, j->tables);
    j->restart = restart;
    return XRIT_OK;
}

int xrit_jpeg_set_tables(xrit_jpeg *j, const uint8_t *tables128, uint32_t restart)
{
    if (!j || !tables128) { set_error("null argument"); return XRIT_E_INVALID; }
    if (!tables_ok(tables128) || restart > 65535) { set_error("jpeg: table entries 1 .. 255, restart 0 .. 65535"); return XRIT_E_INVALID; }
    memcpy(j->tables, tables128, 128);
    j->restart = restart;
    return XRIT_OK;
}

int xrit_jpeg_quality_tables(uint32_t quality, uint8_t *tables128)
{
    if (!tables128) { set_error("null argument"); return XRIT_E_INVALID; }
    if (quality < 1 || quality > 100) { set_error("jpeg: quality 1 .. 100"); return XRIT_E_INVALID; }
    quality_tables(quality, reinterpret_cast<uint8_t(*)[64]>(tables128));
    return XRIT_OK;
}

int xrit_jpeg_header_for(const uint8_t *tables128, uint32_t restart, uint32_t components, uint32_t columns, uint32_t rows, uint8_t *out,
                         size_t cap, size_t *n)
{
    return copy_header(tables128, restart, components, columns, rows, out, cap, n);
}

int xrit_jpeg_header(const xrit_jpeg *j, uint32_t components, uint32_t columns, uint32_t rows, uint8_t *out, size_t cap, size_t *n)
{
    if (!j) { set_error("null argument"); return XRIT_E_INVALID; }
    return copy_header(&j->tables[0][0], j->restart, components, columns, rows, out, cap, n);
}

uint64_t xrit_jpeg_bound(uint32_t components, uint32_t columns, uint32_t rows, uint32_t restart)
{
    Shape sh;
    if (!shape_of(components, columns, rows, restart, sh)) return 0;
    uint8_t ones[2][64];
    memset(ones, 1, sizeof ones);
    const uint64_t head = make_header(ones, restart, components, columns, rows).n;
    return head + 2 * (((uint64_t)sh.blocks * JPEG_BLOCK_BITS + 7) / 8 + sh.n_int) + 2 * ((uint64_t)sh.n_int - 1) + 2;
}

// the bounds of "JPEG"; pixels: the image's, wherever they lie
static int check_call(const xrit_jpeg *j, const xrit_product_image *im, uint32_t components, const void *out, const void *result, Shape &sh)
{
    if (!j || !im || !im->d_pixels || !out || !result) { set_error("null argument"); return XRIT_E_INVALID; }
    if (!shape_of(components, im->columns, im->rows, j->restart, sh)) {
        set_error("jpeg: components 1 or 3, columns, rows 1 .. 65535, at most 2^22 blocks of 8 x 8");
        return XRIT_E_INVALID;
    }
    if ((uint64_t)im->pitch < (uint64_t)im->columns * components) { set_error("jpeg: pitch >= columns * components"); return XRIT_E_INVALID; }
    return XRIT_OK;
}

static int jpeg_run(xrit_jpeg *j, const xrit_product_image &im, uint32_t components, const Shape &sh, uint8_t *d_out, size_t cap,
                    xrit_jpeg_result *d_result, hipStream_t s)
{
    JpegScratch sc;
    XR_TRY(j->scratch.reserve(jpeg_scratch_carve(nullptr, sh.blocks, sh.n_int, sc)));
    jpeg_scratch_carve(j->scratch.p, sh.blocks, sh.n_int, sc);
    JpegPar p;
    p.pix = im.d_pixels;
    p.columns = im.columns;
    p.rows = im.rows;
    p.pitch = im.pitch;
    p.comps = components;
    p.bw = sh.bw;
    p.mcus = sh.mcus;
    p.blocks = sh.blocks;
    p.ri = sh.ri;
    p.n_int = sh.n_int;
    memcpy(p.q, j->tables, sizeof p.q);
    XR_TRY(launch_jpeg(p, make_header(j->tables, j->restart, components, im.columns, im.rows), sc, d_out, cap, d_result, s));
    j->ran_on(s);
    return XRIT_OK;
}

int xrit_jpeg_encode_device(xrit_jpeg *j, const xrit_product_image *image, uint32_t components, uint8_t *d_out, size_t cap,
                            xrit_jpeg_result *d_result, void *stream)
{
    Shape sh;
    XR_TRY(check_call(j, image, components, d_out, d_result, sh));
    if ((size_t)d_result & 7) { set_error("jpeg: the result record must be 8-byte aligned"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(j->device));
    // a grown scratch is a new allocation: what the handle's last call still reads must have finished
    JpegScratch sc;
    if (jpeg_scratch_carve(nullptr, sh.blocks, sh.n_int, sc) > j->scratch.bytes) XR_TRY(j->wait_last());
    return jpeg_run(j, *image, components, sh, d_out, cap, d_result, (hipStream_t)stream);
}

// the call on pixels in device memory, the file to host memory: the record first, then only the file's bytes
static int jpeg_to_host(xrit_jpeg *j, const xrit_product_image &im, uint32_t components, const Shape &sh, uint8_t *out, size_t cap,
                        xrit_jpeg_result *result, hipStream_t s)
{
    const uint64_t bound = xrit_jpeg_bound(components, im.columns, im.rows, j->restart);
    const size_t d_cap = cap < bound ? cap : (size_t)bound;
    XR_TRY(j->h_out.reserve(16 + d_cap));
    uint8_t *d = j->h_out.as<uint8_t>();
    XR_TRY(jpeg_run(j, im, components, sh, d + 16, d_cap, reinterpret_cast<xrit_jpeg_result *>(d), s));
    XR_HIP(hipMemcpyAsync(result, d, sizeof *result, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    const size_t n = result->size < d_cap ? (size_t)result->size : d_cap;
    if (n) XR_HIP(hipMemcpyAsync(out, d + 16, n, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    if (!result->status) return XRIT_OK;
    set_error("jpeg: a file of %llu bytes: the output buffer is too small", (unsigned long long)result->size);
    return XRIT_E_CAPACITY;
}

int xrit_jpeg_encode(xrit_jpeg *j, const xrit_product_image *image, uint32_t components, uint8_t *out, size_t cap, xrit_jpeg_result *result)
{
    Shape sh;
    XR_TRY(check_call(j, image, components, out, result, sh));
    hipStream_t s;
    XR_TRY(j->adopt_own_stream(s));
    const size_t in_bytes = (size_t)image->pitch * (image->rows - 1) + (size_t)image->columns * components;
    XR_TRY(j->h_in.reserve(in_bytes));
    XR_HIP(hipMemcpyAsync(j->h_in.p, image->d_pixels, in_bytes, hipMemcpyHostToDevice, s));
    xrit_product_image im = *image;
    im.d_pixels = j->h_in.as<uint8_t>();
    return jpeg_to_host(j, im, components, sh, out, cap, result, s);
}

int xrit_jpeg_encode_resident(xrit_jpeg *j, const xrit_product_image *image, uint32_t components, uint8_t *out, size_t cap,
                              xrit_jpeg_result *result)
{
    Shape sh;
    XR_TRY(check_call(j, image, components, out, result, sh));
    hipStream_t s;
    XR_TRY(j->adopt_own_stream(s));
    return jpeg_to_host(j, *image, components, sh, out, cap, result, s);
}
