// product.cpp -- C ABI of the product stage (include/xritdemod_amd.h, "Image products"): the handle owns only scratch in
// device memory -- a histogram of 2^16 bins and a tone table of 2^16 bytes for callers that pass none, the count of
// samples out of range -- and the host-buffer forms' staging; the kernels are in product.hip.
#include <cstddef>

#include "common.h"
#include "kernels.h"
#include "product_rule.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_product_image) == 24 && offsetof(xrit_product_image, columns) == 8 && offsetof(xrit_product_image, bits) == 20,
              "xrit_product_image layout (the ctypes mirror follows it)");
static_assert(sizeof(xrit_product_params) == 16 && offsetof(xrit_product_params, factor) == 12, "xrit_product_params layout");
static_assert(sizeof(xrit_product_summary) == 64 && offsetof(xrit_product_summary, min_nz) == 24 && offsetof(xrit_product_summary, fallback) == 40 &&
                  offsetof(xrit_product_summary, small_columns) == 56,
              "xrit_product_summary layout (PRODUCT_SUMMARY_DTYPE mirrors it)");

namespace {
constexpr size_t HIST_BYTES = sizeof(uint32_t) << 16, LUT_BYTES = (size_t)1 << 16;
constexpr size_t SCRATCH_BYTES = HIST_BYTES + LUT_BYTES + 8;
constexpr size_t COMPOSITE_TABLE_BYTES = 256 * 256 * 3;
constexpr uint64_t MAX_PIXELS = (uint64_t)1 << 31;
}  // namespace

struct xrit_product : StageHandle {
    DevBuf scratch;                                 // the histogram, the tone table, then the out-of-range count
    DevBuf h_in, h_table, h_out;                    // the host-buffer forms'
    const uint8_t *last_tone = nullptr, *last_small = nullptr;      // where the last host-buffer call left them in h_out
    uint32_t *hist() const { return scratch.as<uint32_t>(); }
    unsigned char *lut() const { return scratch.as<unsigned char>() + HIST_BYTES; }
    unsigned long long *over_count() const { return reinterpret_cast<unsigned long long *>(scratch.as<char>() + HIST_BYTES + LUT_BYTES); }
    void close_all() { close({&scratch, &h_in, &h_table, &h_out}); }
};

int xrit_product_create(xrit_product **out, int device)
{
    return stage_create(out, device, [&](xrit_product &pr) { return pr.scratch.reserve(SCRATCH_BYTES); });
}

int xrit_product_destroy(xrit_product *pr) { return stage_destroy(pr); }

int xrit_product_reset(xrit_product *pr)
{
    if (!pr) { set_error("null argument"); return XRIT_E_INVALID; }
    return pr->wait_last();
}

// the bounds of "Image products"; pixels: the image's, wherever they lie
static int check_image(const xrit_product_image *im, const xrit_product_params *pp, const void *table_in)
{
    if (!im || !pp || !im->d_pixels) { set_error("null argument"); return XRIT_E_INVALID; }
    if (im->bits < 1 || im->bits > 16 || im->columns < 1 || im->rows < 1 || (uint64_t)im->columns * im->rows > MAX_PIXELS) {
        set_error("product: 1 .. 16 bits, columns, rows >= 1, columns * rows <= 2^31");
        return XRIT_E_INVALID;
    }
    const uint32_t width = product_width(im->bits);
    if ((uint64_t)im->pitch < (uint64_t)im->columns * width || (width == 2 && ((im->pitch | (size_t)im->d_pixels) & 1))) {
        set_error("product: pitch >= columns * width; samples of two bytes on even addresses");
        return XRIT_E_INVALID;
    }
    if (pp->tone > XRIT_TONE_STRETCH || (pp->tone == XRIT_TONE_TABLE && !table_in)) {
        set_error("product: tone 0 .. 3, XRIT_TONE_TABLE with a table");
        return XRIT_E_INVALID;
    }
    if (pp->tone == XRIT_TONE_STRETCH && (pp->p_lo >= pp->p_hi || pp->p_hi > 10000)) {
        set_error("product: 0 <= p_lo < p_hi <= 10000");
        return XRIT_E_INVALID;
    }
    if (pp->factor > XRIT_PRODUCT_MAX_FACTOR) {
        set_error("product: factor 0 .. %d", XRIT_PRODUCT_MAX_FACTOR);
        return XRIT_E_INVALID;
    }
    return XRIT_OK;
}

static int product_run(xrit_product *pr, const xrit_product_image &im, const xrit_product_params &pp, const uint8_t *d_table_in,
                       uint32_t *d_hist, uint8_t *d_lut, uint8_t *d_tone, uint8_t *d_small, xrit_product_summary *d_summary, hipStream_t s)
{
    XR_TRY(launch_product(im, pp, d_table_in, d_hist ? d_hist : pr->hist(), pr->over_count(), d_lut ? d_lut : pr->lut(), d_tone, d_small,
                          d_summary, s));
    pr->ran_on(s);
    return XRIT_OK;
}

int xrit_product_process_device(xrit_product *pr, const xrit_product_image *image, const xrit_product_params *params,
                                const uint8_t *d_table_in, uint32_t *d_hist, uint8_t *d_lut, uint8_t *d_tone, uint8_t *d_small,
                                xrit_product_summary *d_summary, void *stream)
{
    if (!pr || !d_summary) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(check_image(image, params, d_table_in));
    if (((size_t)d_hist & 3) || ((size_t)d_summary & 7)) {
        set_error("product: the histogram must be 4-byte aligned, the summary 8-byte");
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(pr->device));
    return product_run(pr, *image, *params, d_table_in, d_hist, d_lut, d_tone, d_small, d_summary, (hipStream_t)stream);
}

// the call on an image in device memory, its outputs to host memory: one download behind the kernels, then the wait
static int product_to_host(xrit_product *pr, const xrit_product_image &im, const xrit_product_params &pp, const uint8_t *d_table_in,
                           uint32_t *hist, uint8_t *lut, uint8_t *tone, uint8_t *small, xrit_product_summary *summary, hipStream_t s)
{
    const size_t bins = (size_t)1 << im.bits;
    const size_t tone_bytes = tone ? (size_t)im.columns * im.rows : 0;
    const size_t small_bytes = small ? (size_t)product_small_dim(im.columns, pp.factor) * product_small_dim(im.rows, pp.factor) : 0;
    // the outputs behind one another: the summary, the toned image, the thumbnail (the histogram and the table are the scratch's)
    const size_t at_tone = sizeof(xrit_product_summary), at_small = at_tone + tone_bytes;
    XR_TRY(pr->h_out.reserve(at_small + small_bytes));
    uint8_t *d_out = pr->h_out.as<uint8_t>();
    pr->last_tone = tone_bytes ? d_out + at_tone : nullptr;
    pr->last_small = small_bytes ? d_out + at_small : nullptr;
    XR_TRY(product_run(pr, im, pp, d_table_in, nullptr, nullptr, tone_bytes ? d_out + at_tone : nullptr, small_bytes ? d_out + at_small : nullptr,
                       reinterpret_cast<xrit_product_summary *>(d_out), s));
    XR_HIP(hipMemcpyAsync(summary, d_out, sizeof *summary, hipMemcpyDeviceToHost, s));
    if (hist) XR_HIP(hipMemcpyAsync(hist, pr->hist(), bins * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (lut) XR_HIP(hipMemcpyAsync(lut, pr->lut(), bins, hipMemcpyDeviceToHost, s));
    if (tone_bytes) XR_HIP(hipMemcpyAsync(tone, d_out + at_tone, tone_bytes, hipMemcpyDeviceToHost, s));
    if (small_bytes) XR_HIP(hipMemcpyAsync(small, d_out + at_small, small_bytes, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}

static int upload_table(xrit_product *pr, const xrit_product_image &im, const xrit_product_params &pp, const uint8_t *table_in, hipStream_t s)
{
    if (pp.tone != XRIT_TONE_TABLE) return XRIT_OK;
    const size_t bins = (size_t)1 << im.bits;
    XR_TRY(pr->h_table.reserve(bins));
    XR_HIP(hipMemcpyAsync(pr->h_table.p, table_in, bins, hipMemcpyHostToDevice, s));
    return XRIT_OK;
}

int xrit_product_process(xrit_product *pr, const xrit_product_image *image, const xrit_product_params *params, const uint8_t *table_in,
                         uint32_t *hist, uint8_t *lut, uint8_t *tone, uint8_t *small, xrit_product_summary *summary)
{
    if (!pr || !summary) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(check_image(image, params, table_in));
    hipStream_t s;
    XR_TRY(pr->adopt_own_stream(s));
    const size_t in_bytes = (size_t)image->pitch * (image->rows - 1) + (size_t)image->columns * product_width(image->bits);
    XR_TRY(pr->h_in.reserve(in_bytes));
    XR_HIP(hipMemcpyAsync(pr->h_in.p, image->d_pixels, in_bytes, hipMemcpyHostToDevice, s));
    XR_TRY(upload_table(pr, *image, *params, table_in, s));
    xrit_product_image im = *image;
    im.d_pixels = pr->h_in.as<uint8_t>();
    return product_to_host(pr, im, *params, pr->h_table.as<uint8_t>(), hist, lut, tone, small, summary, s);
}

int xrit_product_process_resident(xrit_product *pr, const xrit_product_image *image, const xrit_product_params *params,
                                  const uint8_t *table_in, uint32_t *hist, uint8_t *lut, uint8_t *tone, uint8_t *small,
                                  xrit_product_summary *summary)
{
    if (!pr || !summary) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(check_image(image, params, table_in));
    hipStream_t s;
    XR_TRY(pr->adopt_own_stream(s));
    XR_TRY(upload_table(pr, *image, *params, table_in, s));
    return product_to_host(pr, *image, *params, pr->h_table.as<uint8_t>(), hist, lut, tone, small, summary, s);
}

int xrit_product_outputs_device(xrit_product *pr, const uint8_t **d_tone, const uint8_t **d_small)
{
    if (!pr || !d_tone || !d_small) { set_error("null argument"); return XRIT_E_INVALID; }
    *d_tone = pr->last_tone;
    *d_small = pr->last_small;
    return XRIT_OK;
}

static int check_composite(const xrit_product *pr, const void *a, uint32_t pitch_a, const void *b, uint32_t pitch_b, uint32_t columns,
                           uint32_t rows, const void *table, const void *rgb)
{
    if (!pr || !a || !b || !table || !rgb) { set_error("null argument"); return XRIT_E_INVALID; }
    if (columns < 1 || rows < 1 || (uint64_t)columns * rows > MAX_PIXELS || pitch_a < columns || pitch_b < columns) {
        set_error("product: columns, rows >= 1, columns * rows <= 2^31, both pitches >= columns");
        return XRIT_E_INVALID;
    }
    return XRIT_OK;
}

int xrit_product_composite_device(xrit_product *pr, const uint8_t *d_a, uint32_t pitch_a, const uint8_t *d_b, uint32_t pitch_b,
                                  uint32_t columns, uint32_t rows, const uint8_t *d_table, uint8_t *d_rgb, void *stream)
{
    XR_TRY(check_composite(pr, d_a, pitch_a, d_b, pitch_b, columns, rows, d_table, d_rgb));
    XR_HIP(hipSetDevice(pr->device));
    XR_TRY(launch_product_composite(d_a, pitch_a, d_b, pitch_b, columns, rows, d_table, d_rgb, (hipStream_t)stream));
    pr->ran_on((hipStream_t)stream);
    return XRIT_OK;
}

int xrit_product_composite(xrit_product *pr, const uint8_t *a, uint32_t pitch_a, const uint8_t *b, uint32_t pitch_b, uint32_t columns,
                           uint32_t rows, const uint8_t *table, uint8_t *rgb)
{
    XR_TRY(check_composite(pr, a, pitch_a, b, pitch_b, columns, rows, table, rgb));
    hipStream_t s;
    XR_TRY(pr->adopt_own_stream(s));
    const size_t a_bytes = (size_t)pitch_a * (rows - 1) + columns, b_bytes = (size_t)pitch_b * (rows - 1) + columns;
    const size_t at_b = (a_bytes + 15) & ~(size_t)15, rgb_bytes = (size_t)columns * rows * 3;
    XR_TRY(pr->h_in.reserve(at_b + b_bytes));
    XR_TRY(pr->h_table.reserve(COMPOSITE_TABLE_BYTES));
    XR_TRY(pr->h_out.reserve(rgb_bytes));
    uint8_t *d_in = pr->h_in.as<uint8_t>();
    XR_HIP(hipMemcpyAsync(d_in, a, a_bytes, hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(d_in + at_b, b, b_bytes, hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(pr->h_table.p, table, COMPOSITE_TABLE_BYTES, hipMemcpyHostToDevice, s));
    XR_TRY(launch_product_composite(d_in, pitch_a, d_in + at_b, pitch_b, columns, rows, pr->h_table.as<uint8_t>(), pr->h_out.as<uint8_t>(), s));
    pr->ran_on(s);
    XR_HIP(hipMemcpyAsync(rgb, pr->h_out.p, rgb_bytes, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}
