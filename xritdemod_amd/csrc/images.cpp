// images.cpp -- C ABI of the image stage (include/xritdemod_amd.h, "Image lines"): the handle owns the per-key state
// (64 x 2048 xrit_image_key records), the counters and grow-only scratch in device memory; the kernels are in images.hip.
#include <cstddef>

#include "common.h"
#include "image_rule.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_image_line) == 32 && offsetof(xrit_image_line, length) == 8 && offsetof(xrit_image_line, row) == 12 &&
                  offsetof(xrit_image_line, piece) == 20 && offsetof(xrit_image_line, samples) == 24 && offsetof(xrit_image_line, status) == 27,
              "xrit_image_line layout (IMAGE_LINE_DTYPE mirrors it; offset and length lie as in xrit_packet)");
static_assert(sizeof(xrit_image_file) == 48 && offsetof(xrit_image_file, first_line) == 16 && offsetof(xrit_image_file, faults) == 28 &&
                  offsetof(xrit_image_file, columns) == 40 && offsetof(xrit_image_file, rice) == 43,
              "xrit_image_file layout (IMAGE_FILE_DTYPE mirrors it)");
static_assert(sizeof(xrit_images_summary) == 80 && offsetof(xrit_images_summary, overflow) == 72, "xrit_images_summary layout");
static_assert(sizeof(xrit_images_counters) == 48, "xrit_images_counters layout");
static_assert(sizeof(xrit_image_key) == 16 && offsetof(xrit_image_key, open) == 12, "xrit_image_key layout");

namespace {
constexpr size_t STATE_BYTES = (size_t)FILES_KEYS * sizeof(xrit_image_key) + sizeof(xrit_images_counters);
}

struct xrit_images : StageHandle {
    DevBuf state, scratch;                          // the keys, then the counters
    DevBuf h_bytes, h_pieces, h_files, h_fsum, h_out, h_lines, h_ifiles, h_summary;
    xrit_image_key *keys() const { return state.as<xrit_image_key>(); }
    xrit_images_counters *counters() const { return reinterpret_cast<xrit_images_counters *>(keys() + FILES_KEYS); }
    void close_all() { close({&state, &scratch, &h_bytes, &h_pieces, &h_files, &h_fsum, &h_out, &h_lines, &h_ifiles, &h_summary}); }
};

int xrit_images_create(xrit_images **out, int device)
{
    return stage_create(out, device, [](xrit_images &im) {
        XR_TRY(im.state.reserve(STATE_BYTES));
        return xrit_images_reset(&im);
    });
}

int xrit_images_destroy(xrit_images *im) { return stage_destroy(im); }

int xrit_images_reset(xrit_images *im)
{
    if (!im) { set_error("null argument"); return XRIT_E_INVALID; }
    return im->write_state(im->state.p, nullptr, STATE_BYTES);
}

static int images_run(xrit_images *im, const uint8_t *d_bytes, size_t n_bytes, const xrit_file_piece *d_pieces, size_t max_pieces_in,
                      const xrit_file_record *d_files, size_t max_files_in, const xrit_files_summary *d_fsum, uint8_t *d_out,
                      size_t max_bytes, xrit_image_line *d_lines, size_t max_lines, xrit_image_file *d_ifiles,
                      xrit_images_summary *d_summary, hipStream_t s)
{
    ImagesScratch sc;
    XR_TRY(im->scratch.reserve(images_scratch_carve(nullptr, max_files_in, max_pieces_in, sc)));
    images_scratch_carve(im->scratch.p, max_files_in, max_pieces_in, sc);
    XR_TRY(launch_images(d_bytes, n_bytes, d_pieces, max_pieces_in, d_files, max_files_in, d_fsum, im->keys(), im->counters(), sc, d_out,
                         max_bytes, d_lines, max_lines, d_ifiles, d_summary, s));
    im->ran_on(s);
    return XRIT_OK;
}

static int check_bounds(size_t max_pieces_in, size_t max_files_in)
{
    if (max_pieces_in > XRIT_IMAGES_MAX_PIECES || max_files_in > XRIT_IMAGES_MAX_FILES) {
        set_error("images: at most %zu pieces and %zu records per call", XRIT_IMAGES_MAX_PIECES, XRIT_IMAGES_MAX_FILES);
        return XRIT_E_INVALID;
    }
    return XRIT_OK;
}

int xrit_images_process_device(xrit_images *im, const uint8_t *d_bytes, size_t n_bytes, const xrit_file_piece *d_pieces,
                               size_t max_pieces_in, const xrit_file_record *d_files, size_t max_files_in,
                               const xrit_files_summary *d_files_summary, uint8_t *d_out, size_t max_bytes, xrit_image_line *d_lines,
                               size_t max_lines, xrit_image_file *d_image_files, xrit_images_summary *d_summary, void *stream)
{
    if (!im || !d_files_summary || !d_summary || (n_bytes && !d_bytes) || (max_pieces_in && !d_pieces) ||
        (max_files_in && (!d_files || !d_image_files)) || (max_bytes && !d_out) || (max_lines && !d_lines)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    XR_TRY(check_bounds(max_pieces_in, max_files_in));
    if (((size_t)d_pieces | (size_t)d_files | (size_t)d_files_summary | (size_t)d_out | (size_t)d_lines | (size_t)d_image_files |
         (size_t)d_summary) & 7) {
        set_error("images: the descriptors, the records, the image bytes and the summaries must be 8-byte aligned");
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(im->device));
    return images_run(im, d_bytes, n_bytes, d_pieces, max_pieces_in, d_files, max_files_in, d_files_summary, d_out, max_bytes, d_lines,
                      max_lines, d_image_files, d_summary, (hipStream_t)stream);
}

int xrit_images_process(xrit_images *im, const uint8_t *bytes, size_t n_bytes, const xrit_file_piece *pieces, size_t n_pieces_in,
                        const xrit_file_record *files, size_t n_files_in, const xrit_files_summary *files_summary, uint8_t *out,
                        size_t max_bytes, xrit_image_line *lines, size_t max_lines, xrit_image_file *image_files,
                        xrit_images_summary *summary)
{
    if (!im || !files_summary || !summary || (n_bytes && !bytes) || (n_pieces_in && !pieces) || (n_files_in && (!files || !image_files)) ||
        (max_bytes && !out) || (max_lines && !lines)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    XR_TRY(check_bounds(n_pieces_in, n_files_in));
    hipStream_t s;
    XR_TRY(im->adopt_own_stream(s));
    // no call emits more than this, so the device side of a generous host buffer stays small: every piece of a record a
    // line of the record's width (the records are at hand here; a record that is garbage adds at most a line per piece)
    size_t bound_bytes = 0;
    for (size_t i = 0; i < n_files_in; ++i)
        if (image_params_ok(files[i])) bound_bytes += (size_t)files[i].n_pieces * ((image_line_bytes(files[i]) + 3u) & ~(size_t)3);
    const size_t cap_bytes = max_bytes < bound_bytes ? max_bytes : bound_bytes;
    const size_t cap_lines = max_lines < n_pieces_in ? max_lines : n_pieces_in;
    XR_TRY(im->h_bytes.reserve(n_bytes + 8));
    XR_TRY(im->h_pieces.reserve(n_pieces_in * sizeof(xrit_file_piece) + 8));
    XR_TRY(im->h_files.reserve(n_files_in * sizeof(xrit_file_record) + 8));
    XR_TRY(im->h_fsum.reserve(sizeof(xrit_files_summary)));
    XR_TRY(im->h_out.reserve(cap_bytes + 8));
    XR_TRY(im->h_lines.reserve(cap_lines * sizeof(xrit_image_line) + 8));
    XR_TRY(im->h_ifiles.reserve(n_files_in * sizeof(xrit_image_file) + 8));
    XR_TRY(im->h_summary.reserve(sizeof(xrit_images_summary)));
    if (n_bytes) XR_HIP(hipMemcpyAsync(im->h_bytes.p, bytes, n_bytes, hipMemcpyHostToDevice, s));
    if (n_pieces_in) XR_HIP(hipMemcpyAsync(im->h_pieces.p, pieces, n_pieces_in * sizeof(xrit_file_piece), hipMemcpyHostToDevice, s));
    if (n_files_in) XR_HIP(hipMemcpyAsync(im->h_files.p, files, n_files_in * sizeof(xrit_file_record), hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(im->h_fsum.p, files_summary, sizeof *files_summary, hipMemcpyHostToDevice, s));
    XR_TRY(images_run(im, im->h_bytes.as<uint8_t>(), n_bytes, im->h_pieces.as<xrit_file_piece>(), n_pieces_in,
                      im->h_files.as<xrit_file_record>(), n_files_in, im->h_fsum.as<xrit_files_summary>(), im->h_out.as<uint8_t>(), cap_bytes,
                      im->h_lines.as<xrit_image_line>(), cap_lines, im->h_ifiles.as<xrit_image_file>(), im->h_summary.as<xrit_images_summary>(),
                      s));
    // a refused call wrote its summary alone
    XR_HIP(hipMemcpyAsync(summary, im->h_summary.p, sizeof *summary, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    if (summary->overflow == 2) {
        set_error("images: the files summary has overflow != 0 or counts beyond the %zu pieces and %zu records handed over", n_pieces_in,
                  n_files_in);
        return XRIT_E_ARG;
    }
    // the device's capacities are the host's cut at the bounds above: what exceeds them exceeds the host's too
    const uint64_t n_files = files_summary->files;
    return download_written(s, "images", summary, im->h_summary.p, sizeof *summary, &summary->overflow,
                            {{lines, im->h_lines.p, sizeof(xrit_image_line), &summary->lines, cap_lines, "lines"},
                             {out, im->h_out.p, 1, &summary->bytes, cap_bytes, "bytes"},
                             {image_files, im->h_ifiles.p, sizeof(xrit_image_file), &n_files, n_files_in, "records"}});
}

int xrit_images_stats(xrit_images *im, xrit_images_counters *out)
{
    if (!im || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    return im->read_back(out, im->counters(), sizeof *out);
}

int xrit_images_key(xrit_images *im, unsigned vcid, unsigned apid, xrit_image_key *out)
{
    if (!im || !out || vcid >= (unsigned)NVC || apid >= 2048) { set_error("images: null argument or no such key"); return XRIT_E_INVALID; }
    return im->read_back(out, im->keys() + (size_t)vcid * 2048 + apid, sizeof *out);
}
