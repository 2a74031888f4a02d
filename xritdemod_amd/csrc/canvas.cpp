// canvas.cpp -- C ABI of the canvas stage (include/xritdemod_amd.h, "Image canvases"): the handle owns the slot table, the
// segment tables, the per-key state (64 x 2048 xrit_canvas_key_state records), the counters, the pixels (allocated once) and
// grow-only scratch in device memory; the kernels are in canvas.hip.
#include <cstddef>

#include "canvas_rule.h"
#include "common.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_canvas_file) == 32 && offsetof(xrit_canvas_file, reason) == 4 && offsetof(xrit_canvas_file, faults) == 28,
              "xrit_canvas_file layout (CANVAS_FILE_DTYPE mirrors it)");
static_assert(sizeof(xrit_canvas_slot) == 136 && offsetof(xrit_canvas_slot, image_id) == 24 && offsetof(xrit_canvas_slot, pitch) == 40 &&
                  offsetof(xrit_canvas_slot, generation) == 52 && offsetof(xrit_canvas_slot, in_use) == 64 &&
                  offsetof(xrit_canvas_slot, name) == 72,
              "xrit_canvas_slot layout (CANVAS_SLOT_DTYPE mirrors it)");
static_assert(sizeof(xrit_canvas_segment) == 32 && offsetof(xrit_canvas_segment, placed) == 16 && offsetof(xrit_canvas_segment, apid) == 28 &&
                  offsetof(xrit_canvas_segment, begun) == 30,
              "xrit_canvas_segment layout (CANVAS_SEGMENT_DTYPE mirrors it)");
static_assert(sizeof(xrit_canvas_key_state) == 32 && offsetof(xrit_canvas_key_state, lines) == 24 && offsetof(xrit_canvas_key_state, placed) == 28,
              "xrit_canvas_key_state layout (CANVAS_KEY_DTYPE mirrors it)");
static_assert(sizeof(xrit_canvas_counters) == 120, "xrit_canvas_counters layout");
static_assert(sizeof(xrit_canvas_summary) == 168 && offsetof(xrit_canvas_summary, calls) == 40 && offsetof(xrit_canvas_summary, overflow) == 160,
              "xrit_canvas_summary layout: the counters lie behind the call's five counts");
static_assert(sizeof(CanvasHead) == 40 && sizeof(CanvasPlace) == 24, "the scratch records of canvas.hip");

namespace {
constexpr size_t SLOTS_BYTES = (size_t)XRIT_CANVAS_MAX_SLOTS * sizeof(xrit_canvas_slot);
constexpr size_t SEGS_BYTES = (size_t)XRIT_CANVAS_MAX_SLOTS * XRIT_CANVAS_MAX_SEGMENTS * sizeof(xrit_canvas_segment);
constexpr size_t KEYS_BYTES = (size_t)FILES_KEYS * sizeof(xrit_canvas_key_state);
constexpr size_t STATE_BYTES = SLOTS_BYTES + SEGS_BYTES + KEYS_BYTES + sizeof(xrit_canvas_counters);
}  // namespace

struct xrit_canvas : StageHandle {
    unsigned n_slots = 0;
    size_t slot_bytes = 0;
    DevBuf state, pixels, scratch;                  // the slots, their segments, the keys, then the counters
    DevBuf h_bytes, h_pieces, h_files, h_fsum, h_img, h_lines, h_ifiles, h_isum, h_cfiles, h_slots, h_summary;
    CanvasState st() const
    {
        char *p = state.as<char>();
        return CanvasState{reinterpret_cast<xrit_canvas_slot *>(p), reinterpret_cast<xrit_canvas_segment *>(p + SLOTS_BYTES),
                           reinterpret_cast<xrit_canvas_key_state *>(p + SLOTS_BYTES + SEGS_BYTES),
                           reinterpret_cast<xrit_canvas_counters *>(p + SLOTS_BYTES + SEGS_BYTES + KEYS_BYTES), pixels.as<unsigned char>(),
                           n_slots, slot_bytes};
    }
    void close_all()
    {
        close({&state, &pixels, &scratch, &h_bytes, &h_pieces, &h_files, &h_fsum, &h_img, &h_lines, &h_ifiles, &h_isum, &h_cfiles, &h_slots,
               &h_summary});
    }
};

int xrit_canvas_create(xrit_canvas **out, int device, unsigned slots, size_t slot_bytes)
{
    if (!out) { set_error("null argument"); return XRIT_E_INVALID; }
    *out = nullptr;
    if (slots < 1 || slots > XRIT_CANVAS_MAX_SLOTS || slot_bytes == 0 || (slot_bytes & 15)) {
        set_error("canvas: 1 .. %d slots of a multiple of 16 bytes each", XRIT_CANVAS_MAX_SLOTS);
        return XRIT_E_INVALID;
    }
    return stage_create(out, device, [&](xrit_canvas &cv) {
        cv.n_slots = slots;
        cv.slot_bytes = slot_bytes;
        XR_TRY(cv.state.reserve(STATE_BYTES));
        // exactly slots x slot_bytes, once (DevBuf::reserve would add its growth margin)
        if (hipMalloc(&cv.pixels.p, (size_t)slots * slot_bytes) != hipSuccess) {
            cv.pixels.p = nullptr;
            set_error("canvas: hipMalloc(%zu) failed", (size_t)slots * slot_bytes);
            return (int)XRIT_E_NOMEM;
        }
        cv.pixels.bytes = (size_t)slots * slot_bytes;
        return xrit_canvas_reset(&cv);
    });
}

int xrit_canvas_destroy(xrit_canvas *cv) { return stage_destroy(cv); }

int xrit_canvas_reset(xrit_canvas *cv)
{
    if (!cv) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(cv->write_state(cv->pixels.p, nullptr, (size_t)cv->n_slots * cv->slot_bytes));
    return cv->write_state(cv->state.p, nullptr, STATE_BYTES);
}

static int canvas_run(xrit_canvas *cv, const uint8_t *d_bytes, const xrit_file_piece *d_pieces, const xrit_file_record *d_files,
                      const xrit_files_summary *d_fsum, const uint8_t *d_img, const xrit_image_line *d_lines,
                      const xrit_image_file *d_ifiles, const xrit_images_summary *d_isum, const CanvasBounds &b,
                      xrit_canvas_file *d_cfiles, xrit_canvas_slot *d_slots, xrit_canvas_summary *d_summary, hipStream_t s)
{
    CanvasScratch sc;
    XR_TRY(cv->scratch.reserve(canvas_scratch_carve(nullptr, b.max_files, sc)));
    canvas_scratch_carve(cv->scratch.p, b.max_files, sc);
    XR_TRY(launch_canvas(d_bytes, d_pieces, d_files, d_fsum, d_img, d_lines, d_ifiles, d_isum, b, cv->st(), sc, d_cfiles, d_slots, d_summary,
                         s));
    cv->ran_on(s);
    return XRIT_OK;
}

static int check_bounds(size_t max_pieces_in, size_t max_files_in, size_t max_lines_in)
{
    if (max_pieces_in > XRIT_IMAGES_MAX_PIECES || max_files_in > XRIT_IMAGES_MAX_FILES || max_lines_in > XRIT_IMAGES_MAX_PIECES) {
        set_error("canvas: at most %zu pieces, %zu records and %zu lines per call", XRIT_IMAGES_MAX_PIECES, XRIT_IMAGES_MAX_FILES,
                  XRIT_IMAGES_MAX_PIECES);
        return XRIT_E_INVALID;
    }
    return XRIT_OK;
}

int xrit_canvas_process_device(xrit_canvas *cv, const uint8_t *d_bytes, size_t n_bytes, const xrit_file_piece *d_pieces,
                               size_t max_pieces_in, const xrit_file_record *d_files, size_t max_files_in,
                               const xrit_files_summary *d_files_summary, const uint8_t *d_image_bytes, size_t n_image_bytes,
                               const xrit_image_line *d_lines, size_t max_lines_in, const xrit_image_file *d_image_files,
                               const xrit_images_summary *d_images_summary, xrit_canvas_file *d_canvas_files, xrit_canvas_slot *d_slots,
                               xrit_canvas_summary *d_summary, void *stream)
{
    if (!cv || !d_files_summary || !d_images_summary || !d_summary || !d_slots || (n_bytes && !d_bytes) || (max_pieces_in && !d_pieces) ||
        (max_files_in && (!d_files || !d_image_files || !d_canvas_files)) || (n_image_bytes && !d_image_bytes) || (max_lines_in && !d_lines)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    XR_TRY(check_bounds(max_pieces_in, max_files_in, max_lines_in));
    if ((((size_t)d_pieces | (size_t)d_files | (size_t)d_files_summary | (size_t)d_lines | (size_t)d_image_files | (size_t)d_images_summary |
          (size_t)d_canvas_files | (size_t)d_slots | (size_t)d_summary) & 7) || ((size_t)d_image_bytes & 3)) {
        set_error("canvas: the descriptors, the records, the slot table and the summaries must be 8-byte aligned, the image bytes 4-byte");
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(cv->device));
    const CanvasBounds b{n_bytes, max_pieces_in, max_files_in, n_image_bytes, max_lines_in};
    return canvas_run(cv, d_bytes, d_pieces, d_files, d_files_summary, d_image_bytes, d_lines, d_image_files, d_images_summary, b,
                      d_canvas_files, d_slots, d_summary, (hipStream_t)stream);
}

int xrit_canvas_process(xrit_canvas *cv, const uint8_t *bytes, size_t n_bytes, const xrit_file_piece *pieces, size_t n_pieces_in,
                        const xrit_file_record *files, size_t n_files_in, const xrit_files_summary *files_summary,
                        const uint8_t *image_bytes, size_t n_image_bytes, const xrit_image_line *lines, size_t n_lines_in,
                        const xrit_image_file *image_files, const xrit_images_summary *images_summary, xrit_canvas_file *canvas_files,
                        xrit_canvas_slot *slots, xrit_canvas_summary *summary)
{
    if (!cv || !files_summary || !images_summary || !summary || !slots || (n_bytes && !bytes) || (n_pieces_in && !pieces) ||
        (n_files_in && (!files || !image_files || !canvas_files)) || (n_image_bytes && !image_bytes) || (n_lines_in && !lines)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    XR_TRY(check_bounds(n_pieces_in, n_files_in, n_lines_in));
    hipStream_t s;
    XR_TRY(cv->adopt_own_stream(s));
    struct Up { DevBuf *buf; const void *src; size_t bytes; };
    const Up ups[] = {{&cv->h_bytes, bytes, n_bytes},
                      {&cv->h_pieces, pieces, n_pieces_in * sizeof(xrit_file_piece)},
                      {&cv->h_files, files, n_files_in * sizeof(xrit_file_record)},
                      {&cv->h_fsum, files_summary, sizeof *files_summary},
                      {&cv->h_img, image_bytes, n_image_bytes},
                      {&cv->h_lines, lines, n_lines_in * sizeof(xrit_image_line)},
                      {&cv->h_ifiles, image_files, n_files_in * sizeof(xrit_image_file)},
                      {&cv->h_isum, images_summary, sizeof *images_summary}};
    for (const Up &u : ups) {
        XR_TRY(u.buf->reserve(u.bytes + 8));
        if (u.bytes) XR_HIP(hipMemcpyAsync(u.buf->p, u.src, u.bytes, hipMemcpyHostToDevice, s));
    }
    XR_TRY(cv->h_cfiles.reserve(n_files_in * sizeof(xrit_canvas_file) + 8));
    XR_TRY(cv->h_slots.reserve(SLOTS_BYTES));
    XR_TRY(cv->h_summary.reserve(sizeof(xrit_canvas_summary)));
    const CanvasBounds b{n_bytes, n_pieces_in, n_files_in, n_image_bytes, n_lines_in};
    XR_TRY(canvas_run(cv, cv->h_bytes.as<uint8_t>(), cv->h_pieces.as<xrit_file_piece>(), cv->h_files.as<xrit_file_record>(),
                      cv->h_fsum.as<xrit_files_summary>(), cv->h_img.as<uint8_t>(), cv->h_lines.as<xrit_image_line>(),
                      cv->h_ifiles.as<xrit_image_file>(), cv->h_isum.as<xrit_images_summary>(), b, cv->h_cfiles.as<xrit_canvas_file>(),
                      cv->h_slots.as<xrit_canvas_slot>(), cv->h_summary.as<xrit_canvas_summary>(), s));
    // a refused call wrote its summary alone
    XR_HIP(hipMemcpyAsync(summary, cv->h_summary.p, sizeof *summary, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    if (summary->overflow == 2) {
        set_error("canvas: a summary has overflow != 0 or counts beyond the %zu pieces, %zu records and %zu lines handed over", n_pieces_in,
                  n_files_in, n_lines_in);
        return XRIT_E_ARG;
    }
    const size_t n_files = (size_t)files_summary->files;
    if (n_files) XR_HIP(hipMemcpyAsync(canvas_files, cv->h_cfiles.p, n_files * sizeof(xrit_canvas_file), hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpyAsync(slots, cv->h_slots.p, cv->n_slots * sizeof(xrit_canvas_slot), hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}

static int check_slot(const xrit_canvas *cv, unsigned slot, const void *out)
{
    if (!cv || !out || slot >= cv->n_slots) { set_error("canvas: null argument or no such slot"); return XRIT_E_INVALID; }
    return XRIT_OK;
}

int xrit_canvas_read_device(xrit_canvas *cv, unsigned slot, uint8_t *d_out, size_t n_bytes, void *stream)
{
    XR_TRY(check_slot(cv, slot, d_out));
    if (n_bytes > cv->slot_bytes) { set_error("canvas: a slot has %zu bytes", cv->slot_bytes); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(cv->device));
    if (n_bytes)
        XR_HIP(hipMemcpyAsync(d_out, cv->st().pixels + (size_t)slot * cv->slot_bytes, n_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return XRIT_OK;
}

int xrit_canvas_pixels_device(xrit_canvas *cv, unsigned slot, const uint8_t **d_pixels)
{
    XR_TRY(check_slot(cv, slot, d_pixels));
    *d_pixels = cv->st().pixels + (size_t)slot * cv->slot_bytes;
    return XRIT_OK;
}

int xrit_canvas_read(xrit_canvas *cv, unsigned slot, uint8_t *out, size_t max_bytes, xrit_canvas_slot *info)
{
    XR_TRY(check_slot(cv, slot, info));
    XR_TRY(cv->read_back(info, cv->st().slots + slot, sizeof *info));
    const size_t n = (size_t)info->pitch * info->max_row;           // (the rule: at most slot_bytes)
    if (n > max_bytes || n > cv->slot_bytes || (n && !out)) {
        set_error("canvas: slot %u holds %zu bytes: the output buffer is too small", slot, n);
        return XRIT_E_CAPACITY;
    }
    return n ? cv->read_back(out, cv->st().pixels + (size_t)slot * cv->slot_bytes, n) : XRIT_OK;
}

int xrit_canvas_segments(xrit_canvas *cv, unsigned slot, xrit_canvas_segment *out)
{
    XR_TRY(check_slot(cv, slot, out));
    return cv->read_back(out, cv->st().segs + (size_t)slot * XRIT_CANVAS_MAX_SEGMENTS, XRIT_CANVAS_MAX_SEGMENTS * sizeof *out);
}

int xrit_canvas_key(xrit_canvas *cv, unsigned vcid, unsigned apid, xrit_canvas_key_state *out)
{
    if (!cv || !out || vcid >= (unsigned)NVC || apid >= 2048) { set_error("canvas: null argument or no such key"); return XRIT_E_INVALID; }
    return cv->read_back(out, cv->st().keys + (size_t)vcid * 2048 + apid, sizeof *out);
}

int xrit_canvas_stats(xrit_canvas *cv, xrit_canvas_counters *out)
{
    if (!cv || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    return cv->read_back(out, cv->st().counters, sizeof *out);
}

int xrit_canvas_release(xrit_canvas *cv, unsigned slot)
{
    XR_TRY(check_slot(cv, slot, cv));
    XR_HIP(hipSetDevice(cv->device));
    return launch_canvas_release(cv->st(), slot, cv->last_stream);
}
