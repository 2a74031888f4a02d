// jpegdec.cpp -- C ABI of the JPEG decoder stage (include/xritdemod_amd.h, "JPEG decoder"): the handle owns the form, the
// scratch in device memory and the host-buffer form's staging; the header function is plain host code on jpegdec_rule.h; the
// kernels are in jpegdec.hip.
#include <cstddef>

#include "common.h"
#include "jpegdec_rule.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_jpegdec_record) == 64 && offsetof(xrit_jpegdec_record, columns) == 16 && offsetof(xrit_jpegdec_record, status) == 36,
              "xrit_jpegdec_record layout (JPEGDEC_RECORD_DTYPE mirrors it)");
static_assert(sizeof(xrit_jpegdec_summary) == 64 && offsetof(xrit_jpegdec_summary, by_status) == 16 && offsetof(xrit_jpegdec_summary, overflow) == 56,
              "xrit_jpegdec_summary layout (JPEGDEC_SUMMARY_DTYPE mirrors it)");
static_assert(sizeof(xrit_jpegdec_info) == 32, "xrit_jpegdec_info layout");
static_assert(XRIT_JPEGDEC_MAX_BLOCKS == JPEGDEC_MAX_BLOCKS && XRIT_JPEGDEC_MAX_BYTES == JPEGDEC_MAX_BYTES && XRIT_JPEGDEC_STATUSES == JPEGDEC_N_STATUS &&
                  XRIT_JPEGDEC_MARKER == JPEGDEC_MARKER,
              "the header's constants are the rule's");

struct xrit_jpegdec : StageHandle {
    uint32_t form = 1, S = JPEGDEC_DEFAULT_S;          // form 1 won on every measured input
    DevBuf scratch;                                 // jpegdec_scratch_carve's
    DevBuf h_in, h_out;                             // the host-buffer form's: bytes then records in; summary, records, pixels out
    uint32_t *d_rounds = nullptr;                   // in the scratch of the last call
    void close_all() { close({&scratch, &h_in, &h_out}); }
};

int xrit_jpegdec_create(xrit_jpegdec **out, int device)
{
    return stage_create(out, device, [&](xrit_jpegdec &) { return XRIT_OK; });
}

int xrit_jpegdec_destroy(xrit_jpegdec *d) { return stage_destroy(d); }

int xrit_jpegdec_reset(xrit_jpegdec *d)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    return d->wait_last();
}

int xrit_jpegdec_set_form(xrit_jpegdec *d, uint32_t form, uint32_t subsequence_bits)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    if (form > 1 || (subsequence_bits && (subsequence_bits < JPEGDEC_MIN_S || subsequence_bits > JPEGDEC_MAX_S))) {
        set_error("jpegdec: form 0 or 1, subsequences of 32 .. 2^20 bits (0: 1024)");
        return XRIT_E_INVALID;
    }
    d->form = form;
    d->S = subsequence_bits ? subsequence_bits : JPEGDEC_DEFAULT_S;
    return XRIT_OK;
}

int xrit_jpegdec_header(const uint8_t *data, size_t length, xrit_jpegdec_info *info)
{
    if (!info || (!data && length)) { set_error("null argument"); return XRIT_E_INVALID; }
    if (length > JPEGDEC_MAX_BYTES) { set_error("jpegdec: a stream of at most 2^28 bytes"); return XRIT_E_INVALID; }
    const JpegDecHeader h = jpegdec_parse_header(data, length);
    *info = xrit_jpegdec_info{h.columns, h.rows, h.comps, h.restart, h.status, h.scan, h.blocks, h.intervals};
    return XRIT_OK;
}

static int check_call(const xrit_jpegdec *d, const void *bytes, size_t n_bytes, const void *items, size_t stride, size_t n_items, size_t max_blocks,
                      const void *pixels, size_t cap, const void *records, const void *summary)
{
    if (!d || !summary || (!records && n_items) || (!items && n_items) || (!bytes && n_bytes) || (!pixels && cap)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    if (n_bytes > JPEGDEC_MAX_BYTES || n_items > XRIT_JPEGDEC_MAX_ITEMS || max_blocks > JPEGDEC_MAX_BLOCKS || stride < 12 || (stride & 3)) {
        set_error("jpegdec: at most 2^28 bytes, 2^20 items and 2^22 blocks; a stride of at least 12, a multiple of 4");
        return XRIT_E_INVALID;
    }
    return XRIT_OK;
}

static int jpegdec_run(xrit_jpegdec *d, const uint8_t *d_bytes, size_t n_bytes, const void *d_items, size_t stride, size_t n_items, size_t max_blocks,
                       uint8_t *d_pixels, size_t cap, xrit_jpegdec_record *d_records, xrit_jpegdec_summary *d_summary, hipStream_t s)
{
    const uint32_t blocks = max_blocks ? (uint32_t)max_blocks : XRIT_JPEGDEC_DEFAULT_BLOCKS, scan = n_bytes ? (uint32_t)n_bytes : 1u;
    JpegDecScratch sc;
    // a grown scratch is a new allocation: what the handle's last call still reads must have finished
    const size_t need = jpegdec_scratch_carve(nullptr, (uint32_t)n_items, scan, blocks, sc);
    if (need > d->scratch.bytes) XR_TRY(d->wait_last());
    XR_TRY(d->scratch.reserve(need));
    jpegdec_scratch_carve(d->scratch.p, (uint32_t)n_items, scan, blocks, sc);
    JpegDecPar p;
    p.bytes = d_bytes;
    p.n_bytes = n_bytes;
    p.items = static_cast<const unsigned char *>(d_items);
    p.stride = stride;
    p.n_items = (uint32_t)n_items;
    p.max_blocks = blocks;
    p.max_scan = scan;
    p.form = d->form;
    p.S = d->S;
    p.pixels = d_pixels;
    p.cap = cap;
    p.records = d_records;
    p.summary = d_summary;
    XR_TRY(launch_jpegdec(p, sc, s));
    d->d_rounds = sc.rounds;
    d->ran_on(s);
    return XRIT_OK;
}

int xrit_jpegdec_decode_device(xrit_jpegdec *d, const uint8_t *d_bytes, size_t n_bytes, const void *d_items, size_t stride, size_t n_items,
                               size_t max_blocks, uint8_t *d_pixels, size_t cap, xrit_jpegdec_record *d_records, xrit_jpegdec_summary *d_summary,
                               void *stream)
{
    XR_TRY(check_call(d, d_bytes, n_bytes, d_items, stride, n_items, max_blocks, d_pixels, cap, d_records, d_summary));
    if (((size_t)d_records | (size_t)d_summary) & 7) { set_error("jpegdec: the records and the summary must be 8-byte aligned"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(d->device));
    return jpegdec_run(d, d_bytes, n_bytes, d_items, stride, n_items, max_blocks, d_pixels, cap, d_records, d_summary, (hipStream_t)stream);
}

int xrit_jpegdec_decode(xrit_jpegdec *d, const uint8_t *bytes, size_t n_bytes, const void *items, size_t stride, size_t n_items, uint8_t *pixels,
                        size_t cap, xrit_jpegdec_record *records, xrit_jpegdec_summary *summary)
{
    XR_TRY(check_call(d, bytes, n_bytes, items, stride, n_items, 0, pixels, cap, records, summary));
    // the sizes from the headers, as the device will find them: the blocks of the sound items, their pixel bytes
    uint64_t blocks = 0, out_bytes = 0;
    for (size_t i = 0; i < n_items; ++i) {
        uint64_t off;
        uint32_t len;
        memcpy(&off, static_cast<const char *>(items) + i * stride, 8);
        memcpy(&len, static_cast<const char *>(items) + i * stride + 8, 4);
        if (off > n_bytes || len > n_bytes - off) continue;
        const JpegDecHeader h = jpegdec_parse_header(bytes + off, len);
        if (h.status != JPEGDEC_OK) continue;
        blocks += h.blocks;
        out_bytes += ((uint64_t)h.columns * h.rows * h.comps + 3) & ~3ull;
    }
    const size_t max_blocks = blocks < 1 ? 1 : blocks > JPEGDEC_MAX_BLOCKS ? JPEGDEC_MAX_BLOCKS : (size_t)blocks;
    const size_t d_cap = cap < out_bytes ? cap : (size_t)out_bytes;
    hipStream_t s;
    XR_TRY(d->adopt_own_stream(s));
    const size_t in_items = (n_bytes + 15) & ~(size_t)15, rec_at = 64, pix_at = (rec_at + n_items * sizeof(xrit_jpegdec_record) + 15) & ~(size_t)15;
    XR_TRY(d->h_in.reserve(in_items + n_items * stride + 16));
    XR_TRY(d->h_out.reserve(pix_at + d_cap + 16));
    uint8_t *d_in = d->h_in.as<uint8_t>(), *d_out = d->h_out.as<uint8_t>();
    if (n_bytes) XR_HIP(hipMemcpyAsync(d_in, bytes, n_bytes, hipMemcpyHostToDevice, s));
    if (n_items) XR_HIP(hipMemcpyAsync(d_in + in_items, items, n_items * stride, hipMemcpyHostToDevice, s));
    XR_TRY(jpegdec_run(d, d_in, n_bytes, d_in + in_items, stride, n_items, max_blocks, d_out + pix_at, d_cap,
                       reinterpret_cast<xrit_jpegdec_record *>(d_out + rec_at), reinterpret_cast<xrit_jpegdec_summary *>(d_out), s));
    XR_HIP(hipMemcpyAsync(summary, d_out, sizeof *summary, hipMemcpyDeviceToHost, s));
    if (n_items) XR_HIP(hipMemcpyAsync(records, d_out + rec_at, n_items * sizeof(xrit_jpegdec_record), hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    // the images that fitted are a prefix (offsets only grow): up to the end of the last one of them, which the kernels wrote
    size_t n = 0;
    for (size_t i = 0; i < n_items; ++i) {
        const uint64_t end = records[i].offset + ((records[i].length + 3) & ~3ull);
        if (records[i].length && end <= d_cap) n = (size_t)end;
    }
    if (n) XR_HIP(hipMemcpyAsync(pixels, d_out + pix_at, n, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    if (!summary->overflow) return XRIT_OK;
    set_error("jpegdec: %llu pixel bytes: the output buffer is too small", (unsigned long long)summary->bytes);
    return XRIT_E_CAPACITY;
}

int xrit_jpegdec_rounds(xrit_jpegdec *d, uint32_t *rounds)
{
    if (!d || !rounds) { set_error("null argument"); return XRIT_E_INVALID; }
    *rounds = 0;
    if (!d->d_rounds) return XRIT_OK;
    return d->read_back(rounds, d->d_rounds, sizeof *rounds);
}
