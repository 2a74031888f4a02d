// files.cpp -- C ABI of the file assembler (include/xritdemod_amd.h, "File assembler and Rice decoder"): the handle owns
// the per-key state (64 x 2048 xrit_file_key records), the counters and grow-only scratch in device memory; the kernels
// are in files.hip.
#include <cstddef>

#include "common.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_file_piece) == 32 && offsetof(xrit_file_piece, length) == 8 && offsetof(xrit_file_piece, file) == 16 &&
                  offsetof(xrit_file_piece, vcid) == 24,
              "xrit_file_piece layout (PIECE_DTYPE mirrors it; offset and length lie as in xrit_packet)");
static_assert(offsetof(xrit_file_piece, offset) == offsetof(xrit_packet, offset) &&
                  offsetof(xrit_file_piece, length) == offsetof(xrit_packet, length),
              "either record serves as a Rice line descriptor");
static_assert(sizeof(xrit_file_record) == 80 && offsetof(xrit_file_record, header_length) == 40 &&
                  offsetof(xrit_file_record, file_counter) == 56 && offsetof(xrit_file_record, vcid) == 66,
              "xrit_file_record layout (RECORD_DTYPE mirrors it)");
static_assert(sizeof(xrit_files_summary) == 104 && offsetof(xrit_files_summary, overflow) == 96, "xrit_files_summary layout");
static_assert(sizeof(xrit_files_counters) == 80, "xrit_files_counters layout");
static_assert(sizeof(xrit_file_key) == 56 && offsetof(xrit_file_key, next_seq) == 36 && offsetof(xrit_file_key, open) == 46,
              "xrit_file_key layout");

namespace {
constexpr size_t STATE_BYTES = (size_t)FILES_KEYS * sizeof(xrit_file_key) + sizeof(xrit_files_counters);
}

struct xrit_files : StageHandle {
    DevBuf state, scratch;                          // the keys, then the counters
    DevBuf h_in, h_packets, h_offsets, h_bytes, h_pieces, h_files, h_summary;
    xrit_file_key *keys() const { return state.as<xrit_file_key>(); }
    xrit_files_counters *counters() const { return reinterpret_cast<xrit_files_counters *>(keys() + FILES_KEYS); }
    void close_all() { close({&state, &scratch, &h_in, &h_packets, &h_offsets, &h_bytes, &h_pieces, &h_files, &h_summary}); }
};

int xrit_files_create(xrit_files **out, int device)
{
    return stage_create(out, device, [](xrit_files &fa) {
        XR_TRY(fa.state.reserve(STATE_BYTES));
        return xrit_files_reset(&fa);
    });
}

int xrit_files_destroy(xrit_files *fa) { return stage_destroy(fa); }

int xrit_files_reset(xrit_files *fa)
{
    if (!fa) { set_error("null argument"); return XRIT_E_INVALID; }
    return fa->write_state(fa->state.p, nullptr, STATE_BYTES);
}

static int files_run(xrit_files *fa, const uint8_t *d_in, size_t in_bytes, const xrit_packet *d_packets, const uint32_t *d_pkt_offsets,
                     size_t max_in, uint8_t *d_bytes, size_t max_bytes, xrit_file_piece *d_pieces, size_t max_pieces,
                     xrit_file_record *d_files, size_t max_files, xrit_files_summary *d_summary, hipStream_t s)
{
    FilesScratch sc;
    XR_TRY(fa->scratch.reserve(files_scratch_carve(nullptr, max_in, sc)));
    files_scratch_carve(fa->scratch.p, max_in, sc);
    XR_TRY(launch_files(d_in, in_bytes, d_packets, d_pkt_offsets, max_in, fa->keys(), fa->counters(), sc, d_bytes, max_bytes, d_pieces,
                        max_pieces, d_files, max_files, d_summary, s));
    fa->ran_on(s);
    return XRIT_OK;
}

int xrit_files_process_device(xrit_files *fa, const uint8_t *d_in_bytes, size_t in_bytes, const xrit_packet *d_packets,
                              const uint32_t *d_pkt_offsets, size_t max_packets_in, uint8_t *d_bytes, size_t max_bytes,
                              xrit_file_piece *d_pieces, size_t max_pieces, xrit_file_record *d_files, size_t max_files,
                              xrit_files_summary *d_summary, void *stream)
{
    if (!fa || !d_pkt_offsets || !d_summary || (in_bytes && !d_in_bytes) || (max_packets_in && !d_packets) || (max_bytes && !d_bytes) ||
        (max_pieces && !d_pieces) || (max_files && !d_files)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    if (max_packets_in > XRIT_FILES_MAX_PACKETS) {
        set_error("files: at most %zu packets per call", XRIT_FILES_MAX_PACKETS);
        return XRIT_E_INVALID;
    }
    if (((size_t)d_packets | (size_t)d_pieces | (size_t)d_files | (size_t)d_summary) & 7) {
        set_error("files: the descriptors, the records and the summary must be 8-byte aligned");
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(fa->device));
    return files_run(fa, d_in_bytes, in_bytes, d_packets, d_pkt_offsets, max_packets_in, d_bytes, max_bytes, d_pieces, max_pieces, d_files,
                     max_files, d_summary, (hipStream_t)stream);
}

int xrit_files_process(xrit_files *fa, const uint8_t *in_bytes, size_t n_in_bytes, const xrit_packet *packets,
                       const uint32_t *pkt_offsets, uint8_t *bytes, size_t max_bytes, xrit_file_piece *pieces, size_t max_pieces,
                       xrit_file_record *files, size_t max_files, xrit_files_summary *summary)
{
    if (!fa || !pkt_offsets || !summary || (n_in_bytes && !in_bytes) || (max_bytes && !bytes) || (max_pieces && !pieces) ||
        (max_files && !files)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    const size_t n = pkt_offsets[NVC];
    if (n && !packets) { set_error("null argument"); return XRIT_E_INVALID; }
    if (n > XRIT_FILES_MAX_PACKETS) { set_error("files: at most %zu packets per call", XRIT_FILES_MAX_PACKETS); return XRIT_E_INVALID; }
    hipStream_t s;
    XR_TRY(fa->adopt_own_stream(s));
    // no call emits more than this, so the device side of a generous host buffer stays small
    const size_t bound_files = XRIT_FILES_MAX_FILES(n);
    const size_t cap_bytes = max_bytes < n_in_bytes ? max_bytes : n_in_bytes;
    const size_t cap_pieces = max_pieces < n ? max_pieces : n;
    const size_t cap_files = max_files < bound_files ? max_files : bound_files;
    XR_TRY(fa->h_in.reserve(n_in_bytes + 8));
    XR_TRY(fa->h_packets.reserve(n * sizeof(xrit_packet) + 8));
    XR_TRY(fa->h_offsets.reserve((NVC + 1) * sizeof(uint32_t)));
    XR_TRY(fa->h_bytes.reserve(cap_bytes + 8));
    XR_TRY(fa->h_pieces.reserve(cap_pieces * sizeof(xrit_file_piece) + 8));
    XR_TRY(fa->h_files.reserve(cap_files * sizeof(xrit_file_record) + 8));
    XR_TRY(fa->h_summary.reserve(sizeof(xrit_files_summary)));
    if (n_in_bytes) XR_HIP(hipMemcpyAsync(fa->h_in.p, in_bytes, n_in_bytes, hipMemcpyHostToDevice, s));
    if (n) XR_HIP(hipMemcpyAsync(fa->h_packets.p, packets, n * sizeof(xrit_packet), hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(fa->h_offsets.p, pkt_offsets, (NVC + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    XR_TRY(files_run(fa, fa->h_in.as<uint8_t>(), n_in_bytes, fa->h_packets.as<xrit_packet>(), fa->h_offsets.as<uint32_t>(), n,
                     fa->h_bytes.as<uint8_t>(), cap_bytes, fa->h_pieces.as<xrit_file_piece>(), cap_pieces,
                     fa->h_files.as<xrit_file_record>(), cap_files, fa->h_summary.as<xrit_files_summary>(), s));
    // the written prefix: descriptors and records below their capacities; bytes up to the capacity (a piece's bytes are
    // written iff it fits whole, so what lies beyond the last one that fits is not meaningful)
    return download_written(s, "files", summary, fa->h_summary.p, sizeof *summary, &summary->overflow,
                            {{pieces, fa->h_pieces.p, sizeof(xrit_file_piece), &summary->pieces, cap_pieces, "pieces"},
                             {bytes, fa->h_bytes.p, 1, &summary->bytes, cap_bytes, "bytes"},
                             {files, fa->h_files.p, sizeof(xrit_file_record), &summary->files, cap_files, "records"}});
}

int xrit_files_stats(xrit_files *fa, xrit_files_counters *out)
{
    if (!fa || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    return fa->read_back(out, fa->counters(), sizeof *out);
}

int xrit_files_key(xrit_files *fa, unsigned vcid, unsigned apid, xrit_file_key *out)
{
    if (!fa || !out || vcid >= (unsigned)NVC || apid >= 2048) { set_error("files: null argument or no such key"); return XRIT_E_INVALID; }
    return fa->read_back(out, fa->keys() + (size_t)vcid * 2048 + apid, sizeof *out);
}
