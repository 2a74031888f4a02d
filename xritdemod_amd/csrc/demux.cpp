// demux.cpp -- C ABI of the channel demultiplexer (include/xritdemod_amd.h, "Channel demultiplexer"): the handle owns the
// counters of newdecoder.cpp:44-53 in device memory and grow-only scratch; the kernels are in demux.hip.
#include <cstddef>
#include <ctime>

#include "common.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_frame_stats) == 88, "xrit_frame_stats: 88 bytes (FRAME_STATS_DTYPE mirrors it)");
static_assert(offsetof(xrit_frame_stats, rs_errors) == 48 && offsetof(xrit_frame_stats, vit_errors) == 64 &&
                  offsetof(xrit_frame_stats, scid) == 70 && offsetof(xrit_frame_stats, sync_word) == 76 &&
                  offsetof(xrit_frame_stats, frame_lock) == 80 && offsetof(xrit_frame_stats, valid) == 81,
              "xrit_frame_stats layout");
static_assert(sizeof(xrit_decoder_stats) == 5 * 8 + 3 * 256 * 8 + 8, "xrit_decoder_stats layout");
static_assert(sizeof(xrit_sync_hit) == 16 && sizeof(xrit_frame_info) == 40, "decoder record layouts");

namespace {
DemuxState start_state()
{
    DemuxState s{};
    for (int v = 0; v < NVC; ++v) {
        s.last[v] = -1;           // lastPacketCount (newdecoder.cpp:133-137)
        s.received[v] = -1;       // receivedPacketsPerFrame
        s.lost[v] = 0;            // lostPacketsPerFrame
    }
    return s;
}
}  // namespace

struct xrit_demux : StageHandle {
    uint32_t start_time = 0;
    DevBuf state, scratch;
    DevBuf h_hits, h_cadu, h_block, h_info, h_vcdu, h_offsets, h_records;
    void close_all() { close({&state, &scratch, &h_hits, &h_cadu, &h_block, &h_info, &h_vcdu, &h_offsets, &h_records}); }
};

int xrit_demux_create(xrit_demux **out, int device)
{
    return stage_create(out, device, [](xrit_demux &dm) {
        dm.start_time = (uint32_t)std::time(nullptr);   // Statistics::Statistics(), Statistics.cpp: getTimestamp()
        XR_TRY(dm.state.reserve(sizeof(DemuxState)));
        return xrit_demux_reset(&dm);
    });
}

int xrit_demux_destroy(xrit_demux *dm) { return stage_destroy(dm); }

int xrit_demux_reset(xrit_demux *dm)
{
    if (!dm) { set_error("null argument"); return XRIT_E_INVALID; }
    static const DemuxState s0 = start_state();
    return dm->write_state(dm->state.p, &s0, sizeof s0);
}

// the device path with the cadu rows `cadu_stride` bytes apart (the host path uploads only their first four bytes)
static int demux_run(xrit_demux *dm, const xrit_sync_hit *d_hits, const uint8_t *d_cadu, size_t cadu_stride,
                     const uint8_t *d_block, const xrit_frame_info *d_info, size_t nf, uint8_t *d_vcdu, uint32_t *d_offsets,
                     xrit_frame_stats *d_records, hipStream_t s)
{
    DemuxScratch sc;
    XR_TRY(dm->scratch.reserve(demux_scratch_carve(nullptr, nf, sc)));
    demux_scratch_carve(dm->scratch.p, nf, sc);
    XR_TRY(launch_demux(d_hits, d_cadu, cadu_stride, d_block, d_info, nf, dm->state.as<DemuxState>(), sc, d_vcdu, d_offsets,
                        d_records, s));
    dm->ran_on(s);
    return XRIT_OK;
}

// newdecoder.cpp:309-395 (and ChannelWriter::writeChannel, :356-360) on one call's frames
int xrit_demux_process_device(xrit_demux *dm, const xrit_sync_hit *d_hits, const uint8_t *d_cadu, const uint8_t *d_block,
                              const xrit_frame_info *d_info, size_t nf, uint8_t *d_vcdu, uint32_t *d_offsets,
                              xrit_frame_stats *d_records, void *stream)
{
    if (!dm) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf == 0) return XRIT_OK;
    if (!d_hits || !d_cadu || !d_block || !d_info || !d_vcdu || !d_offsets || !d_records) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    if (nf > MAX_ROWS_PER_CALL) { set_error("demux: at most %zu frames per call", MAX_ROWS_PER_CALL); return XRIT_E_INVALID; }
    if (((size_t)d_cadu | (size_t)d_block | (size_t)d_vcdu) & 3) {
        set_error("demux: cadu, block and vcdu must be 4-byte aligned");
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(dm->device));
    return demux_run(dm, d_hits, d_cadu, CADU_BYTES, d_block, d_info, nf, d_vcdu, d_offsets, d_records, (hipStream_t)stream);
}

int xrit_demux_process(xrit_demux *dm, const xrit_sync_hit *hits, const uint8_t *cadu, const uint8_t *block,
                       const xrit_frame_info *info, size_t nf, uint8_t *vcdu, uint32_t *offsets, xrit_frame_stats *records)
{
    if (!dm) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf > 0 && (!hits || !cadu || !block || !info || !vcdu || !offsets || !records)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    if (nf > MAX_ROWS_PER_CALL) { set_error("demux: at most %zu frames per call", MAX_ROWS_PER_CALL); return XRIT_E_INVALID; }
    if (nf == 0) {
        if (offsets) std::memset(offsets, 0, (NVC + 1) * sizeof(uint32_t));
        return XRIT_OK;
    }
    hipStream_t s;
    XR_TRY(dm->adopt_own_stream(s));
    size_t good = 0;                                 // the rows the call writes: known before it runs
    for (size_t f = 0; f < nf; ++f) good += (info[f].valid && info[f].ok) ? 1 : 0;
    XR_TRY(dm->h_hits.reserve(nf * sizeof(xrit_sync_hit)));
    XR_TRY(dm->h_cadu.reserve(nf * 4));
    XR_TRY(dm->h_block.reserve(nf * BLOCK_BYTES));
    XR_TRY(dm->h_info.reserve(nf * sizeof(xrit_frame_info)));
    XR_TRY(dm->h_vcdu.reserve(nf * VCDU_BYTES));
    XR_TRY(dm->h_offsets.reserve((NVC + 1) * sizeof(uint32_t)));
    XR_TRY(dm->h_records.reserve(nf * sizeof(xrit_frame_stats)));
    XR_HIP(hipMemcpyAsync(dm->h_hits.p, hits, nf * sizeof(xrit_sync_hit), hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpy2DAsync(dm->h_cadu.p, 4, cadu, CADU_BYTES, 4, nf, hipMemcpyHostToDevice, s));       // syncWord only
    XR_HIP(hipMemcpyAsync(dm->h_block.p, block, nf * BLOCK_BYTES, hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(dm->h_info.p, info, nf * sizeof(xrit_frame_info), hipMemcpyHostToDevice, s));
    XR_TRY(demux_run(dm, dm->h_hits.as<xrit_sync_hit>(), dm->h_cadu.as<uint8_t>(), 4, dm->h_block.as<uint8_t>(),
                     dm->h_info.as<xrit_frame_info>(), nf, dm->h_vcdu.as<uint8_t>(), dm->h_offsets.as<uint32_t>(),
                     dm->h_records.as<xrit_frame_stats>(), s));
    if (good) XR_HIP(hipMemcpyAsync(vcdu, dm->h_vcdu.p, good * VCDU_BYTES, hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpyAsync(offsets, dm->h_offsets.p, (NVC + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpyAsync(records, dm->h_records.p, nf * sizeof(xrit_frame_stats), hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}

int xrit_demux_stats(xrit_demux *dm, xrit_decoder_stats *out)
{
    if (!dm || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    DemuxState s;
    XR_TRY(dm->read_back(&s, dm->state.p, sizeof s));
    std::memset(out, 0, sizeof *out);
    out->total_packets = s.frames;
    out->dropped_packets = s.dropped;
    out->lost_packets = s.lost_total;
    out->sum_viterbi_errors = s.sum_vit;
    out->sum_rs_corrections = s.sum_rs;
    for (int v = 0; v < 256; ++v) {
        out->received[v] = v < NVC ? s.received[v] : -1;
        out->lost[v] = v < NVC ? s.lost[v] : 0;
        out->last_counter[v] = v < NVC ? s.last[v] : -1;
    }
    out->start_time = dm->start_time;
    return XRIT_OK;
}

namespace {
struct Wire {
    uint8_t *p;
    void put(uint64_t x, int bytes)
    {
        for (int i = 0; i < bytes; ++i) *p++ = (uint8_t)(x >> (8 * i));
    }
};
}  // namespace

// Statistics::update (Statistics.cpp) of every valid frame, then the packed Statistics_st (Statistics.h:14-36) that
// StatisticsDispatcher::Update sends (newdecoder.cpp:373-395)
int xrit_demux_expand(const xrit_decoder_stats *start, const xrit_frame_stats *records, size_t nf, uint8_t *out)
{
    if (!start || (nf && (!records || !out))) { set_error("null argument"); return XRIT_E_INVALID; }
    int64_t received[256], lost[256];
    std::memcpy(received, start->received, sizeof received);
    std::memcpy(lost, start->lost, sizeof lost);
    size_t n = 0;
    for (size_t f = 0; f < nf; ++f) {
        const xrit_frame_stats &r = records[f];
        if (!r.valid) continue;
        if (r.frame_lock) {
            received[r.vcid] = r.received_vc;
            lost[r.vcid] = r.lost_vc;
        }
        Wire w{out + n * XRIT_STATISTICS_WIRE_BYTES};
        w.put(r.scid, 1);
        w.put(r.vcid, 1);
        w.put(r.packet_number, 8);
        w.put(r.vit_errors, 2);
        w.put(r.frame_bits, 2);
        for (int k = 0; k < 4; ++k) w.put((uint32_t)r.rs_errors[k], 4);
        w.put(r.signal_quality, 1);
        w.put(r.sync_correlation, 1);
        w.put(r.phase_correction, 1);
        w.put(r.lost_packets, 8);
        w.put(r.average_vit_corrections, 2);
        w.put(r.average_rs_corrections, 1);
        w.put(r.dropped_packets, 8);
        for (int v = 0; v < 256; ++v) w.put((uint64_t)received[v], 8);
        for (int v = 0; v < 256; ++v) w.put((uint64_t)lost[v], 8);
        w.put(r.total_packets, 8);
        w.put(start->start_time, 4);
        for (int k = 0; k < 4; ++k) w.put(r.sync_word[k], 1);
        w.put(r.frame_lock, 1);
        w.put(0, 1);                                    // demodulatorFifoUsage: never set by the reference
        w.put(0, 1);                                    // decoderFifoUsage
        ++n;
    }
    if (n > (size_t)0x7FFFFFFF) { set_error("demux: too many records for one expand call"); return XRIT_E_INVALID; }
    return (int)n;
}
