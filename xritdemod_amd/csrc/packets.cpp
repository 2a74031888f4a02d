// packets.cpp -- C ABI of the packet assembler (include/xritdemod_amd.h, "Packet assembler"): the handle owns the
// per-channel state (last counter, pending bytes, counters) in device memory and grow-only scratch; the kernels are in
// packets.hip.
#include <cstddef>

#include "common.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_packet) == 32 && offsetof(xrit_packet, length) == 8 && offsetof(xrit_packet, apid) == 16 &&
                  offsetof(xrit_packet, vcid) == 24,
              "xrit_packet layout (PACKET_DTYPE mirrors it)");
static_assert(sizeof(xrit_packets_summary) == 72 && offsetof(xrit_packets_summary, overflow) == 64, "xrit_packets_summary layout");
static_assert(sizeof(xrit_packets_counters) == 48 + 6 * 512 + 512 + 2 * 256, "xrit_packets_counters layout");

namespace {
PacketsState start_state()
{
    PacketsState s{};
    for (int v = 0; v < NVC; ++v) s.last[v] = -1;
    return s;
}
}  // namespace

struct xrit_packets : StageHandle {
    DevBuf state, pend, scratch;
    DevBuf h_vcdu, h_offsets, h_bytes, h_packets, h_pkt_offsets, h_summary;
    void close_all() { close({&state, &pend, &scratch, &h_vcdu, &h_offsets, &h_bytes, &h_packets, &h_pkt_offsets, &h_summary}); }
};

int xrit_packets_create(xrit_packets **out, int device)
{
    return stage_create(out, device, [](xrit_packets &pa) {
        XR_TRY(pa.state.reserve(sizeof(PacketsState)));
        XR_TRY(pa.pend.reserve((size_t)NVC * PACKETS_PEND_STRIDE));
        return xrit_packets_reset(&pa);
    });
}

int xrit_packets_destroy(xrit_packets *pa) { return stage_destroy(pa); }

int xrit_packets_reset(xrit_packets *pa)
{
    if (!pa) { set_error("null argument"); return XRIT_E_INVALID; }
    static const PacketsState s0 = start_state();
    return pa->write_state(pa->state.p, &s0, sizeof s0);
}

static int packets_run(xrit_packets *pa, const uint8_t *d_vcdu, const uint32_t *d_offsets, size_t max_rows, uint8_t *d_bytes,
                       size_t max_bytes, xrit_packet *d_packets, size_t max_packets, uint32_t *d_pkt_offsets,
                       xrit_packets_summary *d_summary, hipStream_t s)
{
    PacketsScratch sc;
    XR_TRY(pa->scratch.reserve(packets_scratch_carve(nullptr, max_rows, sc)));
    packets_scratch_carve(pa->scratch.p, max_rows, sc);
    XR_TRY(launch_packets(d_vcdu, d_offsets, max_rows, pa->state.as<PacketsState>(), pa->pend.as<unsigned char>(), sc, d_bytes,
                          max_bytes, d_packets, max_packets, d_pkt_offsets, d_summary, s));
    pa->ran_on(s);
    return XRIT_OK;
}

int xrit_packets_process_device(xrit_packets *pa, const uint8_t *d_vcdu, const uint32_t *d_offsets, size_t max_rows,
                                uint8_t *d_bytes, size_t max_bytes, xrit_packet *d_packets, size_t max_packets,
                                uint32_t *d_pkt_offsets, xrit_packets_summary *d_summary, void *stream)
{
    if (!pa || !d_offsets || !d_pkt_offsets || !d_summary || (max_rows && !d_vcdu) || (max_bytes && !d_bytes) ||
        (max_packets && !d_packets)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    if (max_rows > MAX_ROWS_PER_CALL) { set_error("packets: at most %zu rows per call", MAX_ROWS_PER_CALL); return XRIT_E_INVALID; }
    if (((size_t)d_packets | (size_t)d_summary) & 7) {
        set_error("packets: the descriptors and the summary must be 8-byte aligned");
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(pa->device));
    return packets_run(pa, d_vcdu, d_offsets, max_rows, d_bytes, max_bytes, d_packets, max_packets, d_pkt_offsets, d_summary,
                       (hipStream_t)stream);
}

int xrit_packets_process(xrit_packets *pa, const uint8_t *vcdu, const uint32_t *offsets, uint8_t *bytes, size_t max_bytes,
                         xrit_packet *packets, size_t max_packets, uint32_t *pkt_offsets, xrit_packets_summary *summary)
{
    if (!pa || !offsets || !pkt_offsets || !summary || (max_bytes && !bytes) || (max_packets && !packets)) {
        set_error("null argument");
        return XRIT_E_INVALID;
    }
    const size_t rows = offsets[NVC];
    if (rows && !vcdu) { set_error("null argument"); return XRIT_E_INVALID; }
    if (rows > MAX_ROWS_PER_CALL) { set_error("packets: at most %zu rows per call", MAX_ROWS_PER_CALL); return XRIT_E_INVALID; }
    hipStream_t s;
    XR_TRY(pa->adopt_own_stream(s));
    // no call emits more than this, so the device side of a generous host buffer stays small
    const size_t bound_bytes = XRIT_PACKETS_MAX_BYTES(rows), bound_packets = 127 * rows + NVC;
    const size_t cap_bytes = max_bytes < bound_bytes ? max_bytes : bound_bytes;
    const size_t cap_packets = max_packets < bound_packets ? max_packets : bound_packets;
    XR_TRY(pa->h_vcdu.reserve(rows * VCDU_BYTES + 8));
    XR_TRY(pa->h_offsets.reserve((NVC + 1) * sizeof(uint32_t)));
    XR_TRY(pa->h_bytes.reserve(cap_bytes + 8));
    XR_TRY(pa->h_packets.reserve(cap_packets * sizeof(xrit_packet) + 8));
    XR_TRY(pa->h_pkt_offsets.reserve((NVC + 1) * sizeof(uint32_t)));
    XR_TRY(pa->h_summary.reserve(sizeof(xrit_packets_summary)));
    if (rows) XR_HIP(hipMemcpyAsync(pa->h_vcdu.p, vcdu, rows * VCDU_BYTES, hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(pa->h_offsets.p, offsets, (NVC + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    XR_TRY(packets_run(pa, pa->h_vcdu.as<uint8_t>(), pa->h_offsets.as<uint32_t>(), rows, pa->h_bytes.as<uint8_t>(), cap_bytes,
                       pa->h_packets.as<xrit_packet>(), cap_packets, pa->h_pkt_offsets.as<uint32_t>(),
                       pa->h_summary.as<xrit_packets_summary>(), s));
    XR_HIP(hipMemcpyAsync(pkt_offsets, pa->h_pkt_offsets.p, (NVC + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    // the written prefix: descriptors below the capacity; bytes up to the end of the last packet that fits
    return download_written(s, "packets", summary, pa->h_summary.p, sizeof *summary, &summary->overflow,
                            {{packets, pa->h_packets.p, sizeof(xrit_packet), &summary->packets, cap_packets, "packets"},
                             {bytes, pa->h_bytes.p, 1, &summary->bytes, cap_bytes, "bytes"}});
}

int xrit_packets_stats(xrit_packets *pa, xrit_packets_counters *out)
{
    if (!pa || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    PacketsState s;
    XR_TRY(pa->read_back(&s, pa->state.p, sizeof s));
    std::memset(out, 0, sizeof *out);
    for (int v = 0; v < NVC; ++v) {
        out->packets += out->vc_packets[v] = s.packets[v];
        out->crc_failures += out->vc_crc_failures[v] = s.crc_failures[v];
        out->fill_packets += out->vc_fill_packets[v] = s.fill_packets[v];
        out->discarded += out->vc_discarded[v] = s.discarded[v];
        out->bad_fhp += out->vc_bad_fhp[v] = s.bad_fhp[v];
        out->rows += out->vc_rows[v] = s.rows[v];
        out->last_counter[v] = s.last[v];
        out->pending_bytes[v] = s.pend_len[v];
        out->pending_first_counter[v] = s.first_counter[v];
    }
    return XRIT_OK;
}
