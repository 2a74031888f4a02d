// framer.cpp -- C ABI of the stream frame synchroniser (include/xritdemod_amd.h, "Stream frame synchroniser"): the handle
// is a SyncCore (frame_cores.h), which owns the cursor, the counters and the carry in device memory and grow-only
// scratch; a call is the chain's walk without a flywheel (lock.hip) between the bits pass and the gather of framer.hip.
// The plain host parts are in framer_host.h.
#include "frame_cores.h"

using namespace xrit;

static_assert(sizeof(xrit_framer_counters) == 80, "xrit_framer_counters: 80 bytes (FRAMER_STATS_DTYPE mirrors it)");

struct xrit_framer : StageHandle {
    SyncCore sync;
    void close_all()
    {
        close();
        sync.release();
    }
};

int xrit_framer_create(xrit_framer **out, int hrit, int device)
{
    if (out) *out = nullptr;
    if (out && hrit != 0 && hrit != 1) { set_error("hrit = %d: 0 (LRIT) or 1 (HRIT)", hrit); return XRIT_E_INVALID; }
    return stage_create(out, device, [hrit](xrit_framer &fr) {
        XR_TRY(fr.sync.open(hrit));
        return xrit_framer_reset(&fr);
    });
}

int xrit_framer_destroy(xrit_framer *fr) { return stage_destroy(fr); }

int xrit_framer_reset(xrit_framer *fr)
{
    if (!fr) { set_error("null argument"); return XRIT_E_INVALID; }
    return fr->sync.reset(*fr);
}

int xrit_framer_set_frame(xrit_framer *fr, uint32_t frame, uint32_t min_correlation)
{
    if (!fr) { set_error("null argument"); return XRIT_E_INVALID; }
    if (const char *why = framer_host::check_frame(frame, min_correlation, fr->sync.started)) { set_error("%s", why); return XRIT_E_INVALID; }
    fr->sync.frame = frame;
    fr->sync.min_corr = min_correlation;
    return XRIT_OK;
}

int xrit_framer_set_segment(xrit_framer *fr, uint32_t chunks)
{
    if (!fr) { set_error("null argument"); return XRIT_E_INVALID; }
    fr->sync.segment = chunks;
    return XRIT_OK;
}

size_t xrit_framer_rows(const xrit_framer *fr, size_t n) { return fr ? fr->sync.rows(n) : 0; }

int xrit_framer_push_device(xrit_framer *fr, const int8_t *d_symbols, size_t n, int8_t *d_frames, uint8_t *d_valid,
                            xrit_sync_hit *d_hits, uint64_t *d_start, uint32_t *d_count, void *stream)
{
    const size_t cap = fr ? fr->sync.rows(n) : 0;
    if (const char *why = framer_host::check_push(fr, d_symbols, n, cap, d_frames, d_valid, d_hits, d_start, d_count)) {
        set_error("%s", why);
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(fr->device));
    hipStream_t s = (hipStream_t)stream;
    const LockPar lp{1, 0, 1, 0};                       // the walk without a flywheel: no short range, no short0
    fr->ran_on(s);
    XR_TRY(fr->sync.begin(d_symbols, n, lp, s));
    XR_TRY(launch_plain_joints(fr->sync.par, &fr->sync.st()->fr, fr->sync.sc, d_count, s));
    XR_TRY(fr->sync.gather(0, d_symbols, d_frames, d_valid, d_hits, d_start, s));
    fr->sync.end();
    return XRIT_OK;
}

int xrit_framer_push(xrit_framer *fr, const int8_t *symbols, size_t n, int8_t *frames, uint8_t *valid, xrit_sync_hit *hits,
                     uint64_t *start)
{
    const size_t cap = fr ? fr->sync.rows(n) : 0;
    uint32_t count = 0;
    if (const char *why = framer_host::check_push(fr, symbols, n, cap, frames, valid, hits, start, &count)) {
        set_error("%s", why);
        return XRIT_E_INVALID;
    }
    hipStream_t s;
    XR_TRY(fr->adopt_own_stream(s));
    SyncCore &y = fr->sync;
    XR_TRY(y.upload(symbols, n, s));
    XR_TRY(xrit_framer_push_device(fr, y.h_sym.as<int8_t>(), n, y.h_frames.as<int8_t>(), y.h_valid.as<uint8_t>(),
                                   y.h_hits.as<xrit_sync_hit>(), y.h_start.as<uint64_t>(), y.h_count.as<uint32_t>(), s));
    XR_TRY(y.download(n, frames, valid, hits, start, &count, s));
    XR_HIP(hipStreamSynchronize(s));
    return (int)count;
}

int xrit_framer_stats(xrit_framer *fr, xrit_framer_counters *out)
{
    if (!fr || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    FramerState s;
    XR_TRY(fr->read_back(&s, fr->sync.state.p, sizeof s));          // the front of the LockState
    framer_host::copy_counters(s, out);
    return XRIT_OK;
}
