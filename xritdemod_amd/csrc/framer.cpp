// framer.cpp -- C ABI of the stream frame synchroniser (include/xritdemod_amd.h, "Stream frame synchroniser"): the handle
// owns the cursor, the counters and the carry (two buffers, written in turn) in device memory and grow-only scratch; the
// kernels are in framer.hip, the plain host parts in framer_host.h.
#include "common.h"
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

static_assert(sizeof(xrit_framer_counters) == 80, "xrit_framer_counters: 80 bytes (FRAMER_STATS_DTYPE mirrors it)");

struct xrit_framer : StageHandle {
    int hrit = 0;
    uint32_t frame = FRAME_SYMBOLS, min_corr = 46, segment = 0;
    uint64_t words[2] = {0, 0};
    bool started = false;           // a push has run: frame and min_correlation are fixed
    int cur = 0;                    // the carry buffer the next call reads
    DevBuf state, carry[2], scratch;
    DevBuf h_sym, h_frames, h_valid, h_hits, h_start, h_count;
    void close_all() { close({&state, &carry[0], &carry[1], &scratch, &h_sym, &h_frames, &h_valid, &h_hits, &h_start, &h_count}); }
};

int xrit_framer_create(xrit_framer **out, int hrit, int device)
{
    if (out) *out = nullptr;
    if (out && hrit != 0 && hrit != 1) { set_error("hrit = %d: 0 (LRIT) or 1 (HRIT)", hrit); return XRIT_E_INVALID; }
    return stage_create(out, device, [hrit](xrit_framer &fr) {
        fr.hrit = hrit;
        // newdecoder.cpp:21-24
        fr.words[0] = hrit ? 0xfc4ef4fd0cc2df89ull : 0xfca2b63db00d9794ull;
        fr.words[1] = hrit ? 0x25010b02f33d2076ull : 0x035d49c24ff2686bull;
        XR_TRY(fr.state.reserve(sizeof(FramerState)));
        return xrit_framer_reset(&fr);
    });
}

int xrit_framer_destroy(xrit_framer *fr) { return stage_destroy(fr); }

int xrit_framer_reset(xrit_framer *fr)
{
    if (!fr) { set_error("null argument"); return XRIT_E_INVALID; }
    fr->cur = 0;
    return fr->write_state(fr->state.p, nullptr, sizeof(FramerState));
}

int xrit_framer_set_frame(xrit_framer *fr, uint32_t frame, uint32_t min_correlation)
{
    if (!fr) { set_error("null argument"); return XRIT_E_INVALID; }
    if (const char *why = framer_host::check_frame(frame, min_correlation, fr->started)) { set_error("%s", why); return XRIT_E_INVALID; }
    fr->frame = frame;
    fr->min_corr = min_correlation;
    return XRIT_OK;
}

int xrit_framer_set_segment(xrit_framer *fr, uint32_t chunks)
{
    if (!fr) { set_error("null argument"); return XRIT_E_INVALID; }
    fr->segment = chunks;
    return XRIT_OK;
}

size_t xrit_framer_rows(const xrit_framer *fr, size_t n) { return fr ? framer_host::rows_cap(n, fr->frame) : 0; }

int xrit_framer_push_device(xrit_framer *fr, const int8_t *d_symbols, size_t n, int8_t *d_frames, uint8_t *d_valid,
                            xrit_sync_hit *d_hits, uint64_t *d_start, uint32_t *d_count, void *stream)
{
    const size_t cap = fr ? framer_host::rows_cap(n, fr->frame) : 0;
    if (const char *why = framer_host::check_push(fr, d_symbols, n, cap, d_frames, d_valid, d_hits, d_start, d_count)) {
        set_error("%s", why);
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(fr->device));
    if (!fr->started) {
        for (DevBuf &c : fr->carry) XR_TRY(c.reserve(2 * (size_t)fr->frame + 16));
        fr->started = true;
    }
    FramerPar par{};
    par.frame = fr->frame;
    par.min_corr = fr->min_corr;
    par.invert = fr->hrit ? 0u : 1u;
    for (int w = 0; w < 2; ++w) {
        par.whi[w] = (unsigned)(fr->words[w] >> 32);
        par.wlo[w] = (unsigned)(fr->words[w] & 0xFFFFFFFFull);
    }
    par.n = (unsigned)n;
    par.seg_chunks = framer_host::segment_chunks(framer_host::span_max(n, fr->frame), fr->frame, fr->segment);
    par.seg_bytes = par.seg_chunks * fr->frame;
    par.segs = framer_segments(n, fr->frame, par.seg_chunks);
    par.cap = (unsigned)cap;
    FramerScratch sc;
    XR_TRY(fr->scratch.reserve(framer_scratch_carve(nullptr, n, fr->frame, par.seg_chunks, sc)));
    framer_scratch_carve(fr->scratch.p, n, fr->frame, par.seg_chunks, sc);
    hipStream_t s = (hipStream_t)stream;
    XR_TRY(launch_framer(par, fr->state.as<FramerState>(), fr->carry[fr->cur].as<int8_t>(), fr->carry[fr->cur ^ 1].as<int8_t>(),
                         d_symbols, sc, d_frames, d_valid, d_hits, reinterpret_cast<unsigned long long *>(d_start), d_count, s));
    fr->cur ^= 1;
    fr->ran_on(s);
    return XRIT_OK;
}

int xrit_framer_push(xrit_framer *fr, const int8_t *symbols, size_t n, int8_t *frames, uint8_t *valid, xrit_sync_hit *hits,
                     uint64_t *start)
{
    const size_t cap = fr ? framer_host::rows_cap(n, fr->frame) : 0;
    uint32_t count = 0;
    if (const char *why = framer_host::check_push(fr, symbols, n, cap, frames, valid, hits, start, &count)) {
        set_error("%s", why);
        return XRIT_E_INVALID;
    }
    hipStream_t s;
    XR_TRY(fr->adopt_own_stream(s));
    const size_t F = fr->frame;
    XR_TRY(fr->h_sym.reserve(n ? n : 1));
    XR_TRY(fr->h_frames.reserve(cap * F + 4));
    XR_TRY(fr->h_valid.reserve(cap + 4));
    XR_TRY(fr->h_hits.reserve((cap + 1) * sizeof(xrit_sync_hit)));
    XR_TRY(fr->h_start.reserve((cap + 1) * sizeof(uint64_t)));
    XR_TRY(fr->h_count.reserve(sizeof(uint32_t)));
    if (n) XR_HIP(hipMemcpyAsync(fr->h_sym.p, symbols, n, hipMemcpyHostToDevice, s));
    XR_TRY(xrit_framer_push_device(fr, fr->h_sym.as<int8_t>(), n, fr->h_frames.as<int8_t>(), fr->h_valid.as<uint8_t>(),
                                   fr->h_hits.as<xrit_sync_hit>(), fr->h_start.as<uint64_t>(), fr->h_count.as<uint32_t>(), s));
    XR_HIP(hipMemcpyAsync(&count, fr->h_count.p, sizeof count, hipMemcpyDeviceToHost, s));
    if (cap) {
        XR_HIP(hipMemcpyAsync(frames, fr->h_frames.p, cap * F, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(valid, fr->h_valid.p, cap, hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(hits, fr->h_hits.p, cap * sizeof(xrit_sync_hit), hipMemcpyDeviceToHost, s));
        XR_HIP(hipMemcpyAsync(start, fr->h_start.p, cap * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    }
    XR_HIP(hipStreamSynchronize(s));
    return (int)count;
}

int xrit_framer_stats(xrit_framer *fr, xrit_framer_counters *out)
{
    if (!fr || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    FramerState s;
    XR_TRY(fr->read_back(&s, fr->state.p, sizeof s));
    framer_host::copy_counters(s, out);
    return XRIT_OK;
}
