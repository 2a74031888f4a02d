// decoder.cpp -- C ABI of the frame decoder (include/xritdemod_amd.h, "Decoder"): the handle is a DecoderCore
// (frame_cores.h), which owns the carry in device memory and grow-only scratch; the kernels are in viterbi.hip and
// rs.hip.
#include "frame_cores.h"

using namespace xrit;

struct xrit_decoder : StageHandle {
    DecoderCore core;
    DevBuf h_frames, h_valid;
    void close_all()
    {
        close();
        h_frames.release();
        h_valid.release();
        core.release();
    }
};

int xrit_decoder_create(xrit_decoder **out, int hrit, int device)
{
    if (out) *out = nullptr;
    if (out && hrit != 0 && hrit != 1) { set_error("hrit = %d: 0 (LRIT) or 1 (HRIT)", hrit); return XRIT_E_INVALID; }
    return stage_create(out, device, [hrit](xrit_decoder &d) {
        XR_TRY(d.core.open(hrit, d.device));
        return xrit_decoder_reset(&d);
    });
}

int xrit_decoder_destroy(xrit_decoder *d) { return stage_destroy(d); }

int xrit_decoder_reset(xrit_decoder *d)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    return d->core.reset(*d);
}

int xrit_decoder_set_windows(xrit_decoder *d, uint32_t windows)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    d->core.set_windows(windows);
    return XRIT_OK;
}

int xrit_decoder_decode_device(xrit_decoder *d, const int8_t *d_frames, const uint8_t *d_valid, size_t nf, uint8_t *d_cadu,
                               uint8_t *d_block, xrit_frame_info *d_info, void *stream)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf == 0) return XRIT_OK;
    if (!d_frames || !d_valid || !d_cadu || !d_block || !d_info) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf > MAX_ROWS_PER_CALL) { set_error("decoder: at most %zu frames per call", MAX_ROWS_PER_CALL); return XRIT_E_INVALID; }
    if (((size_t)d_cadu | (size_t)d_block) & 15) { set_error("decoder: cadu and block must be 16-byte aligned"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned windows = 0;
    XR_TRY(d->core.reserve(nf, windows));
    XR_TRY(d->core.run(d_frames, d_valid, nf, d_cadu, d_block, d_info, windows, s));
    d->ran_on(s);
    return XRIT_OK;
}

int xrit_decoder_decode(xrit_decoder *d, const int8_t *frames, const uint8_t *valid, size_t nf, uint8_t *cadu, uint8_t *block,
                        xrit_frame_info *info)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf == 0) return XRIT_OK;
    if (!frames || !valid || !cadu || !block || !info) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf > MAX_ROWS_PER_CALL) { set_error("decoder: at most %zu frames per call", MAX_ROWS_PER_CALL); return XRIT_E_INVALID; }
    hipStream_t s;
    XR_TRY(d->adopt_own_stream(s));
    DecoderCore &c = d->core;
    XR_TRY(d->h_frames.reserve(nf * FRAME_SYMBOLS));
    XR_TRY(d->h_valid.reserve(nf));
    XR_TRY(c.stage(nf));
    XR_HIP(hipMemcpyAsync(d->h_frames.p, frames, nf * FRAME_SYMBOLS, hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(d->h_valid.p, valid, nf, hipMemcpyHostToDevice, s));
    XR_TRY(xrit_decoder_decode_device(d, d->h_frames.as<int8_t>(), d->h_valid.as<uint8_t>(), nf, c.h_cadu.as<uint8_t>(),
                                      c.h_block.as<uint8_t>(), c.h_info.as<xrit_frame_info>(), s));
    XR_TRY(c.download(nf, cadu, block, info, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}
