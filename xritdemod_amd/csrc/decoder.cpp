// decoder.cpp -- C ABI of the frame decoder (include/xritdemod_amd.h, "Decoder"): the handle owns the carry (the
// reference's lastFrameEnd, newdecoder.cpp:141,274,300) in device memory and grow-only scratch; the kernels are in
// viterbi.hip and rs.hip.
#include "common.h"
#include "kernels.h"

using namespace xrit;

namespace {
constexpr size_t DEC_FRAME = 16384, DEC_CADU = 1024, DEC_BLOCK = 1020;
constexpr size_t DEC_MAX_FRAMES = (size_t)1 << 24;
constexpr unsigned DEC_WINDOWS_PER_CU = 8;        // resident Viterbi windows per CU: decision scratch of 66 KB each
}  // namespace

struct xrit_decoder {
    int hrit = 0, device = 0;
    unsigned slots = 0;                             // resident windows: CUs x DEC_WINDOWS_PER_CU
    hipStream_t stream = nullptr;                   // the host-buffer path's
    void *last_stream = nullptr;                    // the stream of the most recent call (reset waits for it)
    DevBuf carry, prev, last, dec, verr;
    DevBuf h_frames, h_valid, h_cadu, h_block, h_info;
};

int xrit_decoder_create(xrit_decoder **out, int hrit, int device)
{
    if (!out) { set_error("null argument"); return XRIT_E_INVALID; }
    *out = nullptr;
    if (hrit != 0 && hrit != 1) { set_error("hrit = %d: 0 (LRIT) or 1 (HRIT)", hrit); return XRIT_E_INVALID; }
    XR_TRY(select_device(device));
    int cus = 0;
    XR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    xrit_decoder *d = new (std::nothrow) xrit_decoder;
    if (!d) { set_error("out of host memory"); return XRIT_E_NOMEM; }
    d->hrit = hrit;
    d->device = device;
    d->slots = (unsigned)(cus > 0 ? cus : 1) * DEC_WINDOWS_PER_CU;
    int rc = d->carry.reserve(64);
    if (rc == XRIT_OK) rc = d->last.reserve(sizeof(int));
    if (rc == XRIT_OK && hipMemset(d->carry.p, 0, 64) != hipSuccess) { set_error("hipMemset failed"); rc = XRIT_E_HIP; }
    if (rc == XRIT_OK && hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("hipStreamCreate failed");
        d->stream = nullptr;
        rc = XRIT_E_HIP;
    }
    if (rc != XRIT_OK) {
        xrit_decoder_destroy(d);
        return rc;
    }
    *out = d;
    return XRIT_OK;
}

int xrit_decoder_destroy(xrit_decoder *d)
{
    if (!d) return XRIT_OK;
    (void)hipSetDevice(d->device);
    if (d->stream) {
        (void)hipStreamSynchronize(d->stream);
        (void)hipStreamDestroy(d->stream);
    }
    if (d->last_stream) (void)hipStreamSynchronize((hipStream_t)d->last_stream);
    for (DevBuf *b : {&d->carry, &d->prev, &d->last, &d->dec, &d->verr, &d->h_frames, &d->h_valid, &d->h_cadu, &d->h_block,
                      &d->h_info})
        b->release();
    delete d;
    return XRIT_OK;
}

int xrit_decoder_reset(xrit_decoder *d)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(d->device));
    XR_HIP(hipStreamSynchronize((hipStream_t)d->last_stream));
    XR_HIP(hipMemsetAsync(d->carry.p, 0, 64, d->stream));
    XR_HIP(hipStreamSynchronize(d->stream));
    d->last_stream = d->stream;
    return XRIT_OK;
}

int xrit_decoder_decode_device(xrit_decoder *d, const int8_t *d_frames, const uint8_t *d_valid, size_t nf, uint8_t *d_cadu,
                               uint8_t *d_block, xrit_frame_info *d_info, void *stream)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf == 0) return XRIT_OK;
    if (!d_frames || !d_valid || !d_cadu || !d_block || !d_info) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf > DEC_MAX_FRAMES) { set_error("decoder: at most %zu frames per call", DEC_MAX_FRAMES); return XRIT_E_INVALID; }
    if (((size_t)d_cadu | (size_t)d_block) & 15) { set_error("decoder: cadu and block must be 16-byte aligned"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(d->device));
    const unsigned windows = nf < d->slots ? (unsigned)nf : d->slots;
    XR_TRY(d->prev.reserve(nf * sizeof(int)));
    XR_TRY(d->verr.reserve(nf * sizeof(unsigned)));
    XR_TRY(d->dec.reserve((size_t)windows * viterbi_slot_bytes()));
    hipStream_t s = (hipStream_t)stream;
    XR_TRY(launch_viterbi(d_frames, d_valid, nf, d->hrit, d->carry.as<int8_t>(), d->prev.as<int>(), d->last.as<int>(),
                          d->dec.as<unsigned long long>(), windows, d_cadu, d->verr.as<unsigned>(), s));
    XR_TRY(launch_rs(d_cadu, d_valid, d->verr.as<unsigned>(), nf, d_block, d_info, s));
    d->last_stream = stream;
    return XRIT_OK;
}

int xrit_decoder_decode(xrit_decoder *d, const int8_t *frames, const uint8_t *valid, size_t nf, uint8_t *cadu, uint8_t *block,
                        xrit_frame_info *info)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf == 0) return XRIT_OK;
    if (!frames || !valid || !cadu || !block || !info) { set_error("null argument"); return XRIT_E_INVALID; }
    if (nf > DEC_MAX_FRAMES) { set_error("decoder: at most %zu frames per call", DEC_MAX_FRAMES); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(d->device));
    XR_TRY(d->h_frames.reserve(nf * DEC_FRAME));
    XR_TRY(d->h_valid.reserve(nf));
    XR_TRY(d->h_cadu.reserve(nf * DEC_CADU));
    XR_TRY(d->h_block.reserve(nf * DEC_BLOCK));
    XR_TRY(d->h_info.reserve(nf * sizeof(xrit_frame_info)));
    hipStream_t s = d->stream;
    if (d->last_stream != d->stream) XR_HIP(hipStreamSynchronize((hipStream_t)d->last_stream));   // the carry's last writer
    XR_HIP(hipMemcpyAsync(d->h_frames.p, frames, nf * DEC_FRAME, hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(d->h_valid.p, valid, nf, hipMemcpyHostToDevice, s));
    XR_TRY(xrit_decoder_decode_device(d, d->h_frames.as<int8_t>(), d->h_valid.as<uint8_t>(), nf, d->h_cadu.as<uint8_t>(),
                                      d->h_block.as<uint8_t>(), d->h_info.as<xrit_frame_info>(), s));
    XR_HIP(hipMemcpyAsync(cadu, d->h_cadu.p, nf * DEC_CADU, hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpyAsync(block, d->h_block.p, nf * DEC_BLOCK, hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpyAsync(info, d->h_info.p, nf * sizeof(xrit_frame_info), hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}
