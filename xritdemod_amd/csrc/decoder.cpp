// decoder.cpp -- C ABI of the frame decoder (include/xritdemod_amd.h, "Decoder"): the handle owns the carry (the
// reference's lastFrameEnd, newdecoder.cpp:141,274,300) in device memory and grow-only scratch; the kernels are in
// viterbi.hip and rs.hip.
#include "kernels.h"
#include "stage_handle.h"

using namespace xrit;

namespace {
constexpr unsigned DEC_WINDOWS_PER_CU = 8;        // resident Viterbi windows per CU: decision scratch of 66 KB each
}  // namespace

struct xrit_decoder : StageHandle {
    int hrit = 0;
    unsigned slots = 0;                             // resident windows: CUs x DEC_WINDOWS_PER_CU
    unsigned windows = 0;                           // ... of which a call uses at most this many (xrit_decoder_set_windows)
    DevBuf carry, prev, last, dec, verr;
    DevBuf h_frames, h_valid, h_cadu, h_block, h_info;
    void close_all() { close({&carry, &prev, &last, &dec, &verr, &h_frames, &h_valid, &h_cadu, &h_block, &h_info}); }
};

int xrit_decoder_create(xrit_decoder **out, int hrit, int device)
{
    if (out) *out = nullptr;
    if (out && hrit != 0 && hrit != 1) { set_error("hrit = %d: 0 (LRIT) or 1 (HRIT)", hrit); return XRIT_E_INVALID; }
    return stage_create(out, device, [hrit](xrit_decoder &d) {
        int cus = 0;
        XR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d.device));
        d.hrit = hrit;
        d.slots = (unsigned)(cus > 0 ? cus : 1) * DEC_WINDOWS_PER_CU;
        d.windows = d.slots;
        XR_TRY(d.carry.reserve(64));
        XR_TRY(d.last.reserve(sizeof(int)));
        return xrit_decoder_reset(&d);
    });
}

int xrit_decoder_destroy(xrit_decoder *d) { return stage_destroy(d); }

int xrit_decoder_reset(xrit_decoder *d)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    return d->write_state(d->carry.p, nullptr, 64);
}

int xrit_decoder_set_windows(xrit_decoder *d, uint32_t windows)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    d->windows = windows == 0 || windows > d->slots ? d->slots : windows;
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
    const unsigned windows = nf < d->windows ? (unsigned)nf : d->windows;
    XR_TRY(d->prev.reserve(nf * sizeof(int)));
    XR_TRY(d->verr.reserve(nf * sizeof(unsigned)));
    XR_TRY(d->dec.reserve((size_t)windows * viterbi_slot_bytes()));
    hipStream_t s = (hipStream_t)stream;
    XR_TRY(launch_viterbi(d_frames, d_valid, nf, d->hrit, d->carry.as<int8_t>(), d->prev.as<int>(), d->last.as<int>(),
                          d->dec.as<unsigned long long>(), windows, d_cadu, d->verr.as<unsigned>(), s));
    XR_TRY(launch_rs(d_cadu, d_valid, d->verr.as<unsigned>(), nf, d_block, d_info, s));
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
    XR_TRY(d->h_frames.reserve(nf * FRAME_SYMBOLS));
    XR_TRY(d->h_valid.reserve(nf));
    XR_TRY(d->h_cadu.reserve(nf * CADU_BYTES));
    XR_TRY(d->h_block.reserve(nf * BLOCK_BYTES));
    XR_TRY(d->h_info.reserve(nf * sizeof(xrit_frame_info)));
    XR_HIP(hipMemcpyAsync(d->h_frames.p, frames, nf * FRAME_SYMBOLS, hipMemcpyHostToDevice, s));
    XR_HIP(hipMemcpyAsync(d->h_valid.p, valid, nf, hipMemcpyHostToDevice, s));
    XR_TRY(xrit_decoder_decode_device(d, d->h_frames.as<int8_t>(), d->h_valid.as<uint8_t>(), nf, d->h_cadu.as<uint8_t>(),
                                      d->h_block.as<uint8_t>(), d->h_info.as<xrit_frame_info>(), s));
    XR_HIP(hipMemcpyAsync(cadu, d->h_cadu.p, nf * CADU_BYTES, hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpyAsync(block, d->h_block.p, nf * BLOCK_BYTES, hipMemcpyDeviceToHost, s));
    XR_HIP(hipMemcpyAsync(info, d->h_info.p, nf * sizeof(xrit_frame_info), hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    return XRIT_OK;
}
