// stages_abi.cpp -- the C ABI (include/xritdemod_amd.h) beside the chain handle: the five stand-alone stage objects
// (xrit_fir, xrit_agc, xrit_costas, xrit_clock, xrit_rtl), the one-shot wrappers around single kernels (frame sync, int8
// quantiser, synthetic burst, read bandwidth, the loop's sincosf) and the filter designs.  None of them shares state with
// a chain handle (demod.cpp).
#include "kernels.h"

#include <cmath>
#include <new>
#include <vector>

using namespace xrit;

struct xrit_fir { int device; hipStream_t stream; FirStage st; DevBuf in, out; };
struct xrit_agc { int device; hipStream_t stream; AgcStage st; DevBuf in, out; };
struct xrit_costas { int device; hipStream_t stream; CostasStage st; DevBuf in, out; };
struct xrit_clock { int device; hipStream_t stream; ClockStage st; DevBuf in, out; };
struct xrit_rtl { int device; hipStream_t stream; RtlIngestStage st; DevBuf in, out; };

template <typename H> static int stage_open(H *h, int device)
{
    XR_TRY(select_device(device));
    h->device = device;
    XR_HIP(hipStreamCreate(&h->stream));
    return XRIT_OK;
}
template <typename H> static void stage_close(H *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); }
    h->st.release();
    h->in.release();
    h->out.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

extern "C" {

// ---------------------------------------------------------------- filter designs
int xrit_lowpass_taps(double gain, double sample_rate, double cutoff, double transition_width, float *taps, int cap)
{
    std::vector<float> h = design_lowpass(gain, sample_rate, cutoff, transition_width);
    if ((int)h.size() > cap || !taps) return -(int)h.size();
    memcpy(taps, h.data(), h.size() * sizeof(float));
    return (int)h.size();
}

int xrit_rrc_taps(double gain, double sample_rate, double symbol_rate, double alpha, int ntaps, float *taps, int cap)
{
    std::vector<float> h = design_rrc(gain, sample_rate, symbol_rate, alpha, ntaps);
    if ((int)h.size() > cap || !taps) return -(int)h.size();
    memcpy(taps, h.data(), h.size() * sizeof(float));
    return (int)h.size();
}

void xrit_mmse_table(float *table) { design_mmse_table(table); }

// ---------------------------------------------------------------- one-shot wrappers
int xrit_quantize_i8_device(const float *d_soft, int8_t *d_out, size_t n, int device, void *stream)
{
    XR_TRY(select_device(device));
    return launch_quantize_i8(d_soft, d_out, n, (hipStream_t)stream);
}

int xrit_sync_correlate_device(const int8_t *d_symbols, size_t n, const uint64_t *words, int nwords, uint32_t frame,
                               xrit_sync_hit *d_hits, int device, void *stream)
{
    if (!words || (n >= frame && (!d_symbols || !d_hits))) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(select_device(device));
    return launch_sync_correlate(d_symbols, n, reinterpret_cast<const unsigned long long *>(words), nwords, frame, d_hits,
                                 (hipStream_t)stream);
}

int xrit_sync_correlate(const int8_t *symbols, size_t n, const uint64_t *words, int nwords, uint32_t frame,
                        xrit_sync_hit *hits, int device)
{
    if (!words || frame == 0 || (n >= frame && (!symbols || !hits))) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(select_device(device));
    const size_t nf = n / frame;
    if (nf == 0) return XRIT_OK;
    DevBuf din, dh;
    int rc = din.reserve(nf * frame);
    if (rc == XRIT_OK) rc = dh.reserve(nf * sizeof(xrit_sync_hit));
    if (rc == XRIT_OK && hipMemcpy(din.p, symbols, nf * frame, hipMemcpyHostToDevice) != hipSuccess) { set_error("hipMemcpy failed"); rc = XRIT_E_HIP; }
    if (rc == XRIT_OK)
        rc = launch_sync_correlate(din.as<int8_t>(), nf * frame, reinterpret_cast<const unsigned long long *>(words), nwords, frame,
                                   dh.as<xrit_sync_hit>(), nullptr);
    if (rc == XRIT_OK && (hipDeviceSynchronize() != hipSuccess ||
                          hipMemcpy(hits, dh.p, nf * sizeof(xrit_sync_hit), hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error("sync: device error");
        rc = XRIT_E_HIP;
    }
    din.release();
    dh.release();
    return rc;
}

int xrit_sync_fix_frames_device(const int8_t *d_symbols, size_t n, const xrit_sync_hit *d_hits, uint32_t frame,
                                uint32_t min_correlation, int8_t *d_frames, uint8_t *d_valid, int device, void *stream)
{
    if (frame == 0 || (n >= frame && (!d_symbols || !d_hits || !d_frames || !d_valid))) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(select_device(device));
    return launch_sync_fix(d_symbols, n, d_hits, frame, min_correlation, d_frames, d_valid, (hipStream_t)stream);
}

int xrit_sync_fix_frames(const int8_t *symbols, size_t n, const xrit_sync_hit *hits, uint32_t frame,
                         uint32_t min_correlation, int8_t *frames, uint8_t *valid, int device)
{
    if (frame == 0 || (n >= frame && (!symbols || !hits || !frames || !valid))) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(select_device(device));
    const size_t nf = n / frame;
    if (nf == 0) return XRIT_OK;
    DevBuf din, dh, dout, dv;
    int rc = din.reserve(n + 8);
    if (rc == XRIT_OK) rc = dh.reserve(nf * sizeof(xrit_sync_hit));
    if (rc == XRIT_OK) rc = dout.reserve(nf * frame);
    if (rc == XRIT_OK) rc = dv.reserve(nf);
    if (rc == XRIT_OK && (hipMemcpy(din.p, symbols, n, hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemcpy(dh.p, hits, nf * sizeof(xrit_sync_hit), hipMemcpyHostToDevice) != hipSuccess)) {
        set_error("hipMemcpy failed");
        rc = XRIT_E_HIP;
    }
    if (rc == XRIT_OK)
        rc = launch_sync_fix(din.as<int8_t>(), n, dh.as<xrit_sync_hit>(), frame, min_correlation, dout.as<int8_t>(),
                             dv.as<unsigned char>(), nullptr);
    if (rc == XRIT_OK && (hipDeviceSynchronize() != hipSuccess ||
                          hipMemcpy(frames, dout.p, nf * frame, hipMemcpyDeviceToHost) != hipSuccess ||
                          hipMemcpy(valid, dv.p, nf, hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error("sync: device error");
        rc = XRIT_E_HIP;
    }
    din.release(); dh.release(); dout.release(); dv.release();
    return rc;
}

int xrit_loop_sincosf(const float *x, float *sin_out, float *cos_out, size_t n, int device)
{
    if (n && (!x || !sin_out || !cos_out)) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(select_device(device));
    if (n == 0) return XRIT_OK;
    DevBuf dx, ds, dc;
    int rc = dx.reserve(n * sizeof(float));
    if (rc == XRIT_OK) rc = ds.reserve(n * sizeof(float));
    if (rc == XRIT_OK) rc = dc.reserve(n * sizeof(float));
    if (rc == XRIT_OK && hipMemcpy(dx.p, x, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { set_error("hipMemcpy failed"); rc = XRIT_E_HIP; }
    if (rc == XRIT_OK) rc = launch_loop_sincosf(dx.as<float>(), ds.as<float>(), dc.as<float>(), n, nullptr);
    if (rc == XRIT_OK && (hipDeviceSynchronize() != hipSuccess ||
                          hipMemcpy(sin_out, ds.p, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
                          hipMemcpy(cos_out, dc.p, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error("loop_sincosf: device error");
        rc = XRIT_E_HIP;
    }
    dx.release(); ds.release(); dc.release();
    return rc;
}

// ---------------------------------------------------------------- stage objects
int xrit_fir_create(unsigned decimation, const float *taps, int ntaps, int device, xrit_fir **out)
{
    if (!taps || ntaps < 1 || !out) { set_error("bad argument"); return XRIT_E_INVALID; }
    xrit_fir *f = new (std::nothrow) xrit_fir();
    if (!f) return XRIT_E_NOMEM;
    f->stream = nullptr;
    int rc = stage_open(f, device);
    if (rc == XRIT_OK) rc = f->st.init(taps, ntaps, (int)decimation);
    if (rc != XRIT_OK) { stage_close(f); return rc; }
    *out = f;
    return XRIT_OK;
}

int xrit_fir_work(xrit_fir *f, const float *in, float *out, size_t n_out)
{
    if (!f || (n_out && (!in || !out))) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(f->device));
    size_t n_in = n_out * (size_t)f->st.plan.D;
    XR_TRY(f->in.reserve((n_in + 8) * sizeof(float2)));
    XR_TRY(f->out.reserve((n_out + 8) * sizeof(float2)));
    if (n_in) XR_HIP(hipMemcpyAsync(f->in.p, in, n_in * sizeof(float2), hipMemcpyHostToDevice, f->stream));
    XR_TRY(f->st.run(f->in.p, XRIT_SAMPLE_FLOATIQ, f->out.as<float2>(), n_out, f->stream, nullptr));
    if (n_out) XR_HIP(hipMemcpyAsync(out, f->out.p, n_out * sizeof(float2), hipMemcpyDeviceToHost, f->stream));
    XR_HIP(hipStreamSynchronize(f->stream));
    return XRIT_OK;
}

int xrit_fir_set_exact(xrit_fir *f, int exact)
{
    if (!f) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(f->device));
    XR_HIP(hipStreamSynchronize(f->stream));
    return f->st.set_exact(exact != 0);
}

void xrit_fir_destroy(xrit_fir *f) { stage_close(f); }

int xrit_agc_create(float rate, float reference, float gain, float max_gain, int device, xrit_agc **out)
{
    if (!out) return XRIT_E_INVALID;
    xrit_agc *a = new (std::nothrow) xrit_agc();
    if (!a) return XRIT_E_NOMEM;
    a->stream = nullptr;
    int rc = stage_open(a, device);
    if (rc == XRIT_OK) rc = a->st.init(rate, reference, gain, max_gain);
    if (rc != XRIT_OK) { stage_close(a); return rc; }
    *out = a;
    return XRIT_OK;
}

int xrit_agc_work(xrit_agc *a, const float *in, float *out, size_t n)
{
    if (!a || (n && (!in || !out))) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(a->device));
    XR_TRY(a->in.reserve((n + 8) * sizeof(float2)));
    XR_TRY(a->out.reserve((n + 8) * sizeof(float2)));
    if (n) XR_HIP(hipMemcpyAsync(a->in.p, in, n * sizeof(float2), hipMemcpyHostToDevice, a->stream));
    XR_TRY(a->st.run(a->in.as<float2>(), a->out.as<float2>(), n, a->stream, nullptr));
    if (n) XR_HIP(hipMemcpyAsync(out, a->out.p, n * sizeof(float2), hipMemcpyDeviceToHost, a->stream));
    XR_HIP(hipStreamSynchronize(a->stream));
    return XRIT_OK;
}

int xrit_agc_set_exact(xrit_agc *a, int exact)
{
    if (!a) { set_error("null argument"); return XRIT_E_INVALID; }
    a->st.exact = exact != 0;
    return XRIT_OK;
}

int xrit_agc_exact_stats(xrit_agc *a, uint32_t *counters8)
{
    if (!a || !counters8) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(a->device));
    return a->st.exact_counters(counters8, a->stream);
}

float xrit_agc_gain(xrit_agc *a)
{
    float g = NAN;
    if (!a) return g;
    (void)hipSetDevice(a->device);
    (void)a->st.gain(&g, a->stream);
    return g;
}

void xrit_agc_destroy(xrit_agc *a) { stage_close(a); }

int xrit_costas_create(float loop_bw, int order, int device, xrit_costas **out)
{
    if (!out) return XRIT_E_INVALID;
    if (order != 2) { set_error("only the 2nd-order (BPSK) loop is implemented, as the reference uses (LOOP_ORDER 2)"); return XRIT_E_INVALID; }
    xrit_costas *c = new (std::nothrow) xrit_costas();
    if (!c) return XRIT_E_NOMEM;
    c->stream = nullptr;
    int rc = stage_open(c, device);
    if (rc == XRIT_OK) rc = c->st.init(loop_bw, 0, 0);
    if (rc != XRIT_OK) { stage_close(c); return rc; }
    *out = c;
    return XRIT_OK;
}

int xrit_costas_work(xrit_costas *c, const float *in, float *out, size_t n)
{
    if (!c || (n && (!in || !out))) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(c->device));
    XR_TRY(c->in.reserve((n + 8) * sizeof(float2)));
    XR_TRY(c->out.reserve((n + 8) * sizeof(float2)));
    if (n) XR_HIP(hipMemcpyAsync(c->in.p, in, n * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    XR_TRY(c->st.run(c->in.as<float2>(), c->out.as<float2>(), n, c->stream, nullptr));
    if (n) XR_HIP(hipMemcpyAsync(out, c->out.p, n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    XR_HIP(hipStreamSynchronize(c->stream));
    return XRIT_OK;
}

int xrit_costas_set_exact(xrit_costas *c, int exact, int history)
{
    if (!c) { set_error("null argument"); return XRIT_E_INVALID; }
    if (history < 0) { set_error("history = %d", history); return XRIT_E_INVALID; }
    c->st.exact = exact != 0;
    c->st.ex_hist = history > 0 ? history : -1;
    return XRIT_OK;
}

int xrit_costas_exact_stats(xrit_costas *c, uint64_t *blocks, uint64_t *rounds, uint32_t *joints_open, uint32_t *fix_rounds,
                            uint64_t *lattice_segments, uint64_t *lattice_fallbacks)
{
    if (!c) { set_error("null argument"); return XRIT_E_INVALID; }
    if (blocks) *blocks = c->st.ex_blocks;
    if (rounds) *rounds = c->st.ex_picard;
    if (joints_open) *joints_open = c->st.ex_open;
    if (fix_rounds) *fix_rounds = (uint32_t)c->st.ex_rounds;
    if (lattice_segments) *lattice_segments = c->st.ex_segs;
    if (lattice_fallbacks) *lattice_fallbacks = c->st.ex_fallbacks;
    return XRIT_OK;
}

int xrit_costas_state(xrit_costas *c, float *phase, float *freq)
{
    if (!c || !phase || !freq) return XRIT_E_INVALID;
    XR_HIP(hipSetDevice(c->device));
    return c->st.get_state(phase, freq, c->stream);
}

void xrit_costas_destroy(xrit_costas *c) { stage_close(c); }

int xrit_clock_create(float omega, float gain_omega, float mu, float gain_mu, float omega_rel_limit, int device,
                      xrit_clock **out)
{
    if (!out || !(omega >= 1.0f)) { set_error("bad argument"); return XRIT_E_INVALID; }
    xrit_clock *c = new (std::nothrow) xrit_clock();
    if (!c) return XRIT_E_NOMEM;
    c->stream = nullptr;
    int rc = stage_open(c, device);
    if (rc == XRIT_OK) rc = c->st.init(omega, gain_omega, mu, gain_mu, omega_rel_limit, 0, 0);
    if (rc != XRIT_OK) { stage_close(c); return rc; }
    c->st.ov_allow = false;         // (the stage object hands out complex symbols: ClockRecovery::Work's output)
    *out = c;
    return XRIT_OK;
}

int xrit_clock_work(xrit_clock *c, const float *in, size_t n, float *out, size_t cap, size_t *n_out)
{
    if (!c || !n_out || (n && !in)) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(c->device));
    float2 *slot = nullptr;
    XR_TRY(c->st.input_slot(n, &slot, c->stream));
    if (n) XR_HIP(hipMemcpyAsync(slot, in, n * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    XR_TRY(c->out.reserve((cap + 8) * sizeof(float2)));
    XR_TRY(c->st.run(n, nullptr, c->out.as<float2>(), cap, n_out, c->stream, nullptr));
    if (*n_out && out)
        XR_HIP(hipMemcpyAsync(out, c->out.p, *n_out * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    XR_HIP(hipStreamSynchronize(c->stream));
    return XRIT_OK;
}

int xrit_clock_set_serial(xrit_clock *c, int serial)
{
    if (!c) return XRIT_E_INVALID;
    c->st.serial = serial != 0;
    return XRIT_OK;
}

int xrit_clock_set_exact(xrit_clock *c, int exact, int window)
{
    if (!c) return XRIT_E_INVALID;
    if (exact < -3) { set_error("clock_exact = %d: -3 .. n (see xrit_demod_config.clock_exact)", exact); return XRIT_E_INVALID; }
    c->st.exact = exact == -3 ? 0 : exact;          // (-3: the default's plan, its first relay passes approximate -- as in xrit_demod_create)
    c->st.relay_quick = exact == -3;
    c->st.relay_window = window > 0 ? window : 0;
    return XRIT_OK;
}

void xrit_clock_destroy(xrit_clock *c) { stage_close(c); }

int xrit_rtl_create(float sample_rate, int device, xrit_rtl **out)
{
    if (!out || !(sample_rate > 0)) { set_error("bad argument"); return XRIT_E_INVALID; }
    xrit_rtl *r = new (std::nothrow) xrit_rtl();
    if (!r) return XRIT_E_NOMEM;
    r->stream = nullptr;
    int rc = stage_open(r, device);
    if (rc == XRIT_OK) rc = r->st.init(sample_rate);
    if (rc != XRIT_OK) { stage_close(r); return rc; }
    *out = r;
    return XRIT_OK;
}

int xrit_rtl_work(xrit_rtl *r, const uint8_t *data, size_t n_complex, float *out_iq)
{
    if (!r || (n_complex && (!data || !out_iq))) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(r->device));
    XR_TRY(r->in.reserve(2 * n_complex + 16));
    XR_TRY(r->out.reserve((n_complex + 8) * sizeof(float2)));
    if (n_complex) XR_HIP(hipMemcpyAsync(r->in.p, data, 2 * n_complex, hipMemcpyHostToDevice, r->stream));
    XR_TRY(r->st.run(r->in.p, r->out.as<float2>(), n_complex, r->stream, nullptr));
    if (n_complex) XR_HIP(hipMemcpyAsync(out_iq, r->out.p, n_complex * sizeof(float2), hipMemcpyDeviceToHost, r->stream));
    XR_HIP(hipStreamSynchronize(r->stream));
    return XRIT_OK;
}

void xrit_rtl_destroy(xrit_rtl *r) { stage_close(r); }

// ---------------------------------------------------------------- synth
void xrit_synth_defaults(xrit_synth_params *p)
{
    if (!p) return;
    p->fs_in = 1.25e6;
    p->symbol_rate = 293883.0;
    p->alpha = 0.5;
    p->amplitude = 0.1;
    p->carrier_hz = 500.0;
    p->phase0 = 0.7;
    p->timing_offset = 0.3;
    p->clock_ppm = 20.0;
    p->esn0_db = 12.0;
    p->seed = 0x58524954ull;
}

int xrit_synth_generate_device(const xrit_synth_params *p, uint64_t start, size_t n, float *d_out, int device,
                               void *stream)
{
    if (!p || (n && !d_out)) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(select_device(device));
    return launch_synth(*p, start, n, reinterpret_cast<float2 *>(d_out), (hipStream_t)stream);
}

int xrit_device_read_bandwidth(const void *d_buf, size_t bytes, int reps, int device, void *stream, double *gb_per_s)
{
    if (!d_buf || !gb_per_s) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_TRY(select_device(device));
    return launch_read_bw(d_buf, bytes, reps, (hipStream_t)stream, gb_per_s);
}

}  // extern "C"
