// demod.cpp -- the chain handle of the C ABI (include/xritdemod_amd.h): errors and device selection, the configurations,
// xrit_demod.  What the handle decides about its inputs in flight is chain_pipeline.h's; this file performs it with HIP.
// (The stage objects and the one-shot wrappers: stages_abi.cpp; the handle's streams: stream_pool.cpp.)
// Stage order, buffer hand-over and parameter defaults follow
// /root/reference/demodulator/src/demodulator.cpp:100-168 (processSamples) and
// :436-450 (construction); constants from Parameters.h:16-37.
#include "kernels.h"
#include "chain_pipeline.h"
#include "stream_pool.h"

#include <chrono>
#include <cmath>
#include <new>
#include <thread>
#include <vector>

namespace xrit {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }

int select_device(int device)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no usable HIP device (%s); this library has no CPU path",
                  e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return XRIT_E_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        set_error("device %d out of range (0..%d)", device, count - 1);
        return XRIT_E_INVALID;
    }
    XR_HIP(hipSetDevice(device));
    return XRIT_OK;
}

}  // namespace xrit

using namespace xrit;

typedef ChainSlice SliceIO;

static_assert(CHAIN_WALK_STREAMS == XRIT_WALK_STREAMS, "chain_pipeline.h names the walker streams one by one");
constexpr int CHAIN_STREAMS = CHAIN_WALK1 + 1;
// the handle's events, all without timing
enum ChainEvent {
    EV_DONE,            // the current call's clock recovery has left its result
    EV_READY,           // input ready on the caller's stream
    EV_FE0, EV_FE1,     // front end of a set done
    EV_RELAY,           // the relay kernels of the current call come next
    EV_COSTAS,          // the Costas loop started last has run its batch (ChainQueue::costas_event_of: whose)
    CHAIN_EVENTS
};

struct xrit_demod {
    xrit_demod_config cfg{};
    int device = 0;
    // by ChainStream (chain_pipeline.h: what runs on which).  own[CHAIN_CALLER]: where calls without a stream of the
    // caller's run; own[CHAIN_COSTAS] is used with cfg.front_exact = 2 only (q.has_costas_stream)
    hipStream_t own[CHAIN_STREAMS] = {};
    bool pooled = false;        // the streams go back to the process's pool when the handle is destroyed
    hipEvent_t ev[CHAIN_EVENTS] = {};
    ChainQueue q;               // the inputs registered ahead and what has been started for them
    bool costas_idle = false;   // the current call's Costas loop was finished before its clock recovery began: the stage is free
    float sps = 0, circuit_rate = 0;
    int dec_ntaps = 0;
    FirStage dec, rrc;
    AgcStage agc;
    CostasStage costas;
    ClockStage clock;
    // Two sets of front-end buffers: the front end of the NEXT burst (xrit_demod_prefetch_device, on the front ends' stream) fills one
    // while the feedback loops of the current burst read the other.
    DevBuf bufA[2], bufB[2], bufC[2], bufR[2], stat[2], in_dev, soft_dev, q_in, q_out;
    RtlIngestStage rtl;
    bool poisoned = false;      // a call failed after some stage had advanced its carried state
    // what the Costas loop of the CURRENT call reported when it was finished: taken there, because with a registered next input the
    // stage begins the next burst's loop (and resets its counters) before this call returns
    struct CostasSeen { int passes = 0; unsigned unconverged = 0; float max_residual = 0; bool walked = false; } costas_seen;
    bool no_defer = false;      // XRIT_NO_DEFER: registered front ends start at once also with the exact closure on (A/B runs)
    bool keep_stages = false;   // every stage's output is copied (diagnostics, tests): no fusion across stages
    bool keep_symbols = false;  // only the complex symbols of the clock recovery are kept (constellation tap)
    bool agc_fallback_seen = false;   // this call: the AGC's guard sent a slice down the serial path
    DevBuf stage_buf[5];
    size_t stage_n[5] = {0, 0, 0, 0, 0};
    Profiler prof;
    xrit_demod_stats stats{};
    std::vector<std::string> prof_names;
};

extern "C" {

const char *xrit_last_error(void) { return get_error(); }
const char *xrit_version(void) { return "xritdemod_amd 0.1 (gfx950)"; }

int xrit_device_count(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

static void config_common(xrit_demod_config *c, float sample_rate, uint32_t decimation)
{
    memset(c, 0, sizeof *c);
    c->sample_rate = sample_rate;
    c->decimation = decimation ? decimation : 1;
    c->rrc_taps = 63;                                  // RRC_TAPS
    c->agc_rate = 0.01f;                               // AGC_RATE
    c->agc_reference = 0.5f;                           // AGC_REFERENCE
    c->agc_gain = 1.f;                                 // AGC_GAIN
    c->agc_max_gain = 4000;                            // AGC_MAX_GAIN
    c->pll_alpha = 0.0037f;                            // (float)CLOCK_ALPHA, demodulator.cpp:220
    c->clock_mu = 0.5f;                                // CLOCK_MU
    c->clock_alpha = 0.0037f;                          // CLOCK_ALPHA
    c->clock_gain_omega = (0.0037f * 0.0037f) / 4.0f;  // CLOCK_GAIN_OMEGA
    c->clock_omega_limit = 0.005f;                     // CLOCK_OMEGA_LIMIT
}

void xrit_demod_config_lrit(xrit_demod_config *c, float sample_rate, uint32_t decimation)
{
    config_common(c, sample_rate, decimation);
    c->symbol_rate = 293883;   // LRIT_SYMBOL_RATE
    c->rrc_alpha = 0.5f;       // LRIT_RRC_ALPHA
}

void xrit_demod_config_hrit(xrit_demod_config *c, float sample_rate, uint32_t decimation)
{
    config_common(c, sample_rate, decimation);
    c->symbol_rate = 927000;   // HRIT_SYMBOL_RATE
    c->rrc_alpha = 0.3f;       // HRIT_RRC_ALPHA
}

int xrit_demod_create(const xrit_demod_config *cfg, xrit_demod **out)
{
    if (!cfg || !out) { set_error("null argument"); return XRIT_E_INVALID; }
    *out = nullptr;
    if (cfg->decimation < 1 || cfg->symbol_rate == 0 || !(cfg->sample_rate > 0)) {
        set_error("invalid configuration");
        return XRIT_E_INVALID;
    }
    if (cfg->costas_chain_len != 0 && (cfg->costas_chain_len < 16 || cfg->costas_chain_len > 320)) {
        set_error("costas_chain_len = %d: 0 (= 256) or 16..320 samples; beyond that the hand-off solve does not converge reliably",
                  cfg->costas_chain_len);
        return XRIT_E_INVALID;
    }
    if (cfg->rrc_taps < 3) {
        set_error("rrc_taps = %d: the matched filter needs at least 3 taps (RRC_TAPS is 63, Parameters.h:28)", cfg->rrc_taps);
        return XRIT_E_INVALID;
    }
    // the AGC's gain recurrence is evaluated as a scan of maps g -> min(a g + b, c), valid for positive gains
    if (!(cfg->agc_rate > 0) || !(cfg->agc_reference > 0) || !(cfg->agc_gain > 0) || !(cfg->agc_max_gain >= 0)) {
        set_error("AGC rate, reference and initial gain must be positive (Parameters.h:34-37: 0.01, 0.5, 1, 4000)");
        return XRIT_E_INVALID;
    }
    if (cfg->front_exact < -1 || cfg->front_exact > 2) {
        set_error("front_exact = %d: -1 (never), 0 (below the big-burst size), 1 or 2 (always)", cfg->front_exact);
        return XRIT_E_INVALID;
    }
    if (!(cfg->sample_rate / (float)cfg->decimation / (float)cfg->symbol_rate >= 1.0f)) {
        set_error("fewer than one sample per symbol after decimation");
        return XRIT_E_INVALID;
    }
    XR_TRY(select_device(cfg->device));
    xrit_demod *d = new (std::nothrow) xrit_demod();
    if (!d) return XRIT_E_NOMEM;
    d->cfg = *cfg;
    d->device = cfg->device;
    // demodulator.cpp:436-437 (float arithmetic as written there)
    d->circuit_rate = cfg->sample_rate / ((float)cfg->decimation);
    d->sps = d->circuit_rate / ((float)cfg->symbol_rate);
    int rc = XRIT_OK;
    do {
        {
            StreamSet st;
            if (!stream_set_acquire(d->device, &st)) { set_error("hipStreamCreate failed"); rc = XRIT_E_HIP; break; }
            d->own[CHAIN_CALLER] = st.s; d->own[CHAIN_FRONT] = st.s2; d->own[CHAIN_COSTAS] = st.sc;
            for (int i = 0; i < XRIT_WALK_STREAMS; ++i) d->own[CHAIN_WALK0 + i] = st.s3[i];
            d->pooled = true;
        }
        for (auto &e : d->ev)
            if (rc == XRIT_OK && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); rc = XRIT_E_HIP; }
        if (rc != XRIT_OK) break;
        std::vector<float> rrc = design_rrc(1, d->circuit_rate, cfg->symbol_rate, cfg->rrc_alpha, cfg->rrc_taps);
        std::vector<float> lp = design_lowpass(1, cfg->sample_rate, d->circuit_rate / 2, 100e3);
        d->dec_ntaps = (int)lp.size();
        // (cfg.front_exact = 2: both filters summed in the CPU chain's order, the AGC and the Costas loop walked literally --
        // the front end bit for bit the CPU chain's through the Costas loop; fir.hip, agc.hip, costas_exact.hip)
        d->dec.exact = d->rrc.exact = d->agc.exact = d->costas.exact = cfg->front_exact == 2;
        // (... and its Costas loops -- their exact walkers are latency, not work -- beside the next front end)
        d->q.has_costas_stream = cfg->front_exact == 2 && !getenv("XRIT_NO_COSTAS_STREAM");
        // (wherever such a call takes the bit-exact front end -- the default and parity mode --, a call of up to 200 k symbols, i.e.
        // every chunk size of the reference, is ONE exact walk of the clock recovery: the CPU chain's words.  With the fast
        // front end on calls of every size, cfg.front_exact = -1 / 1, the limit stays where one walk costs no more than the
        // relay, 73.7 k symbols: there is no word to keep.)
        if (cfg->front_exact == 2 || cfg->front_exact == 0) d->clock.one_walk_max = 200000;
        if ((rc = d->dec.init(lp.data(), (int)lp.size(), (int)cfg->decimation)) != XRIT_OK) break;
        if ((rc = d->rtl.init(cfg->sample_rate)) != XRIT_OK) break;
        if ((rc = d->agc.init(cfg->agc_rate, cfg->agc_reference, cfg->agc_gain, cfg->agc_max_gain)) != XRIT_OK) break;
        if ((rc = d->rrc.init(rrc.data(), (int)rrc.size(), 1)) != XRIT_OK) break;
        if ((rc = d->costas.init(cfg->pll_alpha, cfg->costas_chain_len, cfg->max_passes)) != XRIT_OK) break;
        // (cfg.front_exact, the opt-in parity mode: the final pass starts every chain four chains early)
        if (cfg->front_exact == 1) d->costas.final_warm = 4;
        if ((rc = d->clock.init(d->sps, cfg->clock_gain_omega, cfg->clock_mu, cfg->clock_alpha, cfg->clock_omega_limit,
                                cfg->clock_chain_syms, cfg->max_passes > 0 ? cfg->max_passes : 0)) != XRIT_OK) break;
        d->clock.serial = cfg->clock_serial != 0;
        d->clock.exact = cfg->clock_exact == -3 ? 0 : cfg->clock_exact;        // (-3: the default's plan, its first relay passes approximate)
        d->clock.relay_quick = cfg->clock_exact == -3;
#ifdef XRIT_EXPERIMENTS
        d->no_defer = getenv("XRIT_NO_DEFER") != nullptr;
#endif
#ifdef XRIT_EXPERIMENTS
        if (const char *e = getenv("XRIT_OV_CSTREAM_BELOW")) d->q.costas_own_stream_below = (size_t)atoll(e);
#endif
        d->clock.relay_window = cfg->clock_exact_window > 0 ? cfg->clock_exact_window : 0;
        if (cfg->clock_min_passes > 0)
            d->clock.min_passes = cfg->clock_min_passes < d->clock.max_passes ? cfg->clock_min_passes : d->clock.max_passes;
    } while (0);
    if (rc != XRIT_OK) { xrit_demod_destroy(d); return rc; }
    *out = d;
    return XRIT_OK;
}

void xrit_demod_destroy(xrit_demod *d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    // a front end that ran ahead may still be at work, or a Costas loop, or walkers; the caller's own stream last
    for (ChainStream st : {CHAIN_FRONT, CHAIN_COSTAS, CHAIN_WALK0, CHAIN_WALK1, CHAIN_CALLER})
        if (d->own[st]) (void)hipStreamSynchronize(d->own[st]);
    d->dec.release(); d->rrc.release(); d->agc.release(); d->costas.release(); d->clock.release();
    for (auto e : d->ev) if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) { d->bufA[i].release(); d->bufB[i].release(); d->bufC[i].release(); d->bufR[i].release(); d->stat[i].release(); }
    d->rtl.release();
    d->in_dev.release(); d->soft_dev.release();
    d->q_in.release(); d->q_out.release();
    for (auto &b : d->stage_buf) b.release();
    if (d->pooled) {
        StreamSet st;
        st.device = d->device; st.s = d->own[CHAIN_CALLER]; st.s2 = d->own[CHAIN_FRONT]; st.sc = d->own[CHAIN_COSTAS];
        for (int i = 0; i < XRIT_WALK_STREAMS; ++i) st.s3[i] = d->own[CHAIN_WALK0 + i];
        stream_set_release(st);
    }
    delete d;
}

int xrit_demod_reset(xrit_demod *d, void *stream)
{
    if (!d) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(d->device));
    hipStream_t s = stream ? (hipStream_t)stream : d->own[CHAIN_CALLER];
    // a front end that ran ahead belongs to the stream being left, and so do Costas loops and walkers
    for (ChainStream st : {CHAIN_FRONT, CHAIN_COSTAS, CHAIN_WALK0, CHAIN_WALK1})
        if (st != CHAIN_COSTAS || d->q.has_costas_stream) XR_HIP(hipStreamSynchronize(d->own[st]));
    if (d->costas.job.n && d->q.count > 0) {
        // (a Costas loop begun ahead and never looked at: the stage's bookkeeping is brought to an end before its state is reset)
        for (int i = 0; i < d->q.count; ++i)
            if (d->q.in[i].costas_begun && !d->q.in[i].costas_finished) { bool redone = false; (void)d->costas.finish(d->own[d->q.in[i].costas_stream], nullptr, &redone); }
    }
    chain_reset(d->q);
    XR_TRY(d->dec.reset(s));
    XR_TRY(d->rrc.reset(s));
    XR_TRY(d->agc.reset(s));
    XR_TRY(d->rtl.reset(s));
    XR_TRY(d->costas.reset(s));
    XR_TRY(d->clock.reset(s));
    d->poisoned = false;
    return XRIT_OK;
}

int xrit_build_experiments(void)
{
#ifdef XRIT_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

void *xrit_demod_stream(xrit_demod *d) { return d ? (void *)d->own[CHAIN_CALLER] : nullptr; }
float xrit_demod_sps(const xrit_demod *d) { return d ? d->sps : 0.f; }
int xrit_demod_decimator_ntaps(const xrit_demod *d) { return d ? d->dec_ntaps : 0; }

static int keep_stage(xrit_demod *d, int idx, const void *src, size_t n, hipStream_t s)
{
    if (!d->keep_stages) return XRIT_OK;
    XR_TRY(d->stage_buf[idx].reserve((n + 1) * sizeof(float2)));
    if (n) XR_HIP(hipMemcpyAsync(d->stage_buf[idx].p, src, n * sizeof(float2), hipMemcpyDeviceToDevice, s));
    d->stage_n[idx] = n;
    return XRIT_OK;
}

// ---- one time slice through the chain, in two halves ------------------------------------------------------
// front_end(): ingest conversion, decimator, AGC, RRC (demodulator.cpp:54-74,136-149) into buffer set `set`;
// loops(): Costas and clock recovery (:152-157) on what front_end() left.  Split so that the front end of the
// next slice can run on a second stream while the feedback loops of this one iterate.
// Which front end a call of n input samples takes.  cfg.front_exact = 2: the bit-exact one, always; 0 (default, round 6): the
// bit-exact one for calls below the big-burst size -- the reference's own chunk sizes (32 Ki .. 512 Ki samples) and everything
// up to a million symbols, where a call is launch latency and not throughput: the soft symbols of a call of up to 74 k symbols
// are then the CPU chain's word for word -- and the fast one for bursts of a million symbols and more, the ones `value` is
// quoted on; 1: the fast one with the Costas loop's final pass warmed up; -1: the fast one, always (round 5's default).
static bool front_exact_call(const xrit_demod *d, size_t n)
{
    if (d->cfg.front_exact == 2) return true;
    if (d->cfg.front_exact != 0) return false;
    const unsigned D = d->cfg.decimation;
    const double length = (double)(D > 1 ? n / D : n);
    return length / (double)d->sps < (double)d->clock.ov_min;
}

int xrit_demod_front_exact_for(const xrit_demod *d, size_t n)
{
    if (!d) return XRIT_E_INVALID;
    return front_exact_call(d, n) ? 1 : 0;
}

static int front_end(xrit_demod *d, const void *in, size_t n, int type, int set, hipStream_t s, Profiler *prof, SliceIO *io)
{
    io->set = set;
    const bool ex = front_exact_call(d, n);
    io->exact = ex;
    const unsigned D = d->cfg.decimation;
    if (type == XRIT_SAMPLE_U8IQ) {
        // RtlFrontend::internalCallback (RtlFrontend.cpp:102-116) hands FLOATIQ to onSamplesAvailable
        XR_TRY(d->bufR[set].reserve((n + 8) * sizeof(float2)));
        XR_TRY(d->rtl.run(in, d->bufR[set].as<float2>(), n, s, prof));
        in = d->bufR[set].p;
        type = XRIT_SAMPLE_FLOATIQ;
    }
    size_t length = n;
    if (D > 1) length = n / D;   // demodulator.cpp:137 -- the remainder of the chunk is dropped
    io->length = length;
    XR_TRY(d->bufA[set].reserve((length + 8) * sizeof(float2)));
    XR_TRY(d->bufB[set].reserve((length + 8) * sizeof(float2)));
    float2 *A = d->bufA[set].as<float2>(), *B = d->bufB[set].as<float2>();
    const float2 *cur = nullptr;
    // with a decimator in front, its epilogue leaves the AGC's composed gain maps: the AGC sweeps the stream
    // twice (scan of the maps aside) instead of three times
    const bool agc_fused = !ex && D > 1 && length > 0 && d->dec.agc_supported();
    if (D > 1) {
        AgcEpilogue epi{};
        if (agc_fused) XR_TRY(d->agc.fused_begin(length, d->dec.plan.RC, s, &epi));
        XR_TRY(d->dec.run(in, type, A, length, s, prof, nullptr, 0, agc_fused ? &epi : nullptr, nullptr, ex));          // :138
        cur = A;
    } else if (type != XRIT_SAMPLE_FLOATIQ) {
        ProfScope ps(prof, "convert", s);
        XR_TRY(launch_convert(in, type, A, length, s));            // :57-70
        cur = A;
    } else {
        cur = reinterpret_cast<const float2 *>(in);
    }
    XR_TRY(keep_stage(d, 0, cur, length, s));
    // ... and when nobody asks for the AGC output itself, the matched filter applies the gains while it fills its
    // window: the AGC then costs the stream no sweep of its own at all
    const bool agc_in_rrc = agc_fused && !d->keep_stages && d->rrc.agc_fill_supported(d->dec.plan.RC);
    // no decimator (C1, C3), or one whose kernel has no such epilogue (the polyphase one, C5): the run maps come
    // from one read-only sweep, the rest is the same
    const bool agc_in_rrc_d1 = !ex && !agc_fused && length > 0 && !d->keep_stages && d->rrc.agc_fill_supported(3);
    AgcFill fill{};
    float2 *Cfb = nullptr;      // where the serial fallback would put the AGC output (guard tripped)
    if (agc_in_rrc || agc_in_rrc_d1) {
        XR_TRY(d->bufC[set].reserve((length + 8) * sizeof(float2)));
        Cfb = d->bufC[set].as<float2>();
        if (agc_in_rrc_d1) XR_TRY(d->agc.fused_reduce(cur, length, 3, s, prof));
        XR_TRY(d->agc.fused_scan(cur, Cfb, length, agc_in_rrc ? d->dec.plan.RC : 3, s, prof, &fill));    // :143
    }
    else if (agc_fused) XR_TRY(d->agc.fused_finish(cur, B, length, d->dec.plan.RC, s, prof));
    else XR_TRY(d->agc.run(cur, B, length, s, prof, ex));
    XR_TRY(keep_stage(d, 1, B, length, s));
    // the RRC epilogue leaves the per-chain statistic of the Costas guess, the Costas final pass the
    // timing-line statistic of the clock-recovery guess: neither stage sweeps its input once more for it
    // (sum z^2 per run of 8 outputs: the chain sums and the loop's sub-block model both come from it, costas.hip)
    constexpr int SUB = 8;
    XR_TRY(d->stat[set].reserve(((length + SUB - 1) / SUB + 2) * sizeof(float2)));
    io->stat_ready = length > 0 && d->rrc.stat_supported(SUB) && d->costas.L % SUB == 0;
    // (fused: A holds the decimator output, which the fill reads; the filter output goes to B's place instead)
    const bool fill_on = agc_in_rrc || agc_in_rrc_d1;
    float2 *rrc_out = fill_on ? B : A;
    XR_TRY(d->rrc.run(fill_on ? Cfb : B, XRIT_SAMPLE_FLOATIQ, rrc_out, length, s, prof, io->stat_ready ? d->stat[set].as<float2>() : nullptr, SUB,
                      nullptr, fill_on ? &fill : nullptr, ex)); // :148
    XR_TRY(keep_stage(d, 2, rrc_out, length, s));
    io->rrc = rrc_out;
    io->agc_flag = d->agc.state.as<float>() + 2 * d->agc.cur + 1;
    return XRIT_OK;
}

// a call of n input samples walks overlapping blocks (clock_overlap.h): bursts of a million symbols and more in the default
// configuration
static bool ov_call(xrit_demod *d, size_t n)
{
    return chain_ov_call(d->clock, d->clock.xpad, d->keep_stages || d->keep_symbols, d->cfg.decimation, n);
}

// the front end of a registered input on the front ends' stream (xrit_demod_prefetch_device); `after`: not before this event
static int launch_prefetched(xrit_demod *d, ChainInput &f, hipEvent_t after)
{
    // the stream may read the input once whatever the caller queued on its stream at registration is done, and may touch
    // the stages once the previous front end (on either stream) is done
    hipStream_t s2 = d->own[CHAIN_FRONT];
    XR_HIP(hipStreamWaitEvent(s2, d->ev[EV_READY], 0));
    if (after) XR_HIP(hipStreamWaitEvent(s2, after, 0));
    const ChainFrontEnd fe = chain_front_end_take(d->q);
    if (fe.behind_set >= 0) XR_HIP(hipStreamWaitEvent(s2, d->ev[EV_FE0 + fe.behind_set], 0));
    Profiler *prof = d->prof.enabled ? &d->prof : nullptr;
    // (the filters' waves in front of the walkers at issue -- where the walkers' latency is hidden: bursts that walk overlapping blocks)
    d->dec.prio = d->rrc.prio = f.ov ? 1 : 0;
    int rc = front_end(d, f.samples, f.n, f.type, fe.set, s2, prof, &f.io);
    d->dec.prio = d->rrc.prio = 0;
    if (rc != XRIT_OK) { d->poisoned = true; return rc; }
    XR_HIP(hipEventRecord(d->ev[EV_FE0 + fe.set], s2));
    chain_front_end_done(d->q, f, fe.set);
    return XRIT_OK;
}

// the Costas loop of a slice (demodulator.cpp:152): guess, a batch of passes with a device-side stop test and the final pass,
// enqueued on s; it writes into the clock recovery's (next) input buffer
static int costas_enqueue(xrit_demod *d, const SliceIO &io, hipStream_t s, Profiler *prof, float2 **slot_out)
{
    const size_t length = io.length;
    const int L = d->costas.L;
    float2 *slot = nullptr;
    XR_TRY(d->clock.input_slot(length, &slot, s));
    double2 *om = nullptr;
    if (length) om = d->clock.om_slot((int)((length + (size_t)L - 1) / (size_t)L), L);
    const double inv_sps = 1.0 / (double)d->sps;
    const float2 *stat = io.stat_ready ? d->stat[io.set].as<float2>() : nullptr;
    XR_TRY(d->costas.begin(static_cast<const float2 *>(io.rrc), slot, length, s, prof, stat, om, 0, inv_sps, io.exact));
    if (length) XR_TRY(d->clock.om_scan(s));     // the timing guess's count curve, behind the final pass that leaves its statistic
    if (length) XR_TRY(d->agc.request_flag_at(static_cast<const float *>(io.agc_flag), s));   // the AGC's guard flag rides along: no wait of its own
    *slot_out = slot;
    return XRIT_OK;
}

// (a registered front end of the next burst goes in front of this call's relay kernels -- and behind it, where this call's
// own Costas loop is done with the stage, the next burst's Costas loop: chain_pipeline.h, the chains path's second moment)
static void set_relay_hook(xrit_demod *d, hipStream_t s)
{
    d->clock.before_relay = [d, s](int phase) -> int {
        // phase 0: in front of the relay kernels (an event marks the spot); phase 1: once they are enqueued
        if (!chain_start_under_relay(d->q)) return XRIT_OK;
        if (phase == 0) { XR_HIP(hipEventRecord(d->ev[EV_RELAY], s)); return XRIT_OK; }
        const bool costas_too = chain_costas_under_relay(d->costas_idle);
        if (d->clock.trace_env) fprintf(stderr, "[xrit] the registered front end starts with the relay kernels%s\n", costas_too ? ", its Costas loop behind it" : "");
        ChainInput &f = d->q.in[0];
        XR_TRY(launch_prefetched(d, f, d->ev[EV_RELAY]));
        if (costas_too) {
            float2 *slot = nullptr;
            int rc = costas_enqueue(d, f.io, d->own[CHAIN_FRONT], d->prof.enabled ? &d->prof : nullptr, &slot);
            if (rc != XRIT_OK) { d->poisoned = true; return rc; }
            XR_HIP(hipEventRecord(d->ev[EV_COSTAS], d->own[CHAIN_FRONT]));
            chain_costas_begun(d->q, f, CHAIN_FRONT, slot, -1, 0);      // (no overlap job is noted: its call takes the chains path)
        }
        return XRIT_OK;
    };
}

// clock recovery (:156, SymbolManager.cpp:104) of a slice whose Costas loop has been enqueued on s (costas_done: has been
// finished ahead of this call, on the front ends' stream)
static void costas_note(xrit_demod *d)
{
    d->costas_seen.passes = d->costas.passes;
    d->costas_seen.unconverged = d->costas.unconverged;
    d->costas_seen.max_residual = d->costas.max_residual;
    d->costas_seen.walked = d->costas.job.rescued && d->costas.walked;
}

// the host looks at the Costas loop's stop test (and continues its passes on s where the batch did not close) and notes
// what the loop and the AGC's guard reported for this call
static int costas_look(xrit_demod *d, size_t length, hipStream_t s, Profiler *prof, bool *redone)
{
    if (length && d->agc.requested_flag() == 2.0f) d->agc_fallback_seen = true;
    const int rc = d->costas.finish(s, prof, redone);
    if (rc == XRIT_OK) costas_note(d);
    return rc;
}

// a finished call's statistics, from what the stages and the call's look at its Costas loop hold
static void fill_stats(xrit_demod *d, size_t n, size_t length, size_t nsym, int relay_segments)
{
    d->stage_n[4] = nsym;
    d->stats.samples_in = n;
    d->stats.circuit_samples = length;
    d->stats.symbols_out = nsym;
    d->stats.costas_passes = d->costas_seen.passes;
    d->stats.clock_passes = d->clock.passes;
    d->stats.costas_unconverged = d->costas_seen.unconverged;
    d->stats.clock_unconverged = d->clock.unconverged;
    d->stats.costas_max_residual = d->costas_seen.max_residual;
    d->stats.clock_max_residual = d->clock.max_residual;
    d->stats.agc_serial_fallback = d->agc_fallback_seen;
    d->stats.clock_open_large = d->clock.large_open;
    d->stats.costas_serial_walk = d->costas_seen.walked ? 1 : 0;
    d->stats.clock_relay_passes = d->clock.relay_passes;
    d->stats.clock_relay_closed = d->clock.relay_closed ? 1 : 0;
    d->stats.clock_relay_segments = relay_segments;
}

static int loops(xrit_demod *d, const SliceIO &io, float *d_soft, size_t cap, size_t *nsym, hipStream_t s, Profiler *prof,
                 long call_id, bool costas_done = false, float2 *slot_done = nullptr)
{
    // call_id: the registration this call took (0: none -- and then no input waits behind it either)
    const size_t length = io.length;
    float2 *slot = slot_done;
    // Costas (:152) and clock recovery are enqueued back to back -- guesses, a batch of hand-off passes each with a
    // device-side stop test, final / output passes -- and the host waits once.  Only when a batch did not close (cold
    // start, unlocked input) does it continue pass by pass.
    if (!costas_done) XR_TRY(costas_enqueue(d, io, s, prof, &slot));
    if (chain_costas_first(d->q, costas_done)) {
        // A stream with its next input registered: this call's Costas loop is finished FIRST (one more wait of the host), so
        // that the stage is free for the next burst's loop behind its front end, under this call's relay -- from the next
        // call on that is how every Costas loop of the stream runs and the extra wait is gone.
        XR_HIP(hipEventRecord(d->ev[EV_COSTAS], s));
        d->q.costas_event_of = call_id;
        XR_HIP(hipEventSynchronize(d->ev[EV_COSTAS]));
        bool redone = false;
        XR_TRY(costas_look(d, length, s, prof, &redone));
        if (redone) d->clock.jobs.om_rewritten();     // (the final pass ran again: the statistic is new, begin() unwraps it itself)
        costas_done = true;
    }
    float2 *sym = nullptr;
    if (d->keep_stages || d->keep_symbols) {
        XR_TRY(d->stage_buf[4].reserve((cap + 1) * sizeof(float2)));
        sym = d->stage_buf[4].as<float2>();
    }
    d->costas_idle = costas_done;
    set_relay_hook(d, s);
    const int rc_begin = d->clock.begin(length, d_soft, sym, cap, s, prof);
    d->clock.before_relay = nullptr;
    d->costas_idle = false;
    XR_TRY(rc_begin);
    XR_HIP(hipStreamSynchronize(s));
    if (!costas_done) {
        bool redone = false;
        XR_TRY(costas_look(d, length, s, prof, &redone));
        if (redone) {
            // the Costas output was rewritten after more passes: the clock recovery starts over on it
            const int L = d->costas.L;
            if (length) (void)d->clock.om_slot((int)((length + (size_t)L - 1) / (size_t)L), L);
            XR_TRY(d->clock.begin(length, d_soft, sym, cap, s, prof));
            XR_HIP(hipStreamSynchronize(s));
        }
    }
    XR_TRY(keep_stage(d, 3, slot, length, s));
    int rc = d->clock.finish(nsym, s, prof);
    if (d->keep_stages || d->keep_symbols) XR_HIP(hipStreamSynchronize(s));
    return rc;
}

// a process call takes the oldest registered input, and no other
static int pf_check_front(xrit_demod *d, const void *d_samples, size_t n, int type)
{
    if (chain_front_is(d->q, d_samples, n, type)) return XRIT_OK;
    set_error("process calls must take the prefetched inputs in the order they were prefetched");
    d->poisoned = true;
    return XRIT_E_INVALID;
}

// ---- bursts whose clock recovery walks overlapping blocks (clock_overlap.h): chain_next (chain_pipeline.h) says what may be
// enqueued for the registered inputs; a process call enqueues what the newest registration allows, waits for its own walkers
// and lays out its symbols (ClockStage::ov_finalize) -- the relay's latency, which bounds a relayed burst, is hidden.
struct ChainFacts {
    xrit_demod *d;
    bool costas_event_done() { return hipEventQuery(d->ev[EV_COSTAS]) == hipSuccess; }
    unsigned long long ov_serial() { return d->clock.jobs.serials; }
    bool can_launch_ahead(int job) { return d->clock.jobs.can_launch_ahead(job, d->clock.ov_pad_need); }
};

// one pass of chain_next's steps, each performed with HIP and its outcome written back.  Returns an error code;
// *progress: something was enqueued or finished.
static int ov_service(xrit_demod *d, bool *progress, int limit = 1 << 30)
{
    Profiler *prof = d->prof.enabled ? &d->prof : nullptr;
    if (progress) *progress = false;
    ChainFacts facts{d};
    ChainScan scan;
    for (;;) {
        const ChainStep st = chain_next(d->q, scan, facts, limit);
        if (st.kind == CHAIN_NONE) return XRIT_OK;
        ChainInput &f = d->q.in[st.i];
        hipStream_t s = d->own[st.stream];
        int rc = XRIT_OK;
        switch (st.kind) {
        case CHAIN_FRONT_END:
            XR_TRY(launch_prefetched(d, f, nullptr));
            break;
        case CHAIN_COSTAS_LOOK: {
            if (f.io.length && d->agc.requested_flag() == 2.0f) f.agc_fallback = true;
            bool redone = false;
            rc = d->costas.finish(s, prof, &redone);
            if (rc != XRIT_OK) break;
            f.c_passes = d->costas.passes; f.c_unconverged = d->costas.unconverged; f.c_max_residual = d->costas.max_residual;
            f.c_walked = d->costas.job.rescued && d->costas.walked;
            chain_costas_looked(f, redone);
            break;
        }
        case CHAIN_WALK_RESTART:
            rc = d->clock.ov_restart(f.ov_job);
            if (rc == XRIT_OK) chain_walk_restarted(f);
            break;
        case CHAIN_COSTAS_BEGIN: {
            if (st.wait_fe) XR_HIP(hipStreamWaitEvent(s, d->ev[EV_FE0 + f.io.set], 0));
            float2 *slot = nullptr;
            rc = costas_enqueue(d, f.io, s, prof, &slot);
            if (rc != XRIT_OK) break;
            XR_HIP(hipEventRecord(d->ev[EV_COSTAS], s));
            const int job = d->clock.jobs.setting_up;
            chain_costas_begun(d->q, f, st.stream, slot, job, d->clock.jobs.serial_of(job));
            break;
        }
        case CHAIN_WALK_LAUNCH:
            XR_HIP(hipStreamWaitEvent(s, d->ev[EV_COSTAS], 0));
            rc = d->clock.ov_launch(f.ov_job, s, true, prof);
            if (rc == XRIT_OK) chain_walk_launched(f);
            break;
        case CHAIN_NONE:
            break;
        }
        if (rc != XRIT_OK) { d->poisoned = true; return rc; }
        if (progress) *progress = true;
    }
}

static int process_overlap(xrit_demod *d, const void *d_samples, size_t n, int type, float *d_soft, size_t cap, size_t *n_out,
                           hipStream_t s, Profiler *prof)
{
    // the call's own input goes through the same queue: registered now if it was not registered ahead
    if (d->q.count > 0) {
        XR_TRY(pf_check_front(d, d_samples, n, type));
    } else {
        XR_HIP(hipEventRecord(d->ev[EV_READY], s));
        chain_stage(d->q, d_samples, n, type, true);
        d->q.count = 1;
    }
    auto fail = [&](int rc) { d->poisoned = true; *n_out = 0; return rc; };
    int rc = ov_service(d, nullptr);
    if (rc != XRIT_OK) return fail(rc);
    // this call's Costas loop must have been looked at before its clock recovery is laid out
    // (only THIS input here: what the host enqueues for the inputs behind it -- a Costas loop, a front end: 0.2 ms of launches --
    // goes behind this call's walkers, which are on the critical path when nothing ran ahead)
    ChainInput &f0 = d->q.in[0];
    for (int spins = 0; !f0.costas_finished; ++spins) {
        if (f0.costas_begun) { if (hipEventSynchronize(d->ev[EV_COSTAS]) != hipSuccess) { set_error("hipEventSynchronize failed"); return fail(XRIT_E_HIP); } }
        if ((rc = ov_service(d, nullptr, 1)) != XRIT_OK) return fail(rc);
        if (spins > 8) { set_error("the Costas loop of the call could not be started"); return fail(XRIT_E_INVALID); }
    }
    d->agc_fallback_seen = f0.agc_fallback;
    d->costas_seen.passes = f0.c_passes; d->costas_seen.unconverged = f0.c_unconverged;
    d->costas_seen.max_residual = f0.c_max_residual; d->costas_seen.walked = f0.c_walked;
    // joints, output and result behind this call's walkers (started here if they did not run ahead), on the call's stream.
    // (the host has SEEN the end of everything the other streams did for this input -- the Costas loop's event, a continued
    // loop's synchronise --, so s needs no event of theirs; the finalize kernels wait for the walkers' event)
    rc = d->clock.begin(f0.io.length, d_soft, nullptr, cap, s, prof);
    if (rc != XRIT_OK) return fail(rc);
    if (hipEventRecord(d->ev[EV_DONE], s) != hipSuccess) { set_error("hipEventRecord failed"); return fail(XRIT_E_HIP); }
    if ((rc = ov_service(d, nullptr)) != XRIT_OK) return fail(rc);
    // while the walkers finish: keep the inputs behind this one moving (the Costas loop of the next one may close meanwhile,
    // which frees the stage for the one after it)
    for (;;) {
        const hipError_t q = hipEventQuery(d->ev[EV_DONE]);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { set_error("hipEventQuery failed: %s", hipGetErrorString(q)); return fail(XRIT_E_HIP); }
        bool progress = false;
        if ((rc = ov_service(d, &progress)) != XRIT_OK) return fail(rc);
        if (!progress) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    size_t nsym = 0;
    rc = d->clock.finish(&nsym, s, prof);
    const size_t length = f0.io.length;
    chain_pop(d->q);
    if (rc != XRIT_OK) return fail(rc);
    if (prof) d->prof.collect();
    fill_stats(d, n, length, nsym, d->clock.relay_segments);       // (the walkers count as the call's segments)
    *n_out = nsym;
    if (d->cfg.strict && d->costas_seen.unconverged) {
        set_error("Costas hand-off did not close: %u boundaries above tolerance", d->costas_seen.unconverged);
        return XRIT_E_NOT_CONVERGED;
    }
    return XRIT_OK;
}

int xrit_demod_process_device(xrit_demod *d, const void *d_samples, size_t n, int type, float *d_soft, size_t cap,
                              size_t *n_out, void *stream)
{
    if (!d || !n_out || (n && !d_samples)) { set_error("null argument"); return XRIT_E_INVALID; }
    if (type < 0 || type > 3) { set_error("unknown sample type %d", type); return XRIT_E_INVALID; }
    *n_out = 0;
    XR_HIP(hipSetDevice(d->device));
    hipStream_t s = stream ? (hipStream_t)stream : d->own[CHAIN_CALLER];
    Profiler *prof = d->prof.enabled ? &d->prof : nullptr;
    const unsigned D = d->cfg.decimation;
    if (d->poisoned) {
        set_error("this handle's carried state is inconsistent after an earlier failed call: destroy it and create a new one");
        return XRIT_E_INVALID;
    }
    // the symbols this call can produce at most (slowest admissible symbol clock, plus the unread tail of the last
    // call): checked before any stage advances its state
    {
        const size_t length = D > 1 ? n / D : n;
        const double min_omega = (double)d->sps * (1.0 - (double)d->cfg.clock_omega_limit);
        const size_t worst = (size_t)(((double)length + (double)d->clock.jobs.carry) / min_omega) + 2;
        if (worst > cap && length > 0) {
            set_error("output capacity %zu is below the %zu symbols this call may produce (n / (decimation * sps * (1 - omega limit)) + 2)", cap, worst);
            *n_out = worst;        // the capacity that suffices; nothing has been consumed, the handle is unchanged: a front
            return XRIT_E_CAPACITY;    // end that ran ahead stays queued for the retry with the same (pointer, n, type)
        }
    }
    // (round 5: bursts of a million symbols and more in the default configuration)
    if (chain_call_overlaps(d->q, ov_call(d, n)))
        return process_overlap(d, d_samples, n, type, d_soft, cap, n_out, s, prof);
    size_t total_sym = 0, total_len = 0;
    d->agc_fallback_seen = false;
    SliceIO io;
    int rc = XRIT_OK;
    bool costas_ahead = false;
    long call_id = 0;
    if (d->q.count > 0) {
        // the front end of this call ran ahead (xrit_demod_prefetch_device): the loops wait for it, nothing else
        XR_TRY(pf_check_front(d, d_samples, n, type));
        // (registered only: the call before had no relay phase to put it in front of)
        if (chain_start_at_call(d->q)) XR_TRY(launch_prefetched(d, d->q.in[0], nullptr));
        const ChainInput f = d->q.in[0];
        chain_pop(d->q);
        io = f.io;
        call_id = f.id;
        if (f.costas_begun) {
            // its Costas loop ran ahead as well (under the relay of the call before): the host looks at its stop test now
            // (continuing the passes on the front ends' stream in the rare case the batch did not close), the clock recovery follows on s.
            // The host has WAITED for everything that stream was given for this burst -- front end, Costas loop, count curve; a
            // continued loop ends with a stream synchronise of its own -- so s needs no event to wait for (every runtime
            // call here sits between the end of one burst's relay and the start of the next one's, with the device idle:
            // measured, steady state: 8 us between two calls, 6 us from entry to ClockStage::begin, 30 us to enqueue
            // tail + guess + relay kernels, of which the device spends 20 in the first two).
            // (from here on the registered input has been consumed: a failure poisons the handle below, no early return)
            if (hipEventSynchronize(d->ev[EV_COSTAS]) != hipSuccess) { set_error("hipEventSynchronize failed"); rc = XRIT_E_HIP; }
            bool redone = false;
            if (rc == XRIT_OK) rc = costas_look(d, io.length, d->own[f.costas_stream], prof, &redone);
            if (redone) d->clock.jobs.om_rewritten();
            if (rc == XRIT_OK) rc = loops(d, io, d_soft, cap, &total_sym, s, prof, call_id, true, static_cast<float2 *>(f.slot));
            costas_ahead = true;
        } else {
            if (hipStreamWaitEvent(s, d->ev[EV_FE0 + f.io.set], 0) != hipSuccess) { set_error("hipStreamWaitEvent failed"); rc = XRIT_E_HIP; }
        }
    } else {
        const ChainFrontEnd fe = chain_front_end_take(d->q);
        // (a front end that ran ahead on the other stream earlier must be done before this one touches the stages)
        if (fe.behind_set >= 0) XR_HIP(hipStreamWaitEvent(s, d->ev[EV_FE0 + fe.behind_set], 0));
        rc = front_end(d, d_samples, n, type, fe.set, s, prof, &io);
        if (rc == XRIT_OK) { XR_HIP(hipEventRecord(d->ev[EV_FE0 + fe.set], s)); chain_front_end_started(d->q, fe.set); }
    }
    if (rc == XRIT_OK && !costas_ahead) rc = loops(d, io, d_soft, cap, &total_sym, s, prof, call_id);
    if (rc != XRIT_OK) {
        // some stage has flipped its ping-pong state, a later one has not: the handle cannot go on
        d->poisoned = true;
        *n_out = 0;
        return rc;
    }
    total_len = io.length;
    const unsigned unc_c = d->costas_seen.unconverged, large_k = d->clock.large_open;
    if (prof) d->prof.collect();
    fill_stats(d, n, total_len, total_sym, d->clock.job.relay ? d->clock.relay_segments : 0);
    *n_out = total_sym;
    if (d->cfg.strict && unc_c) {
        set_error("Costas hand-off did not close: %u boundaries above tolerance", unc_c);
        return XRIT_E_NOT_CONVERGED;
    }
    if (d->cfg.strict && large_k) {
        set_error("clock hand-off ended with %u boundaries beyond 0.02 sample or with an open symbol slip", large_k);
        return XRIT_E_NOT_CONVERGED;
    }
    return XRIT_OK;
}

// ---- between two plain calls: what touches the carried state of the loops.  The shared prologue: arguments, a poisoned
// handle, no registered input in flight (`why_not`: the entry's own end of that sentence), the device, the stream.
// (A registered input's front end / Costas loop may have started from the state as it was, and left the clock stage its
// timing statistic.)
static int between_calls(xrit_demod *d, bool args_ok, const char *null_text, size_t *n_out, const char *why_not, void *stream, hipStream_t *s)
{
    if (!d || !args_ok) { set_error("%s", null_text); return XRIT_E_INVALID; }
    if (n_out) *n_out = 0;
    if (d->poisoned) { set_error("this handle's carried state is inconsistent after an earlier failed call"); return XRIT_E_INVALID; }
    if (d->q.count > 0) { set_error("a prefetched input waits for its process call: %s", why_not); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(d->device));
    *s = stream ? (hipStream_t)stream : d->own[CHAIN_CALLER];
    return XRIT_OK;
}

// a clock recovery run again: where its complex symbols go, and what it leaves in the statistics
static float2 *redo_symbols(xrit_demod *d) { return (d->keep_stages || d->keep_symbols) ? d->stage_buf[4].as<float2>() : nullptr; }
static int redo_done(xrit_demod *d, int rc, size_t k, size_t *n_out)
{
    if (rc != XRIT_OK) { d->poisoned = true; return rc; }
    d->stage_n[4] = k;
    d->stats.symbols_out = k;
    d->stats.clock_passes = d->clock.passes;
    d->stats.clock_relay_passes = d->clock.relay_passes;
    d->stats.clock_relay_closed = d->clock.relay_closed ? 1 : 0;
    *n_out = k;
    return XRIT_OK;
}

int xrit_demod_prepare_flipped(xrit_demod *d, void *stream)
{
    hipStream_t s;
    XR_TRY(between_calls(d, true, "null argument", nullptr, "the flipped re-run belongs between plain calls", stream, &s));
    int rc = d->clock.make_alt(s, d->prof.enabled ? &d->prof : nullptr);
    if (rc != XRIT_OK) d->poisoned = true;
    return rc;
}

size_t xrit_demod_clock_carry_bytes(void) { return ClockStage::CARRY_BYTES; }

int xrit_demod_export_clock_carry(xrit_demod *d, int which, void *d_rec, void *stream)
{
    hipStream_t s;
    XR_TRY(between_calls(d, d_rec && which >= 0 && which <= 1, "null or invalid argument", nullptr,
                         "the carried state is not between two calls", stream, &s));
    return d->clock.export_carry(d_rec, which, s);
}

int xrit_demod_last_clock_exact(const xrit_demod *d)
{
    if (!d) return XRIT_E_INVALID;
    return d->clock.last_walk_exact() ? 1 : 0;
}

int xrit_demod_redo_clock_from(xrit_demod *d, const void *d_rec, float *d_soft, size_t cap, size_t *n_out, void *stream)
{
    hipStream_t s;
    XR_TRY(between_calls(d, d_rec && n_out && d_soft, "null argument", n_out, "the re-run belongs between plain calls", stream, &s));
    unsigned head[4] = {0, 0, 0, 0};
    XR_HIP(hipMemcpyAsync(head, d_rec, sizeof head, hipMemcpyDeviceToHost, s));
    XR_HIP(hipStreamSynchronize(s));
    if (head[0] != 1u || head[1] > 1024u) { set_error("not a carried clock state (xrit_demod_export_clock_carry)"); return XRIT_E_INVALID; }
    size_t k = 0;
    const int rc = d->clock.redo_from(d_rec, head[1], d_soft, redo_symbols(d), cap, &k, s, d->prof.enabled ? &d->prof : nullptr);
    return redo_done(d, rc, k, n_out);
}

int xrit_demod_flip_costas_phase(xrit_demod *d, void *stream)
{
    hipStream_t s;
    XR_TRY(between_calls(d, true, "null argument", nullptr, "its Costas loop may already have started", stream, &s));
    return d->costas.flip_phase(s);
}

int xrit_demod_redo_clock_flipped(xrit_demod *d, float *d_soft, size_t cap, size_t *n_out, void *stream)
{
    hipStream_t s;
    XR_TRY(between_calls(d, n_out && d_soft, "null argument", n_out, "the flipped re-run belongs between plain calls", stream, &s));
    size_t k = 0;
    // The negated Costas output is the other lock's output to rounding only, which alone moves a float32 M&M by its
    // 5e-5 .. 1e-4.  The run is repeated in the handle's own configuration (cfg.clock_exact: by
    // default two hand-off passes and three relay passes, csrc/clock_relay.h).
    int rc = d->clock.redo_flipped(d_soft, redo_symbols(d), cap, &k, s, d->prof.enabled ? &d->prof : nullptr);
    if (rc == XRIT_OK) rc = d->costas.flip_phase(s);
    return redo_done(d, rc, k, n_out);
}

int xrit_demod_prefetch_depth(xrit_demod *d, size_t n)
{
    if (!d) return 0;
    if (d->keep_stages || d->keep_symbols || (d->prof.enabled && !d->prof.light)) return 0;
    return ov_call(d, n) ? XRIT_AHEAD : 1;
}

int xrit_demod_prefetch_device(xrit_demod *d, const void *d_samples, size_t n, int type, void *stream)
{
    if (!d || (n && !d_samples)) { set_error("null argument"); return XRIT_E_INVALID; }
    if (type < 0 || type > 3) { set_error("unknown sample type %d", type); return XRIT_E_INVALID; }
    if (d->poisoned) { set_error("this handle's carried state is inconsistent after an earlier failed call"); return XRIT_E_INVALID; }
    const bool ov = ov_call(d, n);
    if (d->q.count >= chain_room(d->q, ov)) { set_error("%d prefetched inputs are already waiting for their process calls", d->q.count); return XRIT_E_INVALID; }
    // stage copies and per-kernel event brackets belong to one call at a time: no running ahead then
    if (d->keep_stages || d->keep_symbols || (d->prof.enabled && !d->prof.light)) return XRIT_OK;
    XR_HIP(hipSetDevice(d->device));
    hipStream_t s = stream ? (hipStream_t)stream : d->own[CHAIN_CALLER];
    // the front ends' stream may read the input once whatever the caller queued on its stream is done
    XR_HIP(hipEventRecord(d->ev[EV_READY], s));
    ChainInput &f = chain_stage(d->q, d_samples, n, type, ov);
    if (!chain_defer(d->clock.relay_by_default(), d->no_defer, ov)) {
        // (front ends run in the order of their inputs: one that is still waiting goes first)
        if (chain_start_oldest_first(d->q)) XR_TRY(launch_prefetched(d, d->q.in[0], nullptr));
        XR_TRY(launch_prefetched(d, f, nullptr));
    }
    ++d->q.count;
    return XRIT_OK;
}

int xrit_demod_process(xrit_demod *d, const void *samples, size_t n, int type, float *soft_out, size_t cap,
                       size_t *n_out)
{
    if (!d || !n_out || (n && !samples) || (cap && !soft_out)) { set_error("null argument"); return XRIT_E_INVALID; }
    if (type < 0 || type > 3) { set_error("unknown sample type %d", type); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(d->device));
    const size_t esz = type == XRIT_SAMPLE_FLOATIQ ? 8 : (type == XRIT_SAMPLE_S16IQ ? 4 : 2);
    XR_TRY(d->in_dev.reserve(n * esz + 16));
    XR_TRY(d->soft_dev.reserve((cap + 1) * sizeof(float)));
    if (n) XR_HIP(hipMemcpyAsync(d->in_dev.p, samples, n * esz, hipMemcpyHostToDevice, d->own[CHAIN_CALLER]));
    int rc = xrit_demod_process_device(d, d->in_dev.p, n, type, d->soft_dev.as<float>(), cap, n_out, d->own[CHAIN_CALLER]);
    if (rc != XRIT_OK) return rc;
    if (*n_out)
        XR_HIP(hipMemcpyAsync(soft_out, d->soft_dev.p, *n_out * sizeof(float), hipMemcpyDeviceToHost, d->own[CHAIN_CALLER]));
    XR_HIP(hipStreamSynchronize(d->own[CHAIN_CALLER]));
    return XRIT_OK;
}

int xrit_demod_read_stage(xrit_demod *d, int stage, float *out, size_t cap, size_t *n)
{
    if (!d || stage < 0 || stage > 4 || !n) { set_error("bad argument"); return XRIT_E_INVALID; }
    if (!d->keep_stages && !(d->keep_symbols && stage == 4)) {
        set_error("stage copies are off: call xrit_demod_keep_stages(d, 1) first (2 keeps stage 4 only)");
        return XRIT_E_INVALID;
    }
    *n = d->stage_n[stage];
    if (!out) return XRIT_OK;
    if (*n > cap) { set_error("stage %d holds %zu elements, capacity %zu", stage, *n, cap); return XRIT_E_CAPACITY; }
    XR_HIP(hipSetDevice(d->device));
    XR_HIP(hipStreamSynchronize(d->own[CHAIN_CALLER]));
    if (*n) XR_HIP(hipMemcpy(out, d->stage_buf[stage].p, *n * sizeof(float2), hipMemcpyDeviceToHost));
    return XRIT_OK;
}

int xrit_demod_keep_stages(xrit_demod *d, int enable)
{
    if (!d) return XRIT_E_INVALID;
    // (what runs ahead of a registered input's call is chosen by these flags: a call whose Costas loop and walkers have already
    // been started as an overlap job must not be taken by the stage-keeping path afterwards)
    if (d->q.count > 0) { set_error("prefetched inputs wait for their process calls: stage copies are switched between plain calls"); return XRIT_E_INVALID; }
    d->keep_stages = enable == 1;
    d->keep_symbols = enable == 2;
    return XRIT_OK;
}

int xrit_demod_get_stats(const xrit_demod *d, xrit_demod_stats *s)
{
    if (!d || !s) return XRIT_E_INVALID;
    *s = d->stats;
    return XRIT_OK;
}

int xrit_demod_profile(xrit_demod *d, int enable)
{
    if (!d) return XRIT_E_INVALID;
    d->prof.enabled = enable != 0;
    d->prof.light = enable == 2;
    d->prof.reset();
    return XRIT_OK;
}

int xrit_demod_profile_read(xrit_demod *d, const char **names, float *total_ms, int *launches, int cap)
{
    if (!d) return XRIT_E_INVALID;
    d->prof_names = d->prof.order;
    int n = 0;
    for (auto &nm : d->prof_names) {
        if (n >= cap) break;
        auto &v = d->prof.acc[nm];
        if (names) names[n] = nm.c_str();
        if (total_ms) total_ms[n] = (float)v.first;
        if (launches) launches[n] = v.second;
        ++n;
    }
    return n;
}

int xrit_demod_profile_samples(xrit_demod *d, const char *name, float *ms, int cap)
{
    if (!d || !name) return XRIT_E_INVALID;
    auto it = d->prof.samples.find(name);
    if (it == d->prof.samples.end()) return 0;
    int n = 0;
    for (float v : it->second) {
        if (n >= cap) break;
        if (ms) ms[n] = v;
        ++n;
    }
    return n;
}

int xrit_quantize_i8(xrit_demod *d, const float *soft, int8_t *out, size_t n)
{
    if (!d || (n && (!soft || !out))) { set_error("null argument"); return XRIT_E_INVALID; }
    XR_HIP(hipSetDevice(d->device));
    XR_TRY(d->q_in.reserve(n * sizeof(float) + 16));
    XR_TRY(d->q_out.reserve(n + 16));
    if (!n) return XRIT_OK;
    XR_HIP(hipMemcpyAsync(d->q_in.p, soft, n * sizeof(float), hipMemcpyHostToDevice, d->own[CHAIN_CALLER]));
    XR_TRY(launch_quantize_i8(d->q_in.as<float>(), d->q_out.as<int8_t>(), n, d->own[CHAIN_CALLER]));
    XR_HIP(hipMemcpyAsync(out, d->q_out.p, n, hipMemcpyDeviceToHost, d->own[CHAIN_CALLER]));
    XR_HIP(hipStreamSynchronize(d->own[CHAIN_CALLER]));
    return XRIT_OK;
}
}  // extern "C"
