// kernels.h -- stage objects of the chain (device state + launch plans).
#pragma once

#include <functional>

#include "common.h"
#include "framer_host.h"
#include "lock_host.h"
#include "clock_jobs.h"
#include "clock_plan.h"
#include "fir_plan.h"
#include "loop_core.h"
#include "taps.h"

namespace xrit {

// ---- FirFilter (demodulator.cpp:446,450; Work at :138,:148) ---------------
struct FirStage {
    FirPlan plan;        // fir_plan.h: kernel form, template key, geometry and tap layout, made once in init
    int cur = 0;
    int prio = 0;        // 1: this launch's waves at a raised issue priority (fir_decim_kernel; set by the chain per front end)
    // cfg.front_exact = 2: summed in the CPU chain's order, no FMA (the plan's exact forms); set before init or through set_exact()
    bool exact = false;
    std::vector<float> taps_host;
    int set_exact(bool on);
    DevBuf g;        // the tap image the plan names (rows, phases or the taps reversed)
    DevBuf mfb;      // matrix-pipe experiment: the Toeplitz tap operand, one float per (step, lane)
    DevBuf hist[2];  // T-1 samples of history (ping-pong)
    int init(const float *taps, int ntaps, int decim);
    int reset(hipStream_t s);     // zero history, as after construction (no reallocation)
    void release();
    // consumes n_out*D samples of `in` (sample_type as in FrontendDevice.h:11-13)
    // stat (optional): sum z^2 per run of statL outputs, written when stat_supported(statL)
    // agc (optional): the AGC's composed gain map per run of 64 * RC outputs, see AgcStage::fused_begin
    // fill (optional, D == 1): the input is the AGC's INPUT stream; the window fill applies the AGC on the fly
    // (AgcStage::fused_scan fills the descriptor) -- the AGC output is never written
    // use_exact (the chain's per-call choice, round 6): this call through the exact-order twin (a second stage object with
    // `exact` set, created beside every stage that is not exact itself; the T - 1 samples of history follow the call)
    int run(const void *in, int sample_type, float2 *out, size_t n_out, hipStream_t s, Profiler *prof,
            float2 *stat = nullptr, int statL = 0, const struct AgcEpilogue *agc = nullptr,
            const struct AgcFill *fill = nullptr, bool use_exact = false);
    FirStage *twin = nullptr;   // (owned: released in release())
    bool last_twin = false;     // the last call went through the twin: the history lives there
    FirStage() = default;
    FirStage(const FirStage &) = delete;
    FirStage &operator=(const FirStage &) = delete;
    bool agc_fill_supported(int per_lane) const { return fir_agc_fill_supported(plan, per_lane); }
    bool stat_supported(int statL) const { return fir_stat_supported(plan, statL); }
    bool agc_supported() const { return fir_agc_supported(plan); }
};

// What the decimator's epilogue needs to leave the AGC's first sweep behind (AgcStage::fused_begin fills it).
constexpr int AGC_RUN_MAX_PER_LANE = 5;
// What the matched filter's window fill needs to apply the AGC itself: the stream in front of the AGC, the
// exclusive prefix of the run maps, the call's start gain.  If the guard flag is up the gains are not the
// scan's: the kernel then reads `in`, which agc_serial_kernel has filled (never seen with normalised samples).
struct AgcFill {
    const float2 *x;
    const struct AgcMap *pre_run;
    const float *state_in;      // [0] gain at the start of the call
    float *state_out;           // [0] gain after the call (written by the history kernel), [1] guard flag
    float rate, ref, maxg;
    int per_lane;               // a run = 64 * per_lane samples
};
struct AgcEpilogue {
    struct AgcMap *maps;     // one per run of 64 * RC outputs (the outputs of one wave of the FIR kernel)
    float *state_out;        // [1] guard flag
    float rate, ref, maxg;
};

// ---- RTL-SDR ingest (RtlFrontend.cpp:26-28,57,102-116): u8 IQ -> float IQ with the frontend's DC tracker ----
struct RtlIngestStage {
    float alpha = 0;
    DevBuf state;    // running average, ping-pong across calls
    DevBuf aggs;
    int cur = 0;
    int init(float sample_rate);
    int reset(hipStream_t s);
    void release();
    int run(const void *in_u8, float2 *out, size_t n_complex, hipStream_t s, Profiler *prof);
};

// ---- AGC (demodulator.cpp:447; Work at :143) ------------------------------
struct AgcStage {
    float rate = 0, ref = 0, maxg = 0;
    DevBuf state;    // two (gain, guard flag) slots, ping-pong across calls
    DevBuf aggs;     // per-block composed maps
    int cur = 0;
    int init(float rate, float reference, float gain, float max_gain);
    int reset(hipStream_t s);
    float gain0 = 1.0f;
    void release();
    int run(const float2 *in, float2 *out, size_t n, hipStream_t s, Profiler *prof, bool use_exact = false);
    // cfg.front_exact = 2: chains walked literally from the scan's gains, warmed up until they ARE the serial recurrence (agc.hip)
    bool exact = false;
    DevBuf joints;   // exact_walk.h's joints, block records and counters
    int ex_walkers = 2048, ex_mode = 3;     // ranges per large call (two walkers per SIMD); scan switches (XRIT_CX_MODE)
    int run_exact(const float2 *in, float2 *out, size_t n, hipStream_t s, Profiler *prof);
    unsigned *ex_cnt = nullptr;             // the last exact call's counters (exact_walk.h: xw::NCNT words, device)
    int exact_counters(unsigned *out8, hipStream_t s);
    // the same in two halves around the kernel that produces `in` (the decimator): fused_begin() before it
    // (hands out the epilogue descriptor), fused_finish() after it -- the stream is swept twice, not three times
    int fused_begin(size_t n, int per_lane, hipStream_t s, AgcEpilogue *epi);      // per_lane: the producer's RC
    int fused_finish(const float2 *in, float2 *out, size_t n, int per_lane, hipStream_t s, Profiler *prof);
    // no producer with an epilogue in front: one read-only sweep composes the run maps (then fused_scan())
    int fused_reduce(const float2 *in, size_t n, int per_lane, hipStream_t s, Profiler *prof);
    // instead of fused_finish(): scan only; the consumer (the matched filter) applies the gains in its window fill.
    // `fallback` receives the serial result if the guard trips.
    int fused_scan(const float2 *in, float2 *fallback, size_t n, int per_lane, hipStream_t s, Profiler *prof, AgcFill *fill);
    int gain(float *g, hipStream_t s);
    int fallback_flag(float *flag, hipStream_t s);
    // the same without a wait of its own: the copy goes into a pinned word behind whatever is queued on s, and
    // the caller reads it after its next synchronise
    int request_flag(hipStream_t s);
    int request_flag_at(const float *flag, hipStream_t s);      // a given call's flag slot (the stage may have moved on)
    float requested_flag() const { return h_flag ? *h_flag : 0.0f; }
    float *h_flag = nullptr;
};

// ---- CostasLoop (demodulator.cpp:448; Work at :152) -----------------------
struct CostasStage {
    CostasGains gains{};
    int L = 256;            // samples per chain
    int max_passes = 32;
    float trust = 1.0f, tol_phase = 1e-5f, tol_freq = 3e-8f;
    DevBuf state;           // float2 (phase, freq) carried across calls
    DevBuf S, E, J, stat, sub, dlin, work, flags, counters, wsolve, rescue;
    // round 4: one Newton step on a model of the loop over runs of 8 samples refines the guesses before the first pass
    // over the samples (costas_model_pass_kernel); that pass is accepted on prediction up to model_accept (rad)
    bool model_step = true;
    float model_accept = 5e-3f;
    bool force_gated = false;         // always the three-launch solve with the trust gate (XRIT_GATED_SOLVE=1)
    int final_warm = 0;             // chains of warm-up in front of every chain of the final pass (cfg.front_exact: 4; costas.hip)
    bool keep_spare = false, trace_env = false, no_serial_walk = false;   // XRIT_KEEP_SPARE, XRIT_TRACE, XRIT_NO_SERIAL_WALK (read in init)
    // a hand-off still open after rescue_after passes is walked serially between its first and last open boundary
    // (costas_serial_states_kernel), if that is at most rescue_max_samples samples
    int rescue_after = 32;
    long long rescue_max_samples = 4 << 20;
    unsigned rescues = 0;             // calls of this handle that took the serial walk
    bool walked = false;              // ... the last call did
    int serial_rescue(hipStream_t s, Profiler *prof);
    unsigned *h_counters = nullptr;   // pinned
    int cur = 0;
    int passes = 0;
    unsigned unconverged = 0;
    float max_residual = 0;
    int init(float loop_bw, int chain_len, int max_passes);
    int reset(hipStream_t s);
    void release();
    // sub_ext (optional): sum z^2 per run of 8 samples already left by the producer (FIR epilogue); om (optional): receives
    // the clock recovery's timing-line statistic per chain (index offset om_off in that stage's input buffer)
    int run(const float2 *in, float2 *out, size_t n, hipStream_t s, Profiler *prof, const float2 *sub_ext = nullptr,
            double2 *om = nullptr, long long om_off = 0, double inv_sps = 0.0);
    // the same in two halves: begin() only enqueues (guess, a batch of passes with a device-side stop test, final
    // pass); finish() runs after the caller synchronised the stream and continues the passes if they did not close
    int begin(const float2 *in, float2 *out, size_t n, hipStream_t s, Profiler *prof, const float2 *sub_ext,
              double2 *om, long long om_off, double inv_sps, bool use_exact = false);
    bool closed() const;
    int finish(hipStream_t s, Profiler *prof, bool *redone);
    int enqueue_passes(int count, hipStream_t s, Profiler *prof);
    int enqueue_final(hipStream_t s, Profiler *prof);
    struct Job {
        const float2 *in = nullptr; float2 *out = nullptr; size_t n = 0; int K = 0; int enqueued = 0;
        double2 *om = nullptr; long long om_off = 0; double inv_sps = 0;
        bool gated = false;     // this call has gone over to the gated solve
        bool rescued = false;   // the serial walk has been tried
        bool exact = false;     // this call's output is put on the serial trajectory (costas_exact.hip)
        float model_accept = 0; // CostasPolicy::model_accept of this call: the stage's on a tracking loop, else 0
    } job;
    int batch = 4;          // passes enqueued before the host looks: what the previous call needed + a spare one
    int stable = 0, last_passes = -1;   // calls in a row that closed inside their batch with the same count
                            // (2 on a locked signal); every surplus pass is ~4 no-op launches of ~5 us
    int get_state(float *phase, float *freq, hipStream_t s);
    // cfg.front_exact = 2 (costas_exact.hip): behind the final pass the output is put ON the serial float32 trajectory by
    // exactly walked, overlapping ranges; finish() closes what joints are still open
    bool exact = false;
    int ex_mode = 3;                // bit 0: the three-instruction systolic round where neither wrap nor limiter acts; bit 1: the
                                    // lattice scan in front of it (XRIT_CX_MODE: A/B runs)
    int ex_hist = -1;               // >= 0: samples of warm-up in front of every range whatever the call (XRIT_CX_HIST); -1: by plan
    int ex_prio = 1;                // the walkers' waves at a raised issue priority (XRIT_CX_PRIO=0: off)
    int ex_walkers = 2048;          // ranges per large call: two walkers per SIMD (set from the device's CU count in init; one wave
                                    // issues a dependent instruction every ~7 cycles, two share a SIMD's port almost for free)
    DevBuf xj, xbs, xcnt;           // joints (start / end / used), block records, counters
    unsigned *h_xcnt = nullptr;     // pinned: [0] joints open, [1] blocks, [2] Picard rounds, [3] blocks that hit the round limit
    int ex_W = 0, ex_rounds = 0;
    bool ex_args_valid = false;
    unsigned ex_open = 0, ex_nonconverged = 0;
    unsigned long long ex_blocks = 0, ex_picard = 0, ex_segs = 0, ex_fallbacks = 0;    // totals over the handle's calls (statistics)
    int exact_plan(size_t n, int *Lw, int *W, int *H) const;
    int enqueue_exact(hipStream_t s, Profiler *prof);
    int finish_exact(hipStream_t s, Profiler *prof, bool *redone);
    int flip_phase(hipStream_t s);      // the carried phase moves by pi: the other of the loop's two locks
};

// the exact Costas loop's sincosf (exact_sincos.h) on an array: what tests/test_gpu_exact.py holds against the oracle's
int launch_loop_sincosf(const float *d_x, float *d_sin, float *d_cos, size_t n, hipStream_t s);

// ---- ClockRecovery (demodulator.cpp:449; Work at :156) --------------------
struct ClockResult;
// What a call does is decided by the plain host functions of clock_plan.h from the knobs (ClockKnobs, the base: the chain
// sets them as members of the stage); the stage reserves and launches by the plan.
struct ClockStage : ClockKnobs {
    // ---- knobs the plans do not read
    float mu0 = 0.5f;
    int jac_passes = 1;     // passes that recompute the chain Jacobians (then quasi-Newton; measured: no gain from more)
    float tol_t = 2e-6f, tol_w = 2e-7f;
    bool force_gated = false;         // always the three-launch solve with the trust gate (XRIT_GATED_SOLVE=1: A/B runs)
    bool relay_no_rec = false;  // XRIT_RELAY_NO_REC: walkers always guess from the nominal rate (A/B runs)
    bool relay_no_claim = false;  // XRIT_RELAY_NO_CLAIM: the walker is always wave 0 of its workgroup, wherever the hardware put it (A/B runs)
    bool relay_rec01 = true;           // a plan from the timing guess records its first pass and guesses from that in its second (XRIT_RELAY_REC01=0: not; A/B runs)
    bool trace_env = false;     // XRIT_TRACE=1 (read at init): per-pass statistics on stderr
    bool no_meanj = false;      // XRIT_NO_MEANJ=1: finite-difference Jacobians in every call
    std::function<int(int)> before_relay;   // called by begin() in front of the relay kernels of a call that plans them (the chain
                                         // starts the front end of the next burst there: xrit_demod_prefetch_device)
    // What the loop carries from one call to the next as ONE device record (one capture across GPUs, csrc/group.hip: the rank
    // in front hands it on, so that the stream has one loop state across all slices as the reference has across all chunks,
    // demodulator.cpp:446-450): [valid, carry, -, -], the ClockState, then the unread tail (1024 samples, zero padded).
    static constexpr size_t CARRY_HEAD = 64, CARRY_BYTES = 64 + 1024 * sizeof(float2);
    // The new samples (the Costas loop's output rows of 128 bytes) start at a fixed place, xpad samples into the buffer, on a
    // 128-byte boundary -- wherever the producer writes them it does not need to know how many samples the call before left
    // unread --; those `carry` samples (at most 1024) are copied in right in front of them when the call begins.  Round 5: the
    // pad also holds the HISTORY the overlapping walkers of clock_overlap.h warm up over (the last samples of the burst before).
    size_t xpad = 1024;
    int ov_pad_need = 0;        // history samples a warm walker 0 needs in front of the new samples

    // ---- what the stream taught
    int batch = 7;          // passes enqueued before the host looks: what the previous call needed + a spare one
    int last_passes = -1;
                            // (5-6 in steady state)
    int relay_batch = 96;       // relay passes enqueued before the host looks
    bool jmean_valid = false;         // jmean holds the mean chain Jacobian of an earlier, locked call with ...
    int jmean_ns = 0;                 // ... this chain length

    // ---- the stream between calls, the sample buffers and the overlap jobs: clock_jobs.h
    ClockJobs jobs;

    // ---- the call in flight
    struct Job : ClockChainPlan {
        size_t n = 0, cap = 0; float *soft = nullptr; float2 *sym = nullptr;
        float2 *base = nullptr;     // where [carry | new] lie when that is not the call's own buffer (a call run again, a fall-back)
        int exact = 0;              // cfg.clock_exact as this call takes it (the overlap plan's fall-back: 1 or 0)
        int enqueued = 0;
        bool mean_j = false;    // the passes use the stream's mean Jacobian: no finite-difference pass
        bool gated = false;     // this call has gone over to the gated solve
        int *dirty = nullptr, *counts = nullptr, *nrun = nullptr, *terminal = nullptr, *written = nullptr;
        int G = 0, cps = 0, relay_enq = 0;      // exact closure: segments, chains per segment, passes enqueued
        int relay_w = 0;                        // waves per walker team (clock_relay_wide.h); 0: the one-wave walker
        bool relay_force = false;               // the relay is on although the tiled hand-off never closed (pass budget used up)
    } job;
    // ---- overlapping exactly walked blocks (clock_overlap.h, round 5): the default configuration's plan for calls of ov_min
    // symbols or more.  A job is one such call; up to three exist at a time (xrit_demod_prefetch_device: the walkers of bursts
    // b and b + 1 at work, burst b + 2's samples being written), each with its own sample buffer (xbuf[job]) and timing curve.
    // (the plain part of job q: jobs.job[q])
    struct OvJob {
        DevBuf om, om_work, segs, S, stage, aux;
        hipEvent_t ev_walk = nullptr;   // the walkers have finished
        hipEvent_t ev_guess = nullptr;  // the history has been copied in and the start states computed
    } ov[NXB];
    float *ov_soft = nullptr; size_t ov_cap = 0;

    // ---- results of the last call
    int passes = 0;
    unsigned unconverged = 0;   // boundaries the last solve still moved (~all of them on any healthy call: the floor)
    unsigned large_open = 0;    // boundaries left with a residual beyond 0.02 sample or an open symbol slip
    float max_residual = 0;
    size_t last_symbols = 0;
    float snr_estimate = 0.f;   // (of the last call that looked)
    bool relay_auto = false;    // the last call was relayed on the host's own decision (clock_relay_look, the stall rule)
    int relay_passes = 0;       // relay passes the last call ran (the closing, change-free one included)
    bool relay_closed = false;  // ... and whether they reproduced the serial trajectory
    int relay_segments = 0, relay_seg_chains = 0;
    bool ov_fell_back = false;  // the last call's overlap result was not taken (low Es/N0, a joint that did not fit): relayed to closure
    int ov_walkers = 0;         // walkers of the last overlap call
    float ov_joint_max = 0.f;   // ... and the largest distance between two trajectories at a joint (samples)

    // ---- buffers
    DevBuf table;           // 129 x 8 MMSE taps
    DevBuf xbuf[NXB];       // [pad | carry | new] input samples of a call.  Three of them (round 5): the producer of the samples of
                            // the call after next (the Costas loop of burst b + 2: xrit_demod_prefetch_device) fills one while the
                            // walkers of bursts b and b + 1 read the other two (round 4: two, one burst ahead)
    DevBuf st;              // carried ClockState + carry count
    DevBuf S, E, J, om, work, counters, sym, dlin, flags, wsolve, jmean;
    DevBuf om_work;
    DevBuf tail;                      // 2 x 1024 samples left unread by a call (ping-pong with the state)
    void *h_res = nullptr;            // pinned copy of the control block + result
    DevBuf relay;               // segment records + per-pass counters
    DevBuf relay_rec;           // per symbol: read index and interpolator arm of the last exact walk (the next walk's first guess)
    DevBuf stage;               // soft symbols of a writing hand-off pass, in wave order (ClockPassOut::stage)
    DevBuf alt;                             // ClockState + 1024 samples of unread tail, twice (the second: scratch)
    DevBuf ov_claim;            // which SIMDs hold a walker (clock_relay.h), shared by the jobs in flight
    float2 *xdata() const { return xbuf[jobs.xb].as<float2>() + xpad; }
    float2 *xbase() const { return job.base ? job.base : xdata() - jobs.carry; }

    int init(float omega, float gain_omega, float mu, float gain_mu, float omega_rel_limit, int chain_syms,
             int max_passes);
    int reset(hipStream_t s);
    void release();
    // where the producer must write the n new samples of this call
    int input_slot(size_t n, float2 **slot, hipStream_t s);
    double2 *om_slot(int nb, int BL);
    int om_scan(hipStream_t s);
    // soft (real parts) and/or complex symbols; either may be null
    int run(size_t n, float *soft_out, float2 *sym_out, size_t cap, size_t *n_out, hipStream_t s, Profiler *prof);
    // The last call once more on its sign-flipped input (one capture across GPUs: this rank's Costas loop turned out
    // to sit pi away from the stream's, csrc/group.hip): the carried state goes back to what it was before the
    // call, its history and unread tail change sign, the call's input is negated in place, the recovery runs again.
    int redo_flipped(float *soft_out, float2 *sym_out, size_t cap, size_t *n_out, hipStream_t s, Profiler *prof);
    // which = 0: what the NEXT call starts from; 1: what the last call started from (untouched since, as redo_flipped relies on)
    int export_carry(void *d_rec, int which, hipStream_t s);
    // The last call once more from the record of another handle (`carry_rec` samples of unread tail in it, read by the caller):
    // the same input, the given loop state in front of it.
    int redo_from(const void *d_rec, size_t carry_rec, float *soft_out, float2 *sym_out, size_t cap, size_t *n_out, hipStream_t s, Profiler *prof);
    // the last call's symbols are those of ONE float32 walk from its start state (cfg.clock_serial, the exact closure, or a call
    // short enough for a single exact walk): what a hand-over of the exact start state turns into the stream's own words
    bool last_walk_exact() const;
    int make_alt(hipStream_t s, Profiler *prof);
    // the same in two halves (see CostasStage): begin() only enqueues, finish() runs after a stream synchronise
    int begin(size_t n, float *soft_out, float2 *sym_out, size_t cap, hipStream_t s, Profiler *prof);
    bool closed() const;
    int finish(size_t *n_out, hipStream_t s, Profiler *prof);
    bool ov_eligible(size_t n) const { return clock_ov_eligible(*this, xpad, false, n); }
    // the walkers of the call whose samples have been produced into the slot input_slot() handed out (and whose timing curve
    // has been scanned): pad copy, start states, walkers, on `sw` -- ahead of the call itself (ahead: the call in front has not
    // finished) or from begin()
    int ov_launch(int job, hipStream_t sw, bool ahead, Profiler *prof);
    // a job whose walkers were started ahead on samples that have since been rewritten (the Costas loop went on from the host):
    // waits for them (the host synchronises the event) and takes the job back to "samples produced"
    int ov_restart(int job);

    // ---- the parts of begin() / finish() (clock.hip)
    // the chains on samples at `base` (null: the call's own buffer), with `exact_` for cfg.clock_exact
    int run_chains(float2 *base, int exact_, size_t n, float *soft_out, float2 *sym_out, size_t cap, size_t *n_out, hipStream_t s, Profiler *prof);
    int begin_chains(float2 *base, int exact_, size_t n, float *soft_out, float2 *sym_out, size_t cap, hipStream_t s, Profiler *prof);
    int begin_short(hipStream_t s);
    int begin_serial(hipStream_t s, Profiler *prof);
    void call_reset(size_t n);
    ClockKnobs call_knobs() const { ClockKnobs k = *this; k.exact = job.exact; return k; }     // the knobs as the call in flight takes them
    int begin_overlap(size_t n, float *soft_out, size_t cap, hipStream_t s, Profiler *prof);
    int launch_chains(bool ext, bool scanned, hipStream_t s, Profiler *prof);
    int finish_overlap(size_t *n_out, hipStream_t s, Profiler *prof);
    int finish_chains(size_t *n_out, hipStream_t s, Profiler *prof);
    int finish_handoff(hipStream_t s, Profiler *prof);
    int finish_relay(hipStream_t s, Profiler *prof);
    int enqueue_passes(int count, hipStream_t s, Profiler *prof);
    int enqueue_output(hipStream_t s, Profiler *prof, bool again = false);
    int enqueue_relay(int count, bool restart, hipStream_t s, Profiler *prof);
    int relay_w_plan() const;
    int relay_cut();
    int ov_finalize(int job, float *soft_out, size_t cap, hipStream_t s, Profiler *prof);
    int ov_fallback(size_t *n_out, hipStream_t s, Profiler *prof, bool to_closure);
    int trace_overlap(int job, const struct ClockResult &r) const;
    int trace_relay() const;
    int trace_passes() const;
};

// ---- helpers ---------------------------------------------------------------
int launch_sync_correlate(const int8_t *data, size_t n, const unsigned long long *words, int nwords, unsigned frame,
                          xrit_sync_hit *hits, hipStream_t s);
int launch_sync_fix(const int8_t *data, size_t n, const xrit_sync_hit *hits, unsigned frame, unsigned min_corr,
                    int8_t *frames, unsigned char *valid, hipStream_t s);
int launch_quantize_i8(const float *in, int8_t *out, size_t n, hipStream_t s);
// ---- the back end (decoder, demux, packets, files, rice) --------------------
// frame geometry: soft symbols of a frame; bytes of a CADU, of the block behind its sync marker, of a VCDU (the block
// without the RS parity) and of a VCDU's packet zone
constexpr int FRAME_SYMBOLS = 16384, CADU_BYTES = 1024, BLOCK_BYTES = 1020, VCDU_BYTES = 892, ZONE_BYTES = 884;
constexpr int NVC = 64;                                 // virtual channels
constexpr size_t MAX_ROWS_PER_CALL = (size_t)1 << 24;   // frames, rows or lines one call takes at most
// Hands out consecutive pieces of one scratch allocation; with p = nullptr it only counts the bytes.
struct Carver {
    char *p;
    size_t n = 0;
    template <class T> T *take(size_t count, size_t align)
    {
        T *r = p ? reinterpret_cast<T *>(p + n) : nullptr;
        n += (count * sizeof(T) + align - 1) & ~(align - 1);
        return r;
    }
    size_t used() const { return n; }
};
// decoder (viterbi.hip, rs.hip): decision words of one resident window; Viterbi + carry, then derandomiser + RS
size_t viterbi_slot_bytes();
int launch_viterbi(const int8_t *frames, const unsigned char *valid, size_t nf, int hrit, int8_t *carry, int *prev, int *last,
                   unsigned long long *dec, unsigned slots, unsigned char *cadu, unsigned *verr, hipStream_t s);
int launch_rs(const unsigned char *cadu, const unsigned char *valid, const unsigned *verr, size_t nf, unsigned char *block,
              xrit_frame_info *info, hipStream_t s);
// demux (demux.hip): one tile of DEMUX_TILE frames per workgroup; the handle's state and the per-call scratch
constexpr int DEMUX_TILE = 1024;
struct DemuxState {                       // newdecoder.cpp:44-53, 133-137 (entries 64..255 are never touched)
    long long last[NVC], received[NVC], lost[NVC];
    unsigned long long frames, dropped, sum_vit, sum_rs, lost_total;
};
struct DemuxScratch {
    unsigned *cnt; int *firstc, *lastc; unsigned *tsum;     // (a): [T][64] x 3, [T][4]
    unsigned *base; int *P; unsigned long long *tin;         // (b): [T][64] x 2, [T][5]
    long long *vcb;                                          // (b): [2][64]
};
size_t demux_scratch_carve(void *p, size_t nf, DemuxScratch &sc);     // returns the bytes; p = nullptr: only that
int launch_demux(const xrit_sync_hit *hits, const unsigned char *cadu, size_t cadu_stride, const unsigned char *block,
                 const xrit_frame_info *info, size_t nf, DemuxState *state, DemuxScratch &sc, unsigned char *vcdu,
                 unsigned *offsets, xrit_frame_stats *records, hipStream_t s);
// stream frame synchroniser and frame lock (framer.hip, lock.hip).  A call's view V is carry ++ new symbols (FramerPar,
// framer_host.h).  The synchroniser's call is bits / maxima, walkers, joints, gather; the lock's is bits / maxima and
// walkers once and then rounds of joints, gather, decoder and commit, where a round ends at a chunk whose hit needs
// the RS outcome of a row that the round itself emitted.
struct FramerCall {                         // what the joints leave for the gather of the same call
    unsigned long long base;                // absolute offset of V[0]
    unsigned carry, total, cursor, count;   // bytes of carry in V, bytes of V, the cursor after the call, rows emitted
};
struct FramerScratch {
    unsigned *bits;                 // hard bits of V, 32 per word, MSB = first byte
    unsigned *bmax;                 // per run of 64 positions: the best (count << 6 | 63 - offset) of word 0 | of word 1 << 16
    uint4 *rec;                     // [segs][S] a walker's steps: (cursor, word | short hit at position 0 << 1 | short word << 2 |
                                    // short count << 8, position, correlation)
    unsigned *nrec;                 // [segs] steps recorded
    uint2 *wout;                    // [segs] (the cursor the walker left with, 1: it stopped for want of symbols)
    uint4 *rows;                    // [cap] the call's rows: (cursor, word, position, correlation) of the hit that was used
    unsigned char *flags;           // [cap] per row: full position != 0 | short position == 0 << 1 | short hit used << 2
    FramerCall *call;
};
struct LockPar {
    unsigned recheck;                       // flywheelRecheck, 1 .. 255; 1: no flywheel, the synchroniser's walk
    unsigned span;                          // the short range: frame / 16 symbols (the synchroniser has none: 0)
    unsigned first;                         // 1: the call's first round (cursor 0, no rows yet)
    unsigned r0;                            // rows the call's earlier rounds emitted
    unsigned short0;                        // 1, only with recheck 1: no chunk was consumed since the reset (fc is 0), so the
                                            // chunk at cursor 0 may be counted sensitive; the walk records its short hit
};
size_t framer_scratch_carve(void *p, size_t n, unsigned frame, unsigned seg_chunks, FramerScratch &sc);
// framer.hip: the hard bits and per-64 maxima of V; the frames, valid, hits and start of par.cap rows (of which
// call->count exist) and the next call's carry
int launch_framer_bits(const FramerPar &par, const FramerState *state, const int8_t *carry_in, const int8_t *symbols,
                       FramerScratch &sc, hipStream_t s);
int launch_framer_gather(const FramerPar &par, const FramerCall *call, const int8_t *carry_in, const int8_t *symbols,
                         const uint4 *rows, int8_t *carry_out, int8_t *frames, unsigned char *valid, xrit_sync_hit *hits,
                         unsigned long long *start, hipStream_t s);
// lock.hip: the chain -- the walk of both, the synchroniser's joints, the lock's joints and commit.  The synchroniser's
// state is a LockState too, of which its joints are given the FramerState in front
int launch_plain_joints(const FramerPar &par, FramerState *state, FramerScratch &sc, unsigned *count, hipStream_t s);
int launch_lock_walk(const FramerPar &par, const LockPar &lp, const LockState *state, FramerScratch &sc, hipStream_t s);
int launch_lock_joints(const FramerPar &par, const LockPar &lp, LockState *state, FramerScratch &sc, unsigned *count, hipStream_t s);
int launch_lock_commit(const FramerPar &par, const LockPar &lp, LockState *state, FramerScratch &sc, const xrit_frame_info *info,
                       unsigned char *mode, hipStream_t s);
// packet assembler (packets.hip): the handle's state, the per-call scratch (R = max(max_rows, 1) rows)
constexpr unsigned PACKETS_PEND_MAX = 65541;        // a pending packet is shorter than the longest packet (65542)
constexpr unsigned PACKETS_TILE = 1024;             // rows per tile of the scan
constexpr unsigned PACKETS_PEND_STRIDE = 65544;     // bytes of pending buffer per channel
struct PacketsState {
    unsigned long long packets[64], crc_failures[64], fill_packets[64], discarded[64], bad_fhp[64], rows[64];
    int last[64];                                   // the last row's counter, -1 at start
    unsigned pend_len[64], first_counter[64];       // the bytes held in the channel's pending buffer, where they began
};
struct PacketsScratch {
    unsigned *rowA;                 // [R] per row, by its own lane: packets inside | fill << 8 | bytes << 16 | discarded << 28 | bad << 29
    uint2 *spanB;                   // [R] per row, by the lane of the tail that ends here: (origin, length | fill << 31)
    uint2 *newp;                    // [64] per channel: (origin, bytes) of what is pending after the call
    unsigned *state_disc;           // [64] the pending state the call began with was discarded
    unsigned *plocal, *blocal;      // [R] descriptor index and byte offset of the row's first packet inside its tile
    uint2 *tsum;                    // [T] packets and bytes of a tile of PACKETS_TILE rows
    unsigned *tbase_c;              // [T] descriptor index of the tile's first packet
    unsigned long long *tbase_b;    // [T] ... and its byte offset
    unsigned *crcfail;              // [R] emitted packets of the row whose CRC does not match
};
size_t packets_scratch_carve(void *p, size_t max_rows, PacketsScratch &sc);
int launch_packets(const unsigned char *vcdu, const unsigned *offsets, size_t max_rows, PacketsState *state,
                   unsigned char *pend, PacketsScratch &sc, unsigned char *bytes, size_t max_bytes, xrit_packet *packets,
                   size_t max_packets, unsigned *pkt_offsets, xrit_packets_summary *summary, hipStream_t s);
// file assembler (files.hip): the handle's state is FILES_KEYS xrit_file_key records and one xrit_files_counters
constexpr unsigned FILES_KEYS = 64 * 2048;          // (vcid, apid), directly indexed
constexpr unsigned FILES_TILE = 2048;               // keys per tile of the scan
constexpr unsigned FILES_TSUM = 10;                 // words of a tile's sums: pieces, records, bytes, seven counter increments
struct FilesScratch {
    unsigned *order;                // [N] packet indices, per VCID stably sorted by APID
    unsigned *kstart, *kcount;      // [FILES_KEYS] a key's run in `order`
    unsigned *kpieces, *krecs;      // [FILES_KEYS] pieces and records the key's walk emits; after the scan: their exclusive prefix inside the tile
    unsigned long long *kbytes;     // [FILES_KEYS] ... and bytes
    unsigned long long *tsum, *tbase;   // [64][FILES_TSUM] a tile's sums; [64][3] its first piece index, record index, byte offset
    unsigned *kcnt;                 // [FILES_KEYS][7] the walk's counter increments: begun, completed, aborted, bad, gaps, short, orphans
    unsigned long long *psrc, *pdst;// [N] per piece: where its payload lies in the input, where it goes
    unsigned *plen;                 // [N]
};
size_t files_scratch_carve(void *p, size_t max_in, FilesScratch &sc);
int launch_files(const unsigned char *in_bytes, size_t n_in_bytes, const xrit_packet *packets, const unsigned *pkt_offsets,
                 size_t max_in, xrit_file_key *keys, xrit_files_counters *counters, FilesScratch &sc, unsigned char *bytes,
                 size_t max_bytes, xrit_file_piece *pieces, size_t max_pieces, xrit_file_record *files, size_t max_files,
                 xrit_files_summary *summary, hipStream_t s);
// Rice decoder (rice.hip)
constexpr int RICE_FORM_LANE = 1, RICE_FORM_WAVE = 2;
int launch_rice(const unsigned char *bytes, size_t n_bytes, const void *desc, size_t stride, size_t n_lines, int n, int J, int S,
                void *out, unsigned char *status, int form, hipStream_t s);
// image stage (images.hip): the handle's state is FILES_KEYS xrit_image_key records and one xrit_images_counters; the
// per-call scratch for R = max(max_files_in, 1) records and P = max(max_pieces_in, 1) pieces
constexpr unsigned IMAGES_TILE = 1024;              // records per tile of the scan
constexpr unsigned IMAGES_TSUM = 6;                 // words of a tile's sums: lines, bytes, images, begun, completed, aborted
struct ImageMark;                                   // image_rule.h
struct ImagesScratch {
    ImageMark *mark;                // [R] the rule's decision per record
    unsigned *rlines;               // [R] the record's lines; after the scan: their exclusive prefix inside the tile
    unsigned long long *rbytes;     // [R] ... and padded bytes
    unsigned *rfaults;              // [R] lines of the record with status != 0
    unsigned long long *tsum, *tbase;   // [T][IMAGES_TSUM] a tile's sums; [T][2] its first line index and byte offset
    unsigned long long *call;       // [IMAGES_TSUM] the call's sums
    unsigned char *lstatus;         // [P] per piece that is a line: its status
};
size_t images_scratch_carve(void *p, size_t max_files_in, size_t max_pieces_in, ImagesScratch &sc);
int launch_images(const unsigned char *bytes, size_t n_bytes, const xrit_file_piece *pieces, size_t max_pieces_in,
                  const xrit_file_record *files, size_t max_files_in, const xrit_files_summary *fsum, xrit_image_key *keys,
                  xrit_images_counters *counters, ImagesScratch &sc, unsigned char *out, size_t max_bytes, xrit_image_line *lines,
                  size_t max_lines, xrit_image_file *image_files, xrit_images_summary *summary, hipStream_t s);
// canvas stage (canvas.hip): the handle's state is 64 xrit_canvas_slot records, their 64 x 64 xrit_canvas_segment,
// FILES_KEYS xrit_canvas_key_state records, one xrit_canvas_counters and the pixels; the per-call scratch for
// R = max(max_files_in, 1) records
struct CanvasHead;                                  // canvas_rule.h
struct CanvasPlace;
struct CanvasBounds {                               // the host's bounds on what the two summaries may say
    unsigned long long n_bytes, max_pieces, max_files, n_image_bytes, max_lines;
};
struct CanvasState {
    xrit_canvas_slot *slots;
    xrit_canvas_segment *segs;
    xrit_canvas_key_state *keys;
    xrit_canvas_counters *counters;
    unsigned char *pixels;
    unsigned n_slots;
    size_t slot_bytes;
};
struct CanvasScratch {
    CanvasHead *heads;              // [R] what the header walk found
    CanvasPlace *place;             // [R] the rule's decision per record
    unsigned long long *call;       // the rule kernel's tallies of the call
};
size_t canvas_scratch_carve(void *p, size_t max_files_in, CanvasScratch &sc);
int launch_canvas(const unsigned char *bytes, const xrit_file_piece *pieces, const xrit_file_record *files, const xrit_files_summary *fsum,
                  const unsigned char *image_bytes, const xrit_image_line *lines, const xrit_image_file *image_files,
                  const xrit_images_summary *isum, const CanvasBounds &b, const CanvasState &st, CanvasScratch &sc,
                  xrit_canvas_file *canvas_files, xrit_canvas_slot *out_slots, xrit_canvas_summary *summary, hipStream_t s);
int launch_canvas_release(const CanvasState &st, unsigned slot, hipStream_t s);
// product stage (product.hip): the whole call -- hist (2^bits uint32) and over_count zeroed, histogram, tone table and
// summary, then the toned image and the thumbnail where asked for (NULL: not written).  hist, over_count and lut are the
// caller's or the handle's scratch, never NULL.
int launch_product(const xrit_product_image &im, const xrit_product_params &pp, const unsigned char *table_in, uint32_t *hist,
                   unsigned long long *over_count, unsigned char *lut, unsigned char *tone, unsigned char *small,
                   xrit_product_summary *summary, hipStream_t s);
int launch_product_composite(const unsigned char *a, uint32_t pitch_a, const unsigned char *b, uint32_t pitch_b, uint32_t columns,
                             uint32_t rows, const unsigned char *table, unsigned char *rgb, hipStream_t s);
// projection stage (geo.hip; geo_rule.h is the rule per pixel): the grid's tables in device memory (A, B: rows doubles;
// C, S: columns), then the three calls.  launch_geo_resample and launch_geo_project zero the summary first.
struct GeoTables {
    const double *A, *B, *C, *S;
    uint32_t columns, rows;
};
int launch_geo_map(const GeoTables &t, const xrit_geo_nav &nav, xrit_geo_point *map, hipStream_t s);
int launch_geo_resample(const GeoTables &t, const xrit_product_image &im, const xrit_geo_point *map, uint32_t mode, unsigned char *out,
                        uint32_t out_pitch, xrit_geo_summary *summary, hipStream_t s);
int launch_geo_project(const GeoTables &t, const xrit_geo_nav &nav, const xrit_product_image &im, uint32_t mode, unsigned char *out,
                       uint32_t out_pitch, xrit_geo_summary *summary, hipStream_t s);
// map overlay stage (overlay.hip; overlay_rule.h is the rule per value): the vertex map, the draw of n vertices into a
// mask in either form (form 1 needs the scratch for that many), the blend.  launch_overlay_draw zeroes the summary (and
// with clear the mask) first, launch_overlay_blend its summary.
struct OverlayDraw {
    const xrit_geo_point *points;
    uint32_t n, layer, width, max_jump;
    unsigned char *mask;
    uint32_t columns, rows, pitch;
};
struct OverlayScratch {
    unsigned long long *prefix;             // [n] a pair's steps, then the steps in front of it; the last element: all of them
    unsigned long long *aggs;               // the scan's aggregates
};
size_t overlay_scratch_carve(void *p, size_t n, OverlayScratch &sc);
struct OverlayBlend {
    const unsigned char *pixels, *mask;
    unsigned char *out;
    uint32_t columns, rows, pitch, mask_pitch, out_pitch, cin, cout;
    uint32_t styles[8];                     // r | g << 8 | b << 16 | alpha << 24
};
int launch_overlay_map(const xrit_geo_nav &nav, const double *quads, size_t n, xrit_geo_point *points, hipStream_t s);
int launch_overlay_draw(const OverlayDraw &d, uint32_t form, uint32_t clear, const OverlayScratch &sc, xrit_overlay_draw_summary *summary,
                        hipStream_t s);
int launch_overlay_blend(const OverlayBlend &b, xrit_overlay_blend_summary *summary, hipStream_t s);
// JPEG stage (jpeg.hip; jpeg_rule.h is the rule per value): one call on blocks = MCUs * comps blocks in n_int restart
// intervals of ri MCUs (restart 0: one interval of all MCUs); the scratch for that many
struct JpegPar {
    const unsigned char *pix;
    uint32_t columns, rows, pitch, comps;
    uint32_t bw, mcus, blocks;              // MCUs per row, MCUs, blocks
    uint32_t ri, n_int;
    unsigned char q[2][64];                 // the quantisation tables, natural order
};
struct JpegHeader {                         // SOI .. SOS, handed to the emit kernel by value
    uint32_t n;
    unsigned char b[640];
};
struct JpegScratch {
    unsigned long long *P, *P_aggs;         // [blocks + 1] the bits in front of a block; its scan's aggregates
    uint32_t *raw;                          // the unstuffed stream, every interval from a byte boundary, as whole groups of 16 bytes
    int16_t *coef;                          // [blocks][64] quantised coefficients, zigzag order
    uint32_t *blen;                         // [blocks] a block's code length in bits
    uint32_t *U, *U_aggs;                   // [n_int + 1] the unstuffed bytes in front of an interval
    uint32_t *F, *F_aggs;                   // [groups + 1] the 0xFF bytes in front of a group of 16 unstuffed bytes
};
size_t jpeg_scratch_carve(void *p, uint32_t blocks, uint32_t n_int, JpegScratch &sc);
int launch_jpeg(const JpegPar &p, const JpegHeader &h, const JpegScratch &sc, unsigned char *out, size_t cap, xrit_jpeg_result *result,
                hipStream_t s);
// JPEG decoder stage (jpegdec.hip; jpegdec_rule.h is the rule per value): one call on n_items streams in `bytes`; the scratch
// for that many items, max_scan bytes of entropy-coded data and max_blocks blocks
struct JpegDecPar {
    const unsigned char *bytes;
    unsigned long long n_bytes;
    const unsigned char *items;             // {uint64 offset; uint32 length} every `stride` bytes
    unsigned long long stride;
    uint32_t n_items, max_blocks, max_scan;
    uint32_t form, S;                       // 0: a lane per restart interval; 1: a wave per interval, subsequences of S bits
    unsigned char *pixels;
    unsigned long long cap;
    xrit_jpegdec_record *records;
    xrit_jpegdec_summary *summary;
};
struct JpegDecItem;
struct JpegDecHuff;
struct JpegDecSum;
struct JpegDecScratch {
    JpegDecItem *item;                      // [n_items] what the header kernel found, the final status
    uint32_t *bbase, *mbase, *ibase, *sbase;        // [n_items + 1] blocks, MCUs, intervals (one more each), scan bytes in front of an item
    uint32_t *kbase, *rbase;                // [n_items + 1] unstuffed bytes, RSTm markers in front of an item
    unsigned long long *obase;              // [n_items + 1] pixel bytes in front of an item
    unsigned long long *tot;                // [8] those sums over the items the call takes
    JpegDecSum *item_aggs;
    JpegDecHuff *huff;                      // [n_items][6] per component its DC and AC table
    unsigned char *q;                       // [n_items][3][64] per component its quantiser table, natural order
    unsigned char *un;                      // [max_scan] the unstuffed scan bytes of all items
    uint32_t *rst_pos;                      // [max_scan / 2 + 1] per RSTm the unstuffed bytes in front of it
    unsigned char *rst_m;                   // its m
    unsigned long long *un_aggs;
    int16_t *coef;                          // [max_blocks][64] zigzag order
    uint32_t *ifault;                       // [max_blocks + n_items] per interval its fault
    uint4 *dc_aggs;
    uint32_t *rounds;                       // the most rounds a tile of form 1 took
};
size_t jpegdec_scratch_carve(void *p, uint32_t n_items, uint32_t max_scan, uint32_t max_blocks, JpegDecScratch &sc);
int launch_jpegdec(const JpegDecPar &p, const JpegDecScratch &sc, hipStream_t s);
// carrier acquisition (acquire.hip; acquire_host.h has the sizes): the handle's state is one xrit_acquire_state; the scratch
// of an estimate of M segments
struct AcquireScratch {
    float2 *spectra;                // [M][4096] every segment's spectrum, in bin order
    double *power;                  // [4096] their powers summed
};
size_t acquire_scratch_carve(void *p, unsigned segments, AcquireScratch &sc);
// the mix of n samples with the state's acc and inc, then acc += n * inc (n = 0: that alone)
int launch_acquire_mix(const void *in, int type, size_t n, float2 *out, xrit_acquire_state *st, hipStream_t s);
int launch_acquire_set_inc(xrit_acquire_state *st, long long inc, hipStream_t s);
// segments = acquire_segments(n, ...): below 31 only the record (TOO_SHORT) is written; tw, win: the tables of acquire.cpp
int launch_acquire_estimate(const void *in, int type, unsigned segments, const xrit_acquire_params &par, const float2 *tw, const float *win,
                            const AcquireScratch &sc, int apply, xrit_acquire_state *st, xrit_acquire_estimate_record *rec, hipStream_t s);
// link monitor (monitor.hip; monitor_host.h has the plan of a push): the reduce kernel over the plan's pieces (none when
// n = 0), then the commit kernel.  parts: two scratch records (piece 0 and the tail); rows takes plan.rows records.
struct MonitorPlan;
int launch_monitor_push(const void *in, int type, const MonitorPlan &plan, xrit_monitor_block *parts, xrit_monitor_state *st,
                        xrit_monitor_block *rows, xrit_monitor_summary *summary, hipStream_t s);
int launch_convert(const void *in, int type, float2 *out, size_t n, hipStream_t s);
int launch_synth(const xrit_synth_params &p, uint64_t start, size_t n, float2 *out, hipStream_t s);
int launch_read_bw(const void *buf, size_t bytes, int reps, hipStream_t s, double *gbs);

}  // namespace xrit
