// clock_jobs.h -- the clock stage's bookkeeping between calls, as plain C++ (no HIP headers): which of the three sample buffers
// a producer gets, which overlap job a call belongs to, which job is in front of which, where the history lies that the next
// job's first walkers warm up over and when it stops being valid, and the ping-pong of the carried state.  Records and pure
// functions: no allocation, no launch.  clock.hip (ClockStage) asks, performs the HIP step and writes the outcome back;
// chain_host_check.cpp runs the same records under the pipeline's scripts (make chain-host-check).
//
// ---- what a launch reads or writes, who wrote it, and what orders the reader behind the writer
// (s: the call's stream; sw: the walkers' stream of a job -- s when begin() launches them, one of the chain's two walker
// streams when they are launched ahead; producer: whoever fills the slot input_slot() handed out, the chain's Costas loop)
//
//   resource                     written by, on                               read by, on                        ordered by
//   new samples xbuf[b][xpad..]  the producer, its own stream                 job b's guess / walkers, sw        the caller (the chain: ev_costas)
//                                                                             the job behind's pad copy, its sw  ev_guess of job b (recorded on b's sw)
//                                                                             ov_finalize's joints, s            ev_walk of job b
//                                                                             begin_chains' kernels, s           the caller (the chain: stream order / ev_fe)
//                                (overwritten by the next producer of b)                                         job b FREE (host: the call's end); ev_guess of
//                                                                                                                every job with hist_src == b (input_slot)
//   pad xbuf[b][xpad-padN..]     ov_launch: the history copy or the carried   job b's guess / walkers, sw        stream order
//                                tail, sw                                     ov_finalize's joints, s            ev_walk
//                                begin_chains: the carried tail, s            the chains, s                      stream order
//   job b's statistic            the producer (om_slot), its stream; else     job b's curve and guess, sw        the caller (ev_costas) / stream order
//                                clock_om_kernel, sw
//   job b's count curve          clock_unwrap in ov_launch, sw                job b's guess, sw                  stream order
//                                                                             the job behind's guess, its sw     ev_guess of job b
//   st[cur], tail[cur]           the end of the call before (joints, output   ov_launch not ahead (walker 0      host: finish() of the call before ran after a
//                                pass or relay finalize), that call's s       from the carried state), s         synchronise / a completed query of its stream;
//                                                                             ov_finalize, begin_chains, s       one caller, one s
//   st[cur^1], tail[cur^1]       this call's joints / output, s               the next call (as st[cur])         as above; redo_*: flipped back by the host
//   ov_claim                     the walkers of every job in flight (atomics) the same                           none needed: claims are atomic; reset() clears it
//                                reset(), s                                                                      on s after the caller has synchronised its streams
//   S, segs, stage, aux of b     job b's guess (S, aux) and walkers, sw       ov_finalize's joints / copy, s     ev_walk of job b
//                                (overwritten by the next job in slot b)                                         job b FREE: the host saw the call's end on s,
//                                                                                                                which was behind ev_walk
#pragma once

#include <stddef.h>
#include <stdio.h>

#include "clock_plan.h"

#ifndef XRIT_AHEAD
#define XRIT_AHEAD 2            // inputs that may wait behind the call in progress (bursts that walk overlapping blocks)
#endif

namespace xrit {

constexpr int NXB = XRIT_AHEAD + 1;     // sample buffers of a clock stage, and overlap jobs: job q's samples lie in buffer q

enum ClockJobState {
    CLK_JOB_FREE,           // 0
    CLK_JOB_SLOT,           // 1: slot handed out (samples being produced)
    CLK_JOB_WALKING,        // 2: walkers enqueued
    CLK_JOB_FINALIZING      // 3: the call's joints and output enqueued
};

// One call that walks overlapping blocks (clock_overlap.h); up to three exist at a time (xrit_demod_prefetch_device: the
// walkers of bursts b and b + 1 at work, burst b + 2's samples being written).  The plain part: ClockStage::OvJob holds the
// device buffers and events that go with it.
struct ClockJob : ClockOvPlan {
    ClockJobState state = CLK_JOB_FREE;
    size_t n = 0;                   // new samples
    bool ahead = false;             // enqueued before the call in front of it had finished (its carry is not known to the plan)
    int nb = 0, BL = 256;           // the timing statistic: nb blocks of BL samples, counted from the first new sample
    bool om_ext = false, om_scanned = false;
    int hist_src = -1;              // the buffer whose last samples this job's first walkers warm up over (-1: none)
    unsigned long long serial = 0;  // order of the calls (the job in front: serial - 1)
};

// what the last finished call left in its buffer: the history the next call's first walkers warm up over
struct ClockHistory {
    int xb = -1;            // buffer
    size_t len = 0;         // samples in it that end where the stream stands ([pad | new] of that call, contiguous)
    int job = -1;           // ... and, when that call was an overlap job, the job whose timing curve covers them
    void forget() { *this = ClockHistory{}; }
};

struct ClockSlotPick {
    int b = -1;                     // the buffer (-1: refused, err)
    bool wait_guess[NXB] = {};      // jobs whose ev_guess the producer's stream goes behind: they read what the buffer holds
    bool forget = false;            // the buffer holds the history: it is forgotten
    char err[96] = {0};
};
struct ClockLaunchHist {
    int xb = -1, job = -1; size_t len = 0;  // where the history lies, how long, whose timing curve covers it
    int wait_guess = -1;                    // ahead: the job in front, whose ev_guess the walkers' stream goes behind
    bool have = false;                      // what clock_ov_plan is told
    const char *err = nullptr;
};
struct ClockOm { bool ext, scanned; };

struct ClockJobs {
    ClockJob job[NXB];
    int setting_up = -1;            // the job of the call being set up (-1: the call is not such a call)
    int ov_cur = -1;                // the overlap job of the call between begin() and finish()
    unsigned long long serials = 0; // jobs handed out so far
    int xb = 0;                     // the buffer the call in flight (the last call) reads
    int x_pending = -1;             // the buffer handed out for the next call
    bool in_flight = false;         // between begin() and finish()
    ClockHistory hist;
    // the stage's own statistic (a producer's for a call that is no overlap job): nb blocks of BL samples; its count curve.
    // (the statistic's phasor counts samples from the first NEW sample of the call: the call turns it by the carried ones)
    // (round 4: the producer's stream also unwraps it into the symbol-count curve, om_scan(): two launches less between the end
    // of one burst's relay and the start of the next one's)
    bool om_ext = false, om_scanned = false;
    int om_nb = 0, om_BL = 256;
    // the carried state: st[cur] / tail[cur] is what the next call starts from, the other half what the last one started from
    int cur = 0;
    size_t carry = 0;                       // samples held over from the previous call
    size_t prev_carry = 0, prev_n = 0;      // of the last call
    bool redo_ok = false;                   // ... which ended normally (its input is still in its buffer)
    // What the recovery would carry had it run on the sign-flipped stream so far (ClockStage::make_alt: the last call -- the
    // halo of a time slice, from a cold start -- is run again on its negated input and the outcome kept aside); a later
    // redo_flipped() starts from it instead of from the other sign's state with its history negated, whose timing sits 1e-3
    // sample off the flipped loop's and takes 1e4..1e5 symbols to come home on the lattice.
    size_t alt_carry = 0;
    bool alt_valid = false;
    char err[128] = {0};

    // ---- reset: the stream starts again (the caller has waited for whatever walked ahead).  The serials go on counting and
    // xb stays: the walkers' streams and the buffers keep alternating from where they are.
    void reset()
    {
        cur = 0;
        carry = 0;
        x_pending = -1;         // (samples a producer has put in place for a call that will not come)
        for (auto &j : job) j.state = CLK_JOB_FREE;
        setting_up = -1;
        hist.forget();
        om_ext = false;         // (... and its timing statistic and count curve)
        om_scanned = false;
        in_flight = false;
        prev_carry = 0;
        prev_n = 0;
        redo_ok = false;        // (nothing of an earlier call is left to run again, nor a flipped loop's state to start it from)
        alt_valid = false;
    }

    // ---- the buffer for the next input: one nobody reads -- not the one of the call in flight, not one of a job, and not the
    // one that holds the stream's last samples, unless nothing else is free
    ClockSlotPick pick_buffer() const
    {
        ClockSlotPick p;
        bool busy[NXB] = {};
        if (in_flight) busy[xb] = true;
        for (int q = 0; q < NXB; ++q) if (job[q].state != CLK_JOB_FREE) busy[q] = true;
        for (int q = 0; q < NXB && p.b < 0; ++q) { const int c = (xb + 1 + q) % NXB; if (!busy[c] && c != hist.xb) p.b = c; }
        for (int q = 0; q < NXB && p.b < 0; ++q) { const int c = (xb + q) % NXB; if (!busy[c]) p.b = c; }
        if (p.b < 0) { snprintf(p.err, sizeof p.err, "clock recovery: no free sample buffer (%d calls are already in flight)", NXB); return p; }
        // (a job whose first walkers warm up over what this buffer holds must have read it: its pad copy and start states)
        for (int q = 0; q < NXB; ++q) p.wait_guess[q] = job[q].state >= CLK_JOB_WALKING && job[q].hist_src == p.b;
        p.forget = p.b == hist.xb;
        return p;
    }
    // ... handed out for a call of n new samples; eligible: the call walks overlapping blocks and becomes a job
    void hand_out(int b, size_t n, bool eligible)
    {
        x_pending = b;
        setting_up = -1;
        if (!eligible) return;
        ClockJob &j = job[b];
        j.state = CLK_JOB_SLOT;
        j.n = n;
        j.om_ext = false; j.om_scanned = false; j.nb = 0;
        j.serial = ++serials;
        setting_up = b;
    }

    // ---- the producer's timing statistic: an overlap job keeps its own (the walkers of the job behind it read it for their
    // first ranges); -1: the stage's
    int om_owner() const { return setting_up >= 0 && job[setting_up].state == CLK_JOB_SLOT ? setting_up : -1; }
    void om_noted(int nb, int BL)
    {
        const int o = om_owner();
        if (o >= 0) { ClockJob &j = job[o]; j.om_ext = true; j.om_scanned = false; j.nb = nb; j.BL = BL; }
        else { om_ext = true; om_scanned = false; om_nb = nb; om_BL = BL; }
    }
    // ... and its count curve on the producer's stream: not an overlap job's (unwrapped on its walkers' stream, at the launch)
    bool om_scan_here() const { return om_owner() < 0 && om_ext && om_nb >= 1; }
    void om_scan_done() { om_scanned = true; }
    // the producer ran again (the Costas loop went on from the host): the statistic is new, the call unwraps it itself
    void om_rewritten() { om_scanned = false; }

    // ---- the job in front of a job (-1: none)
    int front_of(int q0) const
    {
        for (int q = 0; q < NXB; ++q)
            if (q != q0 && job[q].state >= CLK_JOB_SLOT && job[q].serial + 1 == job[q0].serial) return q;
        return -1;
    }
    unsigned long long serial_of(int q) const { return q >= 0 && q < NXB ? job[q].serial : 0; }
    // a job's walkers may start before the call in front has finished: its statistic is in place, and the job in front is an
    // overlap job whose samples and timing curve are in place (its walkers may still be at work)
    bool can_launch_ahead(int q0, int pad_need) const
    {
        if (q0 < 0 || q0 >= NXB || job[q0].state != CLK_JOB_SLOT || !job[q0].om_ext) return false;
        const int f = front_of(q0);
        if (f < 0) return false;
        return job[f].om_scanned && (size_t)job[f].padN + job[f].n >= (size_t)pad_need && job[f].state >= CLK_JOB_WALKING;
    }

    // ---- the history a launch starts from: the job in front when launched ahead (it has not finished: `hist` still describes
    // the call before it), else what the last finished call left
    ClockLaunchHist launch_hist(int q0, bool ahead, int pad_need) const
    {
        ClockLaunchHist h;
        h.xb = hist.xb; h.job = hist.job; h.len = hist.len;
        if (ahead) {
            const int f = front_of(q0);
            if (f < 0) { h.err = "clock recovery: no job in front of a job launched ahead"; return h; }
            h.xb = f; h.job = f; h.len = (size_t)job[f].padN + job[f].n;
            h.wait_guess = f;       // (the curve of the job in front is unwrapped on ITS walkers' stream)
        }
        // (scanned: the job in front has been launched)
        h.have = h.xb >= 0 && h.len >= (size_t)pad_need && h.job >= 0 && job[h.job].om_scanned;
        return h;
    }
    // the plan's walker 0 warms up over history: that needs the job whose buffer and curve it is
    static const char *hist_refusal(const ClockLaunchHist &h, const ClockOvPlan &plan)
    {
        if (plan.w0_carried) return nullptr;
        return !(h.job >= 0 && h.xb == h.job) || h.len < (size_t)plan.padN ? "clock recovery: history without its job" : nullptr;
    }
    void planned(int q0, const ClockOvPlan &plan, bool ahead) { static_cast<ClockOvPlan &>(job[q0]) = plan; job[q0].ahead = ahead; }
    // launched: the statistic (nb blocks of BL samples) and its curve are in place
    void launched(int q0, const ClockLaunchHist &h, int nb, int BL)
    {
        ClockJob &j = job[q0];
        j.nb = nb; j.BL = BL;
        j.om_ext = true;
        if (nb >= 1) j.om_scanned = true;
        j.hist_src = j.w0_carried ? -1 : h.xb;
        j.state = CLK_JOB_WALKING;
    }

    // ---- restart: the samples of a job have been rewritten.  Walkers at work are waited for (ev_walk, by the host) ...
    bool restart_waits(int q0) const { return q0 >= 0 && q0 < NXB && job[q0].state == CLK_JOB_WALKING; }
    // ... and the job goes back to "samples produced"
    void restarted(int q0)
    {
        if (q0 < 0 || q0 >= NXB || job[q0].state < CLK_JOB_SLOT) return;
        job[q0].state = CLK_JOB_SLOT; job[q0].om_scanned = false;
    }

    // ---- a call begins
    void call_reset(size_t n) { prev_carry = carry; prev_n = n; redo_ok = false; ov_cur = -1; }
    // its overlap job, if its samples were produced into one: the oldest job that waits for its call.  Returns the refusal.
    const char *call_job(size_t n, bool sym_out)
    {
        unsigned long long first = ~0ull;
        for (int q = 0; q < NXB; ++q)
            if ((job[q].state == CLK_JOB_SLOT || job[q].state == CLK_JOB_WALKING) && job[q].serial < first) { first = job[q].serial; ov_cur = q; }
        if (ov_cur >= 0 && (job[ov_cur].n != n || sym_out)) return "clock recovery: the call does not match the overlap job its samples were produced for";
        return nullptr;
    }
    void begun_overlap()
    {
        xb = ov_cur;
        x_pending = -1;
        setting_up = -1;
        in_flight = true;
        om_ext = false; om_scanned = false;
    }
    // (known at the call: the call in front has finished)
    void w0_known(int q0) { ClockJob &j = job[q0]; if (j.ahead) j.w0_ii = j.padN - (int)carry; }
    void finalizing(int q0) { job[q0].state = CLK_JOB_FINALIZING; }
    // the chains: a call on its own buffer takes the one handed out ...
    void chains_buffer(bool own) { if (!own) return; if (x_pending >= 0) xb = x_pending; x_pending = -1; }
    // ... and consumes the producer's statistic
    ClockOm begun_chains()
    {
        in_flight = true;
        const ClockOm o{om_ext, om_ext && om_scanned};
        om_ext = false; om_scanned = false;
        return o;
    }

    // ---- a call ends
    void call_ended() { in_flight = false; }        // (the caller has synchronised)
    void flip() { cur ^= 1; }                       // the half the call wrote is the carried one now
    // the samples it left unread; the refusal beyond what the hand-over buffer holds
    const char *carried(long long left)
    {
        carry = (size_t)left;
        if (carry <= 1024) return nullptr;
        snprintf(err, sizeof err, "clock recovery: carry of %zu samples exceeds the hand-over buffer", carry);
        return err;
    }
    // short input: everything is carried
    void ended_short(long long N) { carry = (size_t)N; flip(); }
    // the overlap job of the call is given up (taken, fallen back, the watchdog): free.  Returns it.
    int overlap_released() { const int q = ov_cur; job[q].state = CLK_JOB_FREE; ov_cur = -1; return q; }
    // overlap taken: its buffer and curve are the history
    void ended_overlap(int q) { hist = ClockHistory{q, (size_t)job[q].padN + job[q].n, q}; redo_ok = true; }
    // overlap fell back: the chains run on the job's buffer (base given: their own end leaves the history alone) ...
    int overlap_fell_back() { const int q = overlap_released(); xb = q; return q; }
    // ... and, when they ended well, the job's buffer and curve are the history all the same
    void ended_fallback(int q) { hist = ClockHistory{q, (size_t)job[q].padN + job[q].n, q}; }
    // chains finished.  What the call left in its own buffer is history without a timing curve; a call on samples that lie
    // elsewhere leaves what there was
    void ended_chains(bool own) { redo_ok = true; if (own) hist = ClockHistory{xb, prev_carry + prev_n, -1}; }

    // ---- step back for a rerun of the last call: to the half it started from.  The samples kept as the next call's history
    // are negated / follow another handle's tail: forgotten.
    // redo_flipped: returns whether the flipped loop's own state (make_alt) takes the place of this one's
    bool step_back_flipped()
    {
        flip();
        const bool alt = alt_valid;
        carry = alt ? alt_carry : prev_carry;
        alt_valid = false;
        hist.forget();
        return alt;
    }
    void step_back_from(size_t carry_rec) { flip(); carry = carry_rec; alt_valid = false; hist.forget(); }
    // make_alt: the flipped rerun's outcome is kept aside, this sign's carry comes back
    void alt_made(size_t carry_keep) { alt_carry = carry; carry = carry_keep; alt_valid = true; redo_ok = false; }
};

}  // namespace xrit
