// chain_host_check.cpp -- the chain handle's in-flight pipeline (chain_pipeline.h) on the CPU, under the address and
// undefined-behaviour sanitizers: make chain-host-check.
//
// Scripts -- sequences of registrations (pf), process calls (go), resets, with the answers of the device scripted ("the
// Costas event of input k is not complete at the first m looks", "the loop of input k went on from the host", "the call's
// walkers need p polls") -- are run through a model of the handle that takes every decision from chain_pipeline.h and logs
// every call it would make: (call, stream, event, input, set).  The logs are compared with
// tests/golden/chain_pipeline_table.txt.
//
// How the table was made: NOT from chain_pipeline.h.  The control flow the header was taken out of -- ov_service,
// process_overlap, launch_prefetched, loops, the relay hook, xrit_demod_process_device, xrit_demod_prefetch_device,
// xrit_demod_reset and xrit_demod_keep_stages of demod.cpp as of commit 7624954 -- was copied verbatim into a CPU program
// in which the hip* calls and the stage methods are this file's Device (the same logging, the same scripted answers), and
// the scripts below were run through it (run_script is a template for that reason).  That program is not kept.
//
// Then: one hand-written row per branch of chain_next with both sides of its condition, and the invariants of the
// pipeline over every step of every script.  Recorded sequences that break an invariant are listed in KNOWN below and in
// DESIGN.md section 11; anything else that breaks one fails the check.
//
// The clock stage behind the handle is not restated here: the Device holds clock_jobs.h's ClockJobs (JobsModel: ClockStage's
// methods with every HIP step a log line) and keeps a second log per script -- the waits, records and copies the stage
// enqueues, the history of every launch, the plain state after every step -- which is compared with
// tests/golden/clock_jobs_table.txt, over the scripts above and the stage's own (stage_scripts).  That table was recorded the
// same way: NOT from clock_jobs.h but from ClockStage's methods as of commit e03ce39 copied verbatim into a CPU program behind
// JobsModel's interface (STAGE_MODEL), HIP stubbed; that program is not kept either.  Then one row per branch of the header's
// decisions (check_job_rules), and the ordering count: every access to a resource of the header's table must be ordered behind
// the access before it by its stream, an event or the host (unordered_accesses); the count is printed, not judged.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "chain_pipeline.h"

using namespace xrit;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// ---------------------------------------------------------------- the device and the stages, as far as the pipeline sees them
enum Ev { E_NONE, E_DONE, E_READY, E_FE0, E_FE1, E_RELAY, E_COSTAS };
static const char *const EV_NAME[] = {"-", "ev_done", "ev_ready", "ev_fe0", "ev_fe1", "ev_relay", "ev_costas"};
static const char *const STREAM_NAME[] = {"CALLER", "FRONT", "COSTAS", "WALK0", "WALK1", "-"};
constexpr int NO_STREAM = 5;
constexpr int MAX_IN = 16;

struct Entry {
    std::string op; int stream; int ev; long in; int set; long aux;
    std::string text() const
    {
        char b[160];
        snprintf(b, sizeof b, "%s %s %s in=%ld set=%d aux=%ld", op.c_str(), STREAM_NAME[stream], EV_NAME[ev], in, set, aux);
        return b;
    }
};

// ---------------------------------------------------------------- the clock stage's bookkeeping (clock_jobs.h)
// The stage's plain state after a step.  The jobs' table holds one such line per step; when it was recorded the same record
// was filled from the fields of the ClockStage before clock_jobs.h.
struct Snap {
    struct J { int state; unsigned long long serial; size_t n; bool ext, scanned, ahead, w0c; int src, padN; } j[NXB];
    int setting_up, ov_cur, xb, pend; bool fl; unsigned long long serials;
    int hxb; size_t hlen; int hjob;
    int cur; size_t carry, pc, pn; bool redo, alt; size_t altc; bool ext, scanned;
};
static std::string snap_text(const char *op, int rc, const Snap &s)
{
    char b[512];
    int at = snprintf(b, sizeof b, "%s rc=%d |", op, rc);
    for (const Snap::J &j : s.j)
        at += snprintf(b + at, sizeof b - at, " %d/%llu/%zu/%d%d%d%d/%d/%d", j.state, j.serial, j.n, j.ext, j.scanned, j.ahead, j.w0c, j.src, j.padN);
    snprintf(b + at, sizeof b - at, " | set=%d cur=%d xb=%d pend=%d fl=%d serials=%llu | hist=%d,%zu,%d | st=%d carry=%zu prev=%zu,%zu redo=%d alt=%d,%zu om=%d%d",
             s.setting_up, s.ov_cur, s.xb, s.pend, s.fl, s.serials, s.hxb, s.hlen, s.hjob, s.cur, s.carry, s.pc, s.pn, s.redo, s.alt, s.alt ? s.altc : 0, s.ext, s.scanned);
    return b;
}
// what both models of the stage log beside the snapshots: waits, records, copies, the launch's history
// ... and, for the ordering count, every access to a resource of clock_jobs.h's table with everything that can order it
enum OrdKind { O_RECORD, O_WAIT, O_HOST_EVENT, O_HOST_STREAM, O_READ, O_WRITE };
enum { R_NEW = 0, R_PAD = NXB, R_STAT = 2 * NXB, R_CURVE = 3 * NXB, R_WALK = 4 * NXB, R_ST = 5 * NXB, R_OM = 5 * NXB + 2, R_COUNT };  // per buffer / job; st, tail halves; the stage's statistic
enum { EV_GUESS = 8, EV_WALK = 8 + NXB, EV_COUNT = 8 + 2 * NXB };      // (below 8: the pipeline's events, enum Ev)
struct Ord { OrdKind kind; int stream, id; };
struct JobsLog {
    std::vector<std::string> lines;
    std::vector<Ord> ord;
    void order(OrdKind k, int stream, int id) { ord.push_back(Ord{k, stream, id}); }
    std::function<void(int job, int stream, bool ahead)> on_launch;     // (the pipeline's own log takes the launch from here)
    void say(const char *fmt, ...) __attribute__((format(printf, 2, 3)))
    {
        char b[256];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(b, sizeof b, fmt, ap);
        va_end(ap);
        lines.push_back(b);
    }
    void launch(int job, int stream, bool ahead, int h_xb, size_t h_len, int h_job, bool have)
    {
        say("launch job=%d %s ahead=%d hist=%d,%zu,%d have=%d", job, STREAM_NAME[stream], ahead, h_xb, h_len, h_job, have);
        if (on_launch) on_launch(job, stream, ahead);
    }
};

// ClockStage's methods (clock.hip) without the device: every decision clock_jobs.h's, every HIP step a line of the log.
// Scripted answers of the device: the verdict on the next overlap call's walkers, the samples a call leaves unread.
struct JobsModel {
    ClockKnobs knobs;
    size_t xpad = 1024;
    int pad_need = 0;
    ClockJobs jobs;
    JobsLog *lg = nullptr;
    int verdict = CLK_OV_TAKE;
    long leave = 5;
    struct Call { bool short_input = false, base = false; long long N = 0; } call;

    void init(JobsLog *l) { lg = l; pad_need = clock_ov_pad_need(knobs); }
    int setting_up() const { return jobs.setting_up; }
    int ov_cur() const { return jobs.ov_cur; }
    unsigned long long serial_of(int q) const { return jobs.serial_of(q); }
    unsigned long long serials() const { return jobs.serials; }
    bool can_launch_ahead(int q) const { return jobs.can_launch_ahead(q, pad_need); }
    Snap snap() const
    {
        Snap s{};
        for (int q = 0; q < NXB; ++q) {
            const ClockJob &j = jobs.job[q];
            s.j[q] = Snap::J{(int)j.state, j.serial, j.n, j.om_ext, j.om_scanned, j.ahead, j.w0_carried, j.hist_src, j.padN};
        }
        s.setting_up = jobs.setting_up; s.ov_cur = jobs.ov_cur; s.xb = jobs.xb; s.pend = jobs.x_pending; s.fl = jobs.in_flight; s.serials = jobs.serials;
        s.hxb = jobs.hist.xb; s.hlen = jobs.hist.len; s.hjob = jobs.hist.job;
        s.cur = jobs.cur; s.carry = jobs.carry; s.pc = jobs.prev_carry; s.pn = jobs.prev_n; s.redo = jobs.redo_ok; s.alt = jobs.alt_valid; s.altc = jobs.alt_carry;
        s.ext = jobs.om_ext; s.scanned = jobs.om_scanned;
        return s;
    }
    int done(const char *op, int rc) { lg->lines.push_back(snap_text(op, rc, snap())); return rc; }
    void rd(int res, int s) { lg->order(O_READ, s, res); }
    void wr(int res, int s) { lg->order(O_WRITE, s, res); }
    int pending() const { return jobs.x_pending; }

    int input_slot(size_t n, int stream)
    {
        const ClockSlotPick p = jobs.pick_buffer();
        if (p.b < 0) return done("input_slot", -1);
        for (int q = 0; q < NXB; ++q) if (p.wait_guess[q]) { lg->say("wait ev_guess[%d] %s", q, STREAM_NAME[stream]); lg->order(O_WAIT, stream, EV_GUESS + q); }
        if (p.forget) jobs.hist.forget();
        jobs.hand_out(p.b, n, clock_ov_eligible(knobs, xpad, false, n));
        wr(R_NEW + p.b, stream);        // (the producer: the samples, and its statistic)
        wr(jobs.setting_up >= 0 ? R_STAT + p.b : R_OM, stream);
        return done("input_slot", 0);
    }
    void om_slot(int nb, int BL) { jobs.om_noted(nb, BL); done("om_slot", 0); }
    void om_scan(int stream)
    {
        if (jobs.om_scan_here()) { lg->say("unwrap %s", STREAM_NAME[stream]); rd(R_OM, stream); wr(R_OM, stream); jobs.om_scan_done(); }
        done("om_scan", 0);
    }
    int launch(int q, int sw, bool ahead)
    {
        const ClockJob &j = jobs.job[q];
        const ClockLaunchHist h = jobs.launch_hist(q, ahead, pad_need);
        if (h.err) return -1;
        if (h.wait_guess >= 0) { lg->say("wait ev_guess[%d] %s", h.wait_guess, STREAM_NAME[sw]); lg->order(O_WAIT, sw, EV_GUESS + h.wait_guess); }
        lg->launch(q, sw, ahead, h.xb, h.len, h.job, h.have);
        const ClockOvPlan plan = clock_ov_plan(knobs, j.n, jobs.carry, h.have, ahead);
        if (plan.err[0]) return -1;
        jobs.planned(q, plan, ahead);
        if (!j.w0_carried) {
            if (ClockJobs::hist_refusal(h, j)) return -1;
            lg->say("copy %s", STREAM_NAME[sw]);
            rd(R_NEW + h.xb, sw); wr(R_PAD + q, sw);
        } else if (j.padN > 0) { lg->say("tail %s", STREAM_NAME[sw]); rd(R_ST + jobs.cur, sw); wr(R_PAD + q, sw); }
        int nb = j.nb;
        const int BL = j.om_ext ? j.BL : CLK_OM_BLOCK;
        if (!j.om_ext) { nb = (int)((j.n + CLK_OM_BLOCK - 1) / CLK_OM_BLOCK); lg->say("om %s", STREAM_NAME[sw]); rd(R_NEW + q, sw); wr(R_STAT + q, sw); }
        if (!j.om_scanned && nb >= 1) { lg->say("unwrap %s", STREAM_NAME[sw]); rd(R_STAT + q, sw); wr(R_CURVE + q, sw); }
        if (!j.w0_carried && h.job >= 0 && jobs.job[h.job].BL != BL) return -1;
        // the start states: this job's curve and the one in front's, the samples; walker 0 from the carried state
        rd(R_CURVE + q, sw); rd(R_NEW + q, sw); rd(R_PAD + q, sw);
        if (!j.w0_carried && h.job >= 0) rd(R_CURVE + h.job, sw);
        if (j.w0_carried) rd(R_ST + jobs.cur, sw);
        wr(R_WALK + q, sw);
        lg->say("record ev_guess[%d] %s", q, STREAM_NAME[sw]);
        lg->order(O_RECORD, sw, EV_GUESS + q);
        lg->say("record ev_walk[%d] %s", q, STREAM_NAME[sw]);
        lg->order(O_RECORD, sw, EV_WALK + q);
        jobs.launched(q, h, nb, BL);
        return 0;
    }
    int ov_launch(int q, int sw, bool ahead) { return done("ov_launch", launch(q, sw, ahead)); }
    int ov_restart(int q)
    {
        if (jobs.restart_waits(q)) { lg->say("sync ev_walk[%d]", q); lg->order(O_HOST_EVENT, 0, EV_WALK + q); }
        jobs.restarted(q);
        return done("ov_restart", 0);
    }
    int begin_chains(bool base, int exact_, size_t n, int s)
    {
        ClockKnobs k = knobs;
        k.exact = exact_;
        const ClockChainPlan plan = clock_chain_plan(k, n, jobs.carry, -1, 0);
        call = Call{plan.short_input, base, plan.N};
        jobs.chains_buffer(!base);
        const ClockOm om_in = jobs.begun_chains();
        if (jobs.carry) { lg->say("tail %s", STREAM_NAME[s]); rd(R_ST + jobs.cur, s); wr(R_PAD + jobs.xb, s); }
        rd(R_NEW + jobs.xb, s); rd(R_ST + jobs.cur, s);
        if (om_in.ext) rd(R_OM, s);
        wr(R_ST + (jobs.cur ^ 1), s);
        if (plan.err[0]) return -1;
        if (plan.short_input) { if (plan.N > 0) lg->say("copy %s", STREAM_NAME[s]); lg->say("copy %s", STREAM_NAME[s]); }
        return 0;
    }
    int begin(size_t n, bool sym_out, int s)
    {
        jobs.call_reset(n);
        if (jobs.call_job(n, sym_out)) return done("begin", -1);
        if (jobs.ov_cur < 0) return done("begin", begin_chains(false, knobs.exact, n, s));
        call = Call{};
        jobs.begun_overlap();
        const int q = jobs.ov_cur;
        if (jobs.job[q].state == CLK_JOB_SLOT && launch(q, s, false)) return done("begin", -1);
        lg->say("wait ev_walk[%d] %s", q, STREAM_NAME[s]);
        lg->order(O_WAIT, s, EV_WALK + q);
        rd(R_WALK + q, s); rd(R_NEW + q, s); rd(R_PAD + q, s); rd(R_ST + jobs.cur, s); wr(R_ST + (jobs.cur ^ 1), s);    // the joints, the output, the tail
        jobs.w0_known(q);
        jobs.finalizing(q);
        return done("begin", 0);
    }
    int run_chains(bool base, int exact_, size_t n, int s)
    {
        jobs.call_reset(n);
        if (begin_chains(base, exact_, n, s)) return -1;
        done("sync", 0);
        lg->order(O_HOST_STREAM, s, 0);
        return finish_call(s);
    }
    int finish_call(int s)
    {
        jobs.call_ended();
        if (jobs.ov_cur >= 0) {
            const ClockJob &oj = jobs.job[jobs.ov_cur];
            const int v = verdict;
            verdict = CLK_OV_TAKE;
            if (v == CLK_OV_WATCHDOG) { (void)jobs.overlap_released(); return -1; }
            if (v != CLK_OV_TAKE) {
                const int q = jobs.overlap_fell_back();
                const int rc = run_chains(true, v == CLK_OV_FALLBACK_TO_CLOSURE ? 1 : 0, jobs.job[q].n, s);
                if (rc == 0) jobs.ended_fallback(q);
                return rc;
            }
            const int jb = jobs.overlap_released();
            jobs.flip();
            if (jobs.carried(leave < oj.N ? leave : oj.N)) return -1;
            jobs.ended_overlap(jb);
            return 0;
        }
        if (call.short_input) { jobs.ended_short(call.N); return 0; }
        jobs.flip();
        if (jobs.carried(leave < call.N ? leave : call.N)) return -1;
        jobs.ended_chains(!call.base);
        return 0;
    }
    int finish(int s) { return done("finish", finish_call(s)); }
    int run(size_t n, int s)
    {
        if (const int rc = begin(n, false, s)) return rc;
        done("sync", 0);
        lg->order(O_HOST_STREAM, s, 0);
        return finish(s);
    }
    int redo_flipped_call(int s)
    {
        if (!jobs.redo_ok) return -1;
        const bool from_alt = jobs.step_back_flipped();
        const size_t n = jobs.prev_n;
        wr(R_ST + jobs.cur, s); wr(R_NEW + jobs.xb, s);     // (the state flipped or replaced, the input negated)
        if (from_alt) { lg->say("copy %s", STREAM_NAME[s]); lg->say("copy %s", STREAM_NAME[s]); }
        return run_chains(true, knobs.exact, n, s);
    }
    int redo_flipped(int s) { return done("redo_flipped", redo_flipped_call(s)); }
    int redo_from(size_t carry_rec, int s)
    {
        if (!jobs.redo_ok || carry_rec > 1024) return done("redo_from", -1);
        jobs.step_back_from(carry_rec);
        wr(R_ST + jobs.cur, s);
        return done("redo_from", run_chains(true, knobs.exact, jobs.prev_n, s));
    }
    int make_alt(int s)
    {
        jobs.alt_valid = false;
        if (!jobs.redo_ok) return done("make_alt", -1);
        const size_t carry_keep = jobs.carry;
        for (int i = 0; i < 2; ++i) lg->say("copy %s", STREAM_NAME[s]);
        rd(R_ST + jobs.cur, s);
        if (redo_flipped_call(s)) return done("make_alt", -1);
        for (int i = 0; i < 4; ++i) lg->say("copy %s", STREAM_NAME[s]);
        rd(R_ST + jobs.cur, s); wr(R_ST + jobs.cur, s);
        jobs.alt_made(carry_keep);
        return done("make_alt", 0);
    }
    void reset() { jobs.reset(); wr(R_ST, CHAIN_CALLER); wr(R_ST + 1, CHAIN_CALLER); done("reset", 0); }
};
#ifndef STAGE_MODEL
#define STAGE_MODEL JobsModel       // (when the jobs' table was recorded: the same interface over the ClockStage before clock_jobs.h)
#endif

struct Device {
    std::vector<Entry> log;
    void note(const char *op, int stream = NO_STREAM, int ev = E_NONE, long in = 0, int set = -1, long aux = 0) { log.push_back(Entry{op, stream, ev, in, set, aux}); }
    // ---- scripted answers
    int not_yet[MAX_IN] = {};       // looks at ev_costas that find the loop of input k still at work
    bool redo[MAX_IN] = {};         // the loop of input k does not close in its batch: the host continues it
    int done_polls = 0;             // looks at ev_done that find the call's walkers still at work
    // ---- events: whose Costas loop ev_costas was last recorded behind (the device's own view)
    long costas_owner = 0;
    void wait(int stream, int ev) { jlog.order(O_WAIT, stream, ev); note("wait", stream, ev, ev == E_COSTAS ? costas_owner : 0); }
    void record(int stream, int ev) { jlog.order(O_RECORD, stream, ev); if (ev == E_COSTAS) costas_owner = costas_in; note("record", stream, ev, ev == E_COSTAS ? costas_owner : 0); }
    void sync_event(int ev) { jlog.order(O_HOST_EVENT, 0, ev); if (ev == E_COSTAS && costas_owner > 0) not_yet[costas_owner] = 0; note("sync_event", NO_STREAM, ev, ev == E_COSTAS ? costas_owner : 0); }
    void sync_stream(int stream) { jlog.order(O_HOST_STREAM, stream, 0); note("sync_stream", stream); }
    bool query(int ev)
    {
        bool done = true;
        if (ev == E_COSTAS && costas_owner > 0 && not_yet[costas_owner] > 0) { --not_yet[costas_owner]; done = false; }
        if (ev == E_DONE && done_polls > 0) { --done_polls; done = false; }
        if (done) jlog.order(O_HOST_EVENT, 0, ev);
        note("query", NO_STREAM, ev, ev == E_COSTAS ? costas_owner : 0, -1, done ? 1 : 0);
        return done;
    }
    // ---- the front end (input k's samples "pointer" is k)
    void front_end(int stream, long in, int set) { note("front_end", stream, E_NONE, in, set); }
    // ---- the Costas stage
    long costas_in = 0;             // the input of the loop begun last
    bool costas_out = false;        // ... which has not been looked at
    int slot_of[MAX_IN] = {};       // the buffer the loop of input k writes
    void costas_begin(int stream, long in) { slot_of[in] = stage.pending(); costas_in = in; costas_out = true; note("costas_begin", stream, E_NONE, in, -1, (long)stage.serial_of(stage.setting_up())); }
    bool costas_finish(int stream)  // returns: redone
    {
        const bool r = redo[costas_in];
        // (the loop went on from the host, on its stream, and the host waited for it: the samples are written again)
        if (r && slot_of[costas_in] >= 0) { jlog.order(O_WRITE, stream, R_NEW + slot_of[costas_in]); jlog.order(O_HOST_STREAM, stream, 0); }
        redo[costas_in] = false;
        costas_out = false;
        note("costas_finish", stream, E_NONE, costas_in, -1, r ? 1 : 0);
        return r;
    }
    // ---- the clock stage: clock_jobs.h's bookkeeping (JobsModel), its log beside the pipeline's
    STAGE_MODEL stage;
    JobsLog jlog;
    ClockKnobs &knobs = stage.knobs;
    size_t &xpad = stage.xpad;
    std::function<int(int)> before_relay;
    void stage_init()
    {
        stage.init(&jlog);
        jlog.on_launch = [this](int job, int stream, bool ahead) { note("ov_launch", stream, E_NONE, 0, -1, (long)stage.serial_of(job) * 2 + (ahead ? 1 : 0)); };
    }
    void input_slot(size_t n, int stream) { (void)stage.input_slot(n, stream); }
    void om_slot(size_t n) { stage.om_slot((int)((n + 255) / 256), 256); }
    void ov_launch(int job, int stream, bool ahead) { (void)stage.ov_launch(job, stream, ahead); }
    void ov_restart(int job, int stream) { (void)stage.ov_restart(job); note("ov_restart", stream, E_NONE, 0, -1, (long)stage.serial_of(job)); }
    int clock_begin(size_t n, int stream)
    {
        (void)stage.begin(n, false, stream);
        if (stage.ov_cur() >= 0) { note("clock_begin_overlap", stream, E_NONE, 0, -1, (long)stage.serial_of(stage.ov_cur())); return 0; }
        note("clock_begin_chains", stream, E_NONE, 0, -1, (long)n);
        if (knobs.relay_by_default()) {
            int rc = before_relay ? before_relay(0) : 0;
            if (rc) return rc;
            note("relay_kernels", stream);
            if (before_relay) rc = before_relay(1);
            return rc;
        }
        return 0;
    }
    void clock_finish(int stream) { (void)stage.finish(stream); note("clock_finish", stream); }
    void clock_reset() { stage.reset(); note("stages_reset"); }
};

// ---------------------------------------------------------------- the handle: demod.cpp's flow, every decision chain_pipeline.h's
struct Handle {
    Device &m;
    ChainQueue q;
    bool costas_idle = false, no_defer = false, keep = false, poisoned = false;
    std::string err;
    explicit Handle(Device &dev) : m(dev) {}
    static constexpr unsigned D = 1;
    bool ov_call(size_t n) { return chain_ov_call(m.knobs, m.xpad, keep, D, n); }
    long name(const ChainInput &f) const { return (long)(size_t)f.samples; }

    void launch_prefetched(ChainInput &f, int after)
    {
        m.wait(CHAIN_FRONT, E_READY);
        if (after) m.wait(CHAIN_FRONT, after);
        const ChainFrontEnd fe = chain_front_end_take(q);
        if (fe.behind_set >= 0) m.wait(CHAIN_FRONT, E_FE0 + fe.behind_set);
        f.io.set = fe.set; f.io.length = f.n; f.io.rrc = f.samples;
        m.front_end(CHAIN_FRONT, name(f), fe.set);
        m.record(CHAIN_FRONT, E_FE0 + fe.set);
        chain_front_end_done(q, f, fe.set);
    }
    void costas_enqueue(const ChainSlice &io, int stream)
    {
        m.input_slot(io.length, stream);
        m.om_slot(io.length);
        m.costas_begin(stream, (long)(size_t)io.rrc);
    }
    void set_relay_hook(int s)
    {
        m.before_relay = [this, s](int phase) -> int {
            if (!chain_start_under_relay(q)) return 0;
            if (phase == 0) { m.record(s, E_RELAY); return 0; }
            ChainInput &f = q.in[0];
            launch_prefetched(f, E_RELAY);
            if (chain_costas_under_relay(costas_idle)) {
                costas_enqueue(f.io, CHAIN_FRONT);
                m.record(CHAIN_FRONT, E_COSTAS);
                chain_costas_begun(q, f, CHAIN_FRONT, nullptr, -1, 0);
                CHECK(q.costas_event_of == f.id, "the event's owner in the queue");
            }
            return 0;
        };
    }
    void loops(const ChainSlice &io, int s, long call_id, bool costas_done)
    {
        if (!costas_done) costas_enqueue(io, s);
        if (chain_costas_first(q, costas_done)) {
            m.record(s, E_COSTAS);
            q.costas_event_of = call_id;
            m.sync_event(E_COSTAS);
            (void)m.costas_finish(s);
            costas_done = true;
        }
        costas_idle = costas_done;
        set_relay_hook(s);
        (void)m.clock_begin(io.length, s);
        m.before_relay = nullptr;
        costas_idle = false;
        m.sync_stream(s);
        if (!costas_done && m.costas_finish(s)) { (void)m.clock_begin(io.length, s); m.sync_stream(s); }
        m.clock_finish(s);
        if (keep) m.sync_stream(s);
    }
    struct Facts {
        Handle *h;
        bool costas_event_done() { return h->m.query(E_COSTAS); }
        unsigned long long ov_serial() { return h->m.stage.serials(); }
        bool can_launch_ahead(int job) { return h->m.stage.can_launch_ahead(job); }
    };
    bool ov_service(int limit = 1 << 30)
    {
        Facts facts{this};
        ChainScan scan;
        bool progress = false;
        for (;;) {
            const ChainStep st = chain_next(q, scan, facts, limit);
            if (st.kind == CHAIN_NONE) return progress;
            ChainInput &f = q.in[st.i];
            switch (st.kind) {
            case CHAIN_FRONT_END: launch_prefetched(f, E_NONE); break;
            case CHAIN_COSTAS_LOOK:
                CHECK(st.event_of == f.id && m.costas_owner == name(f), "a look at ev_costas while it stands for another input's loop");
                chain_costas_looked(f, m.costas_finish(st.stream));
                break;
            case CHAIN_WALK_RESTART: m.ov_restart(f.ov_job, st.stream); chain_walk_restarted(f); break;
            case CHAIN_COSTAS_BEGIN:
                if (st.wait_fe) m.wait(st.stream, E_FE0 + f.io.set);
                costas_enqueue(f.io, st.stream);
                m.record(st.stream, E_COSTAS);
                chain_costas_begun(q, f, st.stream, nullptr, m.stage.setting_up(), m.stage.serial_of(m.stage.setting_up()));
                break;
            case CHAIN_WALK_LAUNCH:
                m.wait(st.stream, E_COSTAS);
                m.ov_launch(f.ov_job, st.stream, true);
                chain_walk_launched(f);
                break;
            case CHAIN_NONE: break;
            }
            progress = true;
        }
    }

    int fail(const char *text) { err = text; m.note("error"); return -1; }
    int process_overlap(const void *samples, size_t n, int s)
    {
        if (q.count > 0) {
            if (!chain_front_is(q, samples, n, 0)) { poisoned = true; return fail("process calls must take the prefetched inputs in the order they were prefetched"); }
        } else {
            m.record(s, E_READY);
            chain_stage(q, samples, n, 0, true);
            q.count = 1;
        }
        ov_service();
        ChainInput &f0 = q.in[0];
        for (int spins = 0; !f0.costas_finished; ++spins) {
            if (f0.costas_begun) m.sync_event(E_COSTAS);
            ov_service(1);
            if (spins > 8) { poisoned = true; return fail("the Costas loop of the call could not be started"); }
        }
        (void)m.clock_begin(f0.io.length, s);
        m.record(s, E_DONE);
        ov_service();
        while (!m.query(E_DONE)) (void)ov_service();
        m.clock_finish(s);
        chain_pop(q);
        return 0;
    }
    int go(const void *samples, size_t n)
    {
        const int s = CHAIN_CALLER;
        if (poisoned) return fail("this handle's carried state is inconsistent after an earlier failed call: destroy it and create a new one");
        if (chain_call_overlaps(q, ov_call(n))) return process_overlap(samples, n, s);
        ChainSlice io;
        long call_id = 0;
        if (q.count > 0) {
            if (!chain_front_is(q, samples, n, 0)) { poisoned = true; return fail("process calls must take the prefetched inputs in the order they were prefetched"); }
            if (chain_start_at_call(q)) launch_prefetched(q.in[0], E_NONE);
            const ChainInput f = q.in[0];
            chain_pop(q);
            io = f.io;
            call_id = f.id;
            if (f.costas_begun) {
                m.sync_event(E_COSTAS);
                (void)m.costas_finish(f.costas_stream);
                loops(io, s, call_id, true);
                return 0;
            }
            m.wait(s, E_FE0 + f.io.set);
        } else {
            const ChainFrontEnd fe = chain_front_end_take(q);
            if (fe.behind_set >= 0) m.wait(s, E_FE0 + fe.behind_set);
            io.set = fe.set; io.length = n; io.rrc = samples;
            m.front_end(s, (long)(size_t)samples, fe.set);
            m.record(s, E_FE0 + fe.set);
            chain_front_end_started(q, fe.set);
        }
        loops(io, s, call_id, false);
        return 0;
    }
    int pf(const void *samples, size_t n)
    {
        if (poisoned) return fail("this handle's carried state is inconsistent after an earlier failed call");
        const bool ov = ov_call(n);
        if (q.count >= chain_room(q, ov)) return fail("prefetched inputs are already waiting for their process calls");
        if (keep) return 0;
        m.record(CHAIN_CALLER, E_READY);
        ChainInput &f = chain_stage(q, samples, n, 0, ov);
        if (!chain_defer(m.knobs.relay_by_default(), no_defer, ov)) {
            if (chain_start_oldest_first(q)) launch_prefetched(q.in[0], E_NONE);
            launch_prefetched(f, E_NONE);
        }
        ++q.count;
        return 0;
    }
    int reset()
    {
        for (int st : {CHAIN_FRONT, CHAIN_COSTAS, CHAIN_WALK0, CHAIN_WALK1})
            if (st != CHAIN_COSTAS || q.has_costas_stream) m.sync_stream(st);
        if (m.costas_out && q.count > 0)
            for (int i = 0; i < q.count; ++i)
                if (q.in[i].costas_begun && !q.in[i].costas_finished) (void)m.costas_finish(q.in[i].costas_stream);
        chain_reset(q);
        m.clock_reset();
        poisoned = false;
        return 0;
    }
    int keep_stages(bool on)
    {
        if (q.count > 0) return fail("prefetched inputs wait for their process calls: stage copies are switched between plain calls");
        keep = on;
        return 0;
    }
};

// ---------------------------------------------------------------- scripts
enum Op { PF, GO, RESET, KEEP, NOT_YET, REDO, POLLS };
struct Cmd { Op op; long in; int arg; };       // in: the input's name (1, 2, ... in the order of the stream); PF / GO arg: 1 big, 0 small
struct Script {
    const char *name;
    int clock_exact; bool no_defer, costas_stream; long below;     // of the handle (below: costas_own_stream_below, 0: the default)
    std::vector<Cmd> cmds;
};
constexpr size_t BIG = (size_t)1 << 23, SMALL = (size_t)1 << 19;    // samples at D = 1: 1.97 M symbols (walks overlapping blocks) / 123 k

static std::vector<Script> scripts()
{
    const int B = 1, S = 0;
    std::vector<Script> v;
    // the four plans of test_big_calls_walk_overlapping_blocks
    v.push_back({"plain x4", 0, false, false, 0, {{GO, 1, B}, {GO, 2, B}, {GO, 3, B}, {GO, 4, B}}});
    v.push_back({"three ahead", 0, false, false, 0, {{PF, 1, B}, {PF, 2, B}, {PF, 3, B}, {GO, 1, B}, {PF, 4, B}, {GO, 2, B}, {GO, 3, B}, {GO, 4, B}}});
    v.push_back({"one ahead", 0, false, false, 0, {{PF, 1, B}, {GO, 1, B}, {PF, 2, B}, {GO, 2, B}, {PF, 3, B}, {GO, 3, B}, {PF, 4, B}, {GO, 4, B}}});
    v.push_back({"mixed", 0, false, false, 0, {{GO, 1, B}, {PF, 2, B}, {GO, 2, B}, {PF, 3, B}, {PF, 4, B}, {GO, 3, B}, {GO, 4, B}}});
    v.push_back({"three ahead, steady", 0, false, false, 0, {{PF, 1, B}, {PF, 2, B}, {GO, 1, B}, {PF, 3, B}, {GO, 2, B}, {PF, 4, B}, {GO, 3, B}, {PF, 5, B}, {GO, 4, B}, {PF, 6, B}, {GO, 5, B}, {GO, 6, B}}});
    v.push_back({"three ahead, walkers polled", 0, false, false, 0, {{PF, 1, B}, {PF, 2, B}, {PF, 3, B}, {POLLS, 0, 2}, {GO, 1, B}, {NOT_YET, 2, 1}, {PF, 4, B}, {POLLS, 0, 3}, {GO, 2, B}, {GO, 3, B}, {GO, 4, B}}});
    v.push_back({"three ahead, Costas stream", 0, false, true, 0, {{PF, 1, B}, {PF, 2, B}, {PF, 3, B}, {GO, 1, B}, {PF, 4, B}, {GO, 2, B}, {GO, 3, B}, {GO, 4, B}}});
    v.push_back({"three ahead, Costas on the front ends' stream", 0, false, false, 1, {{PF, 1, B}, {PF, 2, B}, {PF, 3, B}, {GO, 1, B}, {PF, 4, B}, {GO, 2, B}, {GO, 3, B}, {GO, 4, B}}});
    // the reset and destroy sequences of test_prefetched_front_ends_give_the_same_symbols
    v.push_back({"reset with inputs waiting", 0, false, false, 0, {{PF, 1, B}, {PF, 2, B}, {GO, 1, B}, {PF, 3, B}, {RESET, 0, 0}, {GO, 4, B}, {PF, 5, B}, {GO, 5, B}}});
    v.push_back({"reset, chains path", 0, false, false, 0, {{GO, 1, S}, {PF, 2, S}, {GO, 2, S}, {PF, 3, S}, {RESET, 0, 0}, {GO, 4, S}, {PF, 5, S}, {GO, 5, S}}});
    v.push_back({"reset behind a relay that started the next loop", 0, false, false, 0, {{PF, 1, S}, {GO, 1, S}, {PF, 2, S}, {GO, 2, S}, {PF, 3, S}, {PF, 4, S}, {GO, 3, S}, {RESET, 0, 0}, {GO, 5, S}}});
    for (int ce : {0, 1}) {
        static char names[2][64];
        snprintf(names[ce], sizeof names[ce], "reset beside the relay, then left, clock_exact %d", ce);
        v.push_back({names[ce], ce, false, false, 0, {{PF, 1, S}, {PF, 2, S}, {GO, 1, S}, {RESET, 0, 0}, {GO, 3, S}, {PF, 4, S}}});
    }
    v.push_back({"left with inputs waiting", 0, false, false, 0, {{PF, 1, B}, {PF, 2, B}, {GO, 1, B}, {PF, 3, B}}});
    // the chains path: relay on (clock_exact 0 and 1) and off (-1), with and without no_defer
    for (int ce : {0, 1, -1})
        for (bool nd : {false, true}) {
            static char names[6][64];
            static int k = 0;
            snprintf(names[k], sizeof names[k], "chains stream, clock_exact %d%s", ce, nd ? ", no_defer" : "");
            v.push_back({names[k++], ce, nd, false, 0, {{GO, 1, S}, {PF, 2, S}, {GO, 2, S}, {PF, 3, S}, {PF, 4, S}, {GO, 3, S}, {GO, 4, S}, {PF, 5, S}, {GO, 5, S}, {GO, 6, S}}});
        }
    // a queue that mixes the two paths, in both orders
    v.push_back({"big then small", 0, false, false, 0, {{PF, 1, B}, {PF, 2, S}, {GO, 1, B}, {GO, 2, S}}});
    v.push_back({"small then big", 0, false, false, 0, {{PF, 1, S}, {PF, 2, B}, {GO, 1, S}, {GO, 2, B}}});
    v.push_back({"big, small, big in a stream", 0, false, false, 0, {{GO, 1, B}, {PF, 2, S}, {GO, 2, S}, {PF, 3, B}, {GO, 3, B}, {PF, 4, S}, {PF, 5, B}, {GO, 4, S}, {GO, 5, B}}});
    v.push_back({"small then big, no_defer", 0, true, false, 0, {{PF, 1, S}, {PF, 2, B}, {GO, 1, S}, {GO, 2, B}}});
    v.push_back({"big then small, no_defer", 0, true, false, 0, {{PF, 1, B}, {PF, 2, S}, {GO, 1, B}, {GO, 2, S}}});
    // a Costas loop that does not close in its batch: the walkers are restarted
    v.push_back({"loop redone, walkers restarted", 0, false, false, 0, {{PF, 1, B}, {PF, 2, B}, {PF, 3, B}, {GO, 1, B}, {REDO, 3, 0}, {NOT_YET, 3, 2}, {PF, 4, B}, {GO, 2, B}, {GO, 3, B}, {GO, 4, B}}});
    v.push_back({"first loop redone", 0, false, false, 0, {{REDO, 1, 0}, {PF, 1, B}, {PF, 2, B}, {GO, 1, B}, {GO, 2, B}}});
    v.push_back({"loop redone, chains path", 0, false, false, 0, {{GO, 1, S}, {PF, 2, S}, {GO, 2, S}, {REDO, 3, 0}, {PF, 3, S}, {GO, 3, S}, {REDO, 4, 0}, {GO, 4, S}}});
    // what the ABI rejects
    v.push_back({"fourth registration", 0, false, false, 0, {{PF, 1, B}, {PF, 2, B}, {PF, 3, B}, {PF, 4, B}, {GO, 1, B}, {GO, 2, B}, {GO, 3, B}}});
    v.push_back({"third registration, chains path", 0, false, false, 0, {{PF, 1, S}, {PF, 2, S}, {PF, 3, S}, {GO, 1, S}, {GO, 2, S}}});
    v.push_back({"third registration behind a small one", 0, false, false, 0, {{PF, 1, B}, {PF, 2, S}, {PF, 3, B}, {GO, 1, B}, {GO, 2, S}}});
    v.push_back({"go out of order", 0, false, false, 0, {{PF, 1, B}, {PF, 2, B}, {GO, 2, B}, {GO, 1, B}, {RESET, 0, 0}, {GO, 3, B}}});
    v.push_back({"go out of order, chains path", 1, false, false, 0, {{PF, 1, S}, {PF, 2, S}, {GO, 2, S}, {RESET, 0, 0}, {GO, 3, S}}});
    v.push_back({"keep_stages with inputs waiting", 0, false, false, 0, {{PF, 1, B}, {KEEP, 0, 1}, {GO, 1, B}, {KEEP, 0, 1}, {PF, 2, B}, {GO, 2, B}, {KEEP, 0, 0}, {PF, 3, B}, {GO, 3, B}}});
    return v;
}

static void configure(Device &m, const Script &sc)
{
    ClockKnobs &k = m.knobs;
    k.sps = 1.25e6f / 293883.0f;        // LRIT at 1.25 Msamples/s, no decimator
    k.par.omega_mid = k.sps; k.par.omega_lim = k.sps * 0.005f;
    k.exact = sc.clock_exact;
    m.xpad = clock_xpad(k);
    m.stage_init();
}

// H: Handle -- or, when the table was recorded, the copy of the code before it
template <class H> static void run_script(const Script &sc, Device &m)
{
    configure(m, sc);
    H h(m);
    h.no_defer = sc.no_defer;
    h.q.has_costas_stream = sc.costas_stream;
    if (sc.below) h.q.costas_own_stream_below = (size_t)sc.below;
    for (const Cmd &c : sc.cmds) {
        const void *p = (const void *)(size_t)c.in;
        const size_t n = c.arg ? BIG : SMALL;
        switch (c.op) {
        case PF: m.note("PF", NO_STREAM, E_NONE, c.in, -1, c.arg); m.note("ret", NO_STREAM, E_NONE, c.in, -1, h.pf(p, n)); break;
        case GO: m.note("GO", NO_STREAM, E_NONE, c.in, -1, c.arg); m.note("ret", NO_STREAM, E_NONE, c.in, -1, h.go(p, n)); break;
        case RESET: m.note("RESET"); m.note("ret", NO_STREAM, E_NONE, 0, -1, h.reset()); break;
        case KEEP: m.note("KEEP", NO_STREAM, E_NONE, 0, -1, c.arg); m.note("ret", NO_STREAM, E_NONE, 0, -1, h.keep_stages(c.arg != 0)); break;
        case NOT_YET: m.not_yet[c.in] = c.arg; break;
        case REDO: m.redo[c.in] = true; break;
        case POLLS: m.done_polls = c.arg; break;
        }
    }
}

// ---------------------------------------------------------------- the clock stage's own scripts: what the handle's do not reach
// (the jobs' table only: these run the stage model directly, as a stage object's caller would)
enum StageOp { S_SLOT, S_OM, S_SCAN, S_LAUNCH, S_RESTART, S_BEGIN, S_FINISH, S_RUN, S_FLIP, S_FROM, S_ALT, S_RESET, S_VERDICT, S_LEAVE, S_ALLOW, S_BEHIND, S_SYNC, S_CAN, S_OVMIN };
struct StageCmd { StageOp op; size_t a; int b; };      // a: samples / job / carry / verdict / the stream to go behind; b: stream / ahead / sym_out
struct StageScript { const char *name; std::vector<StageCmd> cmds; };
constexpr size_t TINY = 3;

static std::vector<StageScript> stage_scripts()
{
    const int C = CHAIN_CALLER, W0 = CHAIN_WALK0, W1 = CHAIN_WALK1;
    std::vector<StageScript> v;
    // (buffers go round from the one of the last call: the first three slots of a new stage are 1, 2, 0; the producer writes on
    // the caller's stream, and what is launched on a walker stream goes behind it as the chain would put it: S_BEHIND)
    v.push_back({"three jobs in flight and a fourth slot", {{S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_SLOT, BIG, C},
        {S_BEHIND, C, W1}, {S_LAUNCH, 1, W1}, {S_BEHIND, C, W0}, {S_LAUNCH, 2, W0 | 8}, {S_BEHIND, C, W1}, {S_LAUNCH, 0, W1 | 8}, {S_BEGIN, BIG, C}, {S_SLOT, BIG, C}, {S_FINISH, 0, C}, {S_SLOT, BIG, C}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C},
        {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    v.push_back({"a slot over the history buffer", {{S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEHIND, C, W0}, {S_LAUNCH, 2, W0},
        {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_SLOT, BIG, C}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    v.push_back({"a chains call between overlap calls", {{S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_SLOT, SMALL, C}, {S_OM, SMALL, 0}, {S_SCAN, 0, C},
        {S_BEGIN, SMALL, C}, {S_FINISH, 0, C}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_SLOT, BIG, C}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    v.push_back({"restart of a walking job and of one in its slot", {{S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEHIND, C, W1}, {S_LAUNCH, 1, W1}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEHIND, C, W0}, {S_LAUNCH, 2, W0 | 8},
        {S_RESTART, 2, 0}, {S_RESTART, 2, 0}, {S_RESTART, 0, 0}, {S_BEHIND, C, W0}, {S_LAUNCH, 2, W0 | 8}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_RESTART, 2, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    v.push_back({"fallback, both flavours", {{S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_VERDICT, CLK_OV_FALLBACK, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_SLOT, BIG, C}, {S_OM, BIG, 0},
        {S_VERDICT, CLK_OV_FALLBACK_TO_CLOSURE, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    v.push_back({"the watchdog end", {{S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_VERDICT, CLK_OV_WATCHDOG, 0}, {S_BEGIN, BIG, C},
        {S_FINISH, 0, C}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_VERDICT, CLK_OV_WATCHDOG, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C},
        // (two calls have failed since the history was left: it lies in the buffer next in turn, which the first pass skips)
        {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    // (XRIT_OV_MIN in a build with the experiments: jobs shorter than the history a warm walker needs)
    v.push_back({"a job in front that is shorter than the history", {{S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_SLOT, BIG, C}, {S_CAN, 2, 0}, {S_OM, BIG, 0}, {S_CAN, 2, 0}, {S_BEHIND, C, W1}, {S_LAUNCH, 1, W1},
        {S_CAN, 2, 0}, {S_CAN, 1, 0}, {S_CAN, 0, 0}, {S_SYNC, 0, W1}, {S_SYNC, 0, C}, {S_RESET, 0, 0}, {S_OVMIN, 1000, 0}, {S_SLOT, 100000, C}, {S_OM, 100000, 0}, {S_SLOT, 100000, C}, {S_OM, 100000, 0},
        {S_BEHIND, C, W1}, {S_LAUNCH, 1, W1}, {S_CAN, 2, 0}, {S_BEGIN, 100000, C}, {S_FINISH, 0, C}, {S_CAN, 2, 0}, {S_BEGIN, 100000, C}, {S_FINISH, 0, C}}});
    v.push_back({"short input", {{S_SLOT, TINY, C}, {S_BEGIN, TINY, C}, {S_FINISH, 0, C}, {S_SLOT, TINY, C}, {S_BEGIN, TINY, C}, {S_FINISH, 0, C}, {S_LEAVE, 9, 0}, {S_SLOT, SMALL, C},
        {S_BEGIN, SMALL, C}, {S_FINISH, 0, C}, {S_SLOT, BIG, C}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    v.push_back({"begin with the wrong n, and with sym_out", {{S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEGIN, SMALL, C}, {S_BEGIN, BIG, C | 8}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    v.push_back({"reruns behind an overlap call", {{S_FLIP, 0, C}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_FLIP, 0, C}, {S_SLOT, BIG, C}, {S_OM, BIG, 0},
        {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_FROM, 7, C}, {S_FROM, 2000, C}, {S_LEAVE, 11, 0}, {S_ALT, 0, C}, {S_ALT, 0, C}, {S_SLOT, BIG, C}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C},
        {S_LEAVE, 4, 0}, {S_ALT, 0, C}, {S_FLIP, 0, C}, {S_SLOT, BIG, C}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    v.push_back({"reruns behind a chains call", {{S_SLOT, SMALL, C}, {S_BEGIN, SMALL, C}, {S_FINISH, 0, C}, {S_LEAVE, 8, 0}, {S_ALT, 0, C}, {S_FLIP, 0, C}, {S_FROM, 3, C}, {S_SLOT, SMALL, C},
        {S_BEGIN, SMALL, C}, {S_FINISH, 0, C}, {S_FLIP, 0, C}, {S_SLOT, BIG, C}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}}});
    // (the caller of reset() has waited for whatever walked ahead: xrit_demod_reset synchronises its streams)
    v.push_back({"reset with jobs in every state", {{S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEHIND, C, W1}, {S_LAUNCH, 1, W1}, {S_BEGIN, BIG, C}, {S_BEHIND, C, W0}, {S_LAUNCH, 2, W0 | 8}, {S_SLOT, BIG, C},
        {S_SYNC, 0, W0}, {S_SYNC, 0, W1}, {S_SYNC, 0, C}, {S_RESET, 0, 0}, {S_SLOT, BIG, C}, {S_OM, BIG, 0}, {S_BEGIN, BIG, C}, {S_FINISH, 0, C}, {S_SLOT, SMALL, C}, {S_OM, SMALL, 0}, {S_SCAN, 0, C}, {S_RESET, 0, 0}, {S_RUN, SMALL, C}}});
    v.push_back({"a stage object's calls", {{S_ALLOW, 0, 0}, {S_SLOT, BIG, C}, {S_RUN, BIG, C}, {S_SLOT, SMALL, C}, {S_RUN, SMALL, C}, {S_SLOT, TINY, C}, {S_RUN, TINY, C}, {S_ALLOW, 1, 0},
        {S_SLOT, BIG, C}, {S_RUN, BIG, C}}});
    return v;
}

static void run_stage_script(const StageScript &sc, Device &m)
{
    const Script plain{sc.name, 0, false, false, 0, {}};
    configure(m, plain);
    for (const StageCmd &c : sc.cmds) {
        const int stream = c.b & 7;
        const bool flag = (c.b & 8) != 0;
        switch (c.op) {
        case S_SLOT: (void)m.stage.input_slot(c.a, stream); break;
        case S_OM: m.om_slot(c.a); break;
        case S_SCAN: m.stage.om_scan(stream); break;
        case S_LAUNCH: (void)m.stage.ov_launch((int)c.a, stream, flag); break;
        case S_RESTART: (void)m.stage.ov_restart((int)c.a); break;
        case S_BEGIN: (void)m.stage.begin(c.a, flag, stream); break;
        case S_FINISH: m.jlog.order(O_HOST_STREAM, stream, 0); (void)m.stage.finish(stream); break;       // (finish() runs after the caller has synchronised)
        case S_CAN: m.jlog.say("can_launch_ahead job=%d: %d", (int)c.a, m.stage.can_launch_ahead((int)c.a) ? 1 : 0); break;
        case S_OVMIN: m.knobs.ov_min = (long long)c.a; break;
        case S_SYNC: m.jlog.order(O_HOST_STREAM, stream, 0); break;
        case S_BEHIND: m.jlog.order(O_RECORD, (int)c.a, E_COSTAS); m.jlog.order(O_WAIT, stream, E_COSTAS); break;
        case S_RUN: (void)m.stage.run(c.a, stream); break;
        case S_FLIP: (void)m.stage.redo_flipped(stream); break;
        case S_FROM: (void)m.stage.redo_from(c.a, stream); break;
        case S_ALT: (void)m.stage.make_alt(stream); break;
        case S_RESET: m.stage.reset(); break;
        case S_VERDICT: m.stage.verdict = (int)c.a; break;
        case S_LEAVE: m.stage.leave = (long)c.a; break;
        case S_ALLOW: m.knobs.ov_allow = c.a != 0; break;
        }
    }
}

// ---------------------------------------------------------------- the invariants, over one script's log
// Returns the names of the invariants the log breaks ("" if none).
static std::string invariants(const std::vector<Entry> &log)
{
    std::string broken;
    auto fail = [&](const char *what) { if (broken.find(what) == std::string::npos) { if (!broken.empty()) broken += ", "; broken += what; } };
    long last_fe = 0, last_costas = 0;
    bool costas_open = false;
    long set_user[2] = {0, 0};
    bool finished[MAX_IN] = {};
    bool waiting[MAX_IN] = {}, big[MAX_IN] = {};
    long arg_in = 0;
    long last_walk_serial = 0; int last_walk_stream = -1;
    auto behind_other_path = [&](long in) { for (long y = 1; y < in; ++y) if (waiting[y] && big[y] != big[in]) return true; return false; };
    for (const Entry &e : log) {
        if (e.op == "PF") { arg_in = e.in; big[e.in] = e.aux != 0; }
        else if (e.op == "GO") { waiting[e.in] = false; big[e.in] = e.aux != 0; }      // (the call's own input does not wait any more)
        else if (e.op == "ret" && arg_in) { if (e.aux == 0) waiting[arg_in] = true; arg_in = 0; }
        else if (e.op == "RESET") { for (auto &w : waiting) w = false; set_user[0] = set_user[1] = 0; costas_open = false; last_walk_stream = -1; }
        else if (e.op == "front_end") {
            if (e.in <= last_fe) fail("front ends in input order");     // (a reset starts a new stream, with later names)
            last_fe = e.in;
            const long prev = set_user[e.set];
            if (prev && !finished[prev]) fail("a set is free when its last user's Costas loop has been seen finished");
            set_user[e.set] = e.in;
            if (behind_other_path(e.in)) fail("nothing starts behind an input of the other path");
        } else if (e.op == "costas_begin") {
            if (e.in <= last_costas) fail("Costas loops in input order");
            if (costas_open) fail("never two Costas loops at once");
            last_costas = e.in; costas_open = true;
            if (behind_other_path(e.in)) fail("nothing starts behind an input of the other path");
        } else if (e.op == "costas_finish") {
            finished[e.in] = true; costas_open = false;
        } else if (e.op == "ov_launch" && (e.aux & 1)) {
            const long serial = e.aux / 2;
            if (e.stream != CHAIN_WALK0 + (int)(serial % 2)) fail("walkers of consecutive jobs alternate streams");
            if (last_walk_stream >= 0 && serial == last_walk_serial + 1 && e.stream == last_walk_stream) fail("walkers of consecutive jobs alternate streams");
            last_walk_serial = serial; last_walk_stream = e.stream;
        }
    }
    return broken;
}

// recorded sequences that break an invariant as the code stands: script, invariants
static const char *const KNOWN[][2] = {
    // XRIT_NO_DEFER: a small input is not deferred, so its front end starts at registration -- and, in front of it and in
    // order, the front end of the big input that still waited for its own call
    {"big then small, no_defer", "nothing starts behind an input of the other path"},
};

// ---------------------------------------------------------------- one row per branch of chain_next, both sides
struct RowFacts {
    bool done = true, ahead = true; unsigned long long serial = 0; int asked_done = 0, asked_ahead = 0;
    bool costas_event_done() { ++asked_done; return done; }
    unsigned long long ov_serial() { return serial; }
    bool can_launch_ahead(int) { ++asked_ahead; return ahead; }
};
static ChainStep first_step(ChainQueue &q, RowFacts &f, int limit = 1 << 30, bool busy = false)
{
    ChainScan sc;
    sc.costas_busy = busy;
    return chain_next(q, sc, f, limit);
}
static ChainQueue queue_of(int count, bool ov = true)
{
    ChainQueue q;
    for (int i = 0; i < count; ++i) { chain_stage(q, (const void *)(size_t)(i + 1), BIG, 0, ov); ++q.count; }
    return q;
}
static int check_steps()
{
    int rows = 0;
    RowFacts f;
    ChainStep st;
    // the empty queue, the limit, an input of the other path
    { ChainQueue q = queue_of(0); st = first_step(q, f); CHECK(st.kind == CHAIN_NONE, "empty"); ++rows; }
    { ChainQueue q = queue_of(1); st = first_step(q, f, 0); CHECK(st.kind == CHAIN_NONE, "limit 0"); ++rows; }
    { ChainQueue q = queue_of(1, false); st = first_step(q, f); CHECK(st.kind == CHAIN_NONE, "not eligible"); ++rows; }
    // front end: not launched / launched; the third input waits for the first one's loop
    { ChainQueue q = queue_of(1); st = first_step(q, f); CHECK(st.kind == CHAIN_FRONT_END && st.i == 0 && st.stream == CHAIN_FRONT, "front end"); ++rows; }
    { ChainQueue q = queue_of(1); q.in[0].launched = true; st = first_step(q, f); CHECK(st.kind == CHAIN_COSTAS_BEGIN, "launched: the loop next"); ++rows; }
    for (int fin = 0; fin < 2; ++fin) {
        ChainQueue q = queue_of(3);
        for (int i = 0; i < 2; ++i) { q.in[i].launched = q.in[i].costas_begun = q.in[i].costas_finished = q.in[i].walk_launched = true; q.in[i].ov_job = i; }
        q.in[0].costas_finished = fin != 0;
        f = RowFacts{};
        st = first_step(q, f);
        if (fin) CHECK(st.kind == CHAIN_FRONT_END && st.i == 2, "third front end once the first loop is seen finished");
        else CHECK(st.kind == CHAIN_COSTAS_LOOK && st.i == 0, "first loop looked at first");
        if (!fin) { f.done = false; st = first_step(q, f); CHECK(st.kind == CHAIN_NONE, "third front end held back (got %d for %d)", st.kind, st.i); }
        ++rows;
    }
    // the look: event complete / not yet (then nothing behind it begins a loop)
    for (int done = 0; done < 2; ++done) {
        ChainQueue q = queue_of(2);
        q.in[0].launched = q.in[0].costas_begun = true; q.in[0].costas_stream = CHAIN_WALK1; q.in[0].walk_launched = true; q.in[0].ov_job = 0;
        q.in[1].launched = true;
        q.costas_event_of = q.in[0].id;
        f = RowFacts{}; f.done = done != 0;
        st = first_step(q, f);
        if (done) CHECK(st.kind == CHAIN_COSTAS_LOOK && st.i == 0 && st.stream == CHAIN_WALK1 && st.event_of == q.in[0].id, "look");
        else CHECK(st.kind == CHAIN_NONE && f.asked_done == 1, "not yet: the input behind waits (got %d)", st.kind);
        ++rows;
    }
    // the restart: only after a loop that went on from the host, and only with a job
    for (int redone = 0; redone < 2; ++redone)
        for (int job = -1; job < 1; ++job) {
            ChainQueue q = queue_of(1);
            ChainInput &in = q.in[0];
            in.launched = in.costas_begun = in.walk_launched = true; in.ov_job = job;
            chain_costas_looked(in, redone != 0);
            ChainScan sc; sc.part = 2;
            f = RowFacts{}; f.ahead = false;
            st = chain_next(q, sc, f, 1 << 30);
            if (redone && job >= 0) { CHECK(st.kind == CHAIN_WALK_RESTART && st.stream == CHAIN_FRONT, "restart"); chain_walk_restarted(in); CHECK(!in.walk_launched && !in.restart_due, "restarted"); }
            else CHECK(st.kind == CHAIN_NONE, "no restart");
            ++rows;
        }
    // the loop's stream: a Costas stream / a small burst on its own walkers' stream (by the next job's serial) / the front ends'
    for (int cs = 0; cs < 2; ++cs)
        for (int small = 0; small < 2; ++small)
            for (unsigned long long serial = 4; serial < 6; ++serial) {
                ChainQueue q = queue_of(1);
                q.has_costas_stream = cs != 0;
                q.in[0].launched = true; q.in[0].io.length = small ? (2u << 20) : (16u << 20);
                f = RowFacts{}; f.serial = serial;
                st = first_step(q, f);
                const ChainStream want = cs ? CHAIN_COSTAS : small ? (serial + 1) % 2 ? CHAIN_WALK1 : CHAIN_WALK0 : CHAIN_FRONT;
                CHECK(st.kind == CHAIN_COSTAS_BEGIN && st.stream == want && st.wait_fe == (want != CHAIN_FRONT), "loop stream %d, want %d", st.stream, want);
                ++rows;
            }
    // ... and not while the stage is busy
    { ChainQueue q = queue_of(1); q.in[0].launched = true; f = RowFacts{}; st = first_step(q, f, 1 << 30, true); CHECK(st.kind == CHAIN_NONE, "stage busy"); ++rows; }
    // the walkers: begun, a job, not launched, the clock stage allows it -- each missing in turn
    for (int miss = 0; miss < 5; ++miss) {
        ChainQueue q = queue_of(1);
        ChainInput &in = q.in[0];
        in.launched = true; in.costas_begun = true; in.costas_finished = true; in.ov_job = miss == 1 ? -1 : 0; in.walk_launched = miss == 2; in.serial = 7;
        if (miss == 4) { in.costas_begun = false; }
        q.costas_event_of = 99;
        f = RowFacts{}; f.ahead = miss != 3;
        st = first_step(q, f, 1 << 30, miss == 4);
        if (miss == 0) CHECK(st.kind == CHAIN_WALK_LAUNCH && st.stream == CHAIN_WALK1 && st.event_of == 99, "walk launch");
        else CHECK(st.kind == CHAIN_NONE, "no walk launch (%d)", miss);
        ++rows;
    }
    // admission, defer, the path of a call, taking and popping
    { ChainQueue q = queue_of(2); CHECK(chain_room(q, true) == XRIT_AHEAD + 1 && chain_room(q, false) == 2, "room"); q.in[0].ov = false; CHECK(chain_room(q, true) == 2, "room behind a small one"); ++rows; }
    CHECK(chain_defer(true, false, false) && !chain_defer(true, true, false) && !chain_defer(false, false, false) && chain_defer(false, true, true), "defer"); ++rows;
    {
        ChainQueue q = queue_of(1);
        CHECK(chain_call_overlaps(q, true) && !chain_call_overlaps(q, false), "path");
        q.in[0].costas_begun = true; CHECK(!chain_call_overlaps(q, true), "begun under a relay: the chains path");
        q.in[0].ov_job = 1; CHECK(chain_call_overlaps(q, true), "begun as a job");
        ++rows;
    }
    {
        ChainQueue q = queue_of(3);
        CHECK(chain_front_is(q, (const void *)(size_t)1, BIG, 0) && !chain_front_is(q, (const void *)(size_t)2, BIG, 0) && !chain_front_is(q, (const void *)(size_t)1, SMALL, 0) && !chain_front_is(q, (const void *)(size_t)1, BIG, 1), "front");
        chain_pop(q);
        CHECK(q.count == 2 && q.in[0].id == 2 && q.in[1].id == 3, "pop");
        const ChainFrontEnd a = chain_front_end_take(q); chain_front_end_started(q, a.set);
        const ChainFrontEnd b = chain_front_end_take(q);
        CHECK(a.set == 0 && a.behind_set == -1 && b.set == 1 && b.behind_set == 0, "sets alternate");
        chain_reset(q);
        CHECK(q.count == 0 && q.last_fe_set == -1 && q.next_set == 0, "reset");
        ++rows;
    }
    // the chains path's moments
    {
        ChainQueue q = queue_of(1);
        CHECK(chain_start_under_relay(q) && chain_start_at_call(q) && chain_start_oldest_first(q) && chain_costas_first(q, false) && !chain_costas_first(q, true), "waiting");
        q.in[0].launched = true;
        CHECK(!chain_start_under_relay(q) && !chain_start_at_call(q) && !chain_start_oldest_first(q) && !chain_costas_first(q, false), "launched");
        q.count = 0;
        CHECK(!chain_start_under_relay(q) && !chain_start_oldest_first(q), "empty");
        CHECK(chain_costas_under_relay(true) && !chain_costas_under_relay(false), "the loop follows when the stage is idle");
        ++rows;
    }
    return rows;
}

// ---------------------------------------------------------------- the table
// ---------------------------------------------------------------- one row per branch of clock_jobs.h's decisions, both sides
static int check_job_rules()
{
    int rows = 0;
    const int need = 4000;
    auto walking = [](ClockJobs &c, int q, unsigned long long serial, size_t n, int padN) {
        ClockJob &j = c.job[q];
        j.state = CLK_JOB_WALKING; j.serial = serial; j.n = n; j.padN = padN; j.om_ext = j.om_scanned = true;
    };
    // the buffer: round from the last call's; busy: the call in flight, any job; the history skipped unless nothing else is free
    { ClockJobs c; ClockSlotPick p = c.pick_buffer(); CHECK(p.b == 1 && !p.forget, "first buffer"); c.xb = 2; p = c.pick_buffer(); CHECK(p.b == 0, "round"); ++rows; }
    { ClockJobs c; c.xb = 0; c.in_flight = true; c.job[1].state = CLK_JOB_SLOT; ClockSlotPick p = c.pick_buffer(); CHECK(p.b == 2, "a job's buffer is busy");
      c.in_flight = false; c.job[2].state = CLK_JOB_FINALIZING; p = c.pick_buffer(); CHECK(p.b == 0, "the last call's buffer is free once it has finished"); ++rows; }
    for (int others = 0; others < 2; ++others) {
        ClockJobs c; c.xb = 0; c.hist = ClockHistory{1, 9000, 1};
        if (others) c.job[2].state = CLK_JOB_SLOT;
        c.in_flight = others != 0;
        const ClockSlotPick p = c.pick_buffer();
        if (others) CHECK(p.b == 1 && p.forget, "the history buffer when nothing else is free"); else CHECK(p.b == 2 && !p.forget, "the history buffer skipped");
        ++rows;
    }
    { ClockJobs c; c.in_flight = true; c.job[1].state = c.job[2].state = CLK_JOB_WALKING; const ClockSlotPick p = c.pick_buffer(); CHECK(p.b < 0 && strstr(p.err, "no free sample buffer"), "refused"); ++rows; }
    for (int st = CLK_JOB_SLOT; st <= CLK_JOB_FINALIZING; ++st) {
        ClockJobs c; c.job[2].state = (ClockJobState)st; c.job[2].hist_src = 1; c.job[0].state = CLK_JOB_WALKING; c.job[0].hist_src = 2;
        const ClockSlotPick p = c.pick_buffer();
        CHECK(p.b == 1 && p.wait_guess[2] == (st >= CLK_JOB_WALKING) && !p.wait_guess[0], "ev_guess of the jobs that read the buffer, once launched");
        ++rows;
    }
    // handing out: a job or not
    { ClockJobs c; c.hand_out(1, 500, false); CHECK(c.x_pending == 1 && c.setting_up == -1 && c.job[1].state == CLK_JOB_FREE && c.serials == 0, "no job");
      c.job[2].om_ext = c.job[2].om_scanned = true; c.hand_out(2, 700, true);
      CHECK(c.x_pending == 2 && c.setting_up == 2 && c.job[2].state == CLK_JOB_SLOT && c.job[2].n == 700 && c.job[2].serial == 1 && !c.job[2].om_ext && !c.job[2].om_scanned, "a job"); ++rows; }
    // the statistic: job-owned / stage-owned; the scan
    { ClockJobs c; c.om_noted(5, 128); CHECK(c.om_owner() == -1 && c.om_ext && c.om_nb == 5 && c.om_BL == 128 && c.om_scan_here(), "the stage's"); c.om_scan_done(); CHECK(c.om_scanned, "scanned");
      c.om_rewritten(); CHECK(!c.om_scanned, "rewritten"); c.om_nb = 0; CHECK(!c.om_scan_here(), "nothing to scan");
      c.hand_out(1, 700, true); c.om_noted(7, 256); CHECK(c.om_owner() == 1 && c.job[1].om_ext && c.job[1].nb == 7 && c.om_nb == 0 && !c.om_scan_here(), "the job's: not scanned here");
      c.job[1].state = CLK_JOB_WALKING; CHECK(c.om_owner() == -1, "a launched job takes no statistic"); ++rows; }
    // the job in front; launching ahead -- each condition missing in turn
    for (int miss = 0; miss < 7; ++miss) {
        ClockJobs c;
        walking(c, 1, 4, 100000, miss == 5 ? 0 : need);
        c.job[2].state = CLK_JOB_SLOT; c.job[2].serial = 5; c.job[2].om_ext = miss != 1;
        if (miss == 2) c.job[1].serial = 3;
        if (miss == 3) c.job[1].om_scanned = false;
        if (miss == 4) c.job[1].state = CLK_JOB_SLOT;
        if (miss == 5) c.job[1].n = need - 1;
        if (miss == 6) c.job[2].state = CLK_JOB_WALKING;
        CHECK(c.front_of(2) == (miss == 2 ? -1 : 1), "front (%d)", miss);
        CHECK(c.can_launch_ahead(2, need) == (miss == 0), "ahead (%d)", miss);
        ++rows;
    }
    { ClockJobs c; CHECK(!c.can_launch_ahead(-1, need) && !c.can_launch_ahead(NXB, need) && c.serial_of(-1) == 0, "no such job"); c.job[0].state = CLK_JOB_FREE; c.job[0].serial = 4; c.job[1].serial = 5;
      CHECK(c.front_of(1) == -1, "a free job is in front of nothing"); ++rows; }
    // the history of a launch
    { ClockJobs c; walking(c, 1, 4, 100000, need); c.job[2].state = CLK_JOB_SLOT; c.job[2].serial = 5; c.hist = ClockHistory{0, 50000, -1};
      ClockLaunchHist h = c.launch_hist(2, true, need); CHECK(!h.err && h.xb == 1 && h.job == 1 && h.len == 100000 + (size_t)need && h.wait_guess == 1 && h.have, "ahead: the job in front");
      h = c.launch_hist(2, false, need); CHECK(h.xb == 0 && h.job == -1 && h.wait_guess == -1 && !h.have, "not ahead: the stage's record; no curve, no history");
      c.hist = ClockHistory{1, 100000, 1}; h = c.launch_hist(2, false, need); CHECK(h.have, "history with its job");
      c.hist.len = need - 1; CHECK(!c.launch_hist(2, false, need).have, "too short"); c.hist.len = need; c.job[1].om_scanned = false; CHECK(!c.launch_hist(2, false, need).have, "curve not in place");
      c.hist.forget(); CHECK(c.hist.xb == -1 && c.hist.len == 0 && c.hist.job == -1 && !c.launch_hist(2, false, need).have, "forgotten");
      c.job[2].serial = 9; CHECK(c.launch_hist(2, true, need).err != nullptr, "ahead with no job in front"); ++rows; }
    { ClockOvPlan plan; plan.padN = need; ClockLaunchHist h; h.xb = 1; h.job = 1; h.len = need;
      CHECK(!ClockJobs::hist_refusal(h, plan), "fits"); h.len = need - 1; CHECK(ClockJobs::hist_refusal(h, plan), "short"); h.len = need; h.job = -1; CHECK(ClockJobs::hist_refusal(h, plan), "no job");
      h.job = 2; CHECK(ClockJobs::hist_refusal(h, plan), "another job's buffer"); plan.w0_carried = true; CHECK(!ClockJobs::hist_refusal(h, plan), "walker 0 from the carried state asks for none"); ++rows; }
    // launched; restart
    for (int carried = 0; carried < 2; ++carried) {
        ClockJobs c; c.hand_out(2, 700, true);
        ClockOvPlan plan; plan.w0_carried = carried != 0; plan.padN = 17;
        c.planned(2, plan, !carried);
        ClockLaunchHist h; h.xb = 1;
        c.launched(2, h, carried ? 0 : 3, 256);
        const ClockJob &j = c.job[2];
        CHECK(j.state == CLK_JOB_WALKING && j.om_ext && j.om_scanned == !carried && j.hist_src == (carried ? -1 : 1) && j.ahead == !carried && j.padN == 17, "launched");
        CHECK(c.restart_waits(2) && !c.restart_waits(1) && !c.restart_waits(-1), "waits for walkers at work only");
        c.restarted(2); CHECK(j.state == CLK_JOB_SLOT && !j.om_scanned && j.om_ext && !c.restart_waits(2), "back in its slot");
        c.restarted(1); c.restarted(NXB); CHECK(c.job[1].state == CLK_JOB_FREE, "a free job stays free");
        ++rows;
    }
    // the call's job: the oldest in SLOT / WALKING; the refusals
    { ClockJobs c; c.carry = 6; c.redo_ok = true; c.ov_cur = 2; c.call_reset(900); CHECK(c.prev_carry == 6 && c.prev_n == 900 && !c.redo_ok && c.ov_cur == -1, "call_reset");
      CHECK(!c.call_job(900, false) && c.ov_cur == -1, "no job: the chains");
      c.job[0].state = CLK_JOB_FINALIZING; c.job[0].serial = 1; c.job[1].state = CLK_JOB_WALKING; c.job[1].serial = 3; c.job[1].n = 900; c.job[2].state = CLK_JOB_SLOT; c.job[2].serial = 2; c.job[2].n = 800;
      CHECK(c.call_job(900, false) && c.ov_cur == 2, "the oldest waiting job, and its n"); c.ov_cur = -1; CHECK(!c.call_job(800, false) && c.ov_cur == 2, "fits"); c.ov_cur = -1;
      CHECK(c.call_job(800, true), "sym_out"); ++rows; }
    // what the two begins set
    { ClockJobs c; c.ov_cur = 2; c.x_pending = 2; c.setting_up = 2; c.om_ext = c.om_scanned = true; c.begun_overlap();
      CHECK(c.xb == 2 && c.x_pending == -1 && c.setting_up == -1 && c.in_flight && !c.om_ext && !c.om_scanned, "begun_overlap");
      c.carry = 5; c.job[2].padN = 100; c.job[2].w0_ii = 0; c.w0_known(2); CHECK(c.job[2].w0_ii == 0, "not ahead: the plan knew"); c.job[2].ahead = true; c.w0_known(2); CHECK(c.job[2].w0_ii == 95, "ahead: known now");
      c.finalizing(2); CHECK(c.job[2].state == CLK_JOB_FINALIZING, "finalizing"); ++rows; }
    { ClockJobs c; c.xb = 0; c.x_pending = 2; c.chains_buffer(false); CHECK(c.xb == 0 && c.x_pending == 2, "samples elsewhere: nothing taken"); c.chains_buffer(true); CHECK(c.xb == 2 && c.x_pending == -1, "the slot handed out");
      c.chains_buffer(true); CHECK(c.xb == 2, "none handed out: the last buffer");
      c.om_ext = true; ClockOm o = c.begun_chains(); CHECK(c.in_flight && o.ext && !o.scanned && !c.om_ext, "statistic only"); c.om_ext = c.om_scanned = true; o = c.begun_chains(); CHECK(o.ext && o.scanned && !c.om_scanned, "and curve");
      c.om_scanned = true; o = c.begun_chains(); CHECK(!o.ext && !o.scanned, "a curve without its statistic is none"); ++rows; }
    // the ends of a call
    { ClockJobs c; c.in_flight = true; c.call_ended(); CHECK(!c.in_flight, "ended"); c.flip(); CHECK(c.cur == 1, "flip"); CHECK(!c.carried(1024) && c.carry == 1024, "carry fits");
      const char *e = c.carried(1025); CHECK(e && strstr(e, "1025"), "carry beyond the hand-over buffer"); c.ended_short(3); CHECK(c.carry == 3 && c.cur == 0 && !c.redo_ok, "short"); ++rows; }
    { ClockJobs c; c.job[1].state = CLK_JOB_FINALIZING; c.job[1].padN = 10; c.job[1].n = 90; c.ov_cur = 1; c.xb = 0;
      CHECK(c.overlap_released() == 1 && c.ov_cur == -1 && c.job[1].state == CLK_JOB_FREE && c.xb == 0 && c.hist.xb == -1, "released: free, no history yet");
      c.ended_overlap(1); CHECK(c.hist.xb == 1 && c.hist.len == 100 && c.hist.job == 1 && c.redo_ok, "taken");
      c.hist.forget(); c.redo_ok = false; c.job[1].state = CLK_JOB_FINALIZING; c.ov_cur = 1;
      CHECK(c.overlap_fell_back() == 1 && c.xb == 1 && c.job[1].state == CLK_JOB_FREE && c.hist.xb == -1, "fell back, before the chains: its buffer is the call's");
      c.prev_carry = 4; c.prev_n = 90; c.ended_chains(false); CHECK(c.redo_ok && c.hist.xb == -1, "the chains on samples elsewhere leave the history alone");
      c.ended_fallback(1); CHECK(c.hist.xb == 1 && c.hist.len == 100 && c.hist.job == 1, "fell back, after the chains");
      c.xb = 2; c.ended_chains(true); CHECK(c.hist.xb == 2 && c.hist.len == 94 && c.hist.job == -1, "chains on their own buffer: history without a job"); ++rows; }
    // stepping back
    for (int alt = 0; alt < 2; ++alt) {
        ClockJobs c; c.cur = 1; c.carry = 9; c.prev_carry = 4; c.alt_carry = 6; c.alt_valid = alt != 0; c.hist = ClockHistory{1, 100, 1};
        CHECK(c.step_back_flipped() == (alt != 0) && c.cur == 0 && c.carry == (alt ? 6u : 4u) && !c.alt_valid && c.hist.xb == -1 && c.hist.job == -1 && c.hist.len == 0, "step back, flipped");
        ++rows;
    }
    { ClockJobs c; c.cur = 0; c.carry = 9; c.alt_valid = true; c.hist = ClockHistory{1, 100, 1}; c.step_back_from(7);
      CHECK(c.cur == 1 && c.carry == 7 && !c.alt_valid && c.hist.xb == -1, "step back, from a record");
      c.redo_ok = true; c.carry = 12; c.alt_made(9); CHECK(c.alt_carry == 12 && c.carry == 9 && c.alt_valid && !c.redo_ok, "alt made"); ++rows; }
    // reset
    { ClockJobs c; for (int q = 0; q < NXB; ++q) { c.job[q].state = (ClockJobState)(q + 1); c.job[q].serial = 7 + q; }
      c.cur = 1; c.carry = 5; c.x_pending = 2; c.setting_up = 2; c.hist = ClockHistory{1, 100, 1}; c.om_ext = c.om_scanned = c.in_flight = c.redo_ok = c.alt_valid = true; c.prev_carry = 3; c.prev_n = 8; c.xb = 2; c.serials = 9;
      c.reset();
      CHECK(c.cur == 0 && c.carry == 0 && c.x_pending == -1 && c.setting_up == -1 && c.hist.xb == -1 && !c.om_ext && !c.om_scanned && !c.in_flight && !c.redo_ok && !c.alt_valid && c.prev_carry == 0 && c.prev_n == 0, "reset");
      CHECK(c.job[0].state == CLK_JOB_FREE && c.job[1].state == CLK_JOB_FREE && c.job[2].state == CLK_JOB_FREE, "every job free");
      CHECK(c.xb == 2 && c.serials == 9 && c.job[2].serial == 9, "buffers and serials go on from where they are"); ++rows; }
    return rows;
}

// ---------------------------------------------------------------- the ordering count, over one script's accesses
// Every read of a resource must be ordered behind its last write, every write behind the last write and the reads since: by
// the same stream, by a wait for an event recorded behind it, or by the host (a synchronise, or a completed query of such an
// event, before the host enqueued the access).  Returns the accesses ordered by none of the three; names them in `what`.
static int unordered_accesses(const char *script, const std::vector<Ord> &ord, std::vector<std::string> &what)
{
    static const char *const RES[] = {"new samples", "pad", "job statistic", "job curve", "S / segs / stage", "st / tail", "stage statistic"};
    constexpr int NS = 5;
    typedef long Know[NS];
    Know know[NS] = {}, host = {}, ev[EV_COUNT] = {};
    long seq[NS] = {};
    struct Acc { int stream; long seq; };
    Acc writer[R_COUNT];
    std::vector<Acc> readers[R_COUNT];
    for (Acc &w : writer) w = Acc{-1, 0};
    auto merge = [](Know into, const Know from) { for (int t = 0; t < NS; ++t) if (from[t] > into[t]) into[t] = from[t]; };
    int count = 0;
    for (const Ord &o : ord) {
        const int s = o.stream;
        if (o.kind == O_HOST_EVENT) { merge(host, ev[o.id]); continue; }
        if (o.kind == O_HOST_STREAM) { merge(host, know[s]); continue; }
        merge(know[s], host);               // (the host enqueues it after everything it has waited for)
        know[s][s] = ++seq[s];
        if (o.kind == O_RECORD) { memcpy(ev[o.id], know[s], sizeof(Know)); continue; }
        if (o.kind == O_WAIT) { merge(know[s], ev[o.id]); continue; }
        auto behind = [&](const Acc &a, const char *as) {
            if (a.stream < 0 || know[s][a.stream] >= a.seq) return;
            ++count;
            const int r = o.id < R_ST ? o.id / NXB : o.id < R_OM ? 5 : 6;
            char b[256];
            snprintf(b, sizeof b, "%s: %s of %s %d on %s is not ordered behind its last %s on %s", script, o.kind == O_READ ? "read" : "write", RES[r],
                     o.id < R_ST ? o.id % NXB : o.id - R_ST, STREAM_NAME[s], as, STREAM_NAME[a.stream]);
            what.push_back(b);
        };
        behind(writer[o.id], "write");
        if (o.kind == O_READ) readers[o.id].push_back(Acc{s, seq[s]});
        else {
            for (const Acc &a : readers[o.id]) behind(a, "read");
            readers[o.id].clear();
            writer[o.id] = Acc{s, seq[s]};
        }
    }
    return count;
}

static std::vector<std::string> read_table(const char *path)
{
    std::vector<std::string> table;
    FILE *fp = fopen(path, "r");
    if (!fp) { printf("cannot open %s\n", path); exit(2); }
    char line[1024];
    while (fgets(line, sizeof line, fp)) {
        size_t len = strlen(line);
        while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
        if (len && line[0] != '#') table.push_back(line);
    }
    fclose(fp);
    return table;
}
// one script's lines against the table from `at` on ("script NAME", then its lines).  Returns whether they are the same;
// names the first line that differs
static bool same_as_table(const std::vector<std::string> &table, size_t &at, const char *name, const std::vector<std::string> &lines)
{
    const std::string head = std::string("script ") + name;
    CHECK(at < table.size() && table[at] == head, "%s: the table has '%s' here", head.c_str(), at < table.size() ? table[at].c_str() : "<end>");
    ++at;
    bool same = true;
    for (const std::string &l : lines) {
        if (at >= table.size() || table[at] != l) {
            if (same) CHECK(false, "%s: line %zu is '%s', recorded '%s'", name, at, l.c_str(), at < table.size() ? table[at].c_str() : "<end>");
            same = false;
        }
        if (same) ++at;
    }
    if (!same) while (at < table.size() && table[at].compare(0, 7, "script ") != 0) ++at;
    return same;
}

#ifndef CHAIN_CHECK_NO_MAIN
int main(int argc, char **argv)
{
    if (argc < 3) { printf("usage: chain_host_check PIPELINE_TABLE JOBS_TABLE\n"); return 2; }
    const std::vector<std::string> table = read_table(argv[1]), jtable = read_table(argv[2]);
    size_t at = 0, jat = 0, steps = 0, jrows = 0;
    int unordered = 0;
    std::vector<std::string> unordered_what;
    int known_seen = 0, other_owner = 0;      // other_owner: walkers enqueued behind ev_costas while it stood for another input's loop
    const std::vector<Script> all = scripts();
    for (const Script &sc : all) {
        Device m;
        run_script<Handle>(sc, m);
        std::vector<std::string> lines;
        for (const Entry &e : m.log) lines.push_back(e.text());
        (void)same_as_table(table, at, sc.name, lines);
        (void)same_as_table(jtable, jat, sc.name, m.jlog.lines);
        jrows += m.jlog.lines.size();
        unordered += unordered_accesses(sc.name, m.jlog.ord, unordered_what);
        long loop_of[64] = {};      // by job serial: the input
        for (size_t i = 0; i < m.log.size(); ++i) {
            const Entry &e = m.log[i];
            if (e.op == "costas_begin" && e.aux > 0 && e.aux < 64) loop_of[e.aux] = e.in;
            if (e.op == "wait" && e.ev == E_COSTAS && i + 1 < m.log.size() && m.log[i + 1].op == "ov_launch" && loop_of[m.log[i + 1].aux / 2] != e.in) ++other_owner;
        }
        steps += m.log.size();
        const std::string broken = invariants(m.log);
        const char *known = nullptr;
        for (auto &k : KNOWN) if (k[0] && !strcmp(k[0], sc.name)) known = k[1];
        if (known) { ++known_seen; CHECK(broken == known, "%s: breaks '%s', listed with '%s'", sc.name, broken.c_str(), known); }
        else CHECK(broken.empty(), "%s: breaks '%s'", sc.name, broken.c_str());
    }
    CHECK(at == table.size(), "the table has %zu more lines", table.size() - at);
    const std::vector<StageScript> stage_all = stage_scripts();
    for (const StageScript &sc : stage_all) {
        Device m;
        run_stage_script(sc, m);
        (void)same_as_table(jtable, jat, sc.name, m.jlog.lines);
        jrows += m.jlog.lines.size();
        unordered += unordered_accesses(sc.name, m.jlog.ord, unordered_what);
    }
    CHECK(jat == jtable.size(), "the jobs' table has %zu more lines", jtable.size() - jat);
    const int rows = check_steps();
    const int jrules = check_job_rules();
    for (const std::string &w : unordered_what) printf("unordered: %s\n", w.c_str());      // (a finding, not a failure: DESIGN.md section 11)
    if (g_fail) { printf("chain_host_check: %d failures\n", g_fail); return 1; }
    printf("chain_host_check: %zu scripts, %zu logged calls against the recorded table, %d known invariant breaks, %d walker waits behind another input's event, %d rule rows; "
           "clock jobs: %zu scripts, %zu rows against the recorded table, %d known differences, %d rule rows, %d accesses ordered by nothing: ok\n",
           all.size(), steps, known_seen, other_owner, rows, all.size() + stage_all.size(), jrows, 0, jrules, unordered);
    return 0;
}
#endif
