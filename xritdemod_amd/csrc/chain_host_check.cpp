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

struct Device {
    std::vector<Entry> log;
    void note(const char *op, int stream = NO_STREAM, int ev = E_NONE, long in = 0, int set = -1, long aux = 0) { log.push_back(Entry{op, stream, ev, in, set, aux}); }
    // ---- scripted answers
    int not_yet[MAX_IN] = {};       // looks at ev_costas that find the loop of input k still at work
    bool redo[MAX_IN] = {};         // the loop of input k does not close in its batch: the host continues it
    int done_polls = 0;             // looks at ev_done that find the call's walkers still at work
    // ---- events: whose Costas loop ev_costas was last recorded behind (the device's own view)
    long costas_owner = 0;
    void wait(int stream, int ev) { note("wait", stream, ev, ev == E_COSTAS ? costas_owner : 0); }
    void record(int stream, int ev) { if (ev == E_COSTAS) costas_owner = costas_in; note("record", stream, ev, ev == E_COSTAS ? costas_owner : 0); }
    void sync_event(int ev) { if (ev == E_COSTAS && costas_owner > 0) not_yet[costas_owner] = 0; note("sync_event", NO_STREAM, ev, ev == E_COSTAS ? costas_owner : 0); }
    void sync_stream(int stream) { note("sync_stream", stream); }
    bool query(int ev)
    {
        bool done = true;
        if (ev == E_COSTAS && costas_owner > 0 && not_yet[costas_owner] > 0) { --not_yet[costas_owner]; done = false; }
        if (ev == E_DONE && done_polls > 0) { --done_polls; done = false; }
        note("query", NO_STREAM, ev, ev == E_COSTAS ? costas_owner : 0, -1, done ? 1 : 0);
        return done;
    }
    // ---- the front end (input k's samples "pointer" is k)
    void front_end(int stream, long in, int set) { note("front_end", stream, E_NONE, in, set); }
    // ---- the Costas stage
    long costas_in = 0;             // the input of the loop begun last
    bool costas_out = false;        // ... which has not been looked at
    void costas_begin(int stream, long in) { costas_in = in; costas_out = true; note("costas_begin", stream, E_NONE, in, -1, ov_job >= 0 ? (long)ov[ov_job].serial : 0); }
    bool costas_finish(int stream)  // returns: redone
    {
        const bool r = redo[costas_in];
        redo[costas_in] = false;
        costas_out = false;
        note("costas_finish", stream, E_NONE, costas_in, -1, r ? 1 : 0);
        return r;
    }
    // ---- the clock stage: its overlap jobs (ClockStage::input_slot, om_slot, ov_launch, ov_restart, begin, finish)
    ClockKnobs knobs;
    size_t xpad = 1024;
    struct Job { int state = 0; bool om_ext = false, om_scanned = false; unsigned long long serial = 0; } ov[XRIT_AHEAD + 1];
    int ov_job = -1, ov_cur = -1, xb = 0;
    unsigned long long ov_serial = 0;
    std::function<int(int)> before_relay;
    void input_slot(size_t n)
    {
        int b = -1;
        for (int q = 0; q <= XRIT_AHEAD && b < 0; ++q) { const int c = (xb + 1 + q) % (XRIT_AHEAD + 1); if (ov[c].state == 0) b = c; }
        if (b < 0) b = xb;
        ov_job = -1;
        if (clock_ov_eligible(knobs, xpad, false, n)) { ov[b] = Job{}; ov[b].state = 1; ov[b].serial = ++ov_serial; ov_job = b; }
        else xb = b;
    }
    void om_slot() { if (ov_job >= 0 && ov[ov_job].state == 1) ov[ov_job].om_ext = true; }
    bool ov_can_launch_ahead(int job) const
    {
        if (job < 0 || job > XRIT_AHEAD || ov[job].state != 1 || !ov[job].om_ext) return false;
        for (int q = 0; q <= XRIT_AHEAD; ++q)
            if (q != job && ov[q].state >= 1 && ov[q].serial + 1 == ov[job].serial) return ov[q].om_scanned && ov[q].state >= 2;
        return false;
    }
    void ov_launch(int job, int stream, bool ahead) { ov[job].om_ext = ov[job].om_scanned = true; ov[job].state = 2; note("ov_launch", stream, E_NONE, 0, -1, (long)ov[job].serial * 2 + (ahead ? 1 : 0)); }
    void ov_restart(int job, int stream) { if (ov[job].state >= 1) { ov[job].state = 1; ov[job].om_scanned = false; } note("ov_restart", stream, E_NONE, 0, -1, (long)ov[job].serial); }
    int clock_begin(size_t n, int stream)
    {
        unsigned long long first = ~0ull;
        ov_cur = -1;
        for (int q = 0; q <= XRIT_AHEAD; ++q)
            if ((ov[q].state == 1 || ov[q].state == 2) && ov[q].serial < first) { first = ov[q].serial; ov_cur = q; }
        if (ov_cur >= 0) {
            xb = ov_cur; ov_job = -1;
            if (ov[ov_cur].state == 1) ov_launch(ov_cur, stream, false);
            ov[ov_cur].state = 3;
            note("clock_begin_overlap", stream, E_NONE, 0, -1, (long)ov[ov_cur].serial);
            return 0;
        }
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
    void clock_finish(int stream) { if (ov_cur >= 0) { ov[ov_cur].state = 0; ov_cur = -1; } note("clock_finish", stream); }
    void clock_reset() { for (auto &j : ov) j.state = 0; ov_job = ov_cur = -1; note("stages_reset"); }
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
        m.input_slot(io.length);
        m.om_slot();
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
        unsigned long long ov_serial() { return h->m.ov_serial; }
        bool can_launch_ahead(int job) { return h->m.ov_can_launch_ahead(job); }
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
                chain_costas_begun(q, f, st.stream, nullptr, m.ov_job, m.ov_job >= 0 ? m.ov[m.ov_job].serial : 0);
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
#ifndef CHAIN_CHECK_NO_MAIN
int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: chain_host_check TABLE\n"); return 2; }
    FILE *fp = fopen(argv[1], "r");
    if (!fp) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<std::string> table;
    char line[256];
    while (fgets(line, sizeof line, fp)) {
        size_t len = strlen(line);
        while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
        if (len && line[0] != '#') table.push_back(line);
    }
    fclose(fp);
    size_t at = 0, steps = 0;
    int known_seen = 0, other_owner = 0;      // other_owner: walkers enqueued behind ev_costas while it stood for another input's loop
    const std::vector<Script> all = scripts();
    for (const Script &sc : all) {
        Device m;
        run_script<Handle>(sc, m);
        const std::string head = std::string("script ") + sc.name;
        CHECK(at < table.size() && table[at] == head, "%s: the table has '%s' here", head.c_str(), at < table.size() ? table[at].c_str() : "<end>");
        ++at;
        bool same = true;
        for (const Entry &e : m.log) {
            if (at >= table.size() || table[at] != e.text()) {
                if (same) CHECK(false, "%s: step %zu is '%s', recorded '%s'", sc.name, at, e.text().c_str(), at < table.size() ? table[at].c_str() : "<end>");
                same = false;
            }
            if (same) ++at;
        }
        long loop_of[64] = {};      // by job serial: the input
        for (size_t i = 0; i < m.log.size(); ++i) {
            const Entry &e = m.log[i];
            if (e.op == "costas_begin" && e.aux > 0 && e.aux < 64) loop_of[e.aux] = e.in;
            if (e.op == "wait" && e.ev == E_COSTAS && i + 1 < m.log.size() && m.log[i + 1].op == "ov_launch" && loop_of[m.log[i + 1].aux / 2] != e.in) ++other_owner;
        }
        if (!same) while (at < table.size() && table[at].compare(0, 7, "script ") != 0) ++at;
        steps += m.log.size();
        const std::string broken = invariants(m.log);
        const char *known = nullptr;
        for (auto &k : KNOWN) if (k[0] && !strcmp(k[0], sc.name)) known = k[1];
        if (known) { ++known_seen; CHECK(broken == known, "%s: breaks '%s', listed with '%s'", sc.name, broken.c_str(), known); }
        else CHECK(broken.empty(), "%s: breaks '%s'", sc.name, broken.c_str());
    }
    CHECK(at == table.size(), "the table has %zu more lines", table.size() - at);
    const int rows = check_steps();
    if (g_fail) { printf("chain_host_check: %d failures\n", g_fail); return 1; }
    printf("chain_host_check: %zu scripts, %zu logged calls against the recorded table, %d known invariant breaks, %d walker waits behind another input's event, %d rule rows: ok\n",
           all.size(), steps, known_seen, other_owner, rows);
    return 0;
}
#endif
