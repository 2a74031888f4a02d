// chain_pipeline.h -- what the chain handle (demod.cpp) decides about its inputs in flight, as plain C++ (no HIP headers):
// which registered input may start what, on which stream, into which of the two sets of front-end buffers, behind which
// event.  Records and pure functions: no allocation, no launch.  demod.cpp performs the steps with HIP and writes the
// outcomes back; chain_host_check.cpp holds the rules against tables recorded from the code they were taken out of, under
// sanitizers (make chain-host-check).
//
// ---- the streams of a handle, what runs on each, and which event orders it (DESIGN.md section 6 has the same table)
//
//   stream        runs                                                    waits for                      records
//   CHAIN_CALLER  a plain call's front end                                ev_fe[last front end's set]    ev_fe[set]
//   (the call's)  the chains path's Costas loop and clock recovery        ev_fe[set] (front end ran      ev_costas (only when the next
//                                                                         ahead, its Costas loop not)    input waits for the relay)
//                 the relay kernels                                       --                             ev_relay in front of them
//                 an overlap call's joints / output (ClockStage::begin),  the walkers' own event         ev_done
//                 its walkers when nothing launched them ahead            (ClockStage)
//                 a registration                                          --                             ev_ready
//   CHAIN_FRONT   the front end of a registered input                     ev_ready, ev_relay (started    ev_fe[set]
//   (stream2)                                                             under the relay), ev_fe[last]
//                 the Costas loop behind it: chains path under the relay; (stream order)                 ev_costas
//                 overlap path, bursts of costas_own_stream_below circuit
//                 samples and more
//   CHAIN_COSTAS  the overlap path's Costas loops with cfg.front_exact 2  ev_fe[set]                     ev_costas
//   (stream_c)
//   CHAIN_WALK0/1 the walkers of an overlap job launched ahead:           ev_costas                      (ClockStage's own)
//   (stream3[])   job serial % 2
//                 the overlap path's Costas loop of a burst below         ev_fe[set]                     ev_costas
//                 costas_own_stream_below: the stream its own walkers
//                 will take
//
// There is ONE ev_costas per handle: it is recorded again for every Costas loop that starts.  ChainQueue::costas_event_of
// names the input it was last recorded for; a step that waits for the event carries that name (ChainStep::event_of), so
// that a wait for another input's loop can be seen.
#pragma once

#include <stddef.h>

#include "clock_jobs.h"     // XRIT_AHEAD: inputs that may wait behind the call in progress
#include "clock_plan.h"

namespace xrit {

enum ChainStream { CHAIN_CALLER, CHAIN_FRONT, CHAIN_COSTAS, CHAIN_WALK0, CHAIN_WALK1 };
constexpr int CHAIN_WALK_STREAMS = 2;

// what a front end leaves for the loops behind it (the pointers are the device's: opaque here)
struct ChainSlice {
    size_t length = 0;          // circuit-rate samples
    const void *rrc = nullptr;  // float2: the matched filter's output
    bool stat_ready = false;
    int set = 0;                // which set of front-end buffers
    const void *agc_flag = nullptr;     // float: the AGC guard flag of THIS front end (the stage's slot moves on with the next)
    bool exact = false;         // this call's front end is the bit-exact one (cfg.front_exact = 2, or 0 on a call below the big-burst size)
};

// an input registered ahead of its process call (xrit_demod_prefetch_device), or an overlap call's own
struct ChainInput {
    const void *samples = nullptr; size_t n = 0; int type = 0;
    long id = 0;                    // which registration of the handle this is (ChainQueue::costas_event_of names inputs by it)
    bool ov = false;                // its clock recovery walks overlapping blocks: everything up to the walkers may run ahead
    ChainSlice io;                  // what its front end left
    bool launched = false;          // its front end has been enqueued.  false: registered only -- a handle whose clock recovery
                                    // is relayed (cfg.clock_exact >= 1) starts the front end of the next burst in front of the relay
                                    // kernels of the current one, which leave most of the chip idle, instead of under the loops that fill it
    bool costas_begun = false;      // the Costas loop of this input has been started too (behind its front end)
    void *slot = nullptr;           // ... writing here (float2: the clock recovery's next input buffer)
    ChainStream costas_stream = CHAIN_FRONT;    // ... on this stream
    // bursts whose clock recovery walks overlapping blocks (clock_overlap.h)
    bool costas_finished = false;   // the host has looked at the loop's stop test (and continued it where it had not closed)
    bool restart_due = false;       // ... and the loop rewrote its output: walkers started behind the first batch have read the old one
    int ov_job = -1;                // the clock stage's job of this input
    unsigned long long serial = 0;  // ... and that job's place in the order of the calls (its walkers' stream)
    bool walk_launched = false;     // its walkers have been enqueued
    // what the AGC's guard and the Costas loop reported for this input
    bool agc_fallback = false;
    int c_passes = 0; unsigned c_unconverged = 0; float c_max_residual = 0; bool c_walked = false;
};

struct ChainQueue {
    ChainInput in[XRIT_AHEAD + 1];  // oldest first: the one of the next process call and the two behind it
    int count = 0;
    int next_set = 0;               // the set the next front end takes
    int last_fe_set = -1;           // set of the front end that ran last (its event orders the next one behind it)
    long costas_event_of = 0;       // the input ev_costas was last recorded for (0: never recorded)
    long ids = 0;                   // registrations so far
    // of the handle
    bool has_costas_stream = false;                     // cfg.front_exact = 2 (and not XRIT_NO_COSTAS_STREAM)
    size_t costas_own_stream_below = 16u << 20;         // circuit-rate samples per burst (XRIT_OV_CSTREAM_BELOW)
};

// ---- eligibility: the call of n input samples walks overlapping blocks.  keep: stage or symbol copies are on (the caller
// then takes more than float soft symbols)
inline bool chain_ov_call(ClockKnobs &k, size_t xpad, bool keep, unsigned decimation, size_t n)
{
    k.ov_allow = !keep;
    return clock_ov_eligible(k, xpad, false, decimation > 1 ? n / decimation : n);
}

// ---- admission of a registration
// Two sets of front-end buffers: the front end of the input two behind a call would overwrite what that call's loops still
// read.  Bursts whose clock recovery walks overlapping blocks hold their front ends back until that is safe (chain_next) and
// may wait three deep -- the call in progress and two behind it --; everything else two deep.
inline int chain_room(const ChainQueue &q, bool ov)
{
    bool all_ov = ov;
    for (int i = 0; i < q.count && all_ov; ++i) all_ov = q.in[i].ov;
    return all_ov ? XRIT_AHEAD + 1 : 2;
}
// Unless the relay is off (cfg.clock_exact < 0) the next process call ends in relay kernels that occupy three waves per CU:
// the front end waits for those (ClockStage::before_relay) instead of competing with the Costas and hand-off passes.
// (bursts whose clock recovery walks overlapping blocks: the next process call enqueues everything that can run ahead)
inline bool chain_defer(bool relay_by_default, bool no_defer, bool ov) { return (relay_by_default && !no_defer) || ov; }

// the record behind the waiting ones; the caller counts it in (++q.count) once whatever starts at registration has started
inline ChainInput &chain_stage(ChainQueue &q, const void *samples, size_t n, int type, bool ov)
{
    ChainInput &f = q.in[q.count];
    f = ChainInput{};
    f.samples = samples; f.n = n; f.type = type; f.ov = ov;
    f.id = ++q.ids;
    return f;
}

// ---- a process call
// the overlap path -- unless the call's Costas loop was begun under the relay of a chains-path call (no job is noted for it)
inline bool chain_call_overlaps(const ChainQueue &q, bool ov) { return ov && !(q.count > 0 && q.in[0].costas_begun && q.in[0].ov_job < 0); }
// a process call takes the oldest registered input, and no other
inline bool chain_front_is(const ChainQueue &q, const void *samples, size_t n, int type)
{
    return q.in[0].samples == samples && q.in[0].n == n && q.in[0].type == type;
}
inline void chain_pop(ChainQueue &q)
{
    for (int i = 1; i < q.count; ++i) q.in[i - 1] = q.in[i];
    --q.count;
}
// what a reset leaves of the queue (the sets keep alternating from where they are)
inline void chain_reset(ChainQueue &q) { q.count = 0; q.last_fe_set = -1; }

// ---- a front end: the set it takes, and the set whose event it goes behind (-1: none)
struct ChainFrontEnd { int set, behind_set; };
inline ChainFrontEnd chain_front_end_take(ChainQueue &q)
{
    ChainFrontEnd t{q.next_set, q.last_fe_set};
    q.next_set ^= 1;
    return t;
}
inline void chain_front_end_started(ChainQueue &q, int set) { q.last_fe_set = set; }

// ---- the chains path: the three moments at which a registered front end starts.
// (Registered inputs start in order: the process call that takes one starts it if it still waits, and starts the one behind
// it in front of its own relay kernels.)
// 1. at registration, when it is not deferred: the oldest one first if that still waits (chain_start_oldest_first), then
//    the new one
inline bool chain_start_oldest_first(const ChainQueue &q) { return q.count > 0 && !q.in[0].launched; }
// 2. in front of the relay kernels of the call before: the oldest input, when it still waits
inline bool chain_start_under_relay(const ChainQueue &q) { return q.count > 0 && !q.in[0].launched; }
//    A stream with its next input registered: this call's Costas loop is finished FIRST (one more wait of the host), so
//    that the stage is free for the next burst's loop behind its front end, under this call's relay -- from the next
//    call on that is how every Costas loop of the stream runs and the extra wait is gone.
inline bool chain_costas_first(const ChainQueue &q, bool costas_done) { return !costas_done && chain_start_under_relay(q); }
//    ... and the next input's Costas loop follows its front end there exactly when this call's own loop is done with the
//    stage (costas_idle: finished before its clock recovery began)
inline bool chain_costas_under_relay(bool costas_idle) { return costas_idle; }
// 3. at its own call (registered only: the call before had no relay phase to put it in front of)
inline bool chain_start_at_call(const ChainQueue &q) { return !q.in[0].launched; }

// ---- the overlap path: whatever can be enqueued for the registered inputs, oldest first, without waiting for the device.
// Nothing in such a burst's clock recovery waits for the burst in front of it, so EVERYTHING up to its walkers runs ahead of
// its process call: front end and Costas loop (in the order of the inputs: the stages carry their state from one to the
// next), the walkers behind the Costas loop.  With two inputs registered behind the current call the device holds, at any
// time, the walkers of bursts b and b + 1 and the front end / Costas loop of burst b + 2.
enum ChainStepKind { CHAIN_NONE, CHAIN_FRONT_END, CHAIN_COSTAS_LOOK, CHAIN_WALK_RESTART, CHAIN_COSTAS_BEGIN, CHAIN_WALK_LAUNCH };
struct ChainStep {
    ChainStepKind kind = CHAIN_NONE;
    int i = 0;                              // which input of the queue
    ChainStream stream = CHAIN_FRONT;       // FRONT_END: CHAIN_FRONT; COSTAS_LOOK, COSTAS_BEGIN: the loop's; WALK_LAUNCH: the walkers'
    bool wait_fe = false;                   // COSTAS_BEGIN: the stream is not the front ends': behind ev_fe[the input's set]
    long event_of = 0;                      // COSTAS_LOOK, WALK_LAUNCH: the input ev_costas was last recorded for
};
// one pass over the queue (a call of demod.cpp's ov_service): where it stands
struct ChainScan {
    int i = 0, part = 0;
    bool costas_busy = false;       // a Costas loop begun and not yet finished: the stage takes the next input behind it
};

// The next step of the pass, or CHAIN_NONE at its end.  Facts: what the host cannot know without the device or the clock
// stage -- bool costas_event_done(): ev_costas has completed (asked once per pass and input whose loop is out);
// unsigned long long ov_serial(): overlap jobs the clock stage has handed out; bool can_launch_ahead(int job).
template <class Facts> inline ChainStep chain_next(ChainQueue &q, ChainScan &sc, Facts &facts, int limit)
{
    ChainStep st;
    for (; sc.i < q.count && sc.i < limit; ++sc.i, sc.part = 0) {
        const int i = sc.i;
        ChainInput &f = q.in[i];
        st.i = i;
        if (!f.ov) break;                       // (inputs that take the other path are started by their own calls)
        if (sc.part == 0) {
            sc.part = 1;
            // (two sets of front-end buffers: the input two in front used the set this one takes, and its Costas loop reads that
            // set until the host has seen it close -- a loop that did not close inside its batch goes on from the host)
            if (!f.launched && (i < 2 || q.in[i - 2].costas_finished)) { st.kind = CHAIN_FRONT_END; st.stream = CHAIN_FRONT; return st; }
        }
        if (!f.launched) break;
        if (sc.part == 1) {
            sc.part = 2;
            if (f.costas_begun && !f.costas_finished) {
                if (!facts.costas_event_done()) { sc.costas_busy = true; continue; }
                st.kind = CHAIN_COSTAS_LOOK; st.stream = f.costas_stream; st.event_of = q.costas_event_of;
                return st;
            }
        }
        if (sc.part == 2) {
            sc.part = 3;
            // the loop went on from the host and rewrote its output (and the timing statistic): walkers that were started
            // behind the first batch have read the old one
            if (f.restart_due) { st.kind = CHAIN_WALK_RESTART; st.stream = CHAIN_FRONT; return st; }
        }
        if (sc.part == 3) {
            sc.part = 4;
            if (!f.costas_begun && !sc.costas_busy) {
                // Which stream the loop takes:
                // (on the front ends' stream, behind this input's: measured with every stream on a hardware queue of its own
                // -- GPU_MAX_HW_QUEUES=8 -- a Costas stream beside the front ends' costs 10 %, 2.05 against 1.85 ms per C2 burst: the
                // loop's passes and the next input's decimator fill the chip each and only slow one another)
                // (... unless the loop is a handful of small kernels -- C5: 2 M samples at the circuit rate, 0.3 ms of launches --,
                // which then overlap the next input's decimator: 1.1 -> 0.9 ms per C5 burst)
                // (round 5, late: not a stream of its own but the walker stream this burst's OWN walkers will take -- the one the
                // walkers of the burst two in front are on: the loop then runs behind them instead of beside them, and its walkers
                // behind it.  That is what HIP's dealing of streams onto hardware queues had arranged by accident on the first handle
                // of a process, and measured better than a queue of its own: C5 1.08 against 1.11-1.14 ms per burst)
                // (round 6, cfg.front_exact = 2: the exact AGC chains and the exact Costas walkers are a wave per SIMD or less for
                // milliseconds -- latency, not work --, so the Costas loop of burst b runs on a stream of its own beside the front end
                // of burst b + 1 instead of in front of it)
                st.kind = CHAIN_COSTAS_BEGIN;
                st.stream = q.has_costas_stream ? CHAIN_COSTAS
                          : f.io.length < q.costas_own_stream_below ? (ChainStream)(CHAIN_WALK0 + (int)((facts.ov_serial() + 1) % CHAIN_WALK_STREAMS))
                          : CHAIN_FRONT;
                st.wait_fe = st.stream != CHAIN_FRONT;
                sc.costas_busy = true;
                return st;
            }
        }
        if (sc.part == 4) {
            sc.part = 5;
            if (f.costas_begun && f.ov_job >= 0 && !f.walk_launched && facts.can_launch_ahead(f.ov_job)) {
                // (behind the Costas loop's batch and the timing curve: speculative until the host has seen the loop's stop test)
                // (two walker streams, alternating: the walkers of bursts b and b + 1 side by side, those of b + 2 behind b's)
                st.kind = CHAIN_WALK_LAUNCH;
                st.stream = (ChainStream)(CHAIN_WALK0 + (int)(f.serial % CHAIN_WALK_STREAMS));
                st.event_of = q.costas_event_of;
                return st;
            }
        }
        if (!f.costas_begun || !f.costas_finished) sc.costas_busy = true;      // (the inputs behind wait for this one's loop)
    }
    st.kind = CHAIN_NONE;
    return st;
}

// the outcomes of the steps
inline void chain_front_end_done(ChainQueue &q, ChainInput &f, int set) { chain_front_end_started(q, set); f.launched = true; }
inline void chain_costas_begun(ChainQueue &q, ChainInput &f, ChainStream stream, void *slot, int ov_job, unsigned long long serial)
{
    f.costas_stream = stream; f.slot = slot;
    q.costas_event_of = f.id;
    f.costas_begun = true;
    f.ov_job = ov_job; f.serial = serial;
}
inline void chain_costas_looked(ChainInput &f, bool redone)
{
    f.costas_finished = true;
    f.restart_due = redone && f.ov_job >= 0;
}
inline void chain_walk_restarted(ChainInput &f) { f.walk_launched = false; f.restart_due = false; }
inline void chain_walk_launched(ChainInput &f) { f.walk_launched = true; }

}  // namespace xrit
