// lock_host.h -- the plain host parts of the frame lock (lock.cpp): the handle's state record as the kernels keep it, the
// argument checks, the bookkeeping of the round loop and the counters' copy.  No HIP here, so that a stand-alone program
// can run these under a sanitizer on the CPU.
#pragma once

#include "framer_host.h"

namespace xrit {

// what a round leaves for the host (read back once per round) and for the next round's joints
struct LockRound {
    unsigned count;                 // rows of the call so far
    unsigned stopped;               // 1: the walk stands at a chunk whose outcome needs the RS outcome of a row of this round;
                                    // 2: the commit's replay chose a row's hit otherwise than the joints did (never expected)
    unsigned cursor;                // ... that chunk's offset in the call's view V
    unsigned reserved;
};

// the handle's state in device memory.  fr: written by the joints (the framer's kernels read the carry's length from it,
// so it comes first); ok, fc and the counters behind them: written by the commit kernel alone, once per round
struct LockState {
    FramerState fr;
    unsigned long long short_kept, short_missed, rechecks, sensitive, rounds, frames_ok, frames_bad;
    unsigned ok, fc;                // lastFrameOK, flywheelCount (newdecoder.cpp:218-237)
    LockRound round;
};

namespace lock_host {

constexpr uint32_t FRAME = 16384, MIN_CORRELATION = 46, RECHECK_DEFAULT = 4, RECHECK_MAX = 255;

inline const char *check_flywheel(uint32_t recheck, bool started)
{
    if (started) return "lock: the flywheel is set before the first push";
    if (recheck < 1 || recheck > RECHECK_MAX) return "lock: flywheel recheck 1..255";
    return nullptr;
}

// the outputs are checked for the rows the call may write; on_device: cadu is a device pointer, which the decoder's
// kernels store to 16 bytes at a time
inline const char *check_push(const void *handle, const void *symbols, size_t n, size_t rows, const void *frames,
                              const void *valid, const void *hits, const void *start, const void *mode, const void *cadu,
                              const void *block, const void *info, const void *count, bool on_device)
{
    if (const char *why = framer_host::check_push(handle, symbols, n, rows, frames, valid, hits, start, count)) return why;
    if (rows && (!mode || !cadu || !block || !info)) return "null argument";
    if (rows && on_device && ((size_t)cadu & 15)) return "lock: cadu must be 16-byte aligned";
    return nullptr;
}

// The round loop: `done` rows are behind the call's earlier rounds.  A round's record must stay within the outputs and
// must move on: a round begins with ok and fc known, so it decides at least its first chunk, and a stop comes only after a
// row.  Returns a complaint, or null with `again` set when another round has to run.
struct Rounds {
    size_t cap;
    size_t done = 0;
    unsigned rounds = 0;
    explicit Rounds(size_t rows) : cap(rows) {}
    const char *next(const LockRound &r, bool &again)
    {
        again = false;
        if (r.count > cap || r.count < done) return "lock: a round's row count is out of range";
        if (r.stopped > 1) return "lock: the replay of a round disagrees with its walk";
        if (r.stopped && r.count == done) return "lock: a round made no progress";
        if (r.stopped && r.count == cap) return "lock: a round stopped with the outputs full";
        ++rounds;
        done = r.count;
        again = r.stopped != 0;
        return nullptr;
    }
};

inline void copy_counters(const LockState &s, xrit_lock_counters *out)
{
    std::memset(out, 0, sizeof *out);
    framer_host::copy_counters(s.fr, &out->framer);
    out->short_kept = s.short_kept;
    out->short_missed = s.short_missed;
    out->rechecks = s.rechecks;
    out->sensitive_chunks = s.sensitive;
    out->rounds = s.rounds;
    out->frames_ok = s.frames_ok;
    out->frames_bad = s.frames_bad;
}

}  // namespace lock_host
}  // namespace xrit
