// clock_ctl.h -- the clock recovery's control block: the words its kernels and the host share, by name.
// Plain C++ (no HIP headers): clock.hip, clock_relay.h, clock_overlap.h, clock_plan.h and clock_host_check.cpp include it.
//
// The block lives at the head of ClockStage::counters and is copied to the host (ClockStage::h_res) behind every batch:
//   words [0, CLK_RES_WORD)              the control words below
//   words [CLK_RES_WORD, CLK_CTL_WORDS)  the call's ClockResult
//   from word CLK_CTL_WORDS              one slot of CLK_CNT_WORDS counters per hand-off pass (ClockCnt)
//
//   word                 written by                                              read by
//   DONE            0    ClockPolicy::decide (newton.h calls it), guess: zeroed  every pass / solve kernel (no-op once set), relay walkers,
//                                                                                relay finalize, host: closed(), the hand-off's loop
//   PASSES          1    ClockPolicy::decide                                     decide, host: passes, the batch learnt
//   OPEN            2    ClockPolicy::decide                                     host: unconverged
//   MAX_RESIDUAL    3    ClockPolicy::decide (float bits, samples)               host: max_residual
//   SUM_SQ          4    ClockPolicy::decide (float bits: summed r^2 of the      decide (the pass before), host: the stall rule
//                        last solve, samples^2)
//   GATED           5    guess kernel (1), ClockPolicy::decide                   newton.h: the trust gate scan runs
//   OPEN_LAST       6    ClockPolicy::decide (boundaries not frozen)             decide (the pass before), host: the stall rule
//   STALL_MEMO      7    ClockPolicy::decide (flat runs | acquiring << 8)        decide
//   TAKEOVER        8    newton.h's wave-aligned solve (NEWTON_CTL_TAKEOVER)     pass / solve kernels, host: go over to the gated solve
//   LARGE           9    ClockPolicy::decide                                     host: large_open, the mean Jacobian's "clean"
//   RELAY_PASSES   10    relay finalize; overlap scan (1)                        host: relay_passes
//   RELAY_CLOSED   11    relay finalize; overlap scan (0)                        host: the relay's loop, relay_closed
//   RELAY_SHIFT_SQ 12    relay finalize (float bits: mean squared move of the    host: the "starts still moving" look
//                        segment starts in the last pass, samples^2)
//   SYMBOLS        13    a writing hand-off pass (ClockPassOut::flag)            output, unstage, terminal, finalize kernels
//   SNR2           14    relay finalize, overlap scan (float bits: 2 Es/N0)      host: the Es/N0 looks
//   STUCK          15    relay finalize, overlap scan (a watchdog ended a walk)  host: the call fails
//   RELAY_MOVE_MAX 16    relay finalize (float bits: largest move of a start;    host: the quarter-symbol look
//                        infinity: a watchdog mark)
//   OV_BAD_JOINTS  17    overlap scan (joints that do not fit)                   host: fall back
//   OV_JOINT_MAX   18    overlap scan (float bits: largest distance at a joint)  host: ov_joint_max
//   WALKERS        19    overlap scan                                            (trace)
// The relay's init kernel zeroes words 10, 11, 12, 14, 15 in front of a call's first pass.
#pragma once

#include <string.h>

namespace xrit {

enum ClockCtlWord : int {
    CLK_CTL_DONE = 0,
    CLK_CTL_PASSES = 1,
    CLK_CTL_OPEN = 2,
    CLK_CTL_MAX_RESIDUAL = 3,
    CLK_CTL_SUM_SQ = 4,
    CLK_CTL_GATED = 5,
    CLK_CTL_OPEN_LAST = 6,
    CLK_CTL_STALL_MEMO = 7,
    CLK_CTL_TAKEOVER = 8,
    CLK_CTL_LARGE = 9,
    CLK_CTL_RELAY_PASSES = 10,
    CLK_CTL_RELAY_CLOSED = 11,
    CLK_CTL_RELAY_SHIFT_SQ = 12,
    CLK_CTL_SYMBOLS = 13,
    CLK_CTL_SNR2 = 14,
    CLK_CTL_STUCK = 15,
    CLK_CTL_RELAY_MOVE_MAX = 16,
    CLK_CTL_OV_BAD_JOINTS = 17,
    CLK_CTL_OV_JOINT_MAX = 18,
    CLK_CTL_WALKERS = 19,
};
constexpr int CLK_RES_WORD = 24;        // the ClockResult
constexpr int CLK_CTL_WORDS = 32;       // ... and the first per-pass counter slot

// a hand-off pass's counter slot (ClockPolicy::cnt; newton.h's solve leaves a NewtonStat there)
enum ClockCnt : int {
    CLK_CNT_CHANGED = 0,        // boundaries whose start state changed
    CLK_CNT_OPEN = 1,           // ... that are not frozen
    CLK_CNT_MAX_R = 2,          // largest |r_t| (float bits)
    CLK_CNT_LARGE = 3,          // residual beyond 0.02 sample, or an open slip
    CLK_CNT_SUM_SQ = 4,         // sum r_t^2, fixed point, two words
    CLK_CNT_WORDS = 8,
};

// a relay pass's counters (RelayArgs::changed + RELAY_STAT * pass)
enum RelayStat : int {
    RELAY_STAT_CHANGED = 0,     // segments whose start changed in that pass (0: the relay has closed)
    RELAY_STAT_STEPS = 1,
    RELAY_STAT_ROUNDS = 2,      // guess rounds
    RELAY_STAT_MOVE_MAX = 3,    // largest move of a start (float bits); >= 0x80000000: a watchdog's mark
    RELAY_STAT_MOVE_SQ = 4,     // sum of squared moves, units of 2^-40 sample^2, two words
    RELAY_STAT_MOVED = 6,       // starts that entered the sum
};
constexpr int RELAY_STAT = 8;        // counters per relay pass (RelayArgs::changed)

// the words that carry float bits, on the host's copy of the block
inline float clock_ctl_float(const int *ctl, ClockCtlWord w)
{
    float v;
    memcpy(&v, &ctl[w], sizeof v);
    return v;
}
inline void clock_ctl_set_float(int *ctl, ClockCtlWord w, float v) { memcpy(&ctl[w], &v, sizeof v); }

}  // namespace xrit
