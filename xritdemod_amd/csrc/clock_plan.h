// clock_plan.h -- what the clock recovery decides on the host, as plain C++ (no HIP headers): the knobs, the plan of a call
// (chain geometry, the relay's segments, the overlap job's ranges) and the looks at the control block after a wait.
// Pure functions: values and error text, no allocation, no launch.  ClockStage (kernels.h, clock.hip) reserves and
// launches by them; clock_host_check.cpp holds them against a recorded table under sanitizers (make clock-host-check).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include "clock_ctl.h"

namespace xrit {

// ---- constants the arithmetic shares with the device code (which includes them from here)
#define XR_MM_NTAPS  8
#define XR_MM_NSTEPS 128
#define XR_MM_FUDGE  16
constexpr int CLK_OM_BLOCK = 256;     // samples per timing-estimate block
constexpr int CLK_M = 2;      // samples kept below the start index
constexpr int CLK_SLACK = 3;  // head room above the schedule: R >= CLK_M + CLK_SLACK + A + 8
// The first CLK_MIR slots of a ring are kept twice, once more behind slot R - 1: the 8-sample window of a symbol
// then never wraps, its reads are one address and seven immediate offsets instead of eight masked indices
// (24 of the ~95 vector instructions of a symbol went into those indices).  Row stride WS = R + CLK_MIR float2,
// odd, so the per-lane ds_read_b64 stay spread over the banks.
#ifndef XR_CLK_MIR
#define XR_CLK_MIR (XR_MM_NTAPS - 1)
#endif
constexpr int CLK_MIR = XR_CLK_MIR;      // 0: no mirror, masked window indices (row stride R + 1)
constexpr int CLK_ROW_EXTRA = CLK_MIR > 0 ? CLK_MIR : 1;
constexpr int RELAY_RX = 2048;       // sample ring (RING): about five steps of lead for the prefetching wave (clock_relay.h)
constexpr int RELAY_XCH = 512;       // samples per refill (8 per lane)
constexpr int RELAY_CLAIM_WORDS = 2048;   // one word per CU, indexed by (XCC_ID, SE_ID, SH_ID, CU_ID)

struct ClockPar { float omega_mid, omega_lim, gain_omega, gain_mu; };

// ---- the knobs: what the plans read.  Set by the chain (demod.cpp, group.hip) and, for A/B runs, by ClockStage::init
// from the environment.
struct ClockKnobs {
    ClockPar par{};
    float sps = 0;
    int NS = 64;            // symbols per chain (auto_ns: chosen per call so that its waves fill whole generations)
    int cu_count = 256;     // what the chip holds at once decides the chain length, see clock_chain_plan
    long long lds_per_cu = 160 * 1024;
    bool auto_ns = true;
    bool serial = false;    // one trajectory, no chains (cfg.clock_serial): the floor measurement, ~0.3 us per symbol
    int max_passes = 48, min_passes = 4;
    bool pass_writes = true;    // the last hand-off pass is the output pass (XRIT_NO_PASS_OUTPUT=1, read at init: a separate output pass)
    int ng_max = 8;             // XRIT_CLOCK_NG: one-wave groups per clock workgroup at most
    // ---- exact closure (clock_relay.h, cfg.clock_exact): segments of the call walked exactly, relayed until the
    // serial trajectory is reproduced bit for bit
    int exact = 0;              // 0 (default), by call size (clock_chain_plan): one exact walk / two hand-off passes + auto_passes relay
                                // passes / no hand-off passes, relayed from the timing guess (bursts that fill the chip); four more passes at
                                // a time while the segment starts still move by more than auto_shift (low Es/N0), to closure when the
                                // hand-off never closed (cfg.clock_exact = -3 arrives here as 0 with relay_quick set);
                                // 1: always until closed; n > 1: n relay passes, nothing else; -2: hand-off passes only (the
                                // fast configuration: five of them, 2.6e-4 rms from the serial trajectory), relayed to closure
                                // when they stall above auto_rms or never close (round 2's default); -1: never relayed
    float auto_rms = 3e-4f;     // (calls too short for the relay to be planned -- fewer than auto_min symbols -- and
                                // cfg.clock_exact = 0: closed exactly when the hand-off stalls above this rms residual, samples)
    // the default's three relay passes: measured at C2 after the third, the starts move by 3.8e-4 sample rms at Es/N0
    // 12 dB, 1.1e-3 at 6 dB, 4.3e-3 at 3 dB (XRIT_AUTO_PASSES=n: another count; 0: the hand-off passes' result as in
    // round 2 unless they stall)
    int auto_passes = 3;
    long long auto_guess_min = 6000000;   // symbols from which the default configuration relays straight from the timing guess
    int auto_long_seg = 49152;  // symbols per segment from which two relay passes are the default's budget (clock_chain_plan)
    // A call of up to this many symbols is ONE exact walk from the carried state (0: three of the default's shortest segments,
    // 73.7 k symbols -- no slower than three passes over a third of it).  Handles whose calls of this size take the bit-exact front end (cfg.front_exact 0 / 2) set 200 k: every
    // chunk the reference hands its blocks (up to 512 Ki samples: 123 k symbols LRIT, 194 k HRIT) then comes out as the CPU
    // chain's words, at 56 symbols per microsecond on the one walking wave.
    int one_walk_max = 0;
    long long one_walk_limit() const { return one_walk_max > 0 ? (long long)one_walk_max : 3LL * (auto_long_seg / 2); }
    float auto_shift = 6e-4f;
    float auto_snr = 10.0f;     // ... and to closure outright when the first pass's soft symbols show 2 Es/N0 below this (7 dB)
    float auto_snr_floor = 2.0f;  // ... but not below this: no signal (noise alone shows 1.75)
    long long auto_min = 1;     // (round 4: a short call is one exact walk of a few dozen steps -- cheaper than hand-off passes that run until they close)
    bool relay_by_default() const { return exact >= 1 || (exact == 0 && auto_passes > 0); }
    int relay_window = 0;       // chains per segment (0: chosen per call, ~4 segments per CU)
    bool relay_global = false;  // walk from global memory even where the LDS-staged kernel applies (A/B runs)
    int relay_per_cu = 3;       // XRIT_RELAY_PER_CU: segments (walkers) per CU the relay plans (A/B runs)
    bool relay_per_cu_set = false;
    int relay_no_handoff = -1;       // the relay's first pass starts from the timing guess, no hand-off passes: -1: in the default
                                     // configuration (cfg.clock_exact = 0); XRIT_NO_HANDOFF=0 / 1: never / with every relayed call (A/B runs)
    bool relay_quick = false;          // cfg.clock_exact = -3: the default configuration with its first relay passes walked approximately
    int relay_apx_cfg[2] = {-1, -1};   // XRIT_RELAY_APX=a,b: the walk of the relay's first two passes (-1: the configuration's choice; A/B runs)
    int relay_waves = 1;        // waves per walker team at most (clock_relay_wide.h; < 2: the one-wave walker of clock_relay.h)
    int relay_teams_per_cu = 1; // segments (teams) per CU the relay plans with the wide walker
    // ---- overlapping exactly walked blocks (clock_overlap.h, round 5): the default configuration's plan for calls of ov_min
    // symbols or more
    bool ov_allow = true;       // the caller takes float soft symbols only (the chain sets it per call; stage objects: off)
    bool ov_enabled = true;     // XRIT_NO_OVERLAP=1 (read at init): the relay of clock_relay.h for every call, as in round 4
    long long ov_min = 1000000; // symbols from which the default configuration walks overlapping blocks
    int ov_hist = 49152;        // symbols of exactly walked history in front of every range (XRIT_OV_HIST)
    int ov_min_range = 8192;    // symbols per range at least (XRIT_OV_MINL)
    int ov_min_walkers = 240;   // walkers at least, where ranges of 8192 symbols allow (XRIT_OV_MINW): few walkers, long latency
    bool ov_small_ring = false; // XRIT_OV_SMALL_RING=1: sample rings of 1024 instead of 2048 samples where a block's span allows
    double ov_lratio = 1.0;     // range length aimed at, in histories (XRIT_OV_LRATIO): every symbol is walked 1 + 1 / ov_lratio times
};

// LDS of a clock workgroup: the table, then `ngroups` groups (one per 64 chains) of ring origins and rings, then the dump slots
// (clock_tile_carve)
inline size_t clock_tile_bytes(int WS, int ngroups, int threads)
{
    return 4160 + 256 * (size_t)ngroups + ((size_t)ngroups * 64 * WS + threads) * 2 * sizeof(float);
}

// samples a block of `symbols` symbols can cover at the fastest admissible clock
inline int relay_span(const ClockPar &par, int symbols)
{
    return (int)ceil((double)symbols * ((double)par.omega_mid + (double)par.omega_lim + 0.004)) + 24;
}
// the LDS-staged walker (clock_relay_kernel<.., true>, clock_overlap_kernel) takes what fits its refill chunk
inline bool relay_ring_ok(const ClockPar &par) { return relay_span(par, 64) + 8 <= RELAY_RX - RELAY_XCH - 72; }

// steps of the float32 lattice omega and mu + omega live on, in units of 2^-24 sample (the walkers' integer model)
struct ClockLattice { int q_om, q_mu; };
inline ClockLattice clock_lattice(float omega_mid)
{
    const float om = omega_mid, su = omega_mid + 0.5f;
    const double u = 1.0 / 16777216.0;
    ClockLattice l;
    l.q_om = (int)((double)(nextafterf(om, INFINITY) - om) / u);
    l.q_mu = (int)((double)(nextafterf(su, INFINITY) - su) / u);
    if (l.q_om < 1) l.q_om = 1;
    if (l.q_mu < 1) l.q_mu = 1;
    return l;
}

// ---- the relay's segments
struct ClockRelaySegs { int cps = 0, G = 0; };     // chains per segment, segments
// relay_w: waves per walker team (clock_relay_wide.h, an experiment; 0: the one-wave walker); relay_budget as the call
// stands when the segments are cut (0: to closure)
inline ClockRelaySegs clock_relay_segments(const ClockKnobs &k, int K, int NS, bool no_handoff, int relay_budget, int relay_w)
{
    // (without hand-off passes: two walkers per CU -- 24.8 k symbols per segment at C2, three passes; measured in the streamed
    // bench against one per CU with two passes and three per CU with four: 2.12 / 2.35 / 2.27 ms per burst)
    // ... and where the call is long enough for MORE walkers whose segments still hold auto_long_seg symbols -- the two-pass plan:
    // bursts at the circuit rate, 63 M (LRIT) / 100 M (HRIT) symbols per 2^28 samples -- up to four per CU, one per SIMD: the
    // passes' latency is a segment's length, and a two-pass plan over 62 k / 97 k-symbol segments has the same exact history
    // as over 123 k / 195 k (C3: 6.5 instead of 9.6 ms per burst, C1: 5.7 instead of 6.2, profiles/r4_relay_shortcuts.txt))
    int auto_per_cu = 2;
    if (no_handoff && k.exact == 0)
        for (int p = 4; p > 2; --p)
            if ((long long)K * NS / ((long long)p * k.cu_count) >= k.auto_long_seg) { auto_per_cu = p; break; }
    const int per_cu = relay_w > 0 ? k.relay_teams_per_cu : (no_handoff && !k.relay_per_cu_set ? auto_per_cu : k.relay_per_cu);
    int cps = k.relay_window > 0 ? k.relay_window : (K + per_cu * k.cu_count - 1) / (per_cu * k.cu_count);
    // (a call much shorter than the ~1e5 symbols two trajectories need to meet is walked front to back whatever the
    // cut: segments of at least 2048 symbols then cost the fewest passes -- a pass is a launch)
    // With a budget of relay passes (cfg.clock_exact = n > 1) what the passes buy is their horizon, n x the segment length
    // -- a segment is exact once everything within the merge length in front of it is: segments no shorter than the big
    // bursts' (16 k symbols), whatever the size of the call, so that n means the same parity everywhere.
    // (without hand-off passes -- the default configuration -- a segment must be long enough for the loop to forget the timing
    // guess it starts from: never shorter than auto_long_seg / 2, 24.6 k symbols, which three passes go with.  A call of up
    // to three such segments is ONE segment instead -- one exact walk from the carried state takes no longer than three
    // passes over a third of it, and it IS the serial trajectory.)
    int min_syms = relay_budget > 0 ? 16384 : 2048;
    if (no_handoff && k.exact == 0 && !k.relay_per_cu_set) {
        const long long all = (long long)K * NS;
        min_syms = all <= k.one_walk_limit() ? (int)all : k.auto_long_seg / 2;
    }
    if (k.relay_window <= 0 && cps * NS < min_syms) cps = (min_syms + NS - 1) / NS;
    if (cps < 1) cps = 1;
    ClockRelaySegs r;
    r.cps = cps;
    r.G = (K + cps - 1) / cps;
    return r;
}
// relay passes at most: a pass moves the exact front by at least one segment, G + 1 passes always close
inline int clock_relay_limit(int G, int relay_budget)
{
    const int hard = G + 1;
    return relay_budget > 0 ? (relay_budget < hard ? relay_budget : hard) : hard;
}

// ---- the chains of a call: ring geometry, chain length, and how the call is closed
struct ClockChainPlan {
    char err[128] = {0};        // not empty: the call is refused with this text
    long long N = 0, ni = 0;    // samples in [carry | new], and how many of them a symbol may start at
    bool short_input = false;   // not enough samples for a single symbol: everything is carried to the next call
    int SS = 0, W = 0, WS = 0, A = 0, STEP = 0; bool wide = false;
    int NG = 1, waves_cu = 0;   // one-wave groups per workgroup, and the waves a CU then holds
    size_t tile_bytes = 0, tile_bytes3 = 0;   // one-wave groups (NG per workgroup) / the three-wave Jacobian pass
    int NS = 64, K = 0;
    bool relay = false;                     // the exact closure is on for this call
    bool no_handoff = false;                // ... straight from the timing guess: no hand-off passes at all
    int relay_budget = 0;                   // relay passes at most (0: until closed)
    int relay_apx[2] = {0, 0};              // how the relay's first two passes walk (clock_relay_kernel's apx): 0 exactly
    bool relay_long = false;                // the default configuration on segments of >= auto_long_seg symbols: two passes, no watch on the starts
    int write_from = 0x7fffffff;            // hand-off passes from this one on leave the symbols (ClockPassOut)
    ClockRelaySegs segs;                    // (relay)
};

// n new samples behind `carry` held over; last_passes: the hand-off passes the call before needed (-1: none yet).
// relay_w: see clock_relay_segments (decided by the caller: it depends on device code)
inline ClockChainPlan clock_chain_plan(const ClockKnobs &k, size_t n, size_t carry, int last_passes, int relay_w = 0)
{
    ClockChainPlan j;
    const ClockPar &par = k.par;
    j.NS = k.NS;
    j.N = (long long)(carry + n);
    j.ni = j.N - XR_MM_NTAPS - XR_MM_FUDGE;
    if (j.N >= (1LL << 31)) { snprintf(j.err, sizeof j.err, "clock recovery: more than 2^31 samples in one call"); return j; }
    if (j.ni <= 0) {
        j.short_input = true;
        if (j.N > 1024) snprintf(j.err, sizeof j.err, "clock recovery: unread tail exceeds the hand-over buffer");
        return j;
    }
    if (k.serial) { j.K = 1; return j; }
    // chain budget: the slowest admissible symbol clock plus slack
    const double min_omega = (double)par.omega_mid - (double)par.omega_lim;
    // sample rings (see ClockTile).  Over SS symbols the read index advances by A at most; a ring of R samples
    // must hold CLK_M below the schedule, CLK_SLACK above it, the advance and the 8 interpolator taps.  SS
    // divides the output tile (16 symbols).
    const double max_adv = (double)par.omega_mid + (double)par.omega_lim + 0.004;
    static const int tries[6][2] = {{32, 4}, {32, 2}, {32, 1}, {64, 4}, {64, 2}, {64, 1}};
    int SS = 1, A = 0, R = 64;
    for (int q = 0; q < 6; ++q) {
        R = tries[q][0];
        SS = tries[q][1];
        A = (int)ceil(SS * max_adv) + 1;
        if (CLK_M + CLK_SLACK + A + XR_MM_NTAPS <= R) break;    // else: very large sps, sub-steps run from global memory
    }
    j.wide = R > 32;
    j.SS = SS; j.W = R; j.A = A;
    j.STEP = (int)floor((double)SS * (double)par.omega_mid * 65536.0);
    j.WS = R + CLK_ROW_EXTRA;
    j.tile_bytes3 = clock_tile_bytes(j.WS, 1, 192);
    // one-wave groups share the table: as many groups per workgroup as gives the CU the most waves (the rings
    // fill LDS; two waves per SIMD is what the registers allow)
    j.NG = 1;
    for (int ng = 1; ng <= 8 && ng <= k.ng_max; ++ng) {
        const long long need = (long long)clock_tile_bytes(j.WS, ng, 64 * ng);
        if (need > k.lds_per_cu) break;
        long long wv = (long long)ng * (k.lds_per_cu / need);
        if (wv > 8) wv = 8;
        if (wv >= j.waves_cu) { j.waves_cu = (int)wv; j.NG = ng; }
    }
    if (j.waves_cu < 1) { snprintf(j.err, sizeof j.err, "clock recovery: a ring of %d samples per chain does not fit LDS", R); return j; }
    j.tile_bytes = clock_tile_bytes(j.WS, j.NG, 64 * j.NG);
    if (k.auto_ns) {
        // One wave = 64 chains, and a wave's time is its chain length times a serial per-symbol latency: a pass
        // costs (generations of resident waves) x NS.  So the chain length is chosen from what the chip holds --
        // LDS decides: CUs x floor(LDS / ring tile) waves -- such that the call's waves fill a whole number g of
        // generations: NS = symbols / (g x resident chains), with the smallest g that keeps NS <= 256 (longer
        // chains lose more in the passes than their fewer hand-offs gain).  C2: 1792 resident waves, g = 1,
        // NS = 112 (the former 64 gave 1.66 generations = 2 x 64 symbol times per pass, and 190 k hand-offs
        // instead of 113 k).
        const long long resident = (long long)k.cu_count * j.waves_cu;   // waves
        const double symbols = (double)j.N / min_omega;
        // (calls that do not fill the chip keep 64: 16-symbol chains would make their passes four times shorter,
        // but the fuzz runs found symbol slips and count mismatches with them at low Es/N0; 32-symbol chains are
        // clean and 15-25 % quicker per small call, but at Es/N0 < 3.6 dB 4 % of the cases had a hard decision
        // flipped instead of 2.5 %)
        j.NS = 64;
        for (int g = 1; g <= 64; ++g) {
            const double chains = (double)(g * resident * 64 - 4);          // K = symbols / NS + 3 must fit
            int ns = (int)ceil(symbols / chains);
            ns = (ns + 15) & ~15;                                            // whole output tiles, 64-byte rows
            if (ns <= 256) { j.NS = ns < 64 ? 64 : ns; break; }
        }
    }
    const int NS = j.NS;
    const int K = (int)((double)j.N / (min_omega * NS)) + 3;
    j.K = K;
    // cfg.clock_exact: 1 -- relayed to closure; n > 1 -- n relay passes; 0 -- auto_passes of them, and on to closure from
    // finish() when the walks have not settled by then (calls of fewer than auto_min symbols: hand-off passes, relayed from
    // finish() when they stall high); < 0 -- hand-off passes only
    const int exact = k.exact;
    j.relay = exact >= 1 || (exact == 0 && k.auto_passes > 0 && (long long)K * NS >= k.auto_min);
    j.relay_budget = exact > 1 ? exact : (exact == 1 ? 0 : k.auto_passes);
    // Round 4: the default configuration has NO hand-off passes.  The relay's first pass walks every segment from the timing
    // guess itself: the loop forgets a start that is 2.6e-2 sample off within ~12 time constants (37 k symbols), so with one
    // segment per CU (49.6 k symbols at C2) the end states of that pass are as close to the serial trajectory as those of a
    // walk from a closed hand-off, and the second pass starts from them.  Measured at C2 (steady-state bursts,
    // profiles/r4_handoff_vs_guess.json): guess + 2 passes over 256 segments 5.3e-5 rms from the serial trajectory, where two
    // hand-off passes + 3 relay passes over 766 segments had 6.4e-5 -- for two sweeps of the stream instead of five.
    // (... where the call fills the chip with such segments, or is one segment: in between -- 74 k to 6 M symbols: C5's bursts,
    // calls of 2^19 .. 2^22 samples -- the walkers are few and it is their latency that counts: two hand-off passes, which
    // cost such a call 0.1 ms, start them close enough for three passes over segments of 16 k symbols)
    const long long all_syms = (long long)K * NS;
    j.no_handoff = j.relay && (k.relay_no_handoff >= 0 ? k.relay_no_handoff != 0
                                                       : exact == 0 && (all_syms <= k.one_walk_limit() || all_syms >= k.auto_guess_min));
    if (j.relay) j.segs = clock_relay_segments(k, K, NS, j.no_handoff, j.relay_budget, relay_w);
    if (j.no_handoff && exact == 0) {
        // passes for the default's parity by segment length (measured, same file: 16.5 k symbols per segment: 3 passes 9.6e-5,
        // 4 passes 6.2e-5; 24.8 k: ...; 49.6 k: 2 passes 5.3e-5, 3 passes 2.9e-5)
        const long long L = (long long)j.segs.cps * NS;
        j.relay_budget = L >= k.auto_long_seg ? 2 : (L >= k.auto_long_seg / 2 ? 3 : 4);      // (shorter segments: cfg.clock_exact_window)
        // cfg.clock_exact = -3, the quick relay: the passes in front of the last are there for their end states and are walked
        // approximately (clock_relay_kernel's apx) -- the first ones in one guess round, the one before the last in two, leaving
        // the record of its guesses; no literal verification, no symbols.  Measured at C2 (steady-state bursts, streamed):
        // 1.92 instead of 2.07 ms per burst, soft symbols 1.15e-4 instead of 5.6e-5 rms from the serial trajectory (which is
        // itself 1.0e-4 from the oracle); only the first pass approximate: 1.95 ms, 7.5e-5.  (Few segments: a call of up to
        // `budget` segments closes exactly within its budget if every pass is exact, and stays that way.)
        // (a plan of two passes -- segments of 49 k symbols and more: C1, C3 -- has one pass in front of its last, and walking that
        // one in two rounds saves nothing: measured 10.2 against 9.4 ms per C3 burst)
        if (k.relay_quick && j.relay_budget >= 3 && j.segs.G > j.relay_budget && relay_w == 0) {
            for (int p = 0; p < 2 && p < j.relay_budget - 1; ++p) j.relay_apx[p] = p == j.relay_budget - 2 ? 2 : 1;
        }
    }
    for (int p = 0; p < 2; ++p) if (k.relay_apx_cfg[p] >= 0 && j.relay && j.segs.G > 1) j.relay_apx[p] = k.relay_apx_cfg[p];

    // What the relay passes buy is exact history: after p passes a symbol has between (p - 1) and p segments of exactly
    // walked trajectory in front of it, and the default's three passes are sized for the segments of the big LRIT bursts
    // (16.5 k symbols: 33 k .. 50 k symbols of history).  Where a call's segments are three times that long -- bursts at the
    // circuit rate, 2^28 samples without a decimator: 82 k (LRIT) or 130 k (HRIT) symbols per segment -- two passes leave more
    // history than that (measured at 49 k symbols per segment: 4.4e-5 rms from the serial trajectory against the three
    // passes' 6.4e-5, profiles/r3_late_experiments.txt), and the third pass, a third of the relay's time, is not run; nor is the watch on
    // the segment starts, which compares the starts of the last two passes (here the hand-off's own): the horizon of two
    // such passes already is that of the seven the watch would ask for.  The look at Es/N0 stays (clock_relay_look).
    j.relay_long = j.relay && !j.no_handoff && exact == 0 && k.auto_passes >= 3 && (long long)j.segs.cps * NS >= k.auto_long_seg;
    if (j.relay_long) j.relay_budget = 2;
    // (measured at C2: a pass that writes costs ~40 us more than one that does not -- 16-byte stores, 64 lines per wave
    // instruction --, a call whose last pass did not write pays the output pass, 175 us.  Writing from one pass earlier
    // than the previous call's last (two writing passes per call) was slower: 2.21 against 2.13 ms per step.)
    j.write_from = k.pass_writes ? (last_passes - 1 > 3 ? last_passes - 1 : 3) : 0x7fffffff;
    return j;
}

// ---- the overlap job's ranges
// history a warm walker 0 needs in front of the new samples: its warm-up, the symbols it stages in front of the carried
// position, the two symbols of history its start state interpolates
inline int clock_ov_pad_need(const ClockKnobs &k)
{
    const double wmax = (double)k.par.omega_mid + (double)k.par.omega_lim + 0.004;
    int need = (int)ceil((double)k.ov_hist * wmax) + XR_MM_NTAPS + XR_MM_FUDGE + 6 * (int)ceil(wmax) + 64;
    return (need + 15) & ~15;
}
// samples in front of the new ones in a call's buffer (ClockStage::xpad): the carried tail's 1024, or the history of
// clock_ov_pad_need -- only where the LDS-staged walker applies; else the pad stays what the carried tail needs
inline size_t clock_xpad(const ClockKnobs &k)
{
    const int need = clock_ov_pad_need(k);
    return k.ov_enabled && relay_ring_ok(k.par) && (size_t)need > 1024 ? (size_t)need : 1024;
}
// a call of n new samples is the overlap plan's; fixed_base: the call's samples lie where a caller put them (ClockStage::xbase_fixed)
inline bool clock_ov_eligible(const ClockKnobs &k, size_t xpad, bool fixed_base, size_t n)
{
    if (!k.ov_enabled || !k.ov_allow || k.exact != 0 || k.relay_quick || k.serial || k.relay_global || fixed_base) return false;
    if (k.relay_no_handoff == 0 || k.auto_passes <= 0) return false;       // (A/B switches that ask for round 3's / round 2's plans)
    if (k.relay_window > 0) return false;                                   // (cfg.clock_exact_window: the caller asks for the relay's segments)
    if ((size_t)clock_ov_pad_need(k) > xpad) return false;                  // (no LDS-staged walker at this symbol rate)
    if (n >= ((size_t)1 << 31) - xpad - 4096) return false;
    return (double)n / (double)k.par.omega_mid >= (double)k.ov_min;
}

struct ClockOvPlan {
    char err[128] = {0};
    long long N = 0, ni = 0;        // samples in [history | new], and how many of them a symbol may start at
    int padN = 0;                   // history samples in front of the new ones
    int G = 0, Ls = 0, first_bound = 0, store0 = 0, early = 0, stride = 0, hist = 0;
    bool w0_carried = false;        // walker 0 starts from the carried state (no history to warm up over)
    int w0_ii = 0;                  // buffer index the carried state's read index 0 corresponds to (padN - carry)
};
// have_hist: the call in front left clock_ov_pad_need samples and the timing curve that covers them; ahead: the call in
// front has not finished -- its carry is not known; such a job needs the history.
inline ClockOvPlan clock_ov_plan(const ClockKnobs &k, size_t n, size_t carry, bool have_hist, bool ahead)
{
    ClockOvPlan j;
    const ClockPar &par = k.par;
    const double wmax = (double)par.omega_mid + (double)par.omega_lim + 0.004, wmin = (double)par.omega_mid - (double)par.omega_lim;
    const int cw = (int)ceil(wmax);
    j.hist = (int)ceil((double)k.ov_hist * (double)par.omega_mid);
    j.early = (int)ceil(1.5 * wmax) + 2;
    if (ahead && !have_hist) { snprintf(j.err, sizeof j.err, "clock recovery: an overlap job cannot start ahead without the history of the call in front"); return j; }
    if (have_hist) {
        j.padN = clock_ov_pad_need(k);
        j.w0_carried = false;
        j.w0_ii = ahead ? 0 : j.padN - (int)carry;          // (ahead: the scan kernel is told at the call, ov_finalize)
        // the carried state reads its next symbol 19 .. 24 + a period samples in front of the new ones (the walk in front stops at
        // the first read index within 8 + 16 samples of its end): staging starts a period in front of that
        j.store0 = j.padN - (XR_MM_NTAPS + XR_MM_FUDGE) - cw - 2;
    } else {
        if (carry > 1024) { snprintf(j.err, sizeof j.err, "clock recovery: carry of %zu samples exceeds the hand-over buffer", carry); return j; }
        j.padN = (int)carry;
        j.w0_carried = true;
        j.w0_ii = 0;
        j.store0 = 0;
    }
    j.N = (long long)j.padN + (long long)n;
    j.ni = j.N - XR_MM_NTAPS - XR_MM_FUDGE;
    // walkers: ranges about as long as the history in front of them (every symbol is walked twice), at least 240 of them where
    // the call is long enough for ranges of 8192 symbols (few walkers: their latency is the call's), at most four per CU
    const double nsym = (double)n / (double)par.omega_mid;
    double gt = nsym / ((double)k.ov_hist * k.ov_lratio);
    if (gt < (double)k.ov_min_walkers) gt = (double)k.ov_min_walkers;
    if (nsym / gt < (double)k.ov_min_range) gt = nsym / (double)k.ov_min_range;
    // (at most 2.5 per CU: bursts at the circuit rate -- 63 M / 100 M symbols -- would take four per CU by the rule above; with 640
    // walkers of 98 k / 156 k symbols every symbol is walked 1.5 / 1.3 times instead of 1.8 / 1.5: C1 4.8 instead of 5.1 ms per
    // burst, C3 5.4 instead of 5.55 -- their latency is hidden like any other's)
    if (gt > 2.5 * k.cu_count) gt = 2.5 * k.cu_count;
    if (gt < 1.0) gt = 1.0;
    long long Ls = (long long)ceil((double)n / gt);
    Ls = (Ls + 63) & ~63LL;
    if (Ls < 4096) Ls = 4096;
    j.Ls = (int)Ls;
    // range 0 ends where walker 1 has its whole history behind it
    const long long w0_start = j.w0_carried ? 0 : (long long)j.store0 - j.hist;
    long long fb = w0_start + j.hist + Ls;
    if (fb < (long long)j.padN + Ls) fb = (long long)j.padN + Ls;
    j.first_bound = (int)fb;
    // (the last range is not shorter than a quarter of the others)
    const long long lim = j.N - Ls / 4;
    j.G = fb <= lim ? 2 + (int)((lim - fb) / Ls) : 1;
    const long long last_start = j.G >= 2 ? fb + (long long)(j.G - 2) * Ls : (long long)j.store0;
    long long longest = fb - j.store0;
    if (j.G >= 2 && Ls + j.early > longest) longest = Ls + j.early;
    if (j.N - last_start + j.early > longest) longest = j.N - last_start + j.early;
    if (j.G == 1) longest = j.N - j.store0;
    long long stride = (long long)ceil((double)longest / wmin) + 64;
    stride = (stride + 63) & ~63LL;
    if (stride * j.G >= (1LL << 31)) { snprintf(j.err, sizeof j.err, "clock recovery: call too long for the overlap plan"); return j; }
    j.stride = (int)stride;
    return j;
}

// ---- the looks at the control block after a wait (ctl: the host's copy)
// hand-off passes only -- cfg.clock_exact = 0 on a call too short for the relay to be planned at its start; -2: the fast
// configuration.  The hand-off passes normally stall at the recurrence's own floor, an rms residual of ~1e-4 sample (Es/N0
// 12 dB).  At low Es/N0 they stall at 5e-4 .. 1e-3 instead -- every wrong decision kicks mu by 2e-3 -- and which
// near-zero symbols then fall on the other side differs from the serial loop (a third
// of the 2..6 dB fuzz cases flip 1..5 decisions).  Such a call is closed exactly: the relay reproduces the
// serial trajectory whatever the noise.
// (... and a hand-off that never closed at all -- the pass budget ran out on an acquisition -- has every reason
// to be walked: the relay needs start states, not a closed hand-off)
inline bool clock_handoff_to_closure(const ClockKnobs &k, const int *ctl, int K, bool relay)
{
    if (!((k.exact == 0 || k.exact <= -2) && K > 1 && !relay)) return false;
    const float q = clock_ctl_float(ctl, CLK_CTL_SUM_SQ);
    const int open_ = ctl[CLK_CTL_OPEN_LAST];
    return ctl[CLK_CTL_DONE] == 0 || (open_ > 0 && q > k.auto_rms * k.auto_rms * (float)open_);
}

// the relay, after every wait.  What the call carries from look to look:
struct ClockRelayLook {
    bool first = true;          // nothing has been decided since the call's first batch
    bool relay_auto = false;    // the host has taken the call over (to closure, or four more passes)
    bool relay_force = false, no_handoff = false, relay_long = false;   // of the plan
    int relay_enq = 0, G = 0, relay_budget = 0;
};
enum ClockRelayVerdict {
    CLK_RELAY_TAKE,             // closed, or the budget is used up: the result stands
    CLK_RELAY_TO_CLOSURE,       // budget lifted (look again: continue to the limit)
    CLK_RELAY_FOUR_MORE,        // the starts still move: four more passes
    CLK_RELAY_NO_SIGNAL,        // a closure nobody asked for is not pursued on an input without a signal
    CLK_RELAY_CONTINUE,         // another batch, up to the limit
};
struct ClockRelayStep {
    ClockRelayVerdict verdict;
    bool relay_auto; int relay_budget;      // as the call goes on
    bool snr_seen; float snr2;              // the default's first look read 2 Es/N0
};
inline ClockRelayStep clock_relay_look(const ClockKnobs &k, const int *ctl, const ClockRelayLook &c)
{
    ClockRelayStep r{CLK_RELAY_TAKE, c.relay_auto, c.relay_budget, false, 0.f};
    const bool closed = ctl[CLK_CTL_RELAY_CLOSED] != 0;
    if (c.first && k.exact == 0 && !c.relay_auto && !closed) {
        // The default: after its three passes the segment starts of a clean signal move by a few 1e-4 sample rms from
        // pass to pass.  Where they still move by more -- low Es/N0: every decision that differs kicks mu by 2e-3 --,
        // or the hand-off passes never closed, the call is walked to closure: the serial trajectory whatever the noise.
        // Not to closure at once: four more passes at a time until the starts have settled too (Es/N0 6 dB: after six
        // passes, 4.4 ms per 2^28-sample burst; at 3 dB they never do before the relay closes, 40 passes).
        float shift_sq = clock_ctl_float(ctl, CLK_CTL_RELAY_SHIFT_SQ);
        const float snr2 = clock_ctl_float(ctl, CLK_CTL_SNR2);      // 2 Es/N0 as the first pass's soft symbols show it (12 dB: 32, 7 dB: 10)
        r.snr_seen = true; r.snr2 = snr2;
        // Below auto_snr the call is walked to closure: the serial trajectory whatever the noise (in a 2..6 dB fuzz
        // slice of 60 calls up to 350 k symbols the passes-until-settled rule alone left one hard decision different
        // from the serial trajectory's -- a call of 14 segments whose starts happened to move by 3e-4 -- and the
        // hand-off passes of rounds 2-3 ten).
        // (... unless there is no signal to speak of: |noise| alone shows 2 / (pi - 2) = 1.75, BPSK at Es/N0 0 dB 2.4; a
        // loop that is not locked has no trajectory to close on, the relay would run its G + 1 passes for nothing)
        const bool signal = snr2 >= k.auto_snr_floor;
        bool to_closure = signal && ((c.relay_force && !c.no_handoff) || !(snr2 >= k.auto_snr));
        if (!signal || to_closure || c.relay_long || c.no_handoff) shift_sq = 0.0f;
        // Without hand-off passes nothing has settled symbol slips between the timing guess and the loop: a start that moved
        // by the better part of a symbol between the first pass (the guess) and a later one (the end state of the segment
        // in front) means the guess counted a symbol more or less than the loop there, and every segment behind it is one
        // symbol off until the exact front reaches it -- the call is walked to closure.
        if (c.no_handoff && signal && !to_closure && !(clock_ctl_float(ctl, CLK_CTL_RELAY_MOVE_MAX) < 0.25f * k.sps)) to_closure = true;
        if (to_closure) { r.verdict = CLK_RELAY_TO_CLOSURE; r.relay_auto = true; r.relay_budget = 0; return r; }
        if (!(shift_sq <= k.auto_shift * k.auto_shift) && c.relay_enq < c.G + 1) {
            r.verdict = CLK_RELAY_FOUR_MORE; r.relay_auto = true; r.relay_budget = c.relay_enq + 4;
            return r;
        }
    }
    // the relay goes on until a pass changes nothing (or the pass budget of a partial closure is used up)
    if (closed || c.relay_enq >= clock_relay_limit(c.G, c.relay_budget)) return r;
    // (a closure nobody asked for -- cfg.clock_exact = 0 / -2 -- is not pursued on an input without a signal: an
    // unlocked loop has no trajectory to close on and would take all G + 1 passes)
    if (c.relay_auto && k.exact != 1 && !(clock_ctl_float(ctl, CLK_CTL_SNR2) >= k.auto_snr_floor)) { r.verdict = CLK_RELAY_NO_SIGNAL; return r; }
    r.verdict = CLK_RELAY_CONTINUE;
    return r;
}

// the overlap job: the default configuration's two looks at such a call -- Es/N0 below 7 dB: walked to closure, the serial
// trajectory whatever the noise --, and a joint whose two trajectories do not meet within a quarter symbol -- the timing guess
// and the loop disagree about a symbol count.  (No signal -- the walkers of a loop that is not locked do not meet at the joints
// --: the relay's own default, which does not pursue a closure on such an input either.)
enum ClockOvVerdict { CLK_OV_TAKE, CLK_OV_FALLBACK, CLK_OV_FALLBACK_TO_CLOSURE, CLK_OV_WATCHDOG };
inline ClockOvVerdict clock_overlap_look(const ClockKnobs &k, const int *ctl)
{
    if (ctl[CLK_CTL_STUCK]) return CLK_OV_WATCHDOG;
    const float snr2 = clock_ctl_float(ctl, CLK_CTL_SNR2);
    const bool signal = snr2 >= k.auto_snr_floor;
    if ((signal && !(snr2 >= k.auto_snr)) || ctl[CLK_CTL_OV_BAD_JOINTS] > 0) return signal ? CLK_OV_FALLBACK_TO_CLOSURE : CLK_OV_FALLBACK;
    return CLK_OV_TAKE;
}

// ---- what a call teaches the next one: passes enqueued before the host looks
inline int clock_next_relay_batch(int relay_passes)
{
    const int want = relay_passes + relay_passes / 4 + 8;
    return want < 32 ? 32 : (want > 4096 ? 4096 : want);
}
// one spare pass beyond what this call needed.  Unlike the Costas loop's, it is never dropped: the stall
// rule ends the passes one earlier or later from burst to burst (measured: one C2 burst in ten needs six
// instead of five), and a call that runs out of enqueued passes costs a host round trip, two more passes
// and a second output pass -- 0.5 ms against the 19 us the four idle launches take.
inline int clock_next_batch(int passes, bool relay)
{
    const int want = passes + 1;
    // (small calls run on while boundaries still freeze: 10..20 passes; a call that hands over to the relay after two
    // passes does not need five launches enqueued -- the idle ones are 10 us each)
    const int least = relay && passes <= 2 ? 3 : 5;
    return want < least ? least : (want > 32 ? 32 : want);
}

}  // namespace xrit
