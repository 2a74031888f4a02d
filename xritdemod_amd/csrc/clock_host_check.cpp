// clock_host_check.cpp -- the clock recovery's plain host parts (clock_plan.h, clock_ctl.h) in a program of their own.
// Built and run by `make clock-host-check` with -fsanitize=address,undefined; exits non-zero on the first failed check.
//
// What the plans are held against is NOT this header: EXPECT_ROWS / EXPECT_SUMS below were recorded from the arithmetic as
// it stood inside ClockStage::begin(), relay_plan(), ov_plan(), ov_eligible() and init() before it moved here (those
// lines, copied verbatim into a CPU program, run over run_grid()'s grid).  The default configuration's cases are spelled
// out value by value; every other configuration of the grid is held by a 64-bit FNV-1a sum over all its cases' values.
// The looks' table (check_looks) is written by hand from the rules: one row per branch, both sides of every threshold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "clock_plan.h"

using namespace xrit;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            return 1;                                                               \
        }                                                                           \
    } while (0)

// ---- the grid ------------------------------------------------------------------------------------------------------
struct GridCfg {
    int hrit;           // 0: LRIT (1.25 Msps / 293 883), 1: HRIT (2.5 Msps / 927 000), as the chain derives the symbol period
    int mode;           // cfg.clock_exact 0, 1, 3, -1, -2, and -3 (the default's plan with relay_quick)
    int window;         // cfg.clock_exact_window
    int one_walk_max;
};
static const int GRID_MODES[6] = {0, 1, 3, -1, -2, -3};

// the knobs as ClockStage::init and the chain's create leave them on an MI355X (256 CUs, 160 KiB of LDS)
static ClockKnobs grid_knobs(const GridCfg &c)
{
    ClockKnobs k;
    const float sps = c.hrit ? 2.5e6f / 927000.0f : 1.25e6f / 293883.0f;
    k.sps = sps;
    k.par.omega_mid = sps;
    k.par.omega_lim = sps * 0.005f;
    k.par.gain_omega = (0.0037f * 0.0037f) / 4.0f;
    k.par.gain_mu = 0.0037f;
    k.max_passes = 192;
    k.exact = c.mode == -3 ? 0 : c.mode;
    k.relay_quick = c.mode == -3;
    k.relay_window = c.window;
    k.one_walk_max = c.one_walk_max;
    return k;
}

// What is computed, behind one interface, so that the program that recorded the table could run the same grid over the
// arithmetic as it stood before.
struct PlanModel {
    ClockKnobs k;
    size_t xpad = 1024;
    void configure(const GridCfg &c) { k = grid_knobs(c); xpad = clock_xpad(k); }
    std::vector<long long> chain(size_t n, size_t carry)
    {
        const ClockChainPlan p = clock_chain_plan(k, n, carry, -1);
        if (p.err[0]) return {-1};
        if (p.short_input) return {1, p.N, p.ni};
        return {0, p.N, p.ni, p.SS, p.W, p.A, p.STEP, p.WS, p.wide, p.NG, p.waves_cu, (long long)p.tile_bytes, (long long)p.tile_bytes3,
                p.NS, p.K, p.relay, p.relay_budget, p.no_handoff, p.relay_apx[0], p.relay_apx[1], p.relay_long, p.write_from,
                p.relay ? p.segs.cps : 0, p.relay ? p.segs.G : 0, p.relay ? clock_relay_limit(p.segs.G, p.relay_budget) : 0};
    }
    // the stall rule's relay, cut in finish(): to closure, on the chains of a plan that has none
    std::vector<long long> late_relay(size_t n, size_t carry)
    {
        const ClockChainPlan p = clock_chain_plan(k, n, carry, -1);
        if (p.err[0] || p.short_input || p.relay) return {-1};
        const ClockRelaySegs s = clock_relay_segments(k, p.K, p.NS, p.no_handoff, 0, 0);
        return {s.cps, s.G, clock_relay_limit(s.G, 0)};
    }
    std::vector<long long> overlap(size_t n, size_t carry, bool have_hist, bool ahead)
    {
        const ClockOvPlan p = clock_ov_plan(k, n, carry, have_hist, ahead);
        if (p.err[0]) return {-1};
        return {0, p.hist, p.early, p.padN, p.w0_carried, p.w0_ii, p.store0, p.N, p.ni, p.Ls, p.first_bound, p.G, p.stride};
    }
    long long eligible(size_t n, bool allow) { ClockKnobs q = k; q.ov_allow = allow; return clock_ov_eligible(q, xpad, false, n); }
    long long pad_need() { return clock_ov_pad_need(k); }
    long long pad() { return (long long)xpad; }
    long long span64() { return relay_span(k.par, 64); }
};

struct GridSink {
    virtual void row(const std::string &key, const std::vector<long long> &v) = 0;     // a case spelled out
    virtual void sum(const std::string &key, unsigned long long h, int cases) = 0;      // a configuration's cases, summed
    virtual ~GridSink() {}
};

static void fnv(unsigned long long &h, const std::vector<long long> &v)
{
    for (long long x : v)
        for (int b = 0; b < 8; ++b) { h ^= (unsigned long long)(x >> (8 * b)) & 0xffull; h *= 1099511628211ull; }
    h ^= 0xffull; h *= 1099511628211ull;        // (a case ends)
}

// call sizes: in symbols (times the band's symbol period), and in samples
static std::vector<size_t> grid_sizes(double sps, size_t xpad, size_t carry)
{
    static const long long SYMS[] = {1500, 73000, 74500, 199000, 201000, 999000, 1001000, 5900000, 6100000};
    std::vector<size_t> n;
    n.push_back(0);
    n.push_back(20);                                // fewer samples than one symbol needs (with nothing carried)
    for (long long s : SYMS) n.push_back((size_t)((double)s * sps));
    n.push_back(((size_t)1 << 28) / 5);             // bench.py's bursts of 2^28 input samples: C2 (decimation 5),
    n.push_back(((size_t)1 << 28) / 32);            // C5 (decimation 32),
    n.push_back((size_t)1 << 28);                   // C1 and C3 (at the circuit rate)
    n.push_back(((size_t)1 << 31) - xpad - 4097);   // the longest call the overlap plan is asked about, and the first that is not
    n.push_back(((size_t)1 << 31) - xpad - 4096);
    n.push_back(((size_t)1 << 31) - 1 - carry);     // the longest call of all, and the first that is refused
    n.push_back(((size_t)1 << 31) - carry);
    n.push_back(((size_t)1 << 31) - 1);
    return n;
}
static const size_t GRID_CARRY[3] = {0, 19, 1024};

template <class Model> static void run_grid(Model &m, GridSink &out)
{
    for (int hrit = 0; hrit < 2; ++hrit)
        for (int mi = 0; mi < 6; ++mi)
            for (int window = 0; window <= 64; window += 64)
                for (int owm = 0; owm <= 200000; owm += 200000) {
                    const GridCfg c{hrit, GRID_MODES[mi], window, owm};
                    m.configure(c);
                    const bool spell = c.mode == 0 && window == 0;
                    char cfgkey[96];
                    snprintf(cfgkey, sizeof cfgkey, "%s exact=%d window=%d one_walk_max=%d", hrit ? "hrit" : "lrit", c.mode, window, owm);
                    const double sps = hrit ? (double)(2.5e6f / 927000.0f) : (double)(1.25e6f / 293883.0f);
                    unsigned long long h = 14695981039346656037ull;
                    int cases = 0;
                    fnv(h, {m.pad_need(), m.pad(), m.span64()}); ++cases;
                    if (spell && owm == 0) out.row(std::string(cfgkey) + " pad_need, xpad, span64", {m.pad_need(), m.pad(), m.span64()});
                    for (size_t carry : GRID_CARRY)
                        for (size_t n : grid_sizes(sps, (size_t)m.pad(), carry)) {
                            char key[192];
                            snprintf(key, sizeof key, "%s n=%zu carry=%zu", cfgkey, n, carry);
                            const std::vector<long long> ch = m.chain(n, carry), late = m.late_relay(n, carry);
                            const std::vector<long long> el = {m.eligible(n, true), m.eligible(n, false)};
                            fnv(h, ch); fnv(h, late); fnv(h, el); cases += 3;
                            if (spell && carry == 19) {
                                out.row(std::string(key) + " chain", ch);
                                out.row(std::string(key) + " eligible", el);
                            }
                            // the overlap job's ranges: wherever the plan would be asked, and one size below (its arithmetic
                            // does not depend on the other knobs of the grid: once per band)
                            if (mi == 0 && window == 0 && owm == 0 && n >= (size_t)(990000.0 * sps) && n < ((size_t)1 << 31) - (size_t)m.pad() - 4096)
                                for (int hh = 0; hh < 3; ++hh) {        // from the carried state / with history / with history, ahead
                                    const std::vector<long long> ov = m.overlap(n, carry, hh >= 1, hh == 2);
                                    fnv(h, ov); ++cases;
                                    if (carry == 19) out.row(std::string(key) + (hh == 0 ? " overlap, carried" : hh == 1 ? " overlap, history" : " overlap, ahead"), ov);
                                }
                        }
                    // ahead without history is refused
                    fnv(h, m.overlap((size_t)1 << 24, 0, false, true)); ++cases;
                    out.sum(cfgkey, h, cases);
                }
}

// ---- the recorded table ------------------------------------------------------------------------------------------------
struct ExpectRow { const char *key; std::vector<long long> v; };
struct ExpectSum { const char *key; unsigned long long h; int cases; };
// chain: {0, N, ni, SS, W, A, STEP, WS, wide, NG, waves_cu, tile_bytes, tile_bytes3, NS, K, relay, relay_budget, no_handoff, apx0, apx1,
//         relay_long, write_from, cps, G, relay_limit} | {1, N, ni}: short input | {-1}: refused
// overlap: {0, hist, early, padN, w0_carried, w0_ii, store0, N, ni, Ls, first_bound, G, stride} | {-1}: refused
// eligible: {the chain's call, a call that keeps stages or complex symbols}
static const ExpectRow EXPECT_ROWS[] = {
    {"lrit exact=0 window=0 one_walk_max=0 pad_need, xpad, span64", {210432, 210432, 298}},
    {"lrit exact=0 window=0 one_walk_max=0 n=0 carry=19 chain", {1, 19, -5}},
    {"lrit exact=0 window=0 one_walk_max=0 n=0 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=20 carry=19 chain", {0, 39, 15, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 3, 1, 4, 1, 0, 0, 0, 3, 3, 1, 2}},
    {"lrit exact=0 window=0 one_walk_max=0 n=20 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=6380 carry=19 chain", {0, 6399, 6375, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 26, 1, 4, 1, 0, 0, 0, 3, 26, 1, 2}},
    {"lrit exact=0 window=0 one_walk_max=0 n=6380 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=310497 carry=19 chain", {0, 310516, 310492, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 1149, 1, 2, 1, 0, 0, 0, 3, 1149, 1, 2}},
    {"lrit exact=0 window=0 one_walk_max=0 n=310497 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=316877 carry=19 chain", {0, 316896, 316872, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 1172, 1, 3, 0, 0, 0, 0, 3, 256, 5, 3}},
    {"lrit exact=0 window=0 one_walk_max=0 n=316877 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=846425 carry=19 chain", {0, 846444, 846420, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 3128, 1, 3, 0, 0, 0, 0, 3, 256, 13, 3}},
    {"lrit exact=0 window=0 one_walk_max=0 n=846425 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=854932 carry=19 chain", {0, 854951, 854927, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 3159, 1, 3, 0, 0, 0, 0, 3, 256, 13, 3}},
    {"lrit exact=0 window=0 one_walk_max=0 n=854932 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4249139 carry=19 chain", {0, 4249158, 4249134, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 15690, 1, 3, 0, 0, 0, 0, 3, 256, 62, 3}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4249139 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4249139 carry=19 overlap, carried", {0, 209063, 9, 19, 1, 0, 0, 4249158, 4249134, 34880, 243943, 116, 57728}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4249139 carry=19 overlap, history", {0, 209063, 9, 210432, 0, 210413, 210401, 4459571, 4459547, 34880, 245312, 122, 8320}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4249139 carry=19 overlap, ahead", {0, 209063, 9, 210432, 0, 0, 210401, 4459571, 4459547, 34880, 245312, 122, 8320}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4257646 carry=19 chain", {0, 4257665, 4257641, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 15722, 1, 3, 0, 0, 0, 0, 3, 256, 62, 3}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4257646 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4257646 carry=19 overlap, carried", {0, 209063, 9, 19, 1, 0, 0, 4257665, 4257641, 34880, 243943, 116, 57728}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4257646 carry=19 overlap, history", {0, 209063, 9, 210432, 0, 210413, 210401, 4468078, 4468054, 34880, 245312, 122, 8896}},
    {"lrit exact=0 window=0 one_walk_max=0 n=4257646 carry=19 overlap, ahead", {0, 209063, 9, 210432, 0, 0, 210401, 4468078, 4468054, 34880, 245312, 122, 8896}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25095019 carry=19 chain", {0, 25095038, 25095014, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 92653, 1, 3, 0, 0, 0, 0, 3, 256, 362, 3}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25095019 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25095019 carry=19 overlap, carried", {0, 209063, 9, 19, 1, 0, 0, 25095038, 25095014, 104576, 313639, 238, 74176}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25095019 carry=19 overlap, history", {0, 209063, 9, 210432, 0, 210413, 210401, 25305451, 25305427, 104576, 315008, 240, 24832}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25095019 carry=19 overlap, ahead", {0, 209063, 9, 210432, 0, 0, 210401, 25305451, 25305427, 104576, 315008, 240, 24832}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25945698 carry=19 chain", {0, 25945717, 25945693, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 95794, 1, 3, 1, 0, 0, 0, 3, 384, 250, 3}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25945698 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25945698 carry=19 overlap, carried", {0, 209063, 9, 19, 1, 0, 0, 25945717, 25945693, 108160, 317223, 238, 75072}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25945698 carry=19 overlap, history", {0, 209063, 9, 210432, 0, 210413, 210401, 26156130, 26156106, 108160, 318592, 240, 25664}},
    {"lrit exact=0 window=0 one_walk_max=0 n=25945698 carry=19 overlap, ahead", {0, 209063, 9, 210432, 0, 0, 210401, 26156130, 26156106, 108160, 318592, 240, 25664}},
    {"lrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 chain", {0, 53687110, 53687086, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 112, 113267, 1, 3, 1, 0, 0, 0, 3, 222, 511, 3}},
    {"lrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 overlap, carried", {0, 209063, 9, 19, 1, 0, 0, 53687110, 53687086, 209088, 418151, 256, 98880}},
    {"lrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 overlap, history", {0, 209063, 9, 210432, 0, 210413, 210401, 53897523, 53897499, 209088, 419520, 257, 49536}},
    {"lrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 overlap, ahead", {0, 209063, 9, 210432, 0, 0, 210401, 53897523, 53897499, 209088, 419520, 257, 49536}},
    {"lrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 chain", {0, 8388627, 8388603, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 30973, 1, 3, 0, 0, 0, 0, 3, 256, 121, 3}},
    {"lrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 overlap, carried", {0, 209063, 9, 19, 1, 0, 0, 8388627, 8388603, 35008, 244071, 234, 57792}},
    {"lrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 overlap, history", {0, 209063, 9, 210432, 0, 210413, 210401, 8599040, 8599016, 35008, 245440, 240, 8384}},
    {"lrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 overlap, ahead", {0, 209063, 9, 210432, 0, 0, 210401, 8599040, 8599016, 35008, 245440, 240, 8384}},
    {"lrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 chain", {0, 268435475, 268435451, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 192, 330357, 1, 2, 1, 0, 0, 0, 3, 323, 1023, 2}},
    {"lrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 overlap, carried", {0, 209063, 9, 19, 1, 0, 0, 268435475, 268435451, 419456, 628519, 640, 148608}},
    {"lrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 overlap, history", {0, 209063, 9, 210432, 0, 210413, 210401, 268645888, 268645864, 419456, 629888, 640, 99200}},
    {"lrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 overlap, ahead", {0, 209063, 9, 210432, 0, 0, 210401, 268645888, 268645864, 419456, 629888, 640, 99200}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147269119 carry=19 chain", {0, 2147269138, 2147269114, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 256, 1981931, 1, 2, 1, 0, 0, 0, 3, 1936, 1024, 2}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147269119 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147269119 carry=19 overlap, carried", {0, 209063, 9, 19, 1, 0, 0, 2147269138, 2147269114, 3355136, 3564199, 640, 842304}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147269119 carry=19 overlap, history", {0, 209063, 9, 210432, 0, 210413, 210401, 2147479551, 2147479527, 3355136, 3565568, 640, 792896}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147269119 carry=19 overlap, ahead", {0, 209063, 9, 210432, 0, 0, 210401, 2147479551, 2147479527, 3355136, 3565568, 640, 792896}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147269120 carry=19 chain", {0, 2147269139, 2147269115, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 256, 1981931, 1, 2, 1, 0, 0, 0, 3, 1936, 1024, 2}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147269120 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147483628 carry=19 chain", {0, 2147483647, 2147483623, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 256, 1982129, 1, 2, 1, 0, 0, 0, 3, 1936, 1024, 2}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147483628 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147483629 carry=19 chain", {-1}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147483629 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147483647 carry=19 chain", {-1}},
    {"lrit exact=0 window=0 one_walk_max=0 n=2147483647 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=0 carry=19 chain", {1, 19, -5}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=0 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=20 carry=19 chain", {0, 39, 15, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 3, 1, 4, 1, 0, 0, 0, 3, 3, 1, 2}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=20 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=6380 carry=19 chain", {0, 6399, 6375, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 26, 1, 4, 1, 0, 0, 0, 3, 26, 1, 2}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=6380 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=310497 carry=19 chain", {0, 310516, 310492, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 1149, 1, 2, 1, 0, 0, 0, 3, 1149, 1, 2}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=310497 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=316877 carry=19 chain", {0, 316896, 316872, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 1172, 1, 2, 1, 0, 0, 0, 3, 1172, 1, 2}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=316877 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=846425 carry=19 chain", {0, 846444, 846420, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 3128, 1, 3, 0, 0, 0, 0, 3, 256, 13, 3}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=846425 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=854932 carry=19 chain", {0, 854951, 854927, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 3159, 1, 3, 0, 0, 0, 0, 3, 256, 13, 3}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=854932 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=4249139 carry=19 chain", {0, 4249158, 4249134, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 15690, 1, 3, 0, 0, 0, 0, 3, 256, 62, 3}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=4249139 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=4257646 carry=19 chain", {0, 4257665, 4257641, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 15722, 1, 3, 0, 0, 0, 0, 3, 256, 62, 3}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=4257646 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=25095019 carry=19 chain", {0, 25095038, 25095014, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 92653, 1, 3, 0, 0, 0, 0, 3, 256, 362, 3}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=25095019 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=25945698 carry=19 chain", {0, 25945717, 25945693, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 95794, 1, 3, 1, 0, 0, 0, 3, 384, 250, 3}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=25945698 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=53687091 carry=19 chain", {0, 53687110, 53687086, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 112, 113267, 1, 3, 1, 0, 0, 0, 3, 222, 511, 3}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=53687091 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=8388608 carry=19 chain", {0, 8388627, 8388603, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 64, 30973, 1, 3, 0, 0, 0, 0, 3, 256, 121, 3}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=8388608 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=268435456 carry=19 chain", {0, 268435475, 268435451, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 192, 330357, 1, 2, 1, 0, 0, 0, 3, 323, 1023, 2}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=268435456 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147269119 carry=19 chain", {0, 2147269138, 2147269114, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 256, 1981931, 1, 2, 1, 0, 0, 0, 3, 1936, 1024, 2}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147269119 carry=19 eligible", {1, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147269120 carry=19 chain", {0, 2147269139, 2147269115, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 256, 1981931, 1, 2, 1, 0, 0, 0, 3, 1936, 1024, 2}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147269120 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147483628 carry=19 chain", {0, 2147483647, 2147483623, 4, 32, 19, 1115001, 39, 0, 7, 7, 149312, 25920, 256, 1982129, 1, 2, 1, 0, 0, 0, 3, 1936, 1024, 2}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147483628 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147483629 carry=19 chain", {-1}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147483629 carry=19 eligible", {0, 0}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147483647 carry=19 chain", {-1}},
    {"lrit exact=0 window=0 one_walk_max=200000 n=2147483647 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 pad_need, xpad, span64", {133536, 133536, 198}},
    {"hrit exact=0 window=0 one_walk_max=0 n=0 carry=19 chain", {1, 19, -5}},
    {"hrit exact=0 window=0 one_walk_max=0 n=0 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=20 carry=19 chain", {0, 39, 15, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 3, 1, 4, 1, 0, 0, 0, 3, 3, 1, 2}},
    {"hrit exact=0 window=0 one_walk_max=0 n=20 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=4045 carry=19 chain", {0, 4064, 4040, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 26, 1, 4, 1, 0, 0, 0, 3, 26, 1, 2}},
    {"hrit exact=0 window=0 one_walk_max=0 n=4045 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=196871 carry=19 chain", {0, 196890, 196866, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 1149, 1, 2, 1, 0, 0, 0, 3, 1149, 1, 2}},
    {"hrit exact=0 window=0 one_walk_max=0 n=196871 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=200916 carry=19 chain", {0, 200935, 200911, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 1173, 1, 3, 0, 0, 0, 0, 3, 256, 5, 3}},
    {"hrit exact=0 window=0 one_walk_max=0 n=200916 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=536677 carry=19 chain", {0, 536696, 536672, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 3128, 1, 3, 0, 0, 0, 0, 3, 256, 13, 3}},
    {"hrit exact=0 window=0 one_walk_max=0 n=536677 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=542071 carry=19 chain", {0, 542090, 542066, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 3159, 1, 3, 0, 0, 0, 0, 3, 256, 13, 3}},
    {"hrit exact=0 window=0 one_walk_max=0 n=542071 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2694174 carry=19 chain", {0, 2694193, 2694169, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 15690, 1, 3, 0, 0, 0, 0, 3, 256, 62, 3}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2694174 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2694174 carry=19 overlap, carried", {0, 132557, 7, 19, 1, 0, 0, 2694193, 2694169, 22144, 154701, 116, 57728}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2694174 carry=19 overlap, history", {0, 132557, 7, 133536, 0, 133517, 133507, 2827710, 2827686, 22144, 155680, 122, 8384}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2694174 carry=19 overlap, ahead", {0, 132557, 7, 133536, 0, 0, 133507, 2827710, 2827686, 22144, 155680, 122, 8384}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2699568 carry=19 chain", {0, 2699587, 2699563, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 15722, 1, 3, 0, 0, 0, 0, 3, 256, 62, 3}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2699568 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2699568 carry=19 overlap, carried", {0, 132557, 7, 19, 1, 0, 0, 2699587, 2699563, 22144, 154701, 116, 57728}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2699568 carry=19 overlap, history", {0, 132557, 7, 133536, 0, 133517, 133507, 2833104, 2833080, 22144, 155680, 122, 8384}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2699568 carry=19 overlap, ahead", {0, 132557, 7, 133536, 0, 0, 133507, 2833104, 2833080, 22144, 155680, 122, 8384}},
    {"hrit exact=0 window=0 one_walk_max=0 n=15911541 carry=19 chain", {0, 15911560, 15911536, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 92653, 1, 3, 0, 0, 0, 0, 3, 256, 362, 3}},
    {"hrit exact=0 window=0 one_walk_max=0 n=15911541 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=15911541 carry=19 overlap, carried", {0, 132557, 7, 19, 1, 0, 0, 15911560, 15911536, 66304, 198861, 238, 74176}},
    {"hrit exact=0 window=0 one_walk_max=0 n=15911541 carry=19 overlap, history", {0, 132557, 7, 133536, 0, 133517, 133507, 16045077, 16045053, 66304, 199840, 240, 24832}},
    {"hrit exact=0 window=0 one_walk_max=0 n=15911541 carry=19 overlap, ahead", {0, 132557, 7, 133536, 0, 0, 133507, 16045077, 16045053, 66304, 199840, 240, 24832}},
    {"hrit exact=0 window=0 one_walk_max=0 n=16450916 carry=19 chain", {0, 16450935, 16450911, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 95794, 1, 3, 1, 0, 0, 0, 3, 384, 250, 3}},
    {"hrit exact=0 window=0 one_walk_max=0 n=16450916 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=16450916 carry=19 overlap, carried", {0, 132557, 7, 19, 1, 0, 0, 16450935, 16450911, 68608, 201165, 238, 75072}},
    {"hrit exact=0 window=0 one_walk_max=0 n=16450916 carry=19 overlap, history", {0, 132557, 7, 133536, 0, 133517, 133507, 16584452, 16584428, 68608, 202144, 240, 25664}},
    {"hrit exact=0 window=0 one_walk_max=0 n=16450916 carry=19 overlap, ahead", {0, 132557, 7, 133536, 0, 0, 133507, 16584452, 16584428, 68608, 202144, 240, 25664}},
    {"hrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 chain", {0, 53687110, 53687086, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 176, 113680, 1, 3, 1, 0, 0, 0, 3, 223, 510, 3}},
    {"hrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 overlap, carried", {0, 132557, 7, 19, 1, 0, 0, 53687110, 53687086, 132608, 265165, 404, 98944}},
    {"hrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 overlap, history", {0, 132557, 7, 133536, 0, 133517, 133507, 53820627, 53820603, 132608, 266144, 405, 49536}},
    {"hrit exact=0 window=0 one_walk_max=0 n=53687091 carry=19 overlap, ahead", {0, 132557, 7, 133536, 0, 0, 133507, 53820627, 53820603, 132608, 266144, 405, 49536}},
    {"hrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 chain", {0, 8388627, 8388603, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 48848, 1, 3, 0, 0, 0, 0, 3, 256, 191, 3}},
    {"hrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 overlap, carried", {0, 132557, 7, 19, 1, 0, 0, 8388627, 8388603, 35008, 167565, 236, 62528}},
    {"hrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 overlap, history", {0, 132557, 7, 133536, 0, 133517, 133507, 8522144, 8522120, 35008, 168544, 240, 13184}},
    {"hrit exact=0 window=0 one_walk_max=0 n=8388608 carry=19 overlap, ahead", {0, 132557, 7, 133536, 0, 0, 133507, 8522144, 8522120, 35008, 168544, 240, 13184}},
    {"hrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 chain", {0, 268435475, 268435451, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 224, 446592, 1, 2, 1, 0, 0, 0, 3, 437, 1022, 2}},
    {"hrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 overlap, carried", {0, 132557, 7, 19, 1, 0, 0, 268435475, 268435451, 419456, 552013, 640, 205824}},
    {"hrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 overlap, history", {0, 132557, 7, 133536, 0, 133517, 133507, 268568992, 268568968, 419456, 552992, 640, 156416}},
    {"hrit exact=0 window=0 one_walk_max=0 n=268435456 carry=19 overlap, ahead", {0, 132557, 7, 133536, 0, 0, 133507, 268568992, 268568968, 419456, 552992, 640, 156416}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147346015 carry=19 chain", {0, 2147346034, 2147346010, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 256, 3125929, 1, 2, 1, 0, 0, 0, 3, 3053, 1024, 2}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147346015 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147346015 carry=19 overlap, carried", {0, 132557, 7, 19, 1, 0, 0, 2147346034, 2147346010, 3355264, 3487821, 640, 1299904}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147346015 carry=19 overlap, history", {0, 132557, 7, 133536, 0, 133517, 133507, 2147479551, 2147479527, 3355264, 3488800, 640, 1250496}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147346015 carry=19 overlap, ahead", {0, 132557, 7, 133536, 0, 0, 133507, 2147479551, 2147479527, 3355264, 3488800, 640, 1250496}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147346016 carry=19 chain", {0, 2147346035, 2147346011, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 256, 3125929, 1, 2, 1, 0, 0, 0, 3, 3053, 1024, 2}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147346016 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147483628 carry=19 chain", {0, 2147483647, 2147483623, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 256, 3126129, 1, 2, 1, 0, 0, 0, 3, 3053, 1024, 2}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147483628 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147483629 carry=19 chain", {-1}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147483629 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147483647 carry=19 chain", {-1}},
    {"hrit exact=0 window=0 one_walk_max=0 n=2147483647 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=0 carry=19 chain", {1, 19, -5}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=0 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=20 carry=19 chain", {0, 39, 15, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 3, 1, 4, 1, 0, 0, 0, 3, 3, 1, 2}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=20 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=4045 carry=19 chain", {0, 4064, 4040, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 26, 1, 4, 1, 0, 0, 0, 3, 26, 1, 2}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=4045 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=196871 carry=19 chain", {0, 196890, 196866, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 1149, 1, 2, 1, 0, 0, 0, 3, 1149, 1, 2}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=196871 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=200916 carry=19 chain", {0, 200935, 200911, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 1173, 1, 2, 1, 0, 0, 0, 3, 1173, 1, 2}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=200916 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=536677 carry=19 chain", {0, 536696, 536672, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 3128, 1, 3, 0, 0, 0, 0, 3, 256, 13, 3}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=536677 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=542071 carry=19 chain", {0, 542090, 542066, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 3159, 1, 3, 0, 0, 0, 0, 3, 256, 13, 3}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=542071 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2694174 carry=19 chain", {0, 2694193, 2694169, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 15690, 1, 3, 0, 0, 0, 0, 3, 256, 62, 3}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2694174 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2699568 carry=19 chain", {0, 2699587, 2699563, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 15722, 1, 3, 0, 0, 0, 0, 3, 256, 62, 3}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2699568 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=15911541 carry=19 chain", {0, 15911560, 15911536, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 92653, 1, 3, 0, 0, 0, 0, 3, 256, 362, 3}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=15911541 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=16450916 carry=19 chain", {0, 16450935, 16450911, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 95794, 1, 3, 1, 0, 0, 0, 3, 384, 250, 3}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=16450916 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=53687091 carry=19 chain", {0, 53687110, 53687086, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 176, 113680, 1, 3, 1, 0, 0, 0, 3, 223, 510, 3}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=53687091 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=8388608 carry=19 chain", {0, 8388627, 8388603, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 64, 48848, 1, 3, 0, 0, 0, 0, 3, 256, 191, 3}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=8388608 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=268435456 carry=19 chain", {0, 268435475, 268435451, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 224, 446592, 1, 2, 1, 0, 0, 0, 3, 437, 1022, 2}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=268435456 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147346015 carry=19 chain", {0, 2147346034, 2147346010, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 256, 3125929, 1, 2, 1, 0, 0, 0, 3, 3053, 1024, 2}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147346015 carry=19 eligible", {1, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147346016 carry=19 chain", {0, 2147346035, 2147346011, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 256, 3125929, 1, 2, 1, 0, 0, 0, 3, 3053, 1024, 2}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147346016 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147483628 carry=19 chain", {0, 2147483647, 2147483623, 4, 32, 12, 706968, 39, 0, 7, 7, 149312, 25920, 256, 3126129, 1, 2, 1, 0, 0, 0, 3, 3053, 1024, 2}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147483628 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147483629 carry=19 chain", {-1}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147483629 carry=19 eligible", {0, 0}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147483647 carry=19 chain", {-1}},
    {"hrit exact=0 window=0 one_walk_max=200000 n=2147483647 carry=19 eligible", {0, 0}},
};
static const ExpectSum EXPECT_SUMS[] = {
    {"lrit exact=0 window=0 one_walk_max=0", 0xfd32af3e44036087ull, 245},
    {"lrit exact=0 window=0 one_walk_max=200000", 0xc9bb4aad19d0ad23ull, 173},
    {"lrit exact=0 window=64 one_walk_max=0", 0xd00effdc55d352ecull, 173},
    {"lrit exact=0 window=64 one_walk_max=200000", 0x9ba2edb4f12f35c8ull, 173},
    {"lrit exact=1 window=0 one_walk_max=0", 0xc55f358f9e171f87ull, 173},
    {"lrit exact=1 window=0 one_walk_max=200000", 0xc55f358f9e171f87ull, 173},
    {"lrit exact=1 window=64 one_walk_max=0", 0xc90b8b16bb9589aaull, 173},
    {"lrit exact=1 window=64 one_walk_max=200000", 0xc90b8b16bb9589aaull, 173},
    {"lrit exact=3 window=0 one_walk_max=0", 0x3719d12f9bd637eaull, 173},
    {"lrit exact=3 window=0 one_walk_max=200000", 0x3719d12f9bd637eaull, 173},
    {"lrit exact=3 window=64 one_walk_max=0", 0x5121256b9e712e1dull, 173},
    {"lrit exact=3 window=64 one_walk_max=200000", 0x5121256b9e712e1dull, 173},
    {"lrit exact=-1 window=0 one_walk_max=0", 0x49a3cc6c4613d785ull, 173},
    {"lrit exact=-1 window=0 one_walk_max=200000", 0x49a3cc6c4613d785ull, 173},
    {"lrit exact=-1 window=64 one_walk_max=0", 0x751c2dd1c7417fd2ull, 173},
    {"lrit exact=-1 window=64 one_walk_max=200000", 0x751c2dd1c7417fd2ull, 173},
    {"lrit exact=-2 window=0 one_walk_max=0", 0x49a3cc6c4613d785ull, 173},
    {"lrit exact=-2 window=0 one_walk_max=200000", 0x49a3cc6c4613d785ull, 173},
    {"lrit exact=-2 window=64 one_walk_max=0", 0x751c2dd1c7417fd2ull, 173},
    {"lrit exact=-2 window=64 one_walk_max=200000", 0x751c2dd1c7417fd2ull, 173},
    {"lrit exact=-3 window=0 one_walk_max=0", 0xe7e395538c25cdafull, 173},
    {"lrit exact=-3 window=0 one_walk_max=200000", 0x2d7801f436fe12a4ull, 173},
    {"lrit exact=-3 window=64 one_walk_max=0", 0x39cd6b7e608c478cull, 173},
    {"lrit exact=-3 window=64 one_walk_max=200000", 0x1a175bfe9fa6dbe8ull, 173},
    {"hrit exact=0 window=0 one_walk_max=0", 0x1f2f1897bdfdaf92ull, 245},
    {"hrit exact=0 window=0 one_walk_max=200000", 0xf51a3b8dd3e92afeull, 173},
    {"hrit exact=0 window=64 one_walk_max=0", 0xdf4def4d8acdf876ull, 173},
    {"hrit exact=0 window=64 one_walk_max=200000", 0x3ab4edc186fe52e6ull, 173},
    {"hrit exact=1 window=0 one_walk_max=0", 0x1ea7596ecda24ff7ull, 173},
    {"hrit exact=1 window=0 one_walk_max=200000", 0x1ea7596ecda24ff7ull, 173},
    {"hrit exact=1 window=64 one_walk_max=0", 0xea2c251f4abc6e8dull, 173},
    {"hrit exact=1 window=64 one_walk_max=200000", 0xea2c251f4abc6e8dull, 173},
    {"hrit exact=3 window=0 one_walk_max=0", 0xe6f5b88071bfca52ull, 173},
    {"hrit exact=3 window=0 one_walk_max=200000", 0xe6f5b88071bfca52ull, 173},
    {"hrit exact=3 window=64 one_walk_max=0", 0x64376ced13a13f43ull, 173},
    {"hrit exact=3 window=64 one_walk_max=200000", 0x64376ced13a13f43ull, 173},
    {"hrit exact=-1 window=0 one_walk_max=0", 0x7ce624c3f0620487ull, 173},
    {"hrit exact=-1 window=0 one_walk_max=200000", 0x7ce624c3f0620487ull, 173},
    {"hrit exact=-1 window=64 one_walk_max=0", 0xfe4b6078aa897681ull, 173},
    {"hrit exact=-1 window=64 one_walk_max=200000", 0xfe4b6078aa897681ull, 173},
    {"hrit exact=-2 window=0 one_walk_max=0", 0x7ce624c3f0620487ull, 173},
    {"hrit exact=-2 window=0 one_walk_max=200000", 0x7ce624c3f0620487ull, 173},
    {"hrit exact=-2 window=64 one_walk_max=0", 0xfe4b6078aa897681ull, 173},
    {"hrit exact=-2 window=64 one_walk_max=200000", 0xfe4b6078aa897681ull, 173},
    {"hrit exact=-3 window=0 one_walk_max=0", 0x49a64bc5c3856a69ull, 173},
    {"hrit exact=-3 window=0 one_walk_max=200000", 0xe08158621aa18451ull, 173},
    {"hrit exact=-3 window=64 one_walk_max=0", 0x55b82bba2b0fbb16ull, 173},
    {"hrit exact=-3 window=64 one_walk_max=200000", 0xbf3f98b8729a9006ull, 173},
};

struct CheckSink : GridSink {
    size_t ir = 0, is = 0;
    int bad = 0;
    void row(const std::string &key, const std::vector<long long> &v) override
    {
        const size_t n = sizeof EXPECT_ROWS / sizeof EXPECT_ROWS[0];
        if (ir >= n || key != EXPECT_ROWS[ir].key || v != EXPECT_ROWS[ir].v) {
            if (bad++ < 8) {
                std::fprintf(stderr, "plan differs from the record: %s:", key.c_str());
                for (long long x : v) std::fprintf(stderr, " %lld", x);
                std::fprintf(stderr, "\n  recorded as %s:", ir < n ? EXPECT_ROWS[ir].key : "(nothing)");
                if (ir < n) for (long long x : EXPECT_ROWS[ir].v) std::fprintf(stderr, " %lld", x);
                std::fprintf(stderr, "\n");
            }
        }
        ++ir;
    }
    void sum(const std::string &key, unsigned long long h, int cases) override
    {
        const size_t n = sizeof EXPECT_SUMS / sizeof EXPECT_SUMS[0];
        if (is >= n || key != EXPECT_SUMS[is].key || h != EXPECT_SUMS[is].h || cases != EXPECT_SUMS[is].cases) {
            if (bad++ < 8) std::fprintf(stderr, "plans of \"%s\" differ from the record: sum %016llx over %d cases\n", key.c_str(), h, cases);
        }
        ++is;
    }
    bool complete() const { return ir == sizeof EXPECT_ROWS / sizeof EXPECT_ROWS[0] && is == sizeof EXPECT_SUMS / sizeof EXPECT_SUMS[0]; }
};

// ---- the numbers DESIGN.md sections 5-6 and the comments quote ------------------------------------------------------------
static int check_design_numbers()
{
    const size_t burst = (size_t)1 << 28;
    ClockKnobs lrit = grid_knobs(GridCfg{0, 0, 0, 0}), hrit = grid_knobs(GridCfg{1, 0, 0, 0});
    // C2 (LRIT, decimation 5): 7 waves per CU by LDS, 1792 resident waves, one generation of 112-symbol chains, 113 k hand-offs
    const ClockChainPlan c2 = clock_chain_plan(lrit, burst / 5, 19, -1);
    CHECK(!c2.err[0] && c2.waves_cu == 7 && lrit.cu_count * c2.waves_cu == 1792 && c2.NS == 112 && c2.K == 113267);
    // ... relayed from the timing guess over two segments per CU of 24.8 k symbols, three passes
    CHECK(c2.relay && c2.no_handoff && c2.segs.G == 511 && c2.segs.cps * c2.NS == 24864 && c2.relay_budget == 3);
    // ... three per CU behind hand-off passes (cfg.clock_exact = 1): 766 segments of 16.5 k symbols
    ClockKnobs closure = lrit; closure.exact = 1;
    const ClockChainPlan c2x = clock_chain_plan(closure, burst / 5, 19, -1);
    CHECK(c2x.relay && !c2x.no_handoff && c2x.segs.G == 766 && c2x.segs.cps * c2x.NS == 16576 && c2x.relay_budget == 0);
    // ... one per CU (XRIT_RELAY_PER_CU=1): 256 segments of 49.6 k symbols, which two passes go with
    ClockKnobs one = lrit; one.relay_per_cu = 1; one.relay_per_cu_set = true;
    const ClockChainPlan c2o = clock_chain_plan(one, burst / 5, 19, -1);
    CHECK(c2o.segs.G == 256 && c2o.segs.cps * c2o.NS == 49616 && c2o.relay_budget == 2);
    // C5 (decimation 32, 2 M symbols): two hand-off passes' worth of start, three relay passes over 121 segments of 16 k symbols
    const ClockChainPlan c5 = clock_chain_plan(lrit, burst / 32, 19, -1);
    CHECK(c5.relay && !c5.no_handoff && c5.segs.G == 121 && c5.relay_budget == 3);
    // C1 / C3 at the circuit rate, relayed: four walkers per CU, 1023 / 1022 segments of 62 k / 97 k symbols, two passes
    const ClockChainPlan c1 = clock_chain_plan(lrit, burst, 19, -1), c3 = clock_chain_plan(hrit, burst, 19, -1);
    CHECK(c1.no_handoff && c1.segs.G == 1023 && c1.segs.cps * c1.NS / 1000 == 62 && c1.relay_budget == 2);
    CHECK(c3.no_handoff && c3.segs.G == 1022 && c3.segs.cps * c3.NS / 1000 == 97 && c3.relay_budget == 2);
    // the overlap plan's walkers per burst: C1 and C3 640 (2.5 per CU) over ranges of 98 k / 156 k symbols behind 49 k of
    // history (147 k / 205 k walked), C5 240
    const ClockOvPlan o1 = clock_ov_plan(lrit, burst, 19, true, false), o3 = clock_ov_plan(hrit, burst, 19, true, false);
    const ClockOvPlan o5 = clock_ov_plan(lrit, burst / 32, 19, true, false);
    CHECK(o1.G == 640 && (int)(o1.Ls / lrit.sps / 1000.f) == 98 && (int)((o1.Ls + o1.hist) / lrit.sps / 1000.f) == 147);
    CHECK(o3.G == 640 && (int)(o3.Ls / hrit.sps / 1000.f) == 155 && (int)((o3.Ls + o3.hist) / hrit.sps / 1000.f) == 204);
    CHECK(o5.G == 240 && (int)((o5.Ls + o5.hist) / lrit.sps / 1000.f) == 57);
    // C2: 257 walkers of 98 k symbols (ranges about one history long)
    const ClockOvPlan o2 = clock_ov_plan(lrit, burst / 5, 19, true, false);
    CHECK(o2.G == 257 && (int)((o2.Ls + o2.hist) / lrit.sps / 1000.f) == 98);
    return 0;
}

// ---- the looks ------------------------------------------------------------------------------------------------------------
struct Ctl {
    int w[CLK_CTL_WORDS] = {0};
    Ctl &i(ClockCtlWord k, int v) { w[k] = v; return *this; }
    Ctl &f(ClockCtlWord k, float v) { clock_ctl_set_float(w, k, v); return *this; }
};

static int check_looks()
{
    ClockKnobs k = grid_knobs(GridCfg{0, 0, 0, 0});
    // ---- hand-off passes only: the stall rule (auto_rms 3e-4: summed r^2 against 9e-8 per open boundary)
    {
        ClockKnobs fast = k; fast.exact = -2;
        const float lim = k.auto_rms * k.auto_rms * 100.f;
        Ctl closed_low; closed_low.i(CLK_CTL_DONE, 1).i(CLK_CTL_OPEN_LAST, 100).f(CLK_CTL_SUM_SQ, lim);
        Ctl closed_high; closed_high.i(CLK_CTL_DONE, 1).i(CLK_CTL_OPEN_LAST, 100).f(CLK_CTL_SUM_SQ, nextafterf(lim, 1.f));
        Ctl none_open; none_open.i(CLK_CTL_DONE, 1).i(CLK_CTL_OPEN_LAST, 0).f(CLK_CTL_SUM_SQ, 1.f);
        Ctl never; never.i(CLK_CTL_DONE, 0);
        CHECK(!clock_handoff_to_closure(fast, closed_low.w, 100, false));       // at the threshold: not above it
        CHECK(clock_handoff_to_closure(fast, closed_high.w, 100, false));       // stalled above auto_rms
        CHECK(!clock_handoff_to_closure(fast, none_open.w, 100, false));        // nothing open: nothing stalled
        CHECK(clock_handoff_to_closure(fast, never.w, 100, false));             // never closed
        CHECK(clock_handoff_to_closure(k, closed_high.w, 100, false));          // cfg.clock_exact = 0, a call the relay was not planned for
        CHECK(!clock_handoff_to_closure(k, closed_high.w, 100, true));          // ... the relay is planned: its own looks
        CHECK(!clock_handoff_to_closure(fast, closed_high.w, 1, false));        // one chain: no hand-off
        ClockKnobs off = k; off.exact = -1;
        CHECK(!clock_handoff_to_closure(off, never.w, 100, false));             // -1: never relayed
        ClockKnobs on = k; on.exact = 1;
        CHECK(!clock_handoff_to_closure(on, never.w, 100, false));
    }
    // ---- the relay.  A call of 20 segments, three passes enqueued out of a budget of three
    {
        ClockRelayLook c; c.G = 20; c.relay_enq = 3; c.relay_budget = 3;
        const float shift_ok = k.auto_shift * k.auto_shift, shift_hi = nextafterf(shift_ok, 1.f);
        Ctl clean; clean.f(CLK_CTL_SNR2, 32.f).f(CLK_CTL_RELAY_SHIFT_SQ, shift_ok).f(CLK_CTL_RELAY_MOVE_MAX, 1e-3f);
        ClockRelayStep r = clock_relay_look(k, clean.w, c);
        CHECK(r.verdict == CLK_RELAY_TAKE && !r.relay_auto && r.relay_budget == 3 && r.snr_seen && r.snr2 == 32.f);     // settled: take
        // Es/N0: 2 Es/N0 at auto_snr is taken, just below goes to closure, just below the floor is no signal
        Ctl at_snr = clean; at_snr.f(CLK_CTL_SNR2, k.auto_snr);
        CHECK(clock_relay_look(k, at_snr.w, c).verdict == CLK_RELAY_TAKE);
        Ctl low = clean; low.f(CLK_CTL_SNR2, nextafterf(k.auto_snr, 0.f));
        r = clock_relay_look(k, low.w, c);
        CHECK(r.verdict == CLK_RELAY_TO_CLOSURE && r.relay_auto && r.relay_budget == 0);
        Ctl at_floor = clean; at_floor.f(CLK_CTL_SNR2, k.auto_snr_floor);
        CHECK(clock_relay_look(k, at_floor.w, c).verdict == CLK_RELAY_TO_CLOSURE);
        Ctl noise = clean; noise.f(CLK_CTL_SNR2, nextafterf(k.auto_snr_floor, 0.f)).f(CLK_CTL_RELAY_SHIFT_SQ, 1.f);
        r = clock_relay_look(k, noise.w, c);
        CHECK(r.verdict == CLK_RELAY_TAKE && !r.relay_auto);        // no signal: nothing is pursued, whatever the starts do
        // ... to closure, the look after: on to the limit of G + 1 passes
        ClockRelayLook cc = c; cc.first = false; cc.relay_auto = true; cc.relay_budget = 0;
        CHECK(clock_relay_look(k, low.w, cc).verdict == CLK_RELAY_CONTINUE);
        cc.relay_enq = 21;
        CHECK(clock_relay_look(k, low.w, cc).verdict == CLK_RELAY_TAKE);            // the limit
        cc.relay_enq = 20;
        CHECK(clock_relay_look(k, low.w, cc).verdict == CLK_RELAY_CONTINUE);
        Ctl low_closed = low; low_closed.i(CLK_CTL_RELAY_CLOSED, 1);
        CHECK(clock_relay_look(k, low_closed.w, cc).verdict == CLK_RELAY_TAKE);     // closed
        // ... a taken-over call whose signal is gone is not pursued, unless the closure was asked for
        CHECK(clock_relay_look(k, noise.w, cc).verdict == CLK_RELAY_NO_SIGNAL);
        ClockKnobs on = k; on.exact = 1;
        ClockRelayLook cx = cc; cx.relay_auto = false;
        CHECK(clock_relay_look(on, noise.w, cx).verdict == CLK_RELAY_CONTINUE);     // cfg.clock_exact = 1: to closure whatever the input
        cx.relay_auto = true;
        CHECK(clock_relay_look(on, noise.w, cx).verdict == CLK_RELAY_CONTINUE);
        ClockKnobs fast = k; fast.exact = -2;
        CHECK(clock_relay_look(fast, noise.w, cx).verdict == CLK_RELAY_NO_SIGNAL);
        // the starts still move: four more passes, once; then the result stands
        Ctl moving = clean; moving.f(CLK_CTL_RELAY_SHIFT_SQ, shift_hi);
        r = clock_relay_look(k, moving.w, c);
        CHECK(r.verdict == CLK_RELAY_FOUR_MORE && r.relay_auto && r.relay_budget == 7);
        ClockRelayLook c4 = c; c4.first = false; c4.relay_auto = true; c4.relay_budget = 7; c4.relay_enq = 7;
        CHECK(clock_relay_look(k, moving.w, c4).verdict == CLK_RELAY_TAKE);
        // ... not on a call that has used its G + 1 passes, nor on a two-pass plan, nor without hand-off passes
        ClockRelayLook cfull = c; cfull.G = 2;
        CHECK(clock_relay_look(k, moving.w, cfull).verdict == CLK_RELAY_TAKE);
        ClockRelayLook clong = c; clong.relay_long = true;
        CHECK(clock_relay_look(k, moving.w, clong).verdict == CLK_RELAY_TAKE);
        ClockRelayLook cguess = c; cguess.no_handoff = true;
        CHECK(clock_relay_look(k, moving.w, cguess).verdict == CLK_RELAY_TAKE);
        // a hand-off that never closed: to closure -- where there were hand-off passes
        ClockRelayLook cforce = c; cforce.relay_force = true;
        CHECK(clock_relay_look(k, clean.w, cforce).verdict == CLK_RELAY_TO_CLOSURE);
        cforce.no_handoff = true;
        CHECK(clock_relay_look(k, clean.w, cforce).verdict == CLK_RELAY_TAKE);
        CHECK(clock_relay_look(k, noise.w, cforce).verdict == CLK_RELAY_TAKE);
        // from the timing guess: a start that moved a quarter symbol -> to closure
        Ctl quarter = clean; quarter.f(CLK_CTL_RELAY_MOVE_MAX, 0.25f * k.sps);
        Ctl below = clean; below.f(CLK_CTL_RELAY_MOVE_MAX, nextafterf(0.25f * k.sps, 0.f));
        Ctl mark = clean; mark.i(CLK_CTL_RELAY_MOVE_MAX, 0x7f800000);        // (a watchdog's mark: infinity)
        CHECK(clock_relay_look(k, quarter.w, cguess).verdict == CLK_RELAY_TO_CLOSURE);
        CHECK(clock_relay_look(k, below.w, cguess).verdict == CLK_RELAY_TAKE);
        CHECK(clock_relay_look(k, mark.w, cguess).verdict == CLK_RELAY_TO_CLOSURE);
        CHECK(clock_relay_look(k, quarter.w, c).verdict == CLK_RELAY_TAKE);          // behind hand-off passes: not looked at
        Ctl quarter_noise = quarter; quarter_noise.f(CLK_CTL_SNR2, 1.75f);
        CHECK(clock_relay_look(k, quarter_noise.w, cguess).verdict == CLK_RELAY_TAKE);
        // the first look is the default's alone, and only while the relay is open and the host has not taken over
        Ctl closed = low; closed.i(CLK_CTL_RELAY_CLOSED, 1);
        r = clock_relay_look(k, closed.w, c);
        CHECK(r.verdict == CLK_RELAY_TAKE && !r.snr_seen);
        ClockRelayLook ctaken = c; ctaken.relay_auto = true; ctaken.relay_budget = 0;       // (the stall rule's relay)
        r = clock_relay_look(k, low.w, ctaken);
        CHECK(r.verdict == CLK_RELAY_CONTINUE && !r.snr_seen);
        ClockKnobs three = k; three.exact = 3;
        r = clock_relay_look(three, low.w, c);
        CHECK(r.verdict == CLK_RELAY_TAKE && !r.snr_seen);           // cfg.clock_exact = 3: three passes, nothing else
        ClockRelayLook c1 = c; c1.relay_enq = 1;
        CHECK(clock_relay_look(three, low.w, c1).verdict == CLK_RELAY_CONTINUE);
        // limits
        CHECK(clock_relay_limit(20, 0) == 21 && clock_relay_limit(20, 3) == 3 && clock_relay_limit(1, 3) == 2 && clock_relay_limit(20, 21) == 21);
    }
    // ---- the overlap job
    {
        Ctl good; good.f(CLK_CTL_SNR2, 32.f);
        CHECK(clock_overlap_look(k, good.w) == CLK_OV_TAKE);
        Ctl at; at.f(CLK_CTL_SNR2, k.auto_snr);
        CHECK(clock_overlap_look(k, at.w) == CLK_OV_TAKE);
        Ctl low; low.f(CLK_CTL_SNR2, nextafterf(k.auto_snr, 0.f));
        CHECK(clock_overlap_look(k, low.w) == CLK_OV_FALLBACK_TO_CLOSURE);
        Ctl at_floor; at_floor.f(CLK_CTL_SNR2, k.auto_snr_floor);
        CHECK(clock_overlap_look(k, at_floor.w) == CLK_OV_FALLBACK_TO_CLOSURE);
        Ctl noise; noise.f(CLK_CTL_SNR2, nextafterf(k.auto_snr_floor, 0.f));
        CHECK(clock_overlap_look(k, noise.w) == CLK_OV_TAKE);                   // no signal, the joints fit: taken
        Ctl noise_bad = noise; noise_bad.i(CLK_CTL_OV_BAD_JOINTS, 1);
        CHECK(clock_overlap_look(k, noise_bad.w) == CLK_OV_FALLBACK);          // ... they do not: the relay's default
        Ctl bad = good; bad.i(CLK_CTL_OV_BAD_JOINTS, 1);
        CHECK(clock_overlap_look(k, bad.w) == CLK_OV_FALLBACK_TO_CLOSURE);
        Ctl stuck = good; stuck.i(CLK_CTL_STUCK, 1).i(CLK_CTL_OV_BAD_JOINTS, 1);
        CHECK(clock_overlap_look(k, stuck.w) == CLK_OV_WATCHDOG);
    }
    // ---- the batches learnt for the next call
    CHECK(clock_next_relay_batch(0) == 32 && clock_next_relay_batch(3) == 32 && clock_next_relay_batch(19) == 32 && clock_next_relay_batch(20) == 33);
    CHECK(clock_next_relay_batch(3270) == 4095 && clock_next_relay_batch(3271) == 4096 && clock_next_relay_batch(100000) == 4096);
    CHECK(clock_next_batch(0, false) == 5 && clock_next_batch(4, false) == 5 && clock_next_batch(5, false) == 6 && clock_next_batch(31, false) == 32 &&
          clock_next_batch(32, false) == 32);
    CHECK(clock_next_batch(2, true) == 3 && clock_next_batch(0, true) == 3 && clock_next_batch(3, true) == 5 && clock_next_batch(6, true) == 7);
    // ---- the lattice (4 < sps < 8: omega steps by 2^-21, mu + omega likewise; 2 < sps < 4: 2^-22, and 3.2 + 0.5 < 4)
    {
        const ClockLattice l = clock_lattice(1.25e6f / 293883.0f), h = clock_lattice(2.5e6f / 927000.0f), u = clock_lattice(3.75f);
        CHECK(l.q_om == 8 && l.q_mu == 8 && h.q_om == 4 && h.q_mu == 4 && u.q_om == 4 && u.q_mu == 8);
        const ClockLattice tiny = clock_lattice(1e-3f);
        CHECK(tiny.q_om == 1 && tiny.q_mu >= 1);
    }
    return 0;
}

int main()
{
    // the control block: numbers are part of the device code's contract
    CHECK(CLK_CTL_DONE == 0 && CLK_CTL_PASSES == 1 && CLK_CTL_OPEN == 2 && CLK_CTL_MAX_RESIDUAL == 3 && CLK_CTL_TAKEOVER == 8 &&
          CLK_CTL_SYMBOLS == 13 && CLK_CTL_WALKERS == 19 && CLK_CTL_WALKERS < CLK_RES_WORD && CLK_RES_WORD + 8 == CLK_CTL_WORDS);
    if (check_design_numbers()) return 1;
    if (check_looks()) return 1;
    PlanModel m;
    CheckSink sink;
    run_grid(m, sink);
    if (sink.bad || !sink.complete()) {
        std::fprintf(stderr, "clock_host_check: %d cases differ from the record (%zu of %zu rows, %zu of %zu sums seen)\n", sink.bad, sink.ir,
                     sizeof EXPECT_ROWS / sizeof EXPECT_ROWS[0], sink.is, sizeof EXPECT_SUMS / sizeof EXPECT_SUMS[0]);
        return 1;
    }
    std::printf("clock_host_check: %zu cases spelled out, %zu configurations summed, the looks and the documented numbers: ok\n", sink.ir, sink.is);
    return 0;
}
