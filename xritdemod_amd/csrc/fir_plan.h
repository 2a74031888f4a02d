// fir_plan.h -- the FIR stage's launch plan: which kernel form a stage of T taps and decimation D takes, the template key
// the launch uses, the one geometry that key, the tile, the tap image and the grid are all sized from, and the list of keys
// a kernel instance exists for.  Plain C++, no HIP headers: FirStage (fir.hip) makes the plan once in init and launches
// from it; fir_host_check.cpp walks a grid of configurations through it on the CPU (make fir-host-check).
#pragma once

#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#ifndef XRIT_POLY_PR
#define XRIT_POLY_PR 16
#endif
#ifndef XRIT_POLY_THREADS
#define XRIT_POLY_THREADS 256
#endif

namespace xrit {

enum FirForm {
    FIR_WALK,         // fir_decim_kernel: a lane walks its window once for RC outputs
    FIR_WALK_EXACT,   // fir_decim_kernel<..., EX>: the same walk summed in the CPU chain's order
    FIR_EXACT,        // fir_exact_kernel: one output at a time, any decimation (per-lane count is a launch argument)
    FIR_POLY,         // fir_poly_kernel: lanes = phases, decimation 16 / 32 / 64
};
enum FirTaps {
    FIR_TAPS_ROWS,      // RC x Wpad: g[c][i] = h[T-1 + c D - i]
    FIR_TAPS_PHASES,    // D x POLY_NQ: hq[ph][q] = h[q D + ph]
    FIR_TAPS_REVERSED,  // T: rt[t] = h[T-1 - t]
    FIR_TAPS_TOEPLITZ,  // the matrix-pipe experiment's second operand, beside the rows
};
enum FirTypes { FIR_ANY_TYPE, FIR_CF32_ONLY };

// The template arguments of a launch, the sample type aside.  rc = 0: the form takes the per-lane count at run time.
struct FirKey {
    int form = FIR_WALK, rc = 3;
    bool pad = false;
    int apl = 0, ts = 0, ds = 1;
    bool mf = false;
    constexpr bool operator==(const FirKey &o) const
    {
        return form == o.form && rc == o.rc && pad == o.pad && apl == o.apl && ts == o.ts && ds == o.ds && mf == o.mf;
    }
};

// Every key a kernel instance exists for, written once: X(form, per-lane, PAD, APL, TS, DS, MF, sample types).  The
// dispatch in fir.hip expands it into the launches, fir_instances below into the keys the host check looks plans up in.
// A new kernel variant is a row here and a branch in fir_plan().
#define XR_FIR_INSTANCES(X)                                     \
    X(FIR_WALK, 5, false, 0, 0, 1, false, FIR_ANY_TYPE)         \
    X(FIR_WALK, 3, false, 0, 0, 1, false, FIR_ANY_TYPE)         \
    X(FIR_WALK, 3, true, 0, 0, 1, false, FIR_ANY_TYPE)          \
    X(FIR_WALK, 3, false, 0, 151, 5, false, FIR_CF32_ONLY)      \
    X(FIR_WALK, 5, false, 0, 63, 1, false, FIR_CF32_ONLY)       \
    X(FIR_WALK, 5, false, 3, 0, 1, false, FIR_CF32_ONLY)        \
    X(FIR_WALK, 5, false, 3, 63, 1, false, FIR_CF32_ONLY)       \
    X(FIR_WALK_EXACT, 5, false, 0, 0, 1, false, FIR_ANY_TYPE)   \
    X(FIR_WALK_EXACT, 3, false, 0, 0, 1, false, FIR_ANY_TYPE)   \
    X(FIR_WALK_EXACT, 3, true, 0, 0, 1, false, FIR_ANY_TYPE)    \
    X(FIR_WALK_EXACT, 1, true, 0, 0, 1, false, FIR_ANY_TYPE)    \
    X(FIR_EXACT, 0, true, 0, 0, 1, false, FIR_ANY_TYPE)         \
    X(FIR_EXACT, 0, false, 0, 0, 1, false, FIR_ANY_TYPE)        \
    X(FIR_POLY, 1, false, 0, 0, 16, false, FIR_ANY_TYPE)        \
    X(FIR_POLY, 1, false, 0, 0, 32, false, FIR_ANY_TYPE)        \
    X(FIR_POLY, 1, false, 0, 0, 64, false, FIR_ANY_TYPE)        \
    XR_FIR_EXPERIMENT_INSTANCES(X)
#ifdef XRIT_EXPERIMENTS
#define XR_FIR_EXPERIMENT_INSTANCES(X) X(FIR_WALK, 3, false, 0, 151, 5, true, FIR_CF32_ONLY)
#else
#define XR_FIR_EXPERIMENT_INSTANCES(X)
#endif

struct FirInstance { FirKey key; int types; };
#define XR_FIR_ROW(FORM, RC, PAD, APL, TS, DS, MF, TYPES) {{FORM, RC, PAD, APL, TS, DS, MF}, TYPES},
constexpr FirInstance fir_instances[] = {XR_FIR_INSTANCES(XR_FIR_ROW)};
#undef XR_FIR_ROW

constexpr bool fir_instance_exists(const FirKey &k, bool cf32)
{
    for (const FirInstance &i : fir_instances)
        if (i.key == k && (cf32 || i.types == FIR_ANY_TYPE)) return true;
    return false;
}

// What init reads from the environment once (XRIT_NO_STATIC_DEC, XRIT_NO_STATIC_MF; under XRIT_EXPERIMENTS XRIT_MFMA_DEC
// and the XRIT_DEC_THREADS value, 0 = unset): diagnostic switches for A/B runs.
struct FirKnobs {
    bool no_static_dec = false, no_static_mf = false, mfma_dec = false;
    int dec_threads = 0;
};

struct FirPlan {
    static constexpr int POLY_PR = XRIT_POLY_PR, POLY_NQ = 32;     // outputs per lane group, taps per phase (T <= 32 * D)
    int T = 0, D = 1;
    bool exact = false;
    FirKey key;            // for cf32 input without the AGC in the window fill; fir_key() for the other launches
    // the one geometry: RC outputs per lane (the key's, where the key has one), W window samples per lane in rows of Wpad
    int RC = 3, W = 0, Wpad = 0, threads = 256, tile_len = 0;
    bool pad = false;      // the LDS tile is skewed by one sample per D
    size_t lds_bytes = 0;
    int taps = FIR_TAPS_ROWS;    // the tap layout the form reads
    size_t tap_floats = 0;
    std::string error;     // not empty: no plan
};

inline FirPlan fir_plan(int ntaps, int decim, bool exact, const FirKnobs &knobs)
{
    FirPlan p;
    int &T = p.T, &D = p.D, &RC = p.RC, &W = p.W, &Wpad = p.Wpad, &threads = p.threads, &tile_len = p.tile_len;
    bool &pad = p.pad;
    size_t &lds_bytes = p.lds_bytes;
    constexpr int POLY_PR = FirPlan::POLY_PR, POLY_NQ = FirPlan::POLY_NQ;
    const auto does_not_fit = [&p, &T, &D] {
        char text[96];
        std::snprintf(text, sizeof text, "FIR window of %d taps x decimation %d does not fit LDS", T, D);
        p.error = text;
        return p;
    };
    p.exact = exact;
    T = ntaps;
    D = decim < 1 ? 1 : decim;
    // measured at C2: five outputs per lane halve the decimator's occupancy (52 KiB window) and lose 45 %
    if (D == 1) RC = 5;
    else RC = 3;
    // (cfg.front_exact = 2 at large decimations: one output per lane -- a window of 64 KiB then holds 128 outputs, four workgroups
    // per CU; with three per lane it held 192 on ONE wave per workgroup and two waves per CU: 4.0 ms per C5 burst)
    if (exact && D >= 16) RC = 1;
    // large decimations whose phases map onto lanes take the polyphase kernel
    if (!exact && (D == 16 || D == 32 || D == 64) && (T + D - 1) / D <= POLY_NQ) {
        threads = XRIT_POLY_THREADS;
        RC = 1;
        pad = false;
        const int OB = (threads / D) * POLY_PR;
        tile_len = (POLY_NQ + OB - 1) * D + 2;
        lds_bytes = (size_t)tile_len * 8;
        p.key = FirKey{FIR_POLY, 1, false, 0, 0, D, false};
        p.taps = FIR_TAPS_PHASES;
        p.tap_floats = (size_t)D * POLY_NQ;
        return p;
    }
    pad = ((RC * D) % 2) == 0;
    // the exact order has a shared window walk for unskewed tiles of three and five outputs per lane and for skewed ones
    // at decimations that are a multiple of 4; the rest -- odd decimations from 16 up among them, where one output per
    // lane leaves a walk nothing to share -- is summed one output at a time (fir_exact_kernel; the reversed taps, a tile
    // of at most 64 KiB)
    const bool shared_walk = pad ? D % 4 == 0 : RC != 1;
    if (exact && !shared_walk) {
        pad = (D % 2) == 0;
        threads = 256;
        RC = D == 1 ? 4 : 2;
        for (;;) {
            const long long ob = (long long)threads * RC;
            const long long tl = (ob - 1) * D + T;
            const long long padded = pad ? tl + tl / D + 2 : tl;
            if (padded * 8 <= 64 * 1024 || (threads == 64 && RC == 1)) {
                tile_len = (int)tl;
                lds_bytes = (size_t)padded * 8;
                break;
            }
            if (RC > 1) --RC; else threads /= 2;
        }
        if (lds_bytes > 160 * 1024) return does_not_fit();
        W = T;
        Wpad = (W + 3) & ~3;
        p.key = FirKey{FIR_EXACT, 0, pad, 0, 0, 1, false};
        p.taps = FIR_TAPS_REVERSED;
        p.tap_floats = (size_t)T;
        return p;
    }
    W = T + (RC - 1) * D;
    Wpad = (W + 3) & ~3;
    // block size: keep the LDS window under 64 KiB
    threads = 256;
    // (XRIT_DEC_THREADS: the decimator's workgroup size for A/B runs -- smaller workgroups hold smaller windows, and more of
    // them fit next to the relay's walkers)
    if (D > 1 && (knobs.dec_threads == 64 || knobs.dec_threads == 128 || knobs.dec_threads == 192 || knobs.dec_threads == 256))
        threads = knobs.dec_threads;
    for (;;) {
        long long ob = (long long)threads * RC;
        long long tl = (ob - 1) * D + T + (Wpad - W) + 8;
        long long padded = pad ? tl + tl / D + 8 : tl;
        if (padded * 8 <= 64 * 1024 || threads == 64) {
            tile_len = (int)tl;
            lds_bytes = (size_t)padded * 8;
            break;
        }
        threads = threads == 192 ? 128 : threads / 2;
    }
    if (lds_bytes > 160 * 1024) return does_not_fit();
    p.key = FirKey{exact ? FIR_WALK_EXACT : FIR_WALK, RC, pad, 0, 0, 1, false};
    p.taps = FIR_TAPS_ROWS;
    p.tap_floats = (size_t)RC * Wpad;
    // straight-line walks with the taps in scalar registers: the chain's 151-tap decimator by 5 and its 63-tap matched filter
    if (!exact && RC == 3 && !pad && T == 151 && D == 5) {
        if (knobs.mfma_dec && threads == 256) p.key.ts = 151, p.key.ds = 5, p.key.mf = true;
        else if (!knobs.no_static_dec) p.key.ts = 151, p.key.ds = 5;
    }
    if (!exact && RC == 5 && !pad && T == 63 && D == 1 && !knobs.no_static_mf) p.key.ts = 63;
    return p;
}

// The key of one launch: the static and matrix-pipe forms exist for cf32 input only, the AGC in the window fill (three
// samples per lane of the AGC's runs) is a form of its own.
inline FirKey fir_key(const FirPlan &p, bool cf32, bool agc_fill)
{
    FirKey k = p.key;
    if (!cf32 && k.form != FIR_POLY) k.ts = 0, k.ds = 1, k.mf = false;
    if (agc_fill) k.apl = 3;
    return k;
}

// the matrix-pipe form keeps its tile skewed by 20 samples per 80
inline size_t fir_lds_bytes(const FirPlan &p, const FirKey &k)
{
    return p.lds_bytes + (k.mf ? (size_t)(p.tile_len / 80 + 1) * 20 * 8 : 0);
}

// outputs of one workgroup
inline size_t fir_block_outputs(const FirPlan &p)
{
    return p.key.form == FIR_POLY ? (size_t)(p.threads / p.D) * FirPlan::POLY_PR : (size_t)p.threads * p.RC;
}

// one run per wave: 64 * RC outputs
inline bool fir_agc_supported(const FirPlan &p) { return p.key.form == FIR_WALK && !p.pad; }

// runs must not straddle blocks (the sums are taken from the block's outputs staged in LDS); the skewed exact walk is
// launched without the sums
inline bool fir_stat_supported(const FirPlan &p, int statL)
{
    switch (p.key.form) {
    case FIR_WALK: return statL > 0 && !p.pad && (p.threads * p.RC) % statL == 0;
    case FIR_WALK_EXACT: return statL == 8 && !p.pad;
    case FIR_EXACT: return statL == 8;
    default: return false;
    }
}

inline bool fir_agc_fill_supported(const FirPlan &p, int per_lane)
{
    // the window must be covered by three rounds of the block's waves, one run each
    const long long runs = (p.tile_len + (long long)64 * per_lane - 1) / (64 * per_lane) + 1;
    return p.key.form == FIR_WALK && p.D == 1 && !p.pad && per_lane == 3 && p.RC == 5 && runs <= 3 * (p.threads / 64);
}

// The host image of a tap layout (plan.taps; FIR_TAPS_TOEPLITZ beside the rows where the key says MF).
inline std::vector<float> fir_tap_image(const FirPlan &p, const float *taps, int layout)
{
    const int T = p.T, D = p.D, RC = p.RC, W = p.W, Wpad = p.Wpad;
    constexpr int POLY_NQ = FirPlan::POLY_NQ;
    if (layout == FIR_TAPS_REVERSED) {
        std::vector<float> r((size_t)T);
        for (int i = 0; i < T; ++i) r[(size_t)i] = taps[T - 1 - i];
        return r;
    }
    if (layout == FIR_TAPS_PHASES) {
        std::vector<float> hq((size_t)D * POLY_NQ, 0.0f);
        for (int ph = 0; ph < D; ++ph)
            for (int q = 0; q < POLY_NQ; ++q)
                if (q * D + ph < T) hq[(size_t)ph * POLY_NQ + q] = taps[q * D + ph];
        return hq;
    }
    std::vector<float> rows((size_t)RC * Wpad, 0.0f);
    for (int c = 0; c < RC; ++c)
        for (int i = 0; i < W; ++i) {
            int k = T - 1 + c * D - i;
            if (k >= 0 && k < T) rows[(size_t)c * Wpad + i] = taps[k];
        }
    if (layout == FIR_TAPS_ROWS) return rows;
    // the Toeplitz operand of the matrix-pipe experiment: step q, lane l -> H[4 q + (l >> 4)][l & 15] = g[s - 5 j]
    const int KS = (15 * 5 + 151 + 3) / 4;
    std::vector<float> hb((size_t)KS * 64, 0.0f);
    for (int q = 0; q < KS; ++q)
        for (int l = 0; l < 64; ++l) {
            const int sp = 4 * q + (l >> 4) - 5 * (l & 15);
            if (sp >= 0 && sp < T) hb[(size_t)q * 64 + l] = rows[(size_t)sp];
        }
    return hb;
}

}  // namespace xrit
