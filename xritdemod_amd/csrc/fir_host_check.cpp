// fir_host_check.cpp -- the FIR stage's launch plan (fir_plan.h) over a grid of tap counts, decimations and both summation
// orders: replayed against the table recorded from FirStage::init and FirStage::run as they stood before the plan was taken
// out of them (tests/golden/fir_plan_table.txt), with exact equality in every field, and every plan held to what a launch
// needs whatever the table says.  The rows the table cannot vouch for are the exact order at odd decimations from 17 up:
// there the recorded launch read past its tap rows and its tile; those rows must be the generic exact kernel, unskewed.
// A program of its own for the sanitizers: make fir-host-check.
// A row: T D exact no_static_dec no_static_mf, then "error" or
// form per-lane PAD TS DS MF | RC threads tile_len lds_bytes W Wpad | tap layout, floats.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "fir_plan.h"

using namespace xrit;

static std::string row_of(const FirPlan &p)
{
    if (!p.error.empty()) return "error";
    static const char *const forms[] = {"walk", "walkx", "exact", "poly"}, *const layouts[] = {"rows", "phases", "reversed"};
    char text[160];
    std::snprintf(text, sizeof text, "%s %d %d %d %d %d %d %d %d %zu %d %d %s %zu", forms[p.key.form], p.key.rc, (int)p.key.pad,
                  p.key.ts, p.key.ds, (int)p.key.mf, p.RC, p.threads, p.tile_len, p.lds_bytes, p.W, p.Wpad, layouts[p.taps],
                  p.tap_floats);
    return text;
}

#define NEED(cond)                                                                           \
    do {                                                                                     \
        if (!(cond)) { std::fprintf(stderr, "fir_host_check: %s: not %s\n", what, #cond); return false; } \
    } while (0)

// what a launch from this plan needs, from first principles
static bool sound(const FirPlan &p, const char *what)
{
    const int form = p.key.form;
    const bool walk = form == FIR_WALK || form == FIR_WALK_EXACT;
    const long long outputs = (long long)fir_block_outputs(p);
    for (int cf32 = 0; cf32 < 2; ++cf32) NEED(fir_instance_exists(fir_key(p, cf32 != 0, false), cf32 != 0));
    if (fir_agc_fill_supported(p, 3)) NEED(fir_instance_exists(fir_key(p, true, true), true));
    NEED(p.key.rc == (form == FIR_EXACT ? 0 : p.RC) && p.key.pad == p.pad);
    NEED(p.RC >= 1 && p.threads % 64 == 0 && p.threads >= 64 && p.threads <= 256);
    NEED(p.tile_len >= (outputs - 1) * p.D + p.T);
    if (walk && !p.pad) NEED((long long)(p.threads - 1) * p.RC * p.D + p.Wpad - 1 < p.tile_len);
    NEED(p.Wpad % 4 == 0 && p.Wpad >= p.W);
    NEED(p.lds_bytes >= (size_t)p.tile_len * 8 && p.lds_bytes >= (size_t)p.threads * p.RC * 8);
    NEED((p.lds_bytes <= 64 * 1024 || p.threads == 64) && p.lds_bytes <= 160 * 1024);
    if (form == FIR_WALK_EXACT && p.pad) NEED(p.D % 4 == 0 && !fir_stat_supported(p, 8));
    if (form == FIR_POLY) NEED((p.D == 16 || p.D == 32 || p.D == 64) && (p.T + p.D - 1) / p.D <= 32 && !p.exact);
    NEED(p.exact == (form == FIR_WALK_EXACT || form == FIR_EXACT));
    // the tap image: its size, and every tap once in every row (phase table, reversal)
    std::vector<float> taps((size_t)p.T);
    double sum = 0;
    for (int i = 0; i < p.T; ++i) sum += taps[(size_t)i] = (float)(i % 251 + 1);
    const std::vector<float> image = fir_tap_image(p, taps.data(), p.taps);
    const size_t rows = walk ? (size_t)p.RC : 1;
    NEED(image.size() == p.tap_floats && image.size() == (walk ? (size_t)p.RC * p.Wpad : form == FIR_POLY ? (size_t)p.D * 32 : (size_t)p.T));
    for (size_t c = 0; c < rows; ++c) {
        double s = 0;
        for (size_t i = 0; i < image.size() / rows; ++i) s += image[c * (image.size() / rows) + i];
        NEED(s == sum);
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: fir_host_check TABLE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "fir_host_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string text;
    size_t rows = 0, bad = 0, errors = 0, mended = 0, count[4] = {0, 0, 0, 0};
    while (std::getline(in, text)) {
        int T, D, exact, nsd, nsm, used = 0;
        if (std::sscanf(text.c_str(), "%d %d %d %d %d %n", &T, &D, &exact, &nsd, &nsm, &used) != 5 || T < 1 || T > 8191 || D < 1 || D > 128) {
            std::fprintf(stderr, "fir_host_check: row %zu is no configuration: %s\n", rows, text.c_str());
            return 1;
        }
        ++rows;
        FirKnobs knobs;
        knobs.no_static_dec = nsd != 0;
        knobs.no_static_mf = nsm != 0;
        const FirPlan p = fir_plan(T, D, exact != 0, knobs);
        const std::string what = text.substr(0, (size_t)used), got = row_of(p);
        bool ok;
        if (exact && D >= 17 && D % 2 == 1) {
            ok = p.error.empty() && p.key.form == FIR_EXACT && !p.pad;
            ++mended;
        } else {
            ok = got == text.substr((size_t)used);
        }
        if (ok && p.error.empty()) ok = sound(p, what.c_str());
        if (p.error.empty()) ++count[p.key.form];
        else ++errors;
        if (!ok) {
            std::fprintf(stderr, "fir_host_check: row %zu differs: %s | now %s\n", rows - 1, text.c_str(), got.c_str());
            ++bad;
        }
    }
    if (bad || rows < 2070 || mended != 390) {
        std::fprintf(stderr, "fir_host_check: %zu of %zu rows differ (%zu exact rows at odd decimations from 17 up)\n", bad, rows, mended);
        return 1;
    }
    std::printf("fir_host_check: %zu rows (window walk %zu, exact walk %zu, generic exact %zu of which %zu at odd decimations from 17 "
                "up, polyphase %zu, %zu do not fit LDS), every plan's key an instance sized like its tile and taps: ok\n",
                rows, count[FIR_WALK], count[FIR_WALK_EXACT], count[FIR_EXACT], mended, count[FIR_POLY], errors);
    return 0;
}
