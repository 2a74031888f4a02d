// monitor_host.h -- the plain C++ of the link monitor (include/xritdemod_amd.h, "Link monitor"), shared
// by the C ABI (monitor.cpp), the kernels' launch code (monitor.hip) and a stand-alone program under the sanitizers
// (monitor_host_check.cpp, make monitor-host-check): the argument checks, the geometry of a push (which pieces of a call
// complete which blocks, known on the host without a read-back) and xrit_monitor_derive.  No HIP calls here.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/xritdemod_amd.h"

#if defined(__HIPCC__)
#define XRIT_HD __host__ __device__
#else
#define XRIT_HD
#endif

namespace xrit {

constexpr uint32_t MON_MIN_BLOCK = 64, MON_MAX_BLOCK = 32768, MON_DEFAULT_BLOCK = 16384;
constexpr size_t MON_MAX_SYMBOLS = (size_t)1 << 30;        // per push
constexpr uint64_t MON_Q_MAX = 4095;
// 4095^4 * 32768 < 2^63: s4 of a full block fits with a bit to spare
static_assert(MON_Q_MAX * MON_Q_MAX * MON_Q_MAX * MON_Q_MAX < ((uint64_t)1 << 63) / MON_MAX_BLOCK, "s4 of a block fits 63 bits");

inline bool monitor_block_ok(uint32_t block) { return block >= MON_MIN_BLOCK && block <= MON_MAX_BLOCK && block % 64 == 0; }
// bytes of one symbol (0: refused)
inline size_t monitor_symbol_bytes(int type) { return type == XRIT_SYMBOL_F32 ? 4 : type == XRIT_SYMBOL_I8 ? 1 : 0; }

// A push of n symbols behind an open block of `open` symbols (open < block): piece k covers the stream's symbols
// open + [k * block - open, (k + 1) * block - open) cut to the call, so piece 0 completes the open block (or is a whole
// block when nothing is open), the pieces behind it are whole blocks and the last may be a tail that stays open.
struct MonitorPlan {
    uint32_t block, open;
    size_t n;
    size_t pieces;              // ceil((open + n) / block); 0 when n = 0
    size_t rows;                // floor((open + n) / block): the pieces that complete a block
    uint32_t open_after;        // (open + n) mod block
    // call indices of piece k
    XRIT_HD size_t begin(size_t k) const { return k ? k * (size_t)block - open : 0; }
    XRIT_HD size_t end(size_t k) const { const size_t e = (k + 1) * (size_t)block - open; return e < n ? e : n; }
};

inline MonitorPlan monitor_plan(uint32_t block, uint32_t open, size_t n)
{
    MonitorPlan p{};
    p.block = block;
    p.open = open;
    p.n = n;
    const size_t t = (size_t)open + n;
    p.rows = t / block;
    p.pieces = n ? (t + block - 1) / block : 0;
    p.open_after = (uint32_t)(t % block);
    return p;
}

// One block record in float64.  The difference that cancels, 3 s2^2 - n s4, and the two sign tests are integers.
inline int monitor_derive(const xrit_monitor_block &b, int type, xrit_monitor_quality &out)
{
    typedef unsigned __int128 u128;
    typedef __int128 i128;
    const uint64_t n = b.n, s1 = b.s1, s2 = b.s2, s4 = b.s4;
    const uint64_t mag = b.sum < 0 ? 0 - (uint64_t)b.sum : (uint64_t)b.sum;
    if (!monitor_symbol_bytes(type) || n == 0 || n > MON_MAX_BLOCK || s1 > MON_Q_MAX * n || s2 > MON_Q_MAX * MON_Q_MAX * n ||
        s4 > MON_Q_MAX * MON_Q_MAX * MON_Q_MAX * MON_Q_MAX * n || mag > s1)
        return XRIT_E_INVALID;
    const double scale = type == XRIT_SYMBOL_F32 ? 512.0 : 508.0, dn = (double)n;
    out = xrit_monitor_quality{};
    const double m2 = (double)s2 / dn;
    out.level = std::sqrt(m2) / scale;
    out.dc = (double)b.sum / (scale * dn);
    out.flip_rate = (double)b.flips / dn;
    out.sat_rate = (double)b.sat / dn;
    out.neg_rate = (double)b.neg / dn;
    // s1 <= 2^27 and n s2 <= 2^54: the variance's numerator fits 64 bits
    const int64_t var = (int64_t)(n * s2) - (int64_t)(s1 * s1);
    if (s1 == 0) {
        out.flags |= XRIT_MONITOR_NO_SIGNAL;
        out.esn0_snv_db = -99.0;
    } else if (var <= 0) {
        out.flags |= XRIT_MONITOR_NO_NOISE;
        out.esn0_snv_db = 99.0;
    } else {
        out.esn0_snv_db = 10.0 * std::log10((double)(s1 * s1) / (2.0 * (double)var));
    }
    const u128 sq = (u128)s2 * s2, ns4 = (u128)n * s4;
    const i128 d = (i128)(3 * sq) - (i128)ns4;
    if (d <= 0) {
        out.flags |= XRIT_MONITOR_NO_SIGNAL;
        out.esn0_m2m4_db = -99.0;
    } else if (ns4 <= sq) {
        out.flags |= XRIT_MONITOR_NO_NOISE;
        out.esn0_m2m4_db = 99.0;
    } else {
        const double S = std::sqrt((double)d / 2.0) / dn, N = m2 - S;
        if (N <= 0.0) {                             // float64 rounding at the edge of the integer test
            out.flags |= XRIT_MONITOR_NO_NOISE;
            out.esn0_m2m4_db = 99.0;
        } else {
            out.esn0_m2m4_db = 10.0 * std::log10(S / (2.0 * N));
        }
    }
    return XRIT_OK;
}

}  // namespace xrit
