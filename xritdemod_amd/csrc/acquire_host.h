// acquire_host.h -- the plain C++ of the carrier acquisition stage (include/xritdemod_amd.h, "Carrier acquisition"; DESIGN.md
// section 21), shared by the C ABI (acquire.cpp), the kernels' launch code (acquire.hip) and a stand-alone program under
// the sanitizers (acquire_host_check.cpp, make acquire-host-check): the parameter checks, the phase step from hertz, the
// number of segments of a call and the scratch sizes.  No HIP here.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/xritdemod_amd.h"

namespace xrit {

constexpr unsigned ACQ_N = 4096;                    // points of a segment's FFT
constexpr unsigned ACQ_HOP = ACQ_N / 2;             // the segments overlap by half
constexpr unsigned ACQ_MIN_SEGMENTS = 31, ACQ_MAX_SEGMENTS = 4095, ACQ_DEFAULT_SEGMENTS = 511;
constexpr unsigned ACQ_MAX_PRE_SUM = 64;
// the geometric mean of the largest ratio of noise alone at 31 segments and the smallest of the
// signal cases at Es/N0 = 2 dB, both from tests/acquire_spec.py on the CPU
constexpr double ACQ_DEFAULT_MIN_RATIO = 8.9;
constexpr size_t ACQ_MAX_SAMPLES = (size_t)1 << 40; // per call (the segment index times the hop stays far inside 64 bits)

// 0 selects a default; false: a value out of range
inline bool acquire_params_resolve(const xrit_acquire_params &in, xrit_acquire_params &out)
{
    out = in;
    if (out.pre_sum == 0) out.pre_sum = 1;
    if (out.segments == 0) out.segments = ACQ_DEFAULT_SEGMENTS;
    if (out.min_ratio == 0.0) out.min_ratio = ACQ_DEFAULT_MIN_RATIO;
    return std::isfinite(out.sample_rate) && out.sample_rate > 0.0 && out.pre_sum <= ACQ_MAX_PRE_SUM &&
           out.segments >= ACQ_MIN_SEGMENTS && out.segments <= ACQ_MAX_SEGMENTS && std::isfinite(out.min_ratio) && out.min_ratio > 0.0;
}

// the sample types the stage takes, and the bytes of one complex sample (0: refused)
inline size_t acquire_sample_bytes(int type)
{
    return type == XRIT_SAMPLE_FLOATIQ ? 8 : type == XRIT_SAMPLE_S16IQ ? 4 : type == XRIT_SAMPLE_S8IQ ? 2 : 0;
}

// inc = llrint(ldexp(hz / sample_rate, 64)); false unless |hz| < sample_rate / 2 (|inc| <= 2^63 - 2^10 then: a double
// below 2^63 is a multiple of 2^10 at least)
inline bool acquire_inc_from_hz(double hz, double sample_rate, int64_t &inc)
{
    if (!std::isfinite(hz) || !(std::fabs(hz) < sample_rate * 0.5)) return false;
    inc = (int64_t)std::llrint(std::ldexp(hz / sample_rate, 64));
    return true;
}

// M = min(M_max, floor(floor(n / R) / 2048) - 1), not below 0: the last segment ends at (M + 1) * 2048 * R <= n
inline unsigned acquire_segments(size_t n, unsigned pre_sum, unsigned max_segments)
{
    const size_t hops = n / pre_sum / ACQ_HOP;
    if (hops < 2) return 0;
    return hops - 1 < max_segments ? (unsigned)(hops - 1) : max_segments;
}

// the tables (uploaded once): the twiddles exp(-2 pi i k / N) as float pairs, then the Hann window
constexpr size_t ACQ_TABLE_BYTES = (size_t)ACQ_N * 8 + (size_t)ACQ_N * 4;
// the scratch of an estimate of M segments: every segment's spectrum (float pairs; room for one at least), then the
// summed power row (double)
inline size_t acquire_spectra_bytes(unsigned segments) { return (size_t)(segments ? segments : 1) * ACQ_N * 8; }
constexpr size_t ACQ_POWER_BYTES = (size_t)ACQ_N * 8;

}  // namespace xrit
