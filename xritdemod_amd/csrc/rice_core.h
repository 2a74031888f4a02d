// rice_core.h -- the wave form of the Rice decoder (CCSDS 121.0-B adaptive entropy coder, unit-delay predictor; DESIGN.md
// section 16, tests/rice_spec.py is the serial statement) as device functions, shared by the batch decoder (rice.hip:
// one (n, J, S) per launch) and the image stage (images.hip: (n, J, S) per line, from its file's record).
// One WAVE per line: the blocks one after the other (where a block begins depends on the one before); inside a block
// lane q has the block's q-th sample: the codes' ends found by popcounts over 64 windows of 64 bits, their prefix and a
// binary select; the predictor as an assume-unclipped prefix sum that every lane certifies against the literal step,
// repaired from the first lane that fails.  Fixed fields are read by every lane from the same place.  Stores are
// coalesced.  No LDS, no scratch; everything is integer (one float square root as a starting guess, fixed up exactly).
#pragma once

#include <hip/hip_runtime.h>

#include "wave_ops.h"

namespace xrit {

constexpr unsigned RICE_MAX_LINE = 1u << 20;        // bytes; longer lines are refused (status 2)

template <typename T>
__device__ __forceinline__ void put(T *out, unsigned i, unsigned S, unsigned x)
{
    if (i < S) out[i] = (T)x;
}

// the inverse of the mapper: with delta <= xmax the new sample is inside [0, xmax] (delta or xmax - delta when the
// step is the clipped one), so the specification's last fault cannot occur behind the delta <= xmax test
__device__ __forceinline__ unsigned unmap(unsigned prev, unsigned delta, unsigned xmax)
{
    const unsigned room = xmax - prev, th = prev < room ? prev : room;
    if (delta <= 2 * th) return (delta & 1u) ? prev - ((delta + 1) >> 1) : prev + (delta >> 1);
    return prev <= room ? delta : xmax - delta;
}

// m <= 17 bits at bit position pos; bytes beyond the line are zero
__device__ __forceinline__ unsigned bits_at(const unsigned char *p, unsigned len, unsigned pos, unsigned m)
{
    if (m == 0) return 0;
    const unsigned b = pos >> 3;
    unsigned long long w = 0;
#pragma unroll
    for (unsigned u = 0; u < 4; ++u) w = w << 8 | (b + u < len ? p[b + u] : 0u);
    return (unsigned)(w >> (32 - (pos & 7u) - m)) & ((1u << m) - 1u);
}

// the 64 bits at bit position pos (bytes beyond the line are zero)
__device__ __forceinline__ unsigned long long window_at(const unsigned char *p, unsigned len, unsigned pos)
{
    const unsigned b = pos >> 3, sub = pos & 7u;
    unsigned long long w = 0;
#pragma unroll
    for (unsigned u = 0; u < 8; ++u) w = w << 8 | (b + u < len ? p[b + u] : 0u);
    if (sub) w = w << sub | (unsigned long long)((b + 8 < len ? p[b + 8] : 0u) >> (8 - sub));
    return w;
}

// index from the top of the t-th (0-based) set bit of w (t < popcount(w))
__device__ __forceinline__ unsigned select_bit(unsigned long long w, unsigned t)
{
    unsigned at = 0;
#pragma unroll
    for (unsigned s = 32; s >= 1; s >>= 1) {        // w is 2 s bits wide
        const unsigned long long hi = w >> s;
        const unsigned c = __popcll(hi);
        if (t < c) w = hi;
        else {
            t -= c;
            w &= (1ull << s) - 1ull;
            at += s;
        }
    }
    return at;
}

// `cnt` fundamental-sequence codes from bit position pos, code i for lane first + i: 64 windows of 64 bits at a time, a
// popcount per lane and its prefix over the wave say which window holds the lane's terminating one (a binary search
// through shuffles), a binary select finds it inside the window; the code's value is the distance to the one in front.
// Returns false when the line ends before the last code does; pos moves behind the last code.  No lane diverges.
__device__ __forceinline__ bool fs_section(const unsigned char *p, unsigned len, unsigned &pos, unsigned cnt, unsigned first,
                                           unsigned lane, unsigned &value)
{
    const unsigned N = 8u * len;
    unsigned found = 0, last = pos - 1u, cs = pos;      // ones seen, where the last of them lies, the chunk's start
    value = 0;
    for (;;) {
        if (cs >= N) return false;
        const unsigned long long W = window_at(p, len, cs + 64u * lane);
        const unsigned c = __popcll(W);
        const unsigned P = wave_incl_scan(c, (int)lane), T = wave_total(P);
        // this lane's code ends at the chunk's one of rank t (if 0 <= t < T)
        const int ts = (int)lane - (int)first - (int)found;
        const bool mine = lane >= first && lane < first + cnt && ts >= 0 && (unsigned)ts < T;
        const unsigned t = mine ? (unsigned)ts : 0u;
        unsigned l = 0;
#pragma unroll
        for (unsigned s = 32; s >= 1; s >>= 1) {
            const unsigned Pc = __shfl(P, (int)(l + s - 1u), 64);
            if (Pc <= t) l += s;
        }
        l &= 63u;                                        // (only where T == 0 and the lane is not `mine`)
        const unsigned before = __shfl(P - c, (int)l, 64);
        const unsigned long long Wl = __shfl(W, (int)l, 64);
        const unsigned at = cs + 64u * l + select_bit(Wl, mine ? t - before : 0u);
        const unsigned up = __shfl_up(at, 1, 64);
        if (mine) value = at - (ts == 0 ? last : up) - 1u;
        const unsigned now = found + T < cnt ? found + T : cnt;         // codes resolved so far
        if (T) last = __shfl(at, (int)(first + now - 1u), 64);
        found += T;
        if (found >= cnt) {
            pos = last + 1u;
            return true;
        }
        cs += 4096u;
    }
}

// One line of `len` bytes at p: S samples to out and the status (0, or 1 on a fault: the blocks decoded in front of it
// kept, the rest 0) by lane 0.  STORE = false decodes for the status alone: out is not touched.
template <typename T, bool STORE = true>
__device__ void decode_line_wave(const unsigned char *p, unsigned len, unsigned n, unsigned J, unsigned S, T *out, unsigned char *status,
                                 unsigned lane)
{
    const unsigned B = (S + J - 1) / J, L = n <= 8 ? 3u : 4u, xmax = (1u << n) - 1u, raw_id = (1u << L) - 1u, N = 8u * len;
    unsigned b = 0, pos = 0, prev = 0;
    bool ok = true;
    while (b < B) {
        const bool ref = b == 0;
        const unsigned first = ref ? 1u : 0u, cnt = J - first, base = b * J;
        const bool body = lane >= first && lane < J;        // this lane has a mapped value
        if (pos + L > N) { ok = false; break; }
        const unsigned id = bits_at(p, len, pos, L);
        pos += L;
        unsigned second = 0;
        if (id == 0) {
            if (pos + 1 > N) { ok = false; break; }
            second = bits_at(p, len, pos, 1);
            pos += 1;
        }
        if (ref) {
            if (pos + n > N) { ok = false; break; }
            prev = bits_at(p, len, pos, n);
            pos += n;
        }
        unsigned delta = 0;
        bool bad = false;
        if (id == 0 && !second) {
            unsigned v, nb;
            if (!fs_section(p, len, pos, 1, 0, lane, v)) { ok = false; break; }
            v = __shfl(v, 0, 64);
            if (v == 4) {
                const unsigned seg_end = (b / 64 + 1) * 64;
                nb = (seg_end < B ? seg_end : B) - b;
            } else
                nb = v < 4 ? v + 1 : v;
            if (nb > B - b) { ok = false; break; }
            if (STORE)
                for (unsigned i = lane; i < nb * J; i += 64) put(out, base + i, S, prev);
            b += nb;
            continue;
        }
        if (id == 0) {
            unsigned g;
            if (!fs_section(p, len, pos, J / 2, 0, lane, g)) { ok = false; break; }
            unsigned beta = (unsigned)((sqrtf(8.0f * (float)g + 1.0f) - 1.0f) * 0.5f);      // g < 2^23: fixed up exactly in 32 bits
            while (beta * (beta + 1) / 2 > g) --beta;
            while ((beta + 1) * (beta + 2) / 2 <= g) ++beta;
            const unsigned c = g - beta * (beta + 1) / 2, a = beta - c;
            const unsigned as = __shfl(a, (int)(lane >> 1), 64), cs = __shfl(c, (int)(lane >> 1), 64);
            delta = (lane & 1u) ? cs : as;
            bad = lane < J && (delta > xmax || (ref && lane == 0 && delta != 0));
        } else if (id == raw_id) {
            if ((unsigned long long)pos + (unsigned long long)cnt * n > N) { ok = false; break; }
            delta = body ? bits_at(p, len, pos + (lane - first) * n, n) : 0u;
            pos += cnt * n;
        } else {
            const unsigned k = id - 1;
            unsigned h;
            if (!fs_section(p, len, pos, cnt, first, lane, h)) { ok = false; break; }
            if ((unsigned long long)pos + (unsigned long long)cnt * k > N) { ok = false; break; }
            const unsigned lo = body ? bits_at(p, len, pos + (lane - first) * k, k) : 0u;
            pos += cnt * k;
            bad = body && (h > (xmax >> k) || ((h << k) | lo) > xmax);
            delta = bad ? 0u : (h << k) | lo;
        }
        if (__ballot(bad)) { ok = false; break; }
        if (!body) delta = 0;
        // the predictor: assume no step is clipped, prefix-sum the steps, let every lane certify its step against the
        // literal rule from the sample in front, repair from the first lane that fails and certify the rest again
        const int D = (delta & 1u) ? -(int)((delta + 1u) >> 1) : (int)(delta >> 1);
        const int Sx = wave_incl_scan(D, (int)lane);
        int base_lane = ref ? 0 : -1, bv = (int)prev, Sb = ref ? __shfl(Sx, 0, 64) : 0;
        int x = bv + Sx - Sb;
        for (;;) {
            const int up = __shfl_up(x, 1, 64);
            const int xp = (int)lane == base_lane + 1 ? bv : up;
            bool good = true;
            if ((int)lane > base_lane && lane < J) {
                good = xp >= 0 && xp <= (int)xmax;
                if (good) {
                    const unsigned room = xmax - (unsigned)xp, th = (unsigned)xp < room ? (unsigned)xp : room;
                    good = delta <= 2 * th;
                }
            }
            const unsigned long long fail = __ballot(!good);
            if (!fail) break;
            const int f = __ffsll((long long)fail) - 1;
            const unsigned xf = unmap((unsigned)__shfl(xp, f, 64), __shfl(delta, f, 64), xmax);       // (the lane in front of f is certified)
            const int Sf = __shfl(Sx, f, 64);
            if ((int)lane >= f) x = (int)xf + Sx - Sf;
            base_lane = f;
            bv = (int)xf;
        }
        if (STORE && lane < J) put(out, base + lane, S, (unsigned)x);
        prev = (unsigned)__shfl(x, (int)(J - 1u), 64);
        b += 1;
    }
    if (STORE && !ok)
        for (unsigned i = b * J + lane; i < S; i += 64) out[i] = 0;
    if (lane == 0) *status = ok ? 0 : 1;
}

}  // namespace xrit
