// rice.hip -- the Rice decoder (CCSDS 121.0-B adaptive entropy coder, unit-delay predictor) on a batch of coded lines
// (tests/rice_spec.py is the serial statement).  Two forms, both held to the specification
// (xrit_rice_form chooses; DESIGN.md has both times):
//  - one LANE per line (rice_lane_kernel): the specification's loop, block after block, over a 64-bit window that is
//    refilled a byte at a time; fundamental-sequence codes are read with a count of leading zeros.  A split-sample block
//    is read by two readers, one along the codes and one along the k-bit low parts behind them.  Samples are written as
//    they are decoded; a fault zeroes the line from the faulting block on.
//  - one WAVE per line (rice_wave_kernel): the blocks one after the other, lane q on the block's q-th sample: the codes'
//    ends found by popcounts over 64 windows of 64 bits, their prefix and a binary select; the predictor as an
//    assume-unclipped prefix sum that every lane certifies against the literal step, repaired from the first lane that
//    fails.  Stores are coalesced.
// No LDS, no scratch; everything is integer (one float square root as a starting guess, fixed up exactly).
#include "kernels.h"

namespace xrit {

namespace {
struct Reader {
    const unsigned char *p;         // the line
    unsigned len;                   // its bytes
    unsigned long long buf;         // the next `have` bits, from bit 63 down; zeros below them
    unsigned have;
    unsigned pos;                   // bits consumed
};

__device__ __forceinline__ void refill(Reader &r)
{
    unsigned next = (r.pos + r.have) >> 3;              // (pos + have is a multiple of 8 once a reader stands)
    while (r.have <= 56 && next < r.len) {
        r.buf |= (unsigned long long)r.p[next] << (56 - r.have);
        r.have += 8;
        ++next;
    }
}

__device__ __forceinline__ Reader reader_at(const unsigned char *p, unsigned len, unsigned pos)
{
    Reader r{p, len, 0ull, 0u, pos};
    const unsigned byte = pos >> 3, sub = pos & 7u;
    if (byte < len) {
        r.buf = (unsigned long long)p[byte] << (56 + sub);
        r.have = 8 - sub;
    }
    return r;
}

// m bits (0 .. 16); false when they are not all there
__device__ __forceinline__ bool get(Reader &r, unsigned m, unsigned &v)
{
    v = 0;
    if (m == 0) return true;
    refill(r);
    if (r.have < m) return false;
    v = (unsigned)(r.buf >> (64 - m));
    r.buf <<= m;
    r.have -= m;
    r.pos += m;
    return true;
}

// a fundamental-sequence code: zeros up to the next one; false when the line ends first
__device__ __forceinline__ bool fs(Reader &r, unsigned &v)
{
    v = 0;
    for (;;) {
        refill(r);
        if (r.have == 0) return false;
        if (r.buf == 0) {
            v += r.have;
            r.pos += r.have;
            r.have = 0;
            continue;
        }
        const unsigned z = (unsigned)__clzll((long long)r.buf);     // < have: the bits below `have` are zero
        v += z;
        r.buf = z == 63 ? 0ull : r.buf << (z + 1);
        r.have -= z + 1;
        r.pos += z + 1;
        return true;
    }
}

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

template <typename T>
__device__ void decode_line(const unsigned char *p, unsigned len, unsigned n, unsigned J, unsigned S, T *out, unsigned char *status)
{
    const unsigned B = (S + J - 1) / J, L = n <= 8 ? 3u : 4u, xmax = (1u << n) - 1u, raw_id = (1u << L) - 1u;
    Reader r = reader_at(p, len, 0);
    unsigned b = 0, prev = 0;
    bool ok = true;
    while (b < B) {
        const bool ref = b == 0;
        const unsigned cnt = ref ? J - 1 : J, base = b * J;
        unsigned id, v, nb = 1;
        if (!(ok = get(r, L, id))) break;
        if (id == 0) {
            unsigned second;
            if (!(ok = get(r, 1, second))) break;
            if (ref) {
                if (!(ok = get(r, n, prev))) break;
                put(out, 0u, S, prev);
            }
            if (second) {
                for (unsigned i = 0; i < J / 2 && ok; ++i) {
                    if (!(ok = fs(r, v))) break;
                    // beta: the largest integer with beta (beta + 1) / 2 <= v (a line has at most 2^20 bytes, so v < 2^23 and
                    // beta < 2^12: the float root is a start, fixed up exactly in 32 bits)
                    unsigned beta = (unsigned)((sqrtf(8.0f * (float)v + 1.0f) - 1.0f) * 0.5f);
                    while (beta * (beta + 1) / 2 > v) --beta;
                    while ((beta + 1) * (beta + 2) / 2 <= v) ++beta;
                    const unsigned c = v - beta * (beta + 1) / 2, a = beta - c;
                    if (a > xmax || c > xmax || (ref && i == 0 && a != 0)) { ok = false; break; }
                    if (!(ref && i == 0)) {
                        prev = unmap(prev, a, xmax);
                        put(out, base + 2 * i, S, prev);
                    }
                    prev = unmap(prev, c, xmax);
                    put(out, base + 2 * i + 1, S, prev);
                }
            } else {
                if (!(ok = fs(r, v))) break;
                if (v == 4) {
                    const unsigned seg_end = (b / 64 + 1) * 64;
                    nb = (seg_end < B ? seg_end : B) - b;
                } else
                    nb = v < 4 ? v + 1 : v;
                if (nb > B - b) { ok = false; break; }
                for (unsigned i = ref ? 1u : 0u; i < nb * J; ++i) put(out, base + i, S, prev);
            }
        } else if (id == raw_id) {
            if (ref) {
                if (!(ok = get(r, n, prev))) break;
                put(out, 0u, S, prev);
            }
            for (unsigned i = J - cnt; i < J; ++i) {
                if (!(ok = get(r, n, v))) break;
                prev = unmap(prev, v, xmax);
                put(out, base + i, S, prev);
            }
        } else {
            const unsigned k = id - 1;
            if (ref) {
                if (!(ok = get(r, n, prev))) break;
                put(out, 0u, S, prev);
            }
            // the codes once in front: where the low parts begin, and whether they are all there
            Reader hi = r;
            for (unsigned i = 0; i < cnt; ++i)
                if (!(ok = fs(r, v))) break;
            if (!ok || (unsigned long long)r.pos + (unsigned long long)cnt * k > 8ull * len) { ok = false; break; }
            Reader lo = reader_at(p, len, r.pos);
            const unsigned hmax = xmax >> k;                // (k > n: 0)
            for (unsigned i = J - cnt; i < J; ++i) {
                unsigned h, l;
                fs(hi, h);
                get(lo, k, l);
                if (h > hmax || ((h << k) | l) > xmax) { ok = false; break; }
                prev = unmap(prev, (h << k) | l, xmax);
                put(out, base + i, S, prev);
            }
            r = lo;
        }
        if (!ok) break;
        b += nb;
    }
    if (!ok)
        for (unsigned i = b * J; i < S; ++i) out[i] = 0;
    *status = ok ? 0 : 1;
}

// ---- one wave per line -----------------------------------------------------------------------------------------------
// The wave walks the line's blocks one after the other (where a block begins depends on the one before); inside a block
// lane q has the block's q-th sample.  Fixed fields are read by every lane from the same place.
constexpr unsigned MAX_LINE = 1u << 20;             // bytes; longer lines are refused (status 2)

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
        unsigned P = c;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned y = __shfl_up(P, off, 64);
            if ((int)lane >= off) P += y;
        }
        const unsigned T = __shfl(P, 63, 64);
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

template <typename T>
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
        int Sx = D;
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(Sx, off, 64);
            if ((int)lane >= off) Sx += y;
        }
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
        if (lane < J) put(out, base + lane, S, (unsigned)x);
        prev = (unsigned)__shfl(x, (int)(J - 1u), 64);
        b += 1;
    }
    if (!ok)
        for (unsigned i = b * J + lane; i < S; i += 64) out[i] = 0;
    if (lane == 0) *status = ok ? 0 : 1;
}
}  // namespace

// the descriptor of a line; false (status 2, an all-zero line) when it points outside the bytes or the line is longer than
// MAX_LINE (so that bit positions, code values and the second extension's arithmetic stay inside 32 bits)
__device__ __forceinline__ bool line_of(const unsigned char *desc, unsigned stride, unsigned line, unsigned long long n_bytes,
                                        unsigned long long &off, unsigned &len)
{
    const unsigned char *d = desc + (size_t)line * stride;
    off = *reinterpret_cast<const unsigned long long *>(d);
    len = *reinterpret_cast<const unsigned *>(d + 8);
    return !(off > n_bytes || len > n_bytes - off || len > MAX_LINE);
}

__global__ void __launch_bounds__(64) rice_lane_kernel(const unsigned char *__restrict__ bytes, unsigned long long n_bytes,
                                                      const unsigned char *__restrict__ desc, unsigned stride, unsigned n_lines, unsigned n,
                                                      unsigned J, unsigned S, void *__restrict__ out, unsigned char *__restrict__ status)
{
    const unsigned line = blockIdx.x * 64u + threadIdx.x;
    if (line >= n_lines) return;
    unsigned long long off;
    unsigned len;
    if (!line_of(desc, stride, line, n_bytes, off, len)) {
        if (n <= 8) for (unsigned i = 0; i < S; ++i) static_cast<unsigned char *>(out)[(size_t)line * S + i] = 0;
        else for (unsigned i = 0; i < S; ++i) static_cast<unsigned short *>(out)[(size_t)line * S + i] = 0;
        status[line] = 2;
        return;
    }
    if (n <= 8) decode_line(bytes + off, len, n, J, S, static_cast<unsigned char *>(out) + (size_t)line * S, status + line);
    else decode_line(bytes + off, len, n, J, S, static_cast<unsigned short *>(out) + (size_t)line * S, status + line);
}

__global__ void __launch_bounds__(64) rice_wave_kernel(const unsigned char *__restrict__ bytes, unsigned long long n_bytes,
                                                      const unsigned char *__restrict__ desc, unsigned stride, unsigned n_lines, unsigned n,
                                                      unsigned J, unsigned S, void *__restrict__ out, unsigned char *__restrict__ status)
{
    const unsigned line = blockIdx.x, lane = threadIdx.x;
    if (line >= n_lines) return;
    unsigned long long off;
    unsigned len;
    if (!line_of(desc, stride, line, n_bytes, off, len)) {
        if (n <= 8) for (unsigned i = lane; i < S; i += 64) static_cast<unsigned char *>(out)[(size_t)line * S + i] = 0;
        else for (unsigned i = lane; i < S; i += 64) static_cast<unsigned short *>(out)[(size_t)line * S + i] = 0;
        if (lane == 0) status[line] = 2;
        return;
    }
    if (n <= 8) decode_line_wave(bytes + off, len, n, J, S, static_cast<unsigned char *>(out) + (size_t)line * S, status + line, lane);
    else decode_line_wave(bytes + off, len, n, J, S, static_cast<unsigned short *>(out) + (size_t)line * S, status + line, lane);
}

int launch_rice(const unsigned char *bytes, size_t n_bytes, const void *desc, size_t stride, size_t n_lines, int n, int J, int S,
                void *out, unsigned char *status, int form, hipStream_t s)
{
    if (n_lines == 0) return XRIT_OK;
    if (form == RICE_FORM_LANE)
        hipLaunchKernelGGL(rice_lane_kernel, dim3(div_up(n_lines, 64)), dim3(64), 0, s, bytes, (unsigned long long)n_bytes,
                           static_cast<const unsigned char *>(desc), (unsigned)stride, (unsigned)n_lines, (unsigned)n, (unsigned)J,
                           (unsigned)S, out, status);
    else
        hipLaunchKernelGGL(rice_wave_kernel, dim3((unsigned)n_lines), dim3(64), 0, s, bytes, (unsigned long long)n_bytes,
                           static_cast<const unsigned char *>(desc), (unsigned)stride, (unsigned)n_lines, (unsigned)n, (unsigned)J,
                           (unsigned)S, out, status);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
