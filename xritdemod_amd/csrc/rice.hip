// rice.hip -- the Rice decoder (CCSDS 121.0-B adaptive entropy coder, unit-delay predictor) on a batch of coded lines
// (tests/rice_spec.py is the serial statement).  Two forms, both held to the specification
// (xrit_rice_form chooses; DESIGN.md has both times):
//  - one LANE per line (rice_lane_kernel): the specification's loop, block after block, over a 64-bit window that is
//    refilled a byte at a time; fundamental-sequence codes are read with a count of leading zeros.  A split-sample block
//    is read by two readers, one along the codes and one along the k-bit low parts behind them.  Samples are written as
//    they are decoded; a fault zeroes the line from the faulting block on.
//  - one WAVE per line (rice_wave_kernel; decode_line_wave and its parts are in rice_core.h, which the image stage
//    shares): the blocks one after the other, lane q on the block's q-th sample: the codes'
//    ends found by popcounts over 64 windows of 64 bits, their prefix and a binary select; the predictor as an
//    assume-unclipped prefix sum that every lane certifies against the literal step, repaired from the first lane that
//    fails.  Stores are coalesced.
// No LDS, no scratch; everything is integer (one float square root as a starting guess, fixed up exactly).
#include "kernels.h"
#include "rice_core.h"

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

}  // namespace

// the descriptor of a line; false (status 2, an all-zero line) when it points outside the bytes or the line is longer than
// RICE_MAX_LINE (so that bit positions, code values and the second extension's arithmetic stay inside 32 bits)
__device__ __forceinline__ bool line_of(const unsigned char *desc, unsigned stride, unsigned line, unsigned long long n_bytes,
                                        unsigned long long &off, unsigned &len)
{
    const unsigned char *d = desc + (size_t)line * stride;
    off = *reinterpret_cast<const unsigned long long *>(d);
    len = *reinterpret_cast<const unsigned *>(d + 8);
    return !(off > n_bytes || len > n_bytes - off || len > RICE_MAX_LINE);
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
