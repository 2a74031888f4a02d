// acquire.hip -- the kernels of the carrier acquisition stage (include/xritdemod_amd.h, "Carrier acquisition"; DESIGN.md
// section 21; tests/acquire_spec.py is the specification).
//   mix       one pass: the oscillator's phase of sample i is acc + i * inc (mod 2^64), both read from device memory;
//             sine and cosine are the C library's bit for bit (exact_sincos.h), the rotation is four float32 products and
//             two sums (the Makefile's -ffp-contract=off keeps them apart).  A second, one-thread kernel behind it moves
//             acc on: the mix kernel's blocks all read the acc of the call's start.
//   estimate  one workgroup per segment: convert, pre-sum, square, window, a 4096-point FFT (three radix-16 passes, the
//             first straight from the loads, LDS between them), the spectrum to scratch in bin order; one thread per bin
//             sums the segments' powers in segment order; one wave finds the first maximum, sums the bin's products from
//             segment to segment, writes the record and, if asked and the status is OK, the state's inc.  No atomics.
#include "acquire_host.h"
#include "common.h"
#include "exact_sincos.h"
#include "kernels.h"
#include "wave_ops.h"

namespace xrit {

namespace {

constexpr unsigned N = ACQ_N, HOP = ACQ_HOP;

// ---- samples as onSamplesAvailable converts them (demodulator.cpp:54-74) --------------------------------------
template <int TYPE> __device__ __forceinline__ float2 load_sample(const void *in, size_t i)
{
    if (TYPE == XRIT_SAMPLE_FLOATIQ) return static_cast<const float2 *>(in)[i];
    if (TYPE == XRIT_SAMPLE_S16IQ) {
        const short2 v = static_cast<const short2 *>(in)[i];
        return make_float2((float)v.x * 0x1p-15f, (float)v.y * 0x1p-15f);
    }
    const char2 v = static_cast<const char2 *>(in)[i];
    return make_float2((float)v.x * 0x1p-7f, (float)v.y * 0x1p-7f);
}

// ---- mix --------------------------------------------------------------------------------------------------------
constexpr float PHASE_K = (float)(3.14159265358979323846 * 0x1p-31);      // (float)(pi 2^-31): a power of two times (float)pi

__device__ __forceinline__ float2 rotate(float2 x, unsigned long long a)
{
    const int h = (int)(unsigned)(a >> 32);
    const float theta = (float)h * PHASE_K;         // int -> float rounds to nearest even; |theta| <= pi
    float s, c;
    exact_sincosf(theta, s, c);
    return make_float2(x.x * c + x.y * s, x.y * c - x.x * s);
}

// samples of one 16-byte load
template <int TYPE> struct Group { static constexpr unsigned G = TYPE == XRIT_SAMPLE_FLOATIQ ? 2 : TYPE == XRIT_SAMPLE_S16IQ ? 4 : 8; };

// both pointers 16-byte aligned: a thread takes the G samples of one 16-byte load and stores them as G / 2 16-byte pairs
template <int TYPE>
__global__ void __launch_bounds__(256) acquire_mix_wide_kernel(const uint4 *in, float4 *out, size_t groups,
                                                               const xrit_acquire_state *__restrict__ st)
{
    constexpr unsigned G = Group<TYPE>::G;
    const unsigned long long acc = st->acc, inc = (unsigned long long)st->inc;
    for (size_t g = (size_t)blockIdx.x * 256u + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256u) {
        const uint4 raw = in[g];
        const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
        float2 x[G];
#pragma unroll
        for (unsigned k = 0; k < G; ++k) {
            if (TYPE == XRIT_SAMPLE_FLOATIQ) x[k] = make_float2(__uint_as_float(w[2 * k]), __uint_as_float(w[2 * k + 1]));
            else if (TYPE == XRIT_SAMPLE_S16IQ)
                x[k] = make_float2((float)(short)(w[k] & 0xffffu) * 0x1p-15f, (float)(short)(w[k] >> 16) * 0x1p-15f);
            else {
                const unsigned v = w[k / 2] >> (16 * (k & 1));
                x[k] = make_float2((float)(signed char)(v & 0xffu) * 0x1p-7f, (float)(signed char)((v >> 8) & 0xffu) * 0x1p-7f);
            }
        }
        const unsigned long long a0 = acc + (unsigned long long)g * G * inc;
#pragma unroll
        for (unsigned k = 0; k < G; k += 2) {
            const float2 y0 = rotate(x[k], a0 + k * inc), y1 = rotate(x[k + 1], a0 + (k + 1) * inc);
            out[g * (G / 2) + k / 2] = make_float4(y0.x, y0.y, y1.x, y1.y);
        }
    }
}

// samples first .. n - 1 one by one: the tail of a wide call, or all of a call whose pointers are not 16-byte aligned
template <int TYPE>
__global__ void __launch_bounds__(256) acquire_mix_kernel(const void *in, float2 *out, size_t first, size_t n,
                                                          const xrit_acquire_state *__restrict__ st)
{
    const unsigned long long acc = st->acc, inc = (unsigned long long)st->inc;
    for (size_t i = first + (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u)
        out[i] = rotate(load_sample<TYPE>(in, i), acc + (unsigned long long)i * inc);
}

__global__ void acquire_advance_kernel(xrit_acquire_state *st, unsigned long long n)
{
    st->acc += n * (unsigned long long)st->inc;
    st->samples_mixed += n;
}

__global__ void acquire_set_inc_kernel(xrit_acquire_state *st, long long inc) { st->inc = inc; }

// ---- estimate ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// One radix-4 decimation-in-frequency butterfly in place: y_q = sum_m a_m (-i)^(m q), times W^(q e) (tw[k] = exp(-2 pi i k / N)).
__device__ __forceinline__ void bfly4(float2 &a0, float2 &a1, float2 &a2, float2 &a3, unsigned e, const float2 *__restrict__ tw)
{
    const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y), t3 = make_float2(a1.x - a3.x, a1.y - a3.y);
    a0 = make_float2(t0.x + t2.x, t0.y + t2.y);
    a1 = cmul(make_float2(t1.x + t3.y, t1.y - t3.x), tw[e]);            // t1 - i t3
    a2 = cmul(make_float2(t0.x - t2.x, t0.y - t2.y), tw[2 * e]);
    a3 = cmul(make_float2(t1.x - t3.y, t1.y + t3.x), tw[3 * e]);        // t1 + i t3
}

// Two radix-4 levels on the sixteen elements a thread holds: r[q] is position base + S2 * q of the in-place transform,
// the first level has stride S1 = 4 S2 (butterfly index j = jbase + JSTEP c for the elements c, c + 4, c + 8, c + 12), the
// second stride S2 (j = jbase, elements 4 d .. 4 d + 3).  U1 = N / (4 S1) and U2 = N / (4 S2) scale j to the twiddle table.
template <unsigned JSTEP, unsigned U1, unsigned U2>
__device__ __forceinline__ void radix16(float2 (&r)[16], unsigned jbase, const float2 *__restrict__ tw)
{
#pragma unroll
    for (unsigned c = 0; c < 4; ++c) bfly4(r[c], r[c + 4], r[c + 8], r[c + 12], (jbase + JSTEP * c) * U1, tw);
#pragma unroll
    for (unsigned d = 0; d < 4; ++d) bfly4(r[4 * d], r[4 * d + 1], r[4 * d + 2], r[4 * d + 3], jbase * U2, tw);
}

// one float pair of padding behind every sixteen: the three passes' 8-byte accesses (thread t at t + 256 q, at
// 256 (t / 16) + t % 16 + 16 q, at 16 t + q) then fall on distinct banks within each half wave but for one pair in the first
__device__ __forceinline__ unsigned pad(unsigned p) { return p + (p >> 4); }
constexpr unsigned LDS_PAIRS = N + N / 16;

// the position of bin k in the in-place transform's output: its six base-4 digits reversed
__device__ __forceinline__ unsigned digit_reverse(unsigned k)
{
    const unsigned b = __brev(k) >> 20;
    return ((b & 0xAAAu) >> 1) | ((b & 0x555u) << 1);
}

template <int TYPE>
__global__ void __launch_bounds__(256) acquire_segment_kernel(const void *__restrict__ in, unsigned pre_sum,
                                                              const float2 *__restrict__ tw, const float *__restrict__ win,
                                                              float2 *__restrict__ spectra)
{
    __shared__ float2 lds[LDS_PAIRS];
    const unsigned t = threadIdx.x;
    const size_t seg = blockIdx.x;
    float2 r[16];
#pragma unroll
    for (unsigned q = 0; q < 16; ++q) {
        const unsigned m = t + 256u * q;
        const size_t base = (seg * HOP + m) * pre_sum;
        float2 u = load_sample<TYPE>(in, base);
        for (unsigned i = 1; i < pre_sum; ++i) {
            const float2 v = load_sample<TYPE>(in, base + i);
            u.x += v.x;
            u.y += v.y;
        }
        const float w = win[m];
        r[q] = make_float2((u.x * u.x - u.y * u.y) * w, (2.0f * u.x * u.y) * w);
    }
    radix16<256, 1, 4>(r, t, tw);                   // strides 1024 and 256
#pragma unroll
    for (unsigned q = 0; q < 16; ++q) lds[pad(t + 256u * q)] = r[q];
    __syncthreads();
    const unsigned bB = 256u * (t >> 4) + (t & 15u);
#pragma unroll
    for (unsigned q = 0; q < 16; ++q) r[q] = lds[pad(bB + 16u * q)];
    radix16<16, 16, 64>(r, t & 15u, tw);            // strides 64 and 16
#pragma unroll
    for (unsigned q = 0; q < 16; ++q) lds[pad(bB + 16u * q)] = r[q];
    __syncthreads();
#pragma unroll
    for (unsigned q = 0; q < 16; ++q) r[q] = lds[pad(16u * t + q)];
    radix16<1, 256, 1024>(r, 0, tw);                // strides 4 and 1
#pragma unroll
    for (unsigned q = 0; q < 16; ++q) lds[pad(16u * t + q)] = r[q];
    __syncthreads();
    float2 *out = spectra + seg * N;
#pragma unroll
    for (unsigned q = 0; q < 16; ++q) {
        const unsigned k = t + 256u * q;
        out[k] = lds[pad(digit_reverse(k))];
    }
}

// P[k] = the segments' |X_s[k]|^2 (float32) summed in segment order (float64)
__global__ void __launch_bounds__(256) acquire_power_kernel(const float2 *__restrict__ spectra, unsigned segments, double *__restrict__ P)
{
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    double acc = 0.0;
    for (unsigned s = 0; s < segments; ++s) {
        const float2 v = spectra[(size_t)s * N + k];
        acc += (double)(v.x * v.x + v.y * v.y);
    }
    P[k] = acc;
}

// one wave: the first maximum of P, the phase step of its bin from segment to segment, the record, the state
__global__ void __launch_bounds__(64) acquire_finish_kernel(const float2 *__restrict__ spectra, const double *__restrict__ P,
                                                            unsigned segments, unsigned pre_sum, double sample_rate, double min_ratio,
                                                            int apply, xrit_acquire_state *st, xrit_acquire_estimate_record *rec)
{
    const unsigned lane = threadIdx.x;
    xrit_acquire_estimate_record o{};
    o.segments = segments;
    if (segments < ACQ_MIN_SEGMENTS) {
        o.status = XRIT_ACQUIRE_TOO_SHORT;
        if (lane == 0) {
            *rec = o;
            st->estimates += 1;
        }
        return;
    }
    double best = -1.0, sum = 0.0;
    unsigned bk = 0;
    for (unsigned i = 0; i < N / 64; ++i) {
        const unsigned k = lane + 64u * i;
        const double v = P[k];
        sum += v;
        if (v > best) { best = v; bk = k; }
    }
    for (int off = 32; off > 0; off >>= 1) {            // (no wave_max: value and bin together, ties to the lower bin)
        const double ov = __shfl_xor(best, off);
        const unsigned ok = __shfl_xor(bk, off);
        if (ov > best || (ov == best && ok < bk)) { best = ov; bk = ok; }
    }
    sum = wave_sum(sum);
    const unsigned k0 = bk;
    double cr = 0.0, ci = 0.0;
    for (unsigned s = 1 + lane; s < segments; s += 64u) {
        const float2 a = spectra[(size_t)s * N + k0], b = spectra[(size_t)(s - 1) * N + k0];
        const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
        cr += ax * bx + ay * by;
        ci += ay * bx - ax * by;
    }
    cr = wave_sum(cr);
    ci = wave_sum(ci);
    if (lane != 0) return;
    if (k0 & 1u) { cr = -cr; ci = -ci; }
    const double d = atan2(ci, cr);
    double nu2 = (double)k0 / (double)N + d / (3.14159265358979323846 * (double)N);
    nu2 -= floor(nu2 + 0.5);
    const double nu = nu2 / (double)(2u * pre_sum);
    o.k0 = k0;
    o.ratio = best / (sum / (double)N);
    o.nu = nu;
    o.hz = nu * sample_rate;
    const bool ok = o.ratio >= min_ratio;           // (a NaN is WEAK)
    o.status = ok ? XRIT_ACQUIRE_OK : XRIT_ACQUIRE_WEAK;
    o.inc = nu == nu ? __double2ll_rn(ldexp(nu, 64)) : 0;      // |nu| <= 1/4: within 2^62
    o.applied = (ok && apply) ? 1u : 0u;
    *rec = o;
    st->estimates += 1;
    if (o.applied) {
        st->inc = o.inc;
        st->applied += 1;
    }
}

template <int TYPE> int mix_typed(const void *in, size_t n, float2 *out, const xrit_acquire_state *st, hipStream_t s)
{
    constexpr unsigned G = Group<TYPE>::G;
    size_t first = 0;
    if (((size_t)in & 15) == 0 && ((size_t)out & 15) == 0 && n >= G) {
        const size_t groups = n / G;
        const unsigned grid = div_up(groups, 256) < 16384u ? div_up(groups, 256) : 16384u;
        hipLaunchKernelGGL(acquire_mix_wide_kernel<TYPE>, dim3(grid), dim3(256), 0, s, static_cast<const uint4 *>(in),
                           reinterpret_cast<float4 *>(out), groups, st);
        XR_HIP(hipGetLastError());
        first = groups * G;
    }
    if (first < n) {
        const unsigned grid = div_up(n - first, 256) < 16384u ? div_up(n - first, 256) : 16384u;
        hipLaunchKernelGGL(acquire_mix_kernel<TYPE>, dim3(grid), dim3(256), 0, s, in, out, first, n, st);
        XR_HIP(hipGetLastError());
    }
    return XRIT_OK;
}

}  // namespace

size_t acquire_scratch_carve(void *base, unsigned segments, AcquireScratch &sc)
{
    Carver c{static_cast<char *>(base)};
    sc.spectra = c.take<float2>(acquire_spectra_bytes(segments) / sizeof(float2), 16);
    sc.power = c.take<double>(ACQ_POWER_BYTES / sizeof(double), 16);
    return c.used();
}

int launch_acquire_mix(const void *in, int type, size_t n, float2 *out, xrit_acquire_state *st, hipStream_t s)
{
    if (n) {
        if (type == XRIT_SAMPLE_FLOATIQ) XR_TRY(mix_typed<XRIT_SAMPLE_FLOATIQ>(in, n, out, st, s));
        else if (type == XRIT_SAMPLE_S16IQ) XR_TRY(mix_typed<XRIT_SAMPLE_S16IQ>(in, n, out, st, s));
        else XR_TRY(mix_typed<XRIT_SAMPLE_S8IQ>(in, n, out, st, s));
    }
    hipLaunchKernelGGL(acquire_advance_kernel, dim3(1), dim3(1), 0, s, st, (unsigned long long)n);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_acquire_set_inc(xrit_acquire_state *st, long long inc, hipStream_t s)
{
    hipLaunchKernelGGL(acquire_set_inc_kernel, dim3(1), dim3(1), 0, s, st, inc);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

int launch_acquire_estimate(const void *in, int type, unsigned segments, const xrit_acquire_params &par, const float2 *tw, const float *win,
                            const AcquireScratch &sc, int apply, xrit_acquire_state *st, xrit_acquire_estimate_record *rec, hipStream_t s)
{
    if (segments >= ACQ_MIN_SEGMENTS) {
        if (type == XRIT_SAMPLE_FLOATIQ)
            hipLaunchKernelGGL(acquire_segment_kernel<XRIT_SAMPLE_FLOATIQ>, dim3(segments), dim3(256), 0, s, in, par.pre_sum, tw, win, sc.spectra);
        else if (type == XRIT_SAMPLE_S16IQ)
            hipLaunchKernelGGL(acquire_segment_kernel<XRIT_SAMPLE_S16IQ>, dim3(segments), dim3(256), 0, s, in, par.pre_sum, tw, win, sc.spectra);
        else
            hipLaunchKernelGGL(acquire_segment_kernel<XRIT_SAMPLE_S8IQ>, dim3(segments), dim3(256), 0, s, in, par.pre_sum, tw, win, sc.spectra);
        XR_HIP(hipGetLastError());
        hipLaunchKernelGGL(acquire_power_kernel, dim3(N / 256), dim3(256), 0, s, sc.spectra, segments, sc.power);
        XR_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(acquire_finish_kernel, dim3(1), dim3(64), 0, s, sc.spectra, sc.power, segments, par.pre_sum, par.sample_rate,
                       par.min_ratio, apply, st, rec);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
