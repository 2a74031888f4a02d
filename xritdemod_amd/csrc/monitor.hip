// monitor.hip -- the kernels of the link monitor (include/xritdemod_amd.h, "Link monitor"; DESIGN.md section 22;
// tests/monitor_spec.py is the specification).  Everything summed is an integer: no float atomics, no float reductions,
// the same words whatever the order.
//   reduce   the pieces of a push (monitor_host.h: the head that completes the open block, every whole block, the tail) one
//            by one: a workgroup per piece for blocks of 2048 symbols and more, a wave per piece below.  16-byte loads over
//            the aligned core of the piece (4 floats or 16 int8 per lane), one symbol per lane on the edges in front of and
//            behind it, since a block boundary falls anywhere relative to the pointer's alignment.  64-bit partials per lane
//            for s2 and s4 (32 bits hold the others: at most 32768 * 4095 < 2^27), wave sums, the waves joined through LDS.
//            The sign in front of a symbol is that of the symbol before it in the call, in front of the call's first the
//            state's.  A whole block behind piece 0 goes straight to its row; piece 0 and the tail go to two scratch
//            records.  The 256-bin histogram is kept in LDS (eight copies, picked by the lane, so that a clean signal's few
//            bins do not serialise a wave) and added to the state's bins with one 64-bit global atomic per bin in use.
//   commit   one wave behind it: the open record plus piece 0 becomes row 0, or stays open when the call completes nothing;
//            the tail becomes the open record; totals, the last sign, the summary.  The only writer of the state, the
//            histogram excepted.
#include "common.h"
#include "kernels.h"
#include "monitor_host.h"
#include "wave_ops.h"

namespace xrit {

namespace {

constexpr unsigned HIST_BINS = 256, HIST_COPIES = 8;
constexpr uint32_t WORKGROUP_PIECE = 2048;          // blocks from here on take a workgroup per piece

template <int TYPE> struct Symbol;
template <> struct Symbol<XRIT_SYMBOL_F32> { using type = float; };
template <> struct Symbol<XRIT_SYMBOL_I8> { using type = signed char; };

struct Acc {
    uint32_t flips, s1, sat, clamped, bad, neg;
    int32_t sum;
    uint64_t s2, s4;
};

// ---- the lattice ------------------------------------------------------------------------------------------------
// q < 0 alone (the symbol in front of a lane's first)
__device__ __forceinline__ bool lattice_neg(float x) { return __builtin_rintf(x * 512.0f) <= -1.0f; }
__device__ __forceinline__ bool lattice_neg(signed char v) { return v < 0; }

__device__ __forceinline__ int lattice(float x, Acc &a)
{
    const float r = __builtin_rintf(x * 512.0f);       // the product is exact; v_rndne: ties to even
    const bool bad = r != r;
    a.bad += bad;
    a.clamped += fabsf(r) > 4095.0f;
    const int q = bad ? 0 : (int)fminf(fmaxf(r, -4095.0f), 4095.0f);
    a.sat += abs(q) > 512;
    return q;
}

__device__ __forceinline__ int lattice(signed char v, Acc &a)
{
    a.sat += (v == 127) | (v == -128);
    return 4 * (int)v;
}

__device__ __forceinline__ float element(const uint4 &raw, unsigned k, float)
{
    const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
    return __uint_as_float(w[k]);
}
__device__ __forceinline__ signed char element(const uint4 &raw, unsigned k, signed char)
{
    const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
    return (signed char)((w[k / 4] >> (8 * (k & 3))) & 0xffu);
}

// one symbol into the lane's partials and the histogram; -> its sign
__device__ __forceinline__ bool take(int q, bool have_prev, bool prev_neg, Acc &a, unsigned *hist, unsigned copy)
{
    const unsigned m = (unsigned)abs(q), q2 = m * m;
    const bool neg = q < 0;
    a.s1 += m;
    a.s2 += q2;
    a.s4 += (uint64_t)q2 * q2;
    a.sum += q;
    a.neg += neg;
    a.flips += have_prev & (neg != prev_neg);
    atomicAdd(&hist[((unsigned)(q + 4096) >> 5) * HIST_COPIES + copy], 1u);
    return neg;
}

// the sign in front of call index i
template <typename E>
__device__ __forceinline__ void sign_before(const E *in, size_t i, const xrit_monitor_state *st, bool &have, bool &neg)
{
    if (i) {
        have = true;
        neg = lattice_neg(in[i - 1]);
    } else {
        have = st->have_last != 0;
        neg = st->last_neg != 0;
    }
}

// symbols [a, b) of the call by a team of NT lanes, tid the lane's number in it: this lane's share
template <typename E, unsigned NT>
__device__ __forceinline__ Acc reduce_piece(const E *in, size_t a, size_t b, unsigned tid, const xrit_monitor_state *st, unsigned *hist,
                                            unsigned copy)
{
    constexpr unsigned PER = 16 / sizeof(E);
    Acc acc{};
    size_t c0 = a + (size_t)((0 - reinterpret_cast<uintptr_t>(in + a)) & 15u) / sizeof(E);       // the first 16-byte boundary
    if (c0 > b) c0 = b;
    const size_t groups = (b - c0) / PER, c1 = c0 + groups * PER;
    const unsigned front = (unsigned)(c0 - a), edge = front + (unsigned)(b - c1);                 // below 2 PER <= 32 < NT
    if (tid < edge) {
        const size_t i = tid < front ? a + tid : c1 + (tid - front);
        bool have, prev;
        sign_before(in, i, st, have, prev);
        take(lattice(in[i], acc), have, prev, acc, hist, copy);
    }
    for (size_t g = tid; g < groups; g += NT) {
        const size_t i = c0 + g * PER;
        const uint4 raw = *reinterpret_cast<const uint4 *>(in + i);
        bool have, prev;
        sign_before(in, i, st, have, prev);
#pragma unroll
        for (unsigned k = 0; k < PER; ++k) {
            prev = take(lattice(element(raw, k, E()), acc), have, prev, acc, hist, copy);
            have = true;
        }
    }
    return acc;
}

__device__ __forceinline__ void wave_sum_all(Acc &a)
{
    a.flips = wave_sum(a.flips);
    a.s1 = wave_sum(a.s1);
    a.sat = wave_sum(a.sat);
    a.clamped = wave_sum(a.clamped);
    a.bad = wave_sum(a.bad);
    a.neg = wave_sum(a.neg);
    a.sum = wave_sum(a.sum);
    a.s2 = wave_sum(a.s2);
    a.s4 = wave_sum(a.s4);
}

__device__ __forceinline__ void store_piece(const Acc &a, size_t k, size_t count, const MonitorPlan &plan, xrit_monitor_block *parts,
                                            xrit_monitor_block *rows, const xrit_monitor_state *st)
{
    xrit_monitor_block r{};
    r.n = (uint32_t)count;
    r.flips = a.flips;
    r.s1 = a.s1;
    r.s2 = a.s2;
    r.s4 = a.s4;
    r.sum = a.sum;
    r.sat = a.sat;
    r.clamped = a.clamped;
    r.bad = a.bad;
    r.neg = a.neg;
    if (k == 0) parts[0] = r;                       // the commit kernel joins it with the open record
    else if (k < plan.rows) {                       // a whole block of its own
        r.first = (st->blocks_total + k) * plan.block;
        rows[k] = r;
    } else parts[1] = r;                            // the tail
}

// NT = 256: the workgroup takes one piece at a time; NT = 64: each of its four waves does
template <int TYPE, unsigned NT>
__global__ void __launch_bounds__(256) monitor_reduce_kernel(const typename Symbol<TYPE>::type *in, MonitorPlan plan, xrit_monitor_block *parts,
                                                             xrit_monitor_block *rows, xrit_monitor_state *st)
{
    __shared__ unsigned hist[HIST_BINS * HIST_COPIES];
    __shared__ Acc joined[4];
    for (unsigned i = threadIdx.x; i < HIST_BINS * HIST_COPIES; i += 256) hist[i] = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr unsigned TEAMS = 256 / NT;
    const unsigned tid = NT == 256 ? threadIdx.x : lane;
    const size_t team = (size_t)blockIdx.x * TEAMS + (NT == 256 ? 0 : wave), teams = (size_t)gridDim.x * TEAMS;
    for (size_t k = team; k < plan.pieces; k += teams) {                // NT = 256: k is the workgroup's, the barriers are met by all
        const size_t a = plan.begin(k), b = plan.end(k);
        Acc acc = reduce_piece<typename Symbol<TYPE>::type, NT>(in, a, b, tid, st, hist, lane & (HIST_COPIES - 1));
        wave_sum_all(acc);
        if (NT == 256) {
            if (lane == 0) joined[wave] = acc;
            __syncthreads();
            if (threadIdx.x == 0) {
                for (unsigned w = 1; w < 4; ++w) {
                    const Acc o = joined[w];
                    acc.flips += o.flips;
                    acc.s1 += o.s1;
                    acc.sat += o.sat;
                    acc.clamped += o.clamped;
                    acc.bad += o.bad;
                    acc.neg += o.neg;
                    acc.sum += o.sum;
                    acc.s2 += o.s2;
                    acc.s4 += o.s4;
                }
            }
            __syncthreads();
        }
        if (tid == 0) store_piece(acc, k, b - a, plan, parts, rows, st);
    }
    __syncthreads();
    unsigned count = 0;
    for (unsigned c = 0; c < HIST_COPIES; ++c) count += hist[threadIdx.x * HIST_COPIES + c];
    if (count) atomicAdd(reinterpret_cast<unsigned long long *>(&st->hist[threadIdx.x]), (unsigned long long)count);
}

__device__ __forceinline__ void add_record(xrit_monitor_block &a, const xrit_monitor_block &b)
{
    a.n += b.n;
    a.flips += b.flips;
    a.s1 += b.s1;
    a.s2 += b.s2;
    a.s4 += b.s4;
    a.sum += b.sum;
    a.sat += b.sat;
    a.clamped += b.clamped;
    a.bad += b.bad;
    a.neg += b.neg;
}

template <int TYPE>
__global__ void __launch_bounds__(64) monitor_commit_kernel(const typename Symbol<TYPE>::type *in, MonitorPlan plan, const xrit_monitor_block *parts,
                                                            xrit_monitor_block *rows, xrit_monitor_state *st, xrit_monitor_summary *summary)
{
    if (threadIdx.x) return;
    xrit_monitor_block open = st->open;
    const uint64_t blocks = st->blocks_total;
    if (plan.pieces) {
        add_record(open, parts[0]);
        if (plan.rows) {
            open.first = blocks * plan.block;
            rows[0] = open;
            open = xrit_monitor_block{};
            if (plan.pieces > plan.rows) open = parts[1];
        }
        st->have_last = 1;
        st->last_neg = lattice_neg(in[plan.n - 1]);
    }
    open.first = (blocks + plan.rows) * plan.block;
    st->open = open;
    const uint64_t total = st->symbols_total + plan.n;
    st->symbols_total = total;
    st->blocks_total = blocks + plan.rows;
    st->calls += 1;
    if (summary) {
        summary->rows = plan.rows;
        summary->open_n = open.n;
        summary->symbols_total = total;
        summary->blocks_total = blocks + plan.rows;
    }
}

template <int TYPE>
int push_typed(const void *in, const MonitorPlan &plan, xrit_monitor_block *parts, xrit_monitor_state *st, xrit_monitor_block *rows,
               xrit_monitor_summary *summary, hipStream_t s)
{
    using E = typename Symbol<TYPE>::type;
    const E *x = static_cast<const E *>(in);
    if (plan.pieces) {
        // at most 2048 workgroups: each adds its histogram to the state's once, the fewer the better
        if (plan.block >= WORKGROUP_PIECE) {
            const unsigned grid = (unsigned)(plan.pieces < 2048 ? plan.pieces : 2048);
            hipLaunchKernelGGL((monitor_reduce_kernel<TYPE, 256>), dim3(grid), dim3(256), 0, s, x, plan, parts, rows, st);
        } else {
            const size_t want = (plan.pieces + 63) / 64;               // sixteen pieces per wave where there are that many
            const unsigned grid = (unsigned)(want < 2048 ? want : 2048);
            hipLaunchKernelGGL((monitor_reduce_kernel<TYPE, 64>), dim3(grid), dim3(256), 0, s, x, plan, parts, rows, st);
        }
        XR_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(monitor_commit_kernel<TYPE>, dim3(1), dim3(64), 0, s, x, plan, parts, rows, st, summary);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace

int launch_monitor_push(const void *in, int type, const MonitorPlan &plan, xrit_monitor_block *parts, xrit_monitor_state *st,
                        xrit_monitor_block *rows, xrit_monitor_summary *summary, hipStream_t s)
{
    if (type == XRIT_SYMBOL_F32) return push_typed<XRIT_SYMBOL_F32>(in, plan, parts, st, rows, summary, s);
    return push_typed<XRIT_SYMBOL_I8>(in, plan, parts, st, rows, summary, s);
}

}  // namespace xrit
