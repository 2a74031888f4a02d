// demux.hip -- the channel demultiplexer and the packet accounting of newdecoder.cpp:309-395 (ChannelWriter::writeChannel
// and the Statistics_st of every frame) on one call's decoded frames, in three launches and without any wait between
// workgroups:
//  (a) count, one 1024-thread workgroup per tile of 1024 frames: per VCID the good frames' count and their first and
//      last counters; the tile's valid / dropped / Viterbi / RS sums.
//  (b) scan, one workgroup: per (tile, VCID) the scatter base and the counter in front of the tile (P: the last good
//      counter before it, or first - 1 when there is none, which makes the first frame of a channel lose nothing); the
//      tile scalars in frame order, the lost sum included; the per-call VCID bases; the handle's new state.
//  (c) scatter, four workgroups per tile (65 536 frames are only 64 tiles), each: the stable rank of every good frame
//      of the tile within its VCID (a 7-ballot peer mask per wave, wave counts in LDS), its predecessor's counter and
//      the workgroup prefix of the per-frame sums; then, for its quarter of the tile, the records and the VCDU copies
//      with dword loads (source stride 1020, destination stride 892).
// The lost count of a frame is c - pred - 1 (the reference's test only skips the cases where that is 0 or where there
// is no predecessor), so the per-channel sum telescopes: lostPerVC[v] after the K-th good frame of v in the call is
// lost_in[v] + c - P0[v] - K, and the call adds last - P0 - count.  Everything is integer; no atomics.
#include "kernels.h"
#include "wave_ops.h"

namespace xrit {

namespace {
constexpr int TILE = DEMUX_TILE;            // frames per tile = threads per workgroup
constexpr int WAVES = TILE / 64;
constexpr int DEMUX_PARTS = 4;              // scatter workgroups per tile (each ranks the whole tile, copies a quarter)

// lanes of this wave whose frame is good and on the same VCID (0 for a lane that is not good)
__device__ __forceinline__ unsigned long long vc_peers(bool good, unsigned v)
{
    unsigned long long m = __ballot(good);
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const unsigned long long x = __ballot((v >> b) & 1u);
        m &= ((v >> b) & 1u) ? x : ~x;
    }
    return good ? m : 0ull;
}

struct Frame {
    bool valid, good;
    unsigned vcid, counter, verr, rs;
};

__device__ __forceinline__ Frame load_frame(const xrit_frame_info *info, size_t f, unsigned nf)
{
    Frame q{false, false, 0u, 0u, 0u, 0u};
    if (f < nf) {
        const xrit_frame_info in = info[f];
        q.valid = in.valid != 0;
        q.good = q.valid && in.ok != 0;
        q.vcid = in.vcid & 63u;
        q.counter = in.counter & 0xFFFFFFu;
        q.verr = q.valid ? in.viterbi_errors : 0u;
        if (q.good)
            for (int k = 0; k < 4; ++k) q.rs += in.rs_errors[k] > 0 ? (unsigned)in.rs_errors[k] : 0u;
    }
    return q;
}

}  // namespace

// (a) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) demux_count_kernel(const xrit_frame_info *__restrict__ info, unsigned nf,
                                                           unsigned *__restrict__ cnt, int *__restrict__ firstc,
                                                           int *__restrict__ lastc, unsigned *__restrict__ tsum)
{
    __shared__ unsigned s_cnt[WAVES][NVC];
    __shared__ int s_first[WAVES][NVC], s_last[WAVES][NVC];
    __shared__ unsigned s_red[WAVES][4];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const size_t t = blockIdx.x;
    const Frame q = load_frame(info, t * TILE + tid, nf);
    const unsigned long long peers = vc_peers(q.good, q.vcid);
    s_cnt[w][lane] = 0u;
    __syncthreads();
    if (q.good) {
        const unsigned long long me = 1ull << lane;
        if ((peers & (me - 1)) == 0) s_first[w][q.vcid] = (int)q.counter;
        if ((peers & ~(me | (me - 1))) == 0) {
            s_last[w][q.vcid] = (int)q.counter;
            s_cnt[w][q.vcid] = (unsigned)__popcll(peers);
        }
    }
    const unsigned a = wave_sum((q.valid ? 1u : 0u) | (q.valid && !q.good ? 1u << 16 : 0u));
    const unsigned vit = wave_sum(q.verr), rs = wave_sum(q.rs);
    if (lane == 0) {
        s_red[w][0] = a & 0xFFFFu;
        s_red[w][1] = a >> 16;
        s_red[w][2] = vit;
        s_red[w][3] = rs;
    }
    __syncthreads();
    if (tid < NVC) {
        unsigned c = 0;
        int first = -1, last = -1;
        for (int i = 0; i < WAVES; ++i) {
            if (!s_cnt[i][tid]) continue;
            if (!c) first = s_first[i][tid];
            last = s_last[i][tid];
            c += s_cnt[i][tid];
        }
        cnt[t * NVC + tid] = c;
        firstc[t * NVC + tid] = first;
        lastc[t * NVC + tid] = last;
    } else if (tid < NVC + 4) {
        unsigned s = 0;
        for (int i = 0; i < WAVES; ++i) s += s_red[i][tid - NVC];
        tsum[t * 4 + (tid - NVC)] = s;
    }
}

// (b) ------------------------------------------------------------------------------------------------------------------
// state: DemuxState (kernels.h).  base / P: [T][64]; tin: [T][5] (frames, dropped, Viterbi, RS, lost) in front of each
// tile; vcb: [2][64] (lost_in - P0, max(received_in, 0)); offsets: [65].
__global__ void __launch_bounds__(1024) demux_scan_kernel(unsigned T, const unsigned *__restrict__ cnt,
                                                          const int *__restrict__ firstc, const int *__restrict__ lastc,
                                                          const unsigned *__restrict__ tsum, DemuxState *__restrict__ state,
                                                          unsigned *__restrict__ offsets, unsigned *__restrict__ base,
                                                          int *__restrict__ P, unsigned long long *__restrict__ tin,
                                                          long long *__restrict__ vcb)
{
    __shared__ unsigned s_tot[WAVES][NVC];
    __shared__ unsigned s_off[NVC];
    __shared__ unsigned s_c[WAVES][NVC];
    __shared__ int s_l[WAVES][NVC];
    __shared__ unsigned s_ccnt[NVC];
    __shared__ int s_clast[NVC];
    __shared__ long long s_p0[NVC];
    __shared__ unsigned long long s_ts[WAVES][5];
    const int tid = threadIdx.x, w = tid >> 6, v = tid & 63;

    // per-VCID totals of the call, for the offsets
    unsigned tot = 0;
    for (unsigned t = w; t < T; t += WAVES) tot += cnt[(size_t)t * NVC + v];
    s_tot[w][v] = tot;
    if (tid < NVC) {
        s_ccnt[v] = 0;
        s_clast[v] = (int)state->last[v];               // -1 or a 24-bit counter
        s_p0[v] = state->last[v];
    }
    __syncthreads();
    if (tid < NVC) {
        unsigned s = 0;
        for (int i = 0; i < WAVES; ++i) s += s_tot[i][v];
        s_tot[0][v] = s;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned s = 0;
        for (int i = 0; i < NVC; ++i) {
            s_off[i] = s;
            offsets[i] = s;
            s += s_tot[0][i];
        }
        offsets[NVC] = s;
    }
    __syncthreads();

    // the tiles, 16 at a time: wave w takes tile t0 + w, lane v its VCID
    // thread 0: the scalars in front of the tile, from the handle's counters on
    unsigned long long run[5] = {state->frames, state->dropped, state->sum_vit, state->sum_rs, state->lost_total};
    for (unsigned t0 = 0; t0 < T; t0 += WAVES) {
        const unsigned t = t0 + w;
        const bool in = t < T;
        const unsigned c = in ? cnt[(size_t)t * NVC + v] : 0u;
        const int fc = in ? firstc[(size_t)t * NVC + v] : -1, lc = in ? lastc[(size_t)t * NVC + v] : -1;
        s_c[w][v] = c;
        s_l[w][v] = lc;
        __syncthreads();
        unsigned pre = s_ccnt[v];
        int lastbefore = s_clast[v];
        for (int i = 0; i < w; ++i)
            if (s_c[i][v]) { pre += s_c[i][v]; lastbefore = s_l[i][v]; }
        const int p = lastbefore > -1 ? lastbefore : fc - 1;
        long long lost = 0;
        if (in) {
            base[(size_t)t * NVC + v] = s_off[v] + pre;
            P[(size_t)t * NVC + v] = p;
            if (c) {
                lost = (long long)lc - p - (long long)c;
                if (lastbefore == -1) s_p0[v] = p;        // the call's first good frame of a channel never seen before
            }
        }
        lost = wave_sum(lost);
        if (v == 0 && in) {
            s_ts[w][0] = tsum[(size_t)t * 4 + 0];
            s_ts[w][1] = tsum[(size_t)t * 4 + 1];
            s_ts[w][2] = tsum[(size_t)t * 4 + 2];
            s_ts[w][3] = tsum[(size_t)t * 4 + 3];
            s_ts[w][4] = (unsigned long long)lost;
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < WAVES && t0 + i < T; ++i)
                for (int k = 0; k < 5; ++k) {
                    tin[(size_t)(t0 + i) * 5 + k] = run[k];
                    run[k] += s_ts[i][k];
                }
        } else if (tid >= 64 && tid < 128) {
            for (int i = 0; i < WAVES; ++i)
                if (s_c[i][v]) { s_ccnt[v] += s_c[i][v]; s_clast[v] = s_l[i][v]; }
        }
        __syncthreads();
    }

    // the handle's new state (the old one is read above and by nothing after this kernel)
    if (tid < NVC) {
        const long long recv_in = state->received[v], lost_in = state->lost[v];
        const unsigned n = s_ccnt[v];
        vcb[v] = lost_in - s_p0[v];
        vcb[NVC + v] = recv_in < 0 ? 0 : recv_in;
        if (n) {
            state->last[v] = s_clast[v];
            state->received[v] = (recv_in < 0 ? 0 : recv_in) + n;
            state->lost[v] = lost_in + ((long long)s_clast[v] - s_p0[v] - (long long)n);
        }
    }
    if (tid == 0) {
        state->frames = run[0];
        state->dropped = run[1];
        state->sum_vit = run[2];
        state->sum_rs = run[3];
        state->lost_total = run[4];
    }
}

// (c) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) demux_scatter_kernel(const xrit_sync_hit *__restrict__ hits, const unsigned char *__restrict__ cadu,
                                                             size_t cadu_stride, const unsigned char *__restrict__ block,
                                                             const xrit_frame_info *__restrict__ info, unsigned nf,
                                                             const unsigned *__restrict__ offsets, const unsigned *__restrict__ base,
                                                             const int *__restrict__ P, const unsigned long long *__restrict__ tin,
                                                             const long long *__restrict__ vcb, unsigned char *__restrict__ vcdu,
                                                             xrit_frame_stats *__restrict__ records)
{
    __shared__ unsigned s_cnt[WAVES][NVC];
    __shared__ int s_last[WAVES][NVC];
    __shared__ unsigned s_w32[WAVES][3];
    __shared__ long long s_w64[WAVES];
    __shared__ unsigned s_row[TILE];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const size_t t = blockIdx.x, f = t * TILE + tid;
    const Frame q = load_frame(info, f, nf);
    const unsigned long long peers = vc_peers(q.good, q.vcid);
    const unsigned long long me = 1ull << lane, lt = peers & (me - 1);
    s_cnt[w][lane] = 0u;
    __syncthreads();
    if (q.good && (peers & ~(me | (me - 1))) == 0) {
        s_cnt[w][q.vcid] = (unsigned)__popcll(peers);
        s_last[w][q.vcid] = (int)q.counter;
    }
    // the predecessor inside the wave: the highest peer below this lane
    const int src = lt ? 63 - __clzll((long long)lt) : lane;
    const int pred_wave = __shfl((int)q.counter, src, 64);
    __syncthreads();
    unsigned pre = 0;
    int pred = 0;
    if (q.good) {
        int lastw = -2;
        for (int i = 0; i < w; ++i)
            if (s_cnt[i][q.vcid]) { pre += s_cnt[i][q.vcid]; lastw = s_last[i][q.vcid]; }
        pred = lt ? pred_wave : (lastw != -2 ? lastw : P[t * NVC + q.vcid]);
    }
    const unsigned rank = pre + (unsigned)__popcll(lt);
    const unsigned row = q.good ? base[t * NVC + q.vcid] + rank : 0xFFFFFFFFu;
    s_row[tid] = row;
    const long long lost = q.good ? (long long)(int)(q.counter - (unsigned)pred - 1u) : 0ll;

    // workgroup inclusive prefix of the per-frame sums.  Written out, not four calls of wave_ops.h's block_incl_scan: with a
    // barrier per quantity and the totals it has no use for, the stage's call measured 0.0644 ms against 0.0617 ms
    unsigned a = wave_incl_scan((q.valid ? 1u : 0u) | (q.valid && !q.good ? 1u << 16 : 0u), lane);
    unsigned vit = wave_incl_scan(q.verr, lane), rs = wave_incl_scan(q.rs, lane);
    long long ls = wave_incl_scan(lost, lane);
    if (lane == 63) {
        s_w32[w][0] = a;
        s_w32[w][1] = vit;
        s_w32[w][2] = rs;
        s_w64[w] = ls;
    }
    __syncthreads();
    for (int i = 0; i < w; ++i) {
        a += s_w32[i][0];
        vit += s_w32[i][1];
        rs += s_w32[i][2];
        ls += s_w64[i];
    }

    const unsigned part = blockIdx.y;                   // DEMUX_PARTS workgroups per tile: each writes a quarter
    if (f < nf && (unsigned)tid / (TILE / DEMUX_PARTS) == part) {
        xrit_frame_stats r{};
        if (q.valid) {
            const xrit_frame_info in = info[f];
            const xrit_sync_hit h = hits[f];
            const unsigned long long *ti = tin + t * 5;
            const unsigned long long frames = ti[0] + (a & 0xFFFFu), dropped = ti[1] + (a >> 16);
            const unsigned long long svit = ti[2] + vit, srs = ti[3] + rs;
            r.total_packets = frames;
            r.dropped_packets = dropped;
            r.lost_packets = ti[4] + (unsigned long long)ls;
            r.average_vit_corrections = (uint16_t)(svit / frames);
            r.average_rs_corrections = (uint8_t)(srs / frames);
            for (int k = 0; k < 4; ++k) r.rs_errors[k] = in.rs_errors[k];
            r.vit_errors = (uint16_t)in.viterbi_errors;
            r.frame_bits = 8192;
            r.sync_correlation = (uint8_t)h.correlation;
            const unsigned char *cw = cadu + f * cadu_stride;
            for (int k = 0; k < 4; ++k) r.sync_word[k] = cw[k];
            r.valid = 1;
            if (q.good) {
                // GetPercentBER() = 100 * BER / 8256 (unverified); newdecoder.cpp:289-291
                const float pber = 100.0f * (float)in.viterbi_errors / 8256.0f;
                const float se = 100.0f - pber * 10.0f;
                const unsigned long long K = (unsigned long long)(row - offsets[q.vcid]) + 1ull;
                r.scid = (uint8_t)in.scid;
                r.vcid = (uint8_t)q.vcid;
                r.packet_number = q.counter;
                r.signal_quality = (uint8_t)(se < 0.0f ? 0.0f : se);
                r.phase_correction = h.word ? 180 : 0;
                r.received_vc = vcb[NVC + q.vcid] + (long long)K;
                r.lost_vc = vcb[q.vcid] + (long long)q.counter - (long long)K;
                r.frame_lock = 1;
            }
        }
        records[f] = r;
    }
    __syncthreads();

    // this part's frames' VCDUs, 223 dwords each, as one flat index space over the workgroup, 8 loads in flight per lane
    constexpr unsigned DW = 223, SRC = 255, PF = TILE / DEMUX_PARTS, N = PF * DW;
    const unsigned *src32 = reinterpret_cast<const unsigned *>(block) + (t * TILE + (size_t)part * PF) * SRC;
    unsigned *dst32 = reinterpret_cast<unsigned *>(vcdu);
    for (unsigned i0 = 0; i0 < N; i0 += TILE * 8) {
        unsigned x[8], dr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const unsigned i = i0 + (unsigned)u * TILE + (unsigned)tid;
            const unsigned j = i / DW, d = i - j * DW;
            dr[u] = 0xFFFFFFFFu;
            if (i < N) {
                const unsigned r = s_row[part * PF + j];
                if (r < nf) {                        // good frames only (the rest hold ~0); rows < offsets[64] <= nf
                    x[u] = src32[(size_t)j * SRC + d];
                    dr[u] = r * DW + d;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (dr[u] != 0xFFFFFFFFu) dst32[dr[u]] = x[u];
    }
}

// T tiles: what (a) leaves for (b), then what (b) leaves for (c)
size_t demux_scratch_carve(void *base, size_t nf, DemuxScratch &sc)
{
    const size_t T = div_up(nf, TILE);
    Carver c{static_cast<char *>(base)};
    sc.cnt = c.take<unsigned>(T * NVC, 8);
    sc.firstc = c.take<int>(T * NVC, 8);
    sc.lastc = c.take<int>(T * NVC, 8);
    sc.base = c.take<unsigned>(T * NVC, 8);
    sc.P = c.take<int>(T * NVC, 8);
    sc.tsum = c.take<unsigned>(T * 4, 8);
    sc.tin = c.take<unsigned long long>(T * 5, 8);
    sc.vcb = c.take<long long>(2 * NVC, 8);
    return c.used();
}

int launch_demux(const xrit_sync_hit *hits, const unsigned char *cadu, size_t cadu_stride, const unsigned char *block,
                 const xrit_frame_info *info, size_t nf, DemuxState *state, DemuxScratch &sc, unsigned char *vcdu,
                 unsigned *offsets, xrit_frame_stats *records, hipStream_t s)
{
    if (nf == 0) return XRIT_OK;
    const unsigned T = div_up(nf, TILE);
    hipLaunchKernelGGL(demux_count_kernel, dim3(T), dim3(TILE), 0, s, info, (unsigned)nf, sc.cnt, sc.firstc, sc.lastc, sc.tsum);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(demux_scan_kernel, dim3(1), dim3(1024), 0, s, T, sc.cnt, sc.firstc, sc.lastc, sc.tsum, state, offsets,
                       sc.base, sc.P, sc.tin, sc.vcb);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(demux_scatter_kernel, dim3(T, DEMUX_PARTS), dim3(TILE), 0, s, hits, cadu, cadu_stride, block, info, (unsigned)nf,
                       offsets, sc.base, sc.P, sc.tin, sc.vcb, vcdu, records);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
