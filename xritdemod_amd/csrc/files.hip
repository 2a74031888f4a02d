// files.hip -- LRIT/HRIT files out of the packet assembler's space packets.
// The serial rule (tests/file_spec.py) is serial in the packets of one (vcid, apid) key and independent between keys:
//  (a) sort, one workgroup per VCID: the channel's packet indices stably ordered by APID -- a counting sort over 2048
//      bins in LDS, 512 packets per step: equal APIDs inside a wave are matched with eleven ballots (rank = popcount of
//      the match mask below the lane), the waves' group sizes meet in LDS; a first pass counts, a scan of the bins gives
//      every key's run, a second pass places.  No atomics.
//  (b) count, one lane per key (64 x 2048 of them, most with nothing to do): the serial rule along the key's run without
//      writing anything: the pieces, bytes and records it emits and its counter increments.
//  (c) scan, two levels over the keys: per tile of 2048 keys the exclusive prefix of pieces, bytes and records inside the
//      tile and the tile's sums; then one wave over the 64 tiles: every tile's base, the call's counts, the overflow
//      flag; the handle's counters and the summary.
//  (d) write, one lane per key: the rule once more from the same state, now with the key's bases: piece descriptors,
//      records, where every payload lies and goes, and the key's new state.
//  (e) gather, workgroups of four waves striding over groups of eight pieces: the payloads, 8 byte loads per lane in flight.
// Everything is integer; every launch is sized from the host's bound on the packet count and reads the count itself from
// pkt_offsets[64] on the device.
#include "kernels.h"
#include "wave_ops.h"

namespace xrit {

namespace {
constexpr unsigned NAP = 2048;
constexpr unsigned SORT_WAVES = 8, SORT_THREADS = 64 * SORT_WAVES;
constexpr unsigned NCNT = 7;            // begun, completed, aborted, bad, gaps, short, orphans
constexpr unsigned GPIECES = 8;

// channel v's packets [s, e): the offsets, none beyond the count, never decreasing
__device__ __forceinline__ void vc_range(const unsigned *off, unsigned v, unsigned &s, unsigned &e)
{
    const unsigned n = off[NVC], a = off[v], b = off[v + 1];
    s = a < n ? a : n;
    e = b < n ? b : n;
    if (e < s) e = s;
}

__device__ __forceinline__ unsigned be16(const unsigned char *p) { return (unsigned)p[0] << 8 | p[1]; }
__device__ __forceinline__ unsigned be32(const unsigned char *p) { return be16(p) << 16 | be16(p + 2); }
__device__ __forceinline__ unsigned long long be64(const unsigned char *p) { return (unsigned long long)be32(p) << 32 | be32(p + 4); }

// the header fields of a file from its first piece's payload (fields found before the walk stops are kept)
__device__ void parse_header(xrit_file_key &k, const unsigned char *p, unsigned n)
{
    k.data_bits = 0;
    k.header_length = 0;
    k.columns = k.lines = k.rice_flags = 0;
    k.file_type = k.header_state = k.bits_per_pixel = k.compression = k.pixels_per_block = k.lines_per_packet = 0;
    if (!(n >= 16 && p[0] == 0 && be16(p + 1) == 16)) return;
    k.file_type = p[3];
    const unsigned H = be32(p + 4);
    k.header_length = H;
    k.data_bits = be64(p + 8);
    k.header_state = 1;
    if (H > n) return;
    unsigned q = 16;
    bool image = false, rice = false;
    while (q + 3 <= H) {
        const unsigned t = p[q], l = be16(p + q + 1);
        if (l < 3 || q + l > H) return;
        if (t == 1 && l == 9 && !image) {
            image = true;
            k.bits_per_pixel = p[q + 3];
            k.columns = (uint16_t)be16(p + q + 4);
            k.lines = (uint16_t)be16(p + q + 6);
            k.compression = p[q + 8];
        }
        if (t == 131 && l == 7 && !rice) {
            rice = true;
            k.rice_flags = (uint16_t)be16(p + q + 3);
            k.pixels_per_block = p[q + 5];
            k.lines_per_packet = p[q + 6];
        }
        q += l;
    }
    if (q == H) k.header_state = 2;
}
}  // namespace

// (a) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SORT_THREADS) files_sort_kernel(const xrit_packet *__restrict__ packets, const unsigned *__restrict__ offsets,
                                                                  unsigned max_in, unsigned *__restrict__ order,
                                                                  unsigned *__restrict__ kstart, unsigned *__restrict__ kcount)
{
    __shared__ unsigned short s_w[SORT_WAVES][NAP];     // a wave's group sizes of the step (zero between steps)
    __shared__ unsigned s_run[NAP], s_start[NAP];       // packets of the bin so far; the bin's first place
    __shared__ unsigned s_ws[SORT_WAVES];
    const unsigned tid = threadIdx.x, w = tid >> 6, lane = tid & 63, v = blockIdx.x;
    if (offsets[NVC] > max_in) return;
    unsigned s, e;
    vc_range(offsets, v, s, e);
    for (unsigned a = tid; a < NAP; a += SORT_THREADS) {
        s_run[a] = 0;
#pragma unroll
        for (unsigned u = 0; u < SORT_WAVES; ++u) s_w[u][a] = 0;
    }
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        for (unsigned base = s; base < e; base += SORT_THREADS) {
            const unsigned i = base + tid;
            const bool valid = i < e;
            const unsigned a = valid ? (packets[i].apid & (NAP - 1u)) : 0u;
            unsigned long long mask = __ballot(valid);
#pragma unroll
            for (int bit = 0; bit < 11; ++bit) {
                const bool one = (a >> bit) & 1u;
                const unsigned long long b = __ballot(one);
                mask &= one ? b : ~b;
            }
            const unsigned rank = __popcll(mask & ((1ull << lane) - 1ull)), cnt = __popcll(mask);
            const bool leader = valid && rank == 0;
            if (leader) s_w[w][a] = (unsigned short)cnt;
            __syncthreads();
            unsigned before = 0, total = 0, runbase = 0;
            if (valid) {
#pragma unroll
                for (unsigned u = 0; u < SORT_WAVES; ++u) {
                    const unsigned c = s_w[u][a];
                    total += c;
                    if (u < w) before += c;
                }
                runbase = s_run[a];
            }
            __syncthreads();
            if (leader) {
                s_w[w][a] = 0;
                if (before == 0) s_run[a] = runbase + total;        // the first wave that holds this APID
            }
            if (pass == 1 && valid) order[s + s_start[a] + runbase + before + rank] = i;
        }
        __syncthreads();
        if (pass == 0) {
            // the bins' exclusive prefix: four bins per thread, a wave scan, the waves' sums through LDS
            unsigned c[4], sum = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                c[u] = s_run[4 * tid + u];
                sum += c[u];
            }
            unsigned all;
            unsigned pre = block_incl_scan<SORT_WAVES>(sum, lane, w, s_ws, all) - sum;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned a = 4 * tid + u;
                s_start[a] = pre;
                kstart[v * NAP + a] = s + pre;
                kcount[v * NAP + a] = c[u];
                pre += c[u];
                s_run[a] = 0;
            }
            __syncthreads();
        }
    }
}

// (b), (d) -------------------------------------------------------------------------------------------------------------
template <bool WRITE>
__global__ void __launch_bounds__(256) files_walk_kernel(const unsigned char *__restrict__ in_bytes, unsigned long long n_in_bytes,
                                                         const xrit_packet *__restrict__ packets, const unsigned *__restrict__ offsets,
                                                         unsigned max_in, const unsigned *__restrict__ order,
                                                         const unsigned *__restrict__ kstart, const unsigned *__restrict__ kcount,
                                                         xrit_file_key *__restrict__ keys, unsigned *__restrict__ kpieces,
                                                         unsigned *__restrict__ krecs, unsigned long long *__restrict__ kbytes,
                                                         unsigned *__restrict__ kcnt, const unsigned long long *__restrict__ tbase,
                                                         unsigned long long *__restrict__ psrc, unsigned long long *__restrict__ pdst, unsigned *__restrict__ plen,
                                                         xrit_file_piece *__restrict__ pieces, unsigned long long max_pieces,
                                                         xrit_file_record *__restrict__ files, unsigned long long max_files)
{
    const unsigned key = blockIdx.x * 256u + threadIdx.x;
    if (offsets[NVC] > max_in) return;
    const unsigned cnt = kcount[key], first = kstart[key];
    unsigned np = 0, nr = 0;
    unsigned long long nb = 0;
    unsigned c_begun = 0, c_done = 0, c_abort = 0, c_bad = 0, c_gap = 0, c_short = 0, c_orph = 0;
    if (cnt != 0) {
        if (WRITE) {
            const unsigned long long *tb = tbase + (size_t)(key / FILES_TILE) * 3;     // the key's tile, then the key inside it
            np = (unsigned)tb[0] + kpieces[key];
            nr = (unsigned)tb[1] + krecs[key];
            nb = tb[2] + kbytes[key];
        }
        xrit_file_key k = keys[key];
        const unsigned vcid = key / NAP, apid = key % NAP;
        // the record of the file the key is in, while it has one in this call
        bool have = false;
        unsigned r_idx = 0, r_first = 0, r_np = 0, r_flags = 0;
        unsigned long long r_off = 0, r_len = 0, r_foff = 0;
        auto open_rec = [&](unsigned flags) {
            have = true;
            r_idx = nr++;
            r_first = np;
            r_np = 0;
            r_flags = flags;
            r_off = nb;
            r_len = 0;
            r_foff = k.file_bytes;
        };
        auto close_rec = [&]() {
            if (WRITE && r_idx < max_files) {
                xrit_file_record o{};
                o.offset = r_off;
                o.length = r_len;
                o.file_offset = r_foff;
                o.declared_bits = k.declared_bits;
                o.data_bits = k.data_bits;
                o.header_length = k.header_length;
                o.first_piece = r_first;
                o.n_pieces = r_np;
                o.key_serial = k.key_serial - 1u;
                o.file_counter = k.file_counter;
                o.apid = (uint16_t)apid;
                o.columns = k.columns;
                o.lines = k.lines;
                o.rice_flags = k.rice_flags;
                o.vcid = (uint8_t)vcid;
                o.flags = (uint8_t)r_flags;
                o.file_type = k.file_type;
                o.header_state = k.header_state;
                o.bits_per_pixel = k.bits_per_pixel;
                o.compression = k.compression;
                o.pixels_per_block = k.pixels_per_block;
                o.lines_per_packet = k.lines_per_packet;
                files[r_idx] = o;
            }
            have = false;
        };
        auto abort_file = [&]() {
            if (!have) open_rec(0);
            r_flags |= XRIT_FILE_ABORTED;
            close_rec();
            k.open = 0;
            ++c_abort;
        };
        for (unsigned j = 0; j < cnt; ++j) {
            const xrit_packet d = packets[order[first + j]];
            const unsigned long long off = d.offset;
            const unsigned len = d.length;
            if (d.crc_ok == 0 || len < 8 || off > n_in_bytes || len > n_in_bytes - off) {
                ++c_bad;
                if (k.open) abort_file();
                continue;
            }
            const unsigned seq = d.seq_count, fl = d.seq_flags & 3u;
            if (k.open && seq != k.next_seq) {
                ++c_gap;
                abort_file();
            }
            unsigned long long pay = off + 6;
            unsigned pay_len = len - 8;
            if (fl == 1 || fl == 3) {
                if (k.open) abort_file();
                if (pay_len < 10) {
                    ++c_short;
                    continue;
                }
                const unsigned char *u = in_bytes + pay;
                k.file_counter = (uint16_t)be16(u);
                k.declared_bits = be64(u + 2);
                k.file_bytes = 0;
                k.n_pieces = 0;
                ++k.key_serial;
                ++c_begun;
                pay += 10;
                pay_len -= 10;
                parse_header(k, in_bytes + pay, pay_len);
                open_rec(XRIT_FILE_BEGINS);
                k.open = 1;
            } else {
                if (!k.open) {
                    ++c_orph;
                    continue;
                }
                if (!have) open_rec(0);
            }
            if (WRITE) {
                psrc[np] = pay;                         // (np < the call's packets <= max_in)
                pdst[np] = nb;
                plen[np] = pay_len;
                if (np < max_pieces) {
                    xrit_file_piece o{};
                    o.offset = nb;
                    o.length = pay_len;
                    o.index_in_file = k.n_pieces;
                    o.file = r_idx;
                    o.seq_count = (uint16_t)seq;
                    o.apid = (uint16_t)apid;
                    o.vcid = (uint8_t)vcid;
                    o.seq_flags = (uint8_t)fl;
                    pieces[np] = o;
                }
            }
            ++np;
            nb += pay_len;
            r_len += pay_len;
            ++r_np;
            k.file_bytes += pay_len;
            ++k.n_pieces;
            k.next_seq = (uint16_t)((seq + 1u) & 0x3FFFu);
            if (fl >= 2) {
                r_flags |= XRIT_FILE_ENDS;
                if (8ull * k.file_bytes == k.declared_bits) r_flags |= XRIT_FILE_LENGTH_MATCH;
                close_rec();
                k.open = 0;
                ++c_done;
            }
        }
        if (have) close_rec();
        if (WRITE) keys[key] = k;
    }
    if (!WRITE) {
        kpieces[key] = np;
        krecs[key] = nr;
        kbytes[key] = nb;
        unsigned *c = kcnt + (size_t)key * NCNT;
        c[0] = c_begun; c[1] = c_done; c[2] = c_abort; c[3] = c_bad; c[4] = c_gap; c[5] = c_short; c[6] = c_orph;
    }
}

// (c) ------------------------------------------------------------------------------------------------------------------
// c1, one workgroup per tile of 2048 keys (a channel's): pieces, records and bytes per key -> their exclusive prefix inside
// the tile (in place), the tile's sums and its counter increments
__global__ void __launch_bounds__(1024) files_tile_kernel(const unsigned *__restrict__ offsets, unsigned max_in,
                                                          unsigned *__restrict__ kpieces, unsigned *__restrict__ krecs,
                                                          unsigned long long *__restrict__ kbytes, const unsigned *__restrict__ kcnt,
                                                          unsigned long long *__restrict__ tsum)
{
    __shared__ unsigned s_p[16], s_r[16];
    __shared__ unsigned long long s_b[16];
    __shared__ unsigned s_c[16][NCNT];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if (offsets[NVC] > max_in) return;
    // wave w: keys [128 w, 128 (w + 1)) of the tile in two coalesced rows of 64; the prefix wanted is in key order
    constexpr unsigned ROWS = FILES_TILE / 16 / 64;
    const unsigned k0 = blockIdx.x * FILES_TILE + (unsigned)w * ROWS * 64u;
    // (a call holds at most 2^24 packets: the counts fit 32 bits, the bytes do not)
    unsigned ep[ROWS], er[ROWS];                        // exclusive inside the wave
    unsigned long long eb[ROWS];
    unsigned cp = 0, cr = 0;                            // the rows in front, inside the wave
    unsigned long long cb = 0;
#pragma unroll
    for (unsigned q = 0; q < ROWS; ++q) {
        const unsigned key = k0 + q * 64u + lane;
        ep[q] = wave_excl_scan_step(kpieces[key], lane, cp);
        er[q] = wave_excl_scan_step(krecs[key], lane, cr);
        eb[q] = wave_excl_scan_step(kbytes[key], lane, cb);
    }
    // the counter increments: the wave's 128 x 7 words are contiguous; word j belongs to counter j mod 7
    {
        unsigned tc[NCNT] = {0, 0, 0, 0, 0, 0, 0};
#pragma nounroll
        for (unsigned q = 0; q < ROWS * NCNT; ++q) {
            const unsigned j = q * 64u + lane, x = kcnt[(size_t)k0 * NCNT + j], m = j % NCNT;
#pragma unroll
            for (unsigned u = 0; u < NCNT; ++u) tc[u] += m == u ? x : 0u;
        }
#pragma unroll
        for (unsigned u = 0; u < NCNT; ++u) {
            const unsigned t = wave_sum(tc[u]);
            if (lane == 0) s_c[w][u] = t;
        }
    }
    unsigned ap, ar;
    unsigned long long ab;
    const unsigned bp = block_parts_before<16>(cp, lane, w, s_p, ap), br = block_parts_before<16>(cr, lane, w, s_r, ar);
    const unsigned long long bb = block_parts_before<16>(cb, lane, w, s_b, ab);
#pragma unroll
    for (unsigned q = 0; q < ROWS; ++q) {
        const unsigned key = k0 + q * 64u + lane;
        kpieces[key] = bp + ep[q];
        krecs[key] = br + er[q];
        kbytes[key] = bb + eb[q];
    }
    unsigned long long *ts = tsum + (size_t)blockIdx.x * FILES_TSUM;
    if (tid == 0) {
        ts[0] = ap;
        ts[1] = ar;
        ts[2] = ab;
    }
    if (tid < (int)NCNT) {
        unsigned long long t = 0;
        for (int i = 0; i < 16; ++i) t += s_c[i][tid];
        ts[3 + tid] = t;
    }
}

// c2, one wave, lane t on tile t: every tile's first piece index, record index and byte offset, the call's counts, the
// overflow flag; the handle's counters and the summary
__global__ void __launch_bounds__(64) files_total_kernel(const unsigned *__restrict__ offsets, unsigned max_in,
                                                         const unsigned long long *__restrict__ tsum, unsigned long long *__restrict__ tbase,
                                                         xrit_files_counters *__restrict__ counters, xrit_files_summary *__restrict__ sum,
                                                         unsigned long long max_pieces, unsigned long long max_bytes,
                                                         unsigned long long max_files)
{
    static_assert(FILES_KEYS / FILES_TILE == 64, "one lane per tile");
    const int lane = threadIdx.x;
    const bool run = offsets[NVC] <= max_in;
    unsigned long long v[FILES_TSUM], all[3] = {0, 0, 0};
#pragma unroll
    for (unsigned u = 0; u < FILES_TSUM; ++u) v[u] = run ? tsum[(size_t)lane * FILES_TSUM + u] : 0ull;
#pragma unroll
    for (unsigned u = 0; u < 3; ++u) {
        const unsigned long long before = wave_excl_scan_step(v[u], lane, all[u]);
        if (run) tbase[(size_t)lane * 3 + u] = before;
    }
    const unsigned long long ap = all[0], ar = all[1], ab = all[2];
    unsigned long long c[NCNT];
#pragma unroll
    for (unsigned u = 0; u < NCNT; ++u) c[u] = wave_sum(v[3 + u]);
    if (lane == 0) {
        xrit_files_counters t = *counters;
        t.files_begun += c[0];
        t.files_completed += c[1];
        t.files_aborted += c[2];
        t.bad_packets += c[3];
        t.seq_gaps += c[4];
        t.short_first += c[5];
        t.orphans += c[6];
        t.total_pieces += ap;
        t.total_bytes += ab;
        t.open_files += c[0] - c[1] - c[2];
        *counters = t;
        xrit_files_summary o{};
        o.pieces = ap;
        o.bytes = ab;
        o.files = ar;
        o.files_begun = t.files_begun;
        o.files_completed = t.files_completed;
        o.files_aborted = t.files_aborted;
        o.bad_packets = t.bad_packets;
        o.seq_gaps = t.seq_gaps;
        o.short_first = t.short_first;
        o.orphans = t.orphans;
        o.total_pieces = t.total_pieces;
        o.total_bytes = t.total_bytes;
        o.overflow = !run ? 2u : ((ap > max_pieces || ab > max_bytes || ar > max_files) ? 1u : 0u);
        *sum = o;
    }
}

// (e) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) files_gather_kernel(const unsigned char *__restrict__ in_bytes, const unsigned *__restrict__ offsets,
                                                           unsigned max_in, const xrit_files_summary *__restrict__ sum,
                                                           const unsigned long long *__restrict__ psrc,
                                                           const unsigned long long *__restrict__ pdst, const unsigned *__restrict__ plen,
                                                           unsigned char *__restrict__ bytes, unsigned long long max_bytes)
{
    if (offsets[NVC] > max_in) return;
    const unsigned long long n = sum->pieces;
    const unsigned tid = threadIdx.x;
    for (unsigned long long g = blockIdx.x; g * GPIECES < n; g += gridDim.x)
    for (unsigned long long p = g * GPIECES; p < (g + 1) * GPIECES && p < n; ++p) {
        const unsigned len = plen[p];
        const unsigned long long dst = pdst[p];
        if (dst + len > max_bytes) continue;
        const unsigned char *src = in_bytes + psrc[p];
        unsigned char *out = bytes + dst;
        for (unsigned base = 0; base < len; base += 256u * 8u) {
            unsigned x[8];
#pragma unroll
            for (unsigned u = 0; u < 8; ++u) {
                const unsigned k = base + tid + 256u * u;
                x[u] = k < len ? src[k] : 0u;
            }
#pragma unroll
            for (unsigned u = 0; u < 8; ++u) {
                const unsigned k = base + tid + 256u * u;
                if (k < len) out[k] = (unsigned char)x[u];
            }
        }
    }
}

size_t files_scratch_carve(void *base, size_t max_in, FilesScratch &sc)
{
    const size_t N = max_in ? max_in : 1;
    Carver c{static_cast<char *>(base)};
    sc.psrc = c.take<unsigned long long>(N, 16);
    sc.pdst = c.take<unsigned long long>(N, 16);
    sc.kbytes = c.take<unsigned long long>(FILES_KEYS, 16);
    sc.tsum = c.take<unsigned long long>(64 * FILES_TSUM, 16);
    sc.tbase = c.take<unsigned long long>(64 * 3, 16);
    sc.order = c.take<unsigned>(N, 16);
    sc.plen = c.take<unsigned>(N, 16);
    sc.kstart = c.take<unsigned>(FILES_KEYS, 16);
    sc.kcount = c.take<unsigned>(FILES_KEYS, 16);
    sc.kpieces = c.take<unsigned>(FILES_KEYS, 16);
    sc.krecs = c.take<unsigned>(FILES_KEYS, 16);
    sc.kcnt = c.take<unsigned>((size_t)FILES_KEYS * NCNT, 16);
    return c.used();
}

int launch_files(const unsigned char *in_bytes, size_t n_in_bytes, const xrit_packet *packets, const unsigned *pkt_offsets,
                 size_t max_in, xrit_file_key *keys, xrit_files_counters *counters, FilesScratch &sc, unsigned char *bytes,
                 size_t max_bytes, xrit_file_piece *pieces, size_t max_pieces, xrit_file_record *files, size_t max_files,
                 xrit_files_summary *summary, hipStream_t s)
{
    const unsigned bound = (unsigned)max_in;
    hipLaunchKernelGGL(files_sort_kernel, dim3(NVC), dim3(SORT_THREADS), 0, s, packets, pkt_offsets, bound, sc.order, sc.kstart, sc.kcount);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(files_walk_kernel<false>, dim3(FILES_KEYS / 256), dim3(256), 0, s, in_bytes, (unsigned long long)n_in_bytes, packets,
                       pkt_offsets, bound, sc.order, sc.kstart, sc.kcount, keys, sc.kpieces, sc.krecs, sc.kbytes, sc.kcnt, sc.tbase, sc.psrc, sc.pdst,
                       sc.plen, pieces, (unsigned long long)max_pieces, files, (unsigned long long)max_files);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(files_tile_kernel, dim3(FILES_KEYS / FILES_TILE), dim3(1024), 0, s, pkt_offsets, bound, sc.kpieces, sc.krecs, sc.kbytes,
                       sc.kcnt, sc.tsum);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(files_total_kernel, dim3(1), dim3(64), 0, s, pkt_offsets, bound, sc.tsum, sc.tbase, counters, summary,
                       (unsigned long long)max_pieces, (unsigned long long)max_bytes, (unsigned long long)max_files);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(files_walk_kernel<true>, dim3(FILES_KEYS / 256), dim3(256), 0, s, in_bytes, (unsigned long long)n_in_bytes, packets,
                       pkt_offsets, bound, sc.order, sc.kstart, sc.kcount, keys, sc.kpieces, sc.krecs, sc.kbytes, sc.kcnt, sc.tbase, sc.psrc, sc.pdst,
                       sc.plen, pieces, (unsigned long long)max_pieces, files, (unsigned long long)max_files);
    XR_HIP(hipGetLastError());
    // (the piece count is on the device: a grid no larger than fills the chip a few times over, striding over the groups)
    const unsigned groups = div_up(max_in ? max_in : 1, GPIECES);
    hipLaunchKernelGGL(files_gather_kernel, dim3(groups < 4096u ? groups : 4096u), dim3(256), 0, s, in_bytes, pkt_offsets, bound, summary,
                       sc.psrc, sc.pdst, sc.plen, bytes, (unsigned long long)max_bytes);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
