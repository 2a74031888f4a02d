// packets.hip -- CCSDS space packets out of the demultiplexer's VCDU rows, with CRC-16.
// The serial rule (tests/packet_spec.py) carries one thing from row to row of a channel: the bytes of a packet that has
// begun and not ended.  They are born in exactly one place -- the tail of one row's packet zone, or the handle's state in
// front of the call's first row of a channel -- and a row whose first header pointer is not 2047 ends them whatever they
// were, so every row can be walked on its own and every tail followed on its own:
//  (a) walk, one lane per row (and one per channel for the pending state): from the first header pointer along the
//      headers, the packets that lie wholly inside the zone (fill packets counted apart) and the tail's start; then the
//      tail through the rows behind it (consecutive counters, pointer 2047 until the length is reached, at most 75 rows):
//      it ends as a packet in a later row (noted THERE), is discarded, or is what the channel holds after the call.
//  (b) scan, two levels: per tile of 1024 rows the exclusive prefix of packets and bytes inside the tile; then one
//      workgroup over the tiles' sums: every tile's first descriptor index and byte offset, the per-channel packet
//      offsets, the call's counts and the overflow flag.
//  (c) gather + CRC, one workgroup of four waves per eight rows: a row's packets one after the other, in chunks
//      of 4096 bytes that end where the packet's CRC begins: 16 coalesced byte loads per lane in flight, stored to the
//      output and to LDS.  The CRC register is linear over GF(2), so every lane runs the 16 bytes of its slice of the
//      chunk from a zero register (table in LDS; the header counts as zeros, and zeros in front of the data change
//      nothing from a zero register; the initial 0xFFFF is an XOR on the first two data bytes) and slices, waves and
//      chunks combine as crc(A | B) = crc(A) x^(8 |B|) + crc(B) mod 0x11021, the factors table entries x^(8 2^k).
//  (d) finish, one workgroup per channel: the channel's counters, its new pending bytes and last counter.
//  (e) summary, one wave: the handle's counters over all channels.
// Everything is integer; no atomics; every launch is sized from the host's bound on the row count and reads the count
// itself from offsets[64] on the device.
#include "kernels.h"
#include "wave_ops.h"

namespace xrit {

namespace {
constexpr unsigned ZONE = ZONE_BYTES, ROW = VCDU_BYTES, ZOFF = 8, FILL_VC = 63;
constexpr unsigned FHP_NONE = 2047, APID_FILL = 2047;
constexpr unsigned ORG_NONE = 0, ORG_STATE = 1;     // origin of pending bytes: none, the handle's state, 2 + row
constexpr unsigned FILL_BIT = 0x80000000u;

__device__ __forceinline__ unsigned row_counter(const unsigned char *r) { return (unsigned)r[2] << 16 | (unsigned)r[3] << 8 | r[4]; }
__device__ __forceinline__ unsigned row_fhp(const unsigned char *r) { return ((unsigned)r[6] & 7u) << 8 | r[7]; }

// the offsets, none beyond the row count (s_off[64])
__device__ __forceinline__ void load_offsets(const unsigned *offsets, unsigned *s_off, int tid)
{
    if (tid <= (int)NVC) {
        const unsigned n = offsets[NVC], o = offsets[tid];
        s_off[tid] = o < n ? o : n;
    }
    __syncthreads();
}

// the channel of row r: the largest v with s_off[v] <= r (r < s_off[64])
__device__ __forceinline__ unsigned channel_of(const unsigned *s_off, unsigned r)
{
    unsigned lo = 0, hi = NVC;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (s_off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// a * b mod x^16 + x^12 + x^5 + 1
__device__ __forceinline__ unsigned gf_mul(unsigned a, unsigned b)
{
    unsigned r = 0;
#pragma unroll
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x11021u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// bytes of a packet: `head_len` bytes at head, then the zones of consecutive rows from `follow` (a zone's first byte)
struct Src {
    const unsigned char *head, *follow;
    unsigned head_len;
};
__device__ __forceinline__ unsigned src_byte(const Src &s, unsigned k)
{
    if (k < s.head_len) return s.head[k];
    k -= s.head_len;
    const unsigned q = k / ZONE;
    return s.follow[(size_t)q * ROW + (k - q * ZONE)];
}
}  // namespace

// (a) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) packets_walk_kernel(const unsigned char *__restrict__ vcdu, const unsigned *__restrict__ offsets,
                                                           unsigned max_rows, const PacketsState *__restrict__ state,
                                                           const unsigned char *__restrict__ pend, unsigned *__restrict__ rowA,
                                                           uint2 *__restrict__ spanB, uint2 *__restrict__ newp,
                                                           unsigned *__restrict__ state_disc)
{
    __shared__ unsigned s_off[NVC + 1];
    const int tid = threadIdx.x;
    load_offsets(offsets, s_off, tid);
    const unsigned n = s_off[NVC];
    if (offsets[NVC] > max_rows) return;
    const size_t g = (size_t)blockIdx.x * 256 + tid;

    // what this lane follows: `len` bytes at head (the tail of row g - 64, or channel g's pending state), then rows j .. e
    unsigned v, j, e, len = 0, prevc = 0, org = ORG_NONE, word = 0;
    const unsigned char *head = nullptr;
    if (g < NVC) {
        v = (unsigned)g;
        if (v == FILL_VC) return;
        len = state->pend_len[v];
        if (len == 0) { state_disc[v] = 0; return; }
        j = s_off[v];
        e = s_off[v + 1];
        prevc = (unsigned)state->last[v];
        org = ORG_STATE;
        head = pend + (size_t)v * PACKETS_PEND_STRIDE;
    } else {
        const size_t r = g - NVC;
        if (r >= n) return;
        v = channel_of(s_off, (unsigned)r);
        if (v == FILL_VC) { rowA[r] = 0; return; }
        const unsigned char *row = vcdu + r * ROW;
        const unsigned fhp = row_fhp(row);
        unsigned cnt = 0, fills = 0, bytes = 0;
        if (fhp < ZONE) {
            unsigned p = fhp;
            while (p < ZONE) {
                if (ZONE - p < 6) { len = ZONE - p; break; }
                const unsigned char *h = row + ZOFF + p;
                const unsigned total = 7u + ((unsigned)h[4] << 8 | h[5]);
                if (p + total > ZONE) { len = ZONE - p; break; }
                if ((((unsigned)h[0] & 7u) << 8 | h[1]) == APID_FILL) ++fills;
                else { ++cnt; bytes += total; }
                p += total;
            }
        }
        word = cnt | fills << 8 | bytes << 16 | ((fhp >= ZONE && fhp < 2046u) ? 1u << 29 : 0u);
        if (len == 0) { rowA[r] = word; return; }
        j = (unsigned)r + 1;
        e = s_off[v + 1];
        prevc = row_counter(row);
        org = (unsigned)r + 2u;
        head = row + ZOFF + (ZONE - len);
    }

    const unsigned head_len = len, first_j = j;
    unsigned total = head_len >= 6 ? 7u + ((unsigned)head[4] << 8 | head[5]) : 0u;
    bool discarded = false;
    for (;; ++j) {
        if (j >= e) {                                   // the call's rows ran out: this is what the channel holds now
            newp[v] = make_uint2(org, len);
            break;
        }
        const unsigned char *rj = vcdu + (size_t)j * ROW;
        const unsigned cj = row_counter(rj), fj = row_fhp(rj);
        if (cj != ((prevc + 1u) & 0xFFFFFFu) || (fj >= ZONE && fj != FHP_NONE)) { discarded = true; break; }
        prevc = cj;
        len += fj == FHP_NONE ? ZONE : fj;
        const Src hs{head, vcdu + (size_t)first_j * ROW + ZOFF, head_len};
        if (total == 0 && len >= 6) total = 7u + (src_byte(hs, 4) << 8 | src_byte(hs, 5));     // only where j == first_j
        if (fj == FHP_NONE && len < total) continue;
        if (len >= 6 && len == total) {
            const unsigned apid = (src_byte(hs, 0) & 7u) << 8 | src_byte(hs, 1);
            spanB[j] = make_uint2(org, total | (apid == APID_FILL ? FILL_BIT : 0u));
        } else
            discarded = true;
        break;
    }
    if (g < NVC) state_disc[v] = discarded ? 1u : 0u;
    else rowA[g - NVC] = word | (discarded ? 1u << 28 : 0u);
}

// (b) ------------------------------------------------------------------------------------------------------------------
// b1, one workgroup per tile of 1024 rows: packets and bytes per row -> their exclusive prefix inside the tile, the tile's sums
__global__ void __launch_bounds__(1024) packets_tile_kernel(const unsigned *__restrict__ offsets, unsigned max_rows,
                                                            const unsigned *__restrict__ rowA, const uint2 *__restrict__ spanB,
                                                            unsigned *__restrict__ plocal, unsigned *__restrict__ blocal,
                                                            uint2 *__restrict__ tsum)
{
    __shared__ unsigned s_c[16], s_b[16];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const unsigned n = offsets[NVC];
    if (n > max_rows) return;
    const size_t r = (size_t)blockIdx.x * PACKETS_TILE + tid;
    unsigned c = 0, by = 0;
    if (r < n) {
        const unsigned ra = rowA[r];
        const uint2 sp = spanB[r];
        const bool span = sp.x != ORG_NONE && !(sp.y & FILL_BIT);
        c = (ra & 0xFFu) + (span ? 1u : 0u);
        by = ((ra >> 16) & 0x3FFu) + (span ? sp.y : 0u);        // a tile holds less than 2^27 bytes
    }
    unsigned tc, tb;
    const unsigned pc = block_incl_scan<16>(c, lane, w, s_c, tc) - c, pb = block_incl_scan<16>(by, lane, w, s_b, tb) - by;
    if (r < n) {
        plocal[r] = pc;
        blocal[r] = pb;
    }
    if (tid == 0) tsum[blockIdx.x] = make_uint2(tc, tb);
}

// b2, one workgroup: the tiles' sums -> every tile's first descriptor index and byte offset, the per-channel packet
// offsets, the call's counts and the overflow flag
__global__ void __launch_bounds__(1024) packets_scan_kernel(const unsigned *__restrict__ offsets, unsigned max_rows,
                                                            const uint2 *__restrict__ tsum, const unsigned *__restrict__ plocal,
                                                            unsigned *__restrict__ tbase_c, unsigned long long *__restrict__ tbase_b,
                                                            unsigned *__restrict__ pkt_offsets, xrit_packets_summary *__restrict__ sum,
                                                            unsigned long long max_packets, unsigned long long max_bytes)
{
    __shared__ unsigned s_c[16];
    __shared__ unsigned long long s_b[16];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const unsigned n = offsets[NVC];
    if (n > max_rows) {
        if (tid <= (int)NVC) pkt_offsets[tid] = 0;
        if (tid == 0) {
            sum->packets = 0;
            sum->bytes = 0;
            sum->overflow = 2;
            sum->reserved = 0;
        }
        return;
    }
    // thread t: tiles [t per, (t + 1) per)
    const unsigned T = (n + PACKETS_TILE - 1) / PACKETS_TILE, per = (T + 1023u) / 1024u;
    const unsigned a = (unsigned)tid * per < T ? (unsigned)tid * per : T, b = a + per < T ? a + per : T;
    unsigned c = 0;
    unsigned long long by = 0;
    for (unsigned t = a; t < b; ++t) {
        const uint2 x = tsum[t];
        c += x.x;
        by += x.y;
    }
    unsigned tc;
    unsigned long long tb;
    unsigned pc = block_incl_scan<16>(c, lane, w, s_c, tc) - c;
    unsigned long long pb = block_incl_scan<16>(by, lane, w, s_b, tb) - by;
    for (unsigned t = a; t < b; ++t) {
        tbase_c[t] = pc;
        tbase_b[t] = pb;
        const uint2 x = tsum[t];
        pc += x.x;
        pb += x.y;
    }
    __threadfence_block();
    __syncthreads();
    if (tid <= (int)NVC) {
        const unsigned o = offsets[tid];
        pkt_offsets[tid] = o < n ? tbase_c[o / PACKETS_TILE] + plocal[o] : tc;
    }
    if (tid == 0) {
        sum->packets = tc;
        sum->bytes = tb;
        sum->overflow = (tc > max_packets || tb > max_bytes) ? 1u : 0u;
        sum->reserved = 0;
    }
}

// (c) ------------------------------------------------------------------------------------------------------------------
namespace {
struct CrcTables {
    unsigned short tab[256];        // the byte table of CRC-16/CCITT, MSB first
    unsigned short pw[16];          // x^(8 2^k) mod the polynomial
    unsigned short sh[4];           // x^(8 1024 (3 - w)): what wave w's kilobyte is shifted by inside a chunk
};
constexpr unsigned gf_mul_c(unsigned a, unsigned b)
{
    unsigned r = 0;
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x11021u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
constexpr CrcTables make_tables()
{
    CrcTables t{};
    for (unsigned v = 0; v < 256; ++v) {
        unsigned x = v << 8;
        for (int i = 0; i < 8; ++i) x = (x & 0x8000u) ? ((x << 1) ^ 0x1021u) & 0xFFFFu : (x << 1) & 0xFFFFu;
        t.tab[v] = (unsigned short)x;
    }
    unsigned pw = 0x100u;
    for (int k = 0; k < 16; ++k) {
        t.pw[k] = (unsigned short)pw;
        pw = gf_mul_c(pw, pw);
    }
    t.sh[3] = 1;
    t.sh[2] = t.pw[10];
    t.sh[1] = t.pw[11];
    t.sh[0] = (unsigned short)gf_mul_c(t.pw[10], t.pw[11]);
    return t;
}
__device__ const CrcTables c_tables = make_tables();

constexpr unsigned GWAVES = 4, GTHREADS = 64 * GWAVES, GROWS = 8;       // a workgroup takes eight rows, one after the other
constexpr unsigned PER_LANE = 16, CHUNK = GTHREADS * PER_LANE;      // a lane's CRC slice; bytes the workgroup moves per step
static_assert(GTHREADS == 256 && CHUNK == 4096, "one table entry per thread; the factors sh[] and pw[12] are for kilobytes per wave");

// One packet by one workgroup of four waves.  The bytes in front of the CRC go in chunks of 4096 that END where the CRC
// begins (what lies in front of the packet is not there: zeros in front of the data leave a zero register alone): 16
// coalesced byte loads per lane in flight, stored to the output and to LDS; then every lane runs the 16 bytes of its
// slice of the chunk, the slices of a wave combine in a butterfly and the four waves' kilobytes through LDS.  Returns
// crc_ok (the same in every lane).
__device__ __forceinline__ unsigned emit_packet(const Src &s, unsigned total, unsigned long long idx, unsigned long long off,
                                                unsigned vcid, unsigned first_counter, int tid, const unsigned short *s_tab,
                                                const unsigned short *s_pw, unsigned char *s_buf, unsigned *s_part,
                                                unsigned char *__restrict__ bytes,
                                                unsigned long long max_bytes, xrit_packet *__restrict__ packets,
                                                unsigned long long max_packets)
{
    const bool wr = off + total <= max_bytes;
    const int lane = tid & 63, w = tid >> 6;
    unsigned computed = 0, carried = 0, ok = 0;
    if (total < 8) {
        if (wr && (unsigned)tid < total) bytes[off + tid] = (unsigned char)src_byte(s, tid);
    } else {
        const int e = (int)total - 2, n = e - 6;        // the CRC's place; bytes of data field in front of it
        const int m = (e + (int)CHUNK - 1) / (int)CHUNK;
        unsigned R = 0;
        for (int q = 0; q < m; ++q) {
            const int kb = e - (m - q) * (int)CHUNK;
            unsigned x[PER_LANE];
#pragma unroll
            for (int u = 0; u < (int)PER_LANE; ++u) {
                const int k = kb + tid + (int)GTHREADS * u;
                x[u] = k >= 0 ? src_byte(s, (unsigned)k) : 0u;
            }
#pragma unroll
            for (int u = 0; u < (int)PER_LANE; ++u) {
                const int k = kb + tid + (int)GTHREADS * u;
                if (wr && k >= 0) bytes[off + (unsigned)k] = (unsigned char)x[u];
                // the header does not count; the initial value 0xFFFF is an XOR on the first two bytes of data
                s_buf[tid + (int)GTHREADS * u] = (unsigned char)(k < 6 ? 0u : (k < 8 ? x[u] ^ 0xFFu : x[u]));
            }
            __syncthreads();
            unsigned reg = 0;
            const uint4 sl = *reinterpret_cast<const uint4 *>(s_buf + PER_LANE * tid);
            const unsigned wd[4] = {sl.x, sl.y, sl.z, sl.w};
#pragma unroll
            for (int t = 0; t < (int)PER_LANE; ++t) {
                const unsigned byte = (wd[t >> 2] >> (8 * (t & 3))) & 0xFFu;
                reg = ((reg << 8) & 0xFFFFu) ^ s_tab[(reg >> 8) ^ byte];
            }
#pragma unroll
            for (int l = 0; l < 6; ++l) {           // (no wave_ops.h sum: neighbours' CRCs joined in GF(2^16), offsets 1 up to 32)
                const unsigned o = __shfl_xor(reg, 1 << l, 64), X = s_pw[4 + l];
                reg = ((lane >> l) & 1) ? (gf_mul(o, X) ^ reg) : (gf_mul(reg, X) ^ o);
            }
            if (lane == 0) s_part[w] = gf_mul(reg, c_tables.sh[w]);
            __syncthreads();
            R = gf_mul(R, s_pw[12]) ^ s_part[0] ^ s_part[1] ^ s_part[2] ^ s_part[3];
        }
        // with a data field of one byte the second 0xFF of the initial value has no byte to fall on; with none, neither
        computed = n >= 2 ? R : (n == 1 ? R ^ 0xFF00u : 0xFFFFu);
        const unsigned c0 = src_byte(s, total - 2), c1 = src_byte(s, total - 1);
        if (wr && tid < 2) bytes[off + total - 2 + tid] = (unsigned char)(tid ? c1 : c0);
        carried = c0 << 8 | c1;
        ok = computed == carried ? 1u : 0u;
    }
    if (tid == 0 && idx < max_packets) {
        const unsigned h0 = src_byte(s, 0), h1 = src_byte(s, 1), h2 = src_byte(s, 2), h3 = src_byte(s, 3);
        xrit_packet d{};
        d.offset = off;
        d.length = total;
        d.first_counter = first_counter;
        d.apid = (uint16_t)((h0 & 7u) << 8 | h1);
        d.seq_count = (uint16_t)((h2 & 0x3Fu) << 8 | h3);
        d.crc_computed = (uint16_t)computed;
        d.crc_carried = (uint16_t)carried;
        d.vcid = (uint8_t)vcid;
        d.seq_flags = (uint8_t)(h2 >> 6);
        d.crc_ok = (uint8_t)ok;
        d.header_bits = (uint8_t)(h0 >> 3);
        packets[idx] = d;
    }
    return ok;
}
}  // namespace

__global__ void __launch_bounds__(GTHREADS) packets_gather_kernel(const unsigned char *__restrict__ vcdu, const unsigned *__restrict__ offsets,
                                                            unsigned max_rows, const PacketsState *__restrict__ state,
                                                            const unsigned char *__restrict__ pend, const unsigned *__restrict__ rowA,
                                                            const uint2 *__restrict__ spanB, const unsigned *__restrict__ plocal,
                                                            const unsigned *__restrict__ blocal, const unsigned *__restrict__ tbase_c,
                                                            const unsigned long long *__restrict__ tbase_b,
                                                            unsigned char *__restrict__ bytes, unsigned long long max_bytes,
                                                            xrit_packet *__restrict__ packets, unsigned long long max_packets,
                                                            unsigned *__restrict__ crcfail)
{
    __shared__ unsigned s_off[NVC + 1];
    __shared__ unsigned short s_tab[256], s_pw[16];
    __shared__ __attribute__((aligned(16))) unsigned char s_buf[CHUNK];
    __shared__ unsigned s_part[GWAVES];
    const int tid = threadIdx.x;
    const unsigned n = offsets[NVC];
    if (n > max_rows) return;
    bool ready = false;
    for (size_t r = (size_t)blockIdx.x * GROWS; r < (size_t)(blockIdx.x + 1) * GROWS && r < n; ++r) {
        const unsigned ra = rowA[r];
        const uint2 sp = spanB[r];
        const bool span = sp.x != ORG_NONE && !(sp.y & FILL_BIT);
        if ((ra & 0xFFu) == 0 && !span) {                   // nothing to emit here (the fill channel's rows among them)
            if (tid == 0) crcfail[r] = 0;
            continue;
        }
        if (!ready) {                                       // (the same decision in every thread of the workgroup)
            load_offsets(offsets, s_off, tid);
            s_tab[tid] = c_tables.tab[tid];
            if (tid < 16) s_pw[tid] = c_tables.pw[tid];
            __syncthreads();
            ready = true;
        }
        const unsigned v = channel_of(s_off, (unsigned)r);
        const unsigned char *row = vcdu + r * ROW;
        const unsigned fhp = row_fhp(row), counter = row_counter(row);
        unsigned long long idx = (unsigned long long)tbase_c[r / PACKETS_TILE] + plocal[r], off = tbase_b[r / PACKETS_TILE] + blocal[r];
        unsigned failed = 0;
        if (span) {
            // the packet that ends here: its head, then whole zones, then this row's first bytes
            const unsigned total = sp.y, here = fhp == FHP_NONE ? ZONE : fhp;
            Src s;
            unsigned fc;
            if (sp.x == ORG_STATE) {
                const unsigned first = s_off[v];
                s.head = pend + (size_t)v * PACKETS_PEND_STRIDE;
                s.head_len = total - here - ZONE * ((unsigned)r - first);
                s.follow = vcdu + (size_t)first * ROW + ZOFF;
                fc = state->first_counter[v];
            } else {
                const unsigned i = sp.x - 2u;
                const unsigned char *ri = vcdu + (size_t)i * ROW;
                s.head_len = total - here - ZONE * ((unsigned)r - i - 1u);
                s.head = ri + ZOFF + (ZONE - s.head_len);
                s.follow = ri + ROW + ZOFF;
                fc = row_counter(ri);
            }
            failed += 1u - emit_packet(s, total, idx, off, v, fc, tid, s_tab, s_pw, s_buf, s_part, bytes, max_bytes, packets, max_packets);
            ++idx;
            off += total;
        }
        const unsigned inside = (ra & 0xFFu) + ((ra >> 8) & 0xFFu);
        unsigned p = fhp;
        for (unsigned q = 0; q < inside; ++q) {
            const unsigned char *h = row + ZOFF + p;
            const unsigned total = 7u + ((unsigned)h[4] << 8 | h[5]);
            if ((((unsigned)h[0] & 7u) << 8 | h[1]) != APID_FILL) {
                const Src s{h, h, total};
                failed += 1u - emit_packet(s, total, idx, off, v, counter, tid, s_tab, s_pw, s_buf, s_part, bytes, max_bytes, packets, max_packets);
                ++idx;
                off += total;
            }
            p += total;
        }
        if (tid == 0) crcfail[r] = failed;
    }
}

// (d) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) packets_finish_kernel(const unsigned char *__restrict__ vcdu, const unsigned *__restrict__ offsets,
                                                             unsigned max_rows, PacketsState *__restrict__ state,
                                                             unsigned char *__restrict__ pend, const unsigned *__restrict__ rowA,
                                                             const uint2 *__restrict__ spanB, const uint2 *__restrict__ newp,
                                                             const unsigned *__restrict__ state_disc, const unsigned *__restrict__ crcfail)
{
    __shared__ unsigned s_red[16][5];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const unsigned v = blockIdx.x, n = offsets[NVC];
    if (n > max_rows || v == FILL_VC) return;
    const unsigned o0 = offsets[v], o1 = offsets[v + 1];
    const unsigned s = o0 < n ? o0 : n, e = o1 < n ? o1 : n;
    unsigned pk = 0, fl = 0, dc = 0, bad = 0, cf = 0;
    for (unsigned r = s + (unsigned)tid; r < e; r += 1024) {
        const unsigned ra = rowA[r];
        const uint2 sp = spanB[r];
        pk += (ra & 0xFFu) + ((sp.x != ORG_NONE && !(sp.y & FILL_BIT)) ? 1u : 0u);
        fl += ((ra >> 8) & 0xFFu) + ((sp.x != ORG_NONE && (sp.y & FILL_BIT)) ? 1u : 0u);
        dc += (ra >> 28) & 1u;
        bad += (ra >> 29) & 1u;
        cf += crcfail[r];
    }
    pk = wave_sum(pk); fl = wave_sum(fl); dc = wave_sum(dc); bad = wave_sum(bad); cf = wave_sum(cf);
    if (lane == 0) { s_red[w][0] = pk; s_red[w][1] = fl; s_red[w][2] = dc; s_red[w][3] = bad; s_red[w][4] = cf; }
    const unsigned old_len = state->pend_len[v];
    const bool had = old_len != 0;
    const uint2 np = had || e > s ? newp[v] : make_uint2(ORG_NONE, 0u);      // (written by the walk where there was anything to follow)
    __syncthreads();

    // what the channel holds now: the old bytes and the zones behind them, or a row's tail and the zones behind it
    unsigned new_len = np.x == ORG_NONE ? 0u : (np.y < PACKETS_PEND_MAX ? np.y : PACKETS_PEND_MAX);
    unsigned char *dst = pend + (size_t)v * PACKETS_PEND_STRIDE;
    unsigned fc = state->first_counter[v];
    if (np.x == ORG_STATE) {
        const Src src{dst, vcdu + (size_t)s * ROW + ZOFF, old_len};
        for (unsigned k = old_len + (unsigned)tid; k < new_len; k += 1024) dst[k] = (unsigned char)src_byte(src, k);
    } else if (np.x != ORG_NONE) {
        const unsigned i = np.x - 2u;
        const unsigned char *ri = vcdu + (size_t)i * ROW;
        const unsigned head_len = new_len - ZONE * (e - 1u - i);
        const Src src{ri + ZOFF + (ZONE - head_len), ri + ROW + ZOFF, head_len};
        for (unsigned k = tid; k < new_len; k += 1024) dst[k] = (unsigned char)src_byte(src, k);
        fc = row_counter(ri);
    }
    if (tid == 0) {
        unsigned t[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 16; ++i)
            for (int k = 0; k < 5; ++k) t[k] += s_red[i][k];
        state->packets[v] += t[0];
        state->fill_packets[v] += t[1];
        state->discarded[v] += t[2] + (had ? state_disc[v] : 0u);
        state->bad_fhp[v] += t[3];
        state->crc_failures[v] += t[4];
        state->rows[v] += e - s;
        if (e > s) state->last[v] = (int)row_counter(vcdu + (size_t)(e - 1u) * ROW);
        state->pend_len[v] = new_len;
        state->first_counter[v] = new_len ? fc : 0u;
    }
}

// (e) ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) packets_summary_kernel(const PacketsState *__restrict__ state, xrit_packets_summary *__restrict__ sum)
{
    const int v = threadIdx.x;
    const bool in = v != (int)FILL_VC;
    const unsigned long long a = wave_sum(in ? state->packets[v] : 0ull), b = wave_sum(in ? state->crc_failures[v] : 0ull),
                             c = wave_sum(in ? state->fill_packets[v] : 0ull), d = wave_sum(in ? state->discarded[v] : 0ull),
                             e = wave_sum(in ? state->bad_fhp[v] : 0ull), f = wave_sum(in ? state->rows[v] : 0ull);
    if (v == 0) {
        sum->total_packets = a;
        sum->crc_failures = b;
        sum->fill_packets = c;
        sum->discarded = d;
        sum->bad_fhp = e;
        sum->rows = f;
    }
}

// spanB and newp lie together, state_disc behind them: one memset clears both
size_t packets_scratch_carve(void *base, size_t max_rows, PacketsScratch &sc)
{
    const size_t R = max_rows ? max_rows : 1, T = div_up(R, PACKETS_TILE);
    Carver c{static_cast<char *>(base)};
    sc.spanB = c.take<uint2>(R, 16);
    sc.newp = c.take<uint2>(NVC, 16);
    sc.state_disc = c.take<unsigned>(2 * NVC, 16);      // (64 words used)
    sc.tsum = c.take<uint2>(T, 16);
    sc.tbase_b = c.take<unsigned long long>(T, 16);
    sc.tbase_c = c.take<unsigned>(T, 16);
    sc.rowA = c.take<unsigned>(R, 16);
    sc.plocal = c.take<unsigned>(R, 16);
    sc.blocal = c.take<unsigned>(R, 16);
    sc.crcfail = c.take<unsigned>(R, 16);
    return c.used();
}

int launch_packets(const unsigned char *vcdu, const unsigned *offsets, size_t max_rows, PacketsState *state, unsigned char *pend,
                   PacketsScratch &sc, unsigned char *bytes, size_t max_bytes, xrit_packet *packets, size_t max_packets,
                   unsigned *pkt_offsets, xrit_packets_summary *summary, hipStream_t s)
{
    const size_t R = max_rows ? max_rows : 1;
    const unsigned rows = (unsigned)max_rows;
    XR_HIP(hipMemsetAsync(sc.spanB, 0, (size_t)((char *)sc.state_disc - (char *)sc.spanB), s));
    hipLaunchKernelGGL(packets_walk_kernel, dim3(div_up(max_rows + NVC, 256)), dim3(256), 0, s, vcdu, offsets, rows, state, pend, sc.rowA,
                       sc.spanB, sc.newp, sc.state_disc);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(packets_tile_kernel, dim3(div_up(R, PACKETS_TILE)), dim3(1024), 0, s, offsets, rows, sc.rowA, sc.spanB, sc.plocal,
                       sc.blocal, sc.tsum);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(packets_scan_kernel, dim3(1), dim3(1024), 0, s, offsets, rows, sc.tsum, sc.plocal, sc.tbase_c, sc.tbase_b,
                       pkt_offsets, summary, (unsigned long long)max_packets, (unsigned long long)max_bytes);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(packets_gather_kernel, dim3(div_up(R, 8)), dim3(256), 0, s, vcdu, offsets, rows, state, pend, sc.rowA, sc.spanB,
                       sc.plocal, sc.blocal, sc.tbase_c, sc.tbase_b, bytes, (unsigned long long)max_bytes, packets,
                       (unsigned long long)max_packets, sc.crcfail);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(packets_finish_kernel, dim3(NVC), dim3(1024), 0, s, vcdu, offsets, rows, state, pend, sc.rowA, sc.spanB, sc.newp,
                       sc.state_disc, sc.crcfail);
    XR_HIP(hipGetLastError());
    hipLaunchKernelGGL(packets_summary_kernel, dim3(1), dim3(64), 0, s, state, summary);
    XR_HIP(hipGetLastError());
    return XRIT_OK;
}

}  // namespace xrit
