// jpegdec_rule.h -- the JPEG decoder stage's rules per value, one set of functions for the kernels (jpegdec.hip), the host
// parts (jpegdec.cpp: xrit_jpegdec_header, the host-buffer call's sizes) and the stand-alone check (jpegdec_host_check.cpp,
// make jpegdec-host-check): the walk over the marker chain SOI .. SOS, libjpeg's derived Huffman table (a lookahead table of
// 8 bits, maxcode / valptr behind it) and one decode step, the entropy walk over one restart interval's bits, the 1-D pass
// of the slow-integer inverse DCT (jidctint: 13-bit constants, columns descaled by 11, rows by 18), the range limit and
// jdcolor's 16-bit fixed-point YCbCr -> RGB.  Everything behind the entropy walk is 32-bit two's complement, written on
// uint32_t so that a damaged stream that still decodes has one answer.  tests/jpegdec_spec.py is the specification; every
// function here equals it value for value.
#pragma once

#include <cstdint>

#include "jpeg_rule.h"

namespace xrit {

// the statuses of an image: those of the SERIAL walk (XRIT_JPEGDEC_* of include/xritdemod_amd.h)
enum : uint32_t {
    JPEGDEC_OK = 0,
    JPEGDEC_UNSUPPORTED = 1,        // a JPEG this stage does not decode
    JPEGDEC_DAMAGED = 2,            // the marker chain SOI .. SOS is broken
    JPEGDEC_TOO_LARGE = 3,
    JPEGDEC_BAD_CODE = 4,           // 16 bits that begin no code
    JPEGDEC_INDEX = 5,              // a coefficient index past 63
    JPEGDEC_SHORT = 6,              // an interval out of bits before its MCUs
    JPEGDEC_INTERVALS = 7,          // fewer or more intervals than the geometry asks for
    JPEGDEC_RST_ORDER = 8,          // an RSTm out of sequence
    JPEGDEC_MARKER = 9,             // a marker other than RSTm or EOI in the scan
    JPEGDEC_N_STATUS = 10
};
constexpr uint32_t JPEGDEC_MAX_BLOCKS = JPEG_MAX_BLOCKS;
constexpr uint32_t JPEGDEC_MAX_BYTES = 1u << 28;         // bit positions are 32-bit
constexpr uint32_t JPEGDEC_LOOKAHEAD = 8;
constexpr uint32_t JPEGDEC_DEAD = 0xFFFFFFFFu;           // the bit position of a state behind a fault
constexpr uint32_t JPEGDEC_DEFAULT_S = 1024, JPEGDEC_MIN_S = 32, JPEGDEC_MAX_S = 1u << 20;

// ---- the header -----------------------------------------------------------------------------------------------------------
struct JpegDecHeader {
    uint32_t status, columns, rows, comps, restart;
    uint32_t scan;                  // the first byte behind SOS
    uint32_t blocks, intervals;     // what the geometry asks for
    uint32_t q_at[3], dc_at[3], ac_at[3];       // per component: its 64 quantiser bytes (zigzag order), its tables' 16 counts
};

JPEG_HD JpegDecHeader jpegdec_fail(uint32_t status)
{
    JpegDecHeader h{};
    h.status = status;
    return h;
}

// The chain walked serially over b[0 .. n): the first thing wrong gives the status.  Every read is in front of n.
JPEG_HD JpegDecHeader jpegdec_parse_header(const uint8_t *b, uint64_t n)
{
    if (n < 2 || b[0] != 0xFF || b[1] != 0xD8) return jpegdec_fail(JPEGDEC_DAMAGED);
    uint32_t qt[4] = {0, 0, 0, 0}, ht[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    uint32_t rows = 0, columns = 0, nf = 0, ri = 0, cid[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    uint64_t p = 2;
    for (;;) {
        if (p + 2 > n || b[p] != 0xFF) return jpegdec_fail(JPEGDEC_DAMAGED);
        const uint32_t m = b[p + 1];
        if (m == 0xD8 || m == 0xD9 || m == 0x01 || m == 0x00 || m == 0xFF || (m >= 0xD0 && m <= 0xD7)) return jpegdec_fail(JPEGDEC_DAMAGED);
        if (p + 4 > n) return jpegdec_fail(JPEGDEC_DAMAGED);
        const uint32_t L = (uint32_t)b[p + 2] << 8 | b[p + 3];
        const uint64_t end = p + 2 + L;
        if (L < 2 || end > n) return jpegdec_fail(JPEGDEC_DAMAGED);
        if (m == 0xC0) {
            if (nf || L < 8) return jpegdec_fail(JPEGDEC_DAMAGED);
            if (b[p + 4] != 8) return jpegdec_fail(JPEGDEC_UNSUPPORTED);
            rows = (uint32_t)b[p + 5] << 8 | b[p + 6];
            columns = (uint32_t)b[p + 7] << 8 | b[p + 8];
            const uint32_t f = b[p + 9];
            if (!rows || !columns || L != 8 + 3 * f) return jpegdec_fail(JPEGDEC_DAMAGED);
            if (f != 1 && f != 3) return jpegdec_fail(JPEGDEC_UNSUPPORTED);
            for (uint32_t i = 0; i < f; ++i)
                if (b[p + 11 + 3 * i] != 0x11) return jpegdec_fail(JPEGDEC_UNSUPPORTED);
            for (uint32_t i = 0; i < f; ++i) {
                cid[i] = b[p + 10 + 3 * i];
                ctq[i] = b[p + 12 + 3 * i];
                if (ctq[i] > 3) return jpegdec_fail(JPEGDEC_DAMAGED);
            }
            nf = f;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {
            return jpegdec_fail(JPEGDEC_UNSUPPORTED);               // another SOF, JPG, DAC
        } else if (m == 0xDC || m == 0xDE || m == 0xDF) {
            return jpegdec_fail(JPEGDEC_UNSUPPORTED);               // DNL, DHP, EXP
        } else if (m == 0xC4) {
            uint64_t q = p + 4;
            while (q < end) {
                if (q + 17 > end) return jpegdec_fail(JPEGDEC_DAMAGED);
                const uint32_t tc = b[q] >> 4, th = b[q] & 15;
                if (tc > 1 || th > 3) return jpegdec_fail(JPEGDEC_DAMAGED);
                uint32_t total = 0;
                for (uint32_t l = 1; l <= 16; ++l) total += b[q + l];
                if (total > 256 || q + 17 + total > end) return jpegdec_fail(JPEGDEC_DAMAGED);
                uint32_t code = 0;
                for (uint32_t l = 1; l <= 16; ++l) {
                    code += b[q + l];
                    if (code > (1u << l)) return jpegdec_fail(JPEGDEC_DAMAGED);
                    code <<= 1;
                }
                for (uint32_t i = 0; i < total; ++i) {
                    const uint32_t v = b[q + 17 + i];
                    if (tc == 0 ? v > 11 : (v & 15) > 10) return jpegdec_fail(JPEGDEC_DAMAGED);
                }
                ht[tc][th] = (uint32_t)(q + 1);
                q += 17 + total;
            }
        } else if (m == 0xDB) {
            uint64_t q = p + 4;
            while (q < end) {
                const uint32_t pq = b[q] >> 4, tq = b[q] & 15;
                if (tq > 3 || pq > 1) return jpegdec_fail(JPEGDEC_DAMAGED);
                if (pq == 1) return jpegdec_fail(JPEGDEC_UNSUPPORTED);
                if (q + 65 > end) return jpegdec_fail(JPEGDEC_DAMAGED);
                qt[tq] = (uint32_t)(q + 1);
                q += 65;
            }
        } else if (m == 0xDD) {
            if (L != 4) return jpegdec_fail(JPEGDEC_DAMAGED);
            ri = (uint32_t)b[p + 4] << 8 | b[p + 5];
        } else if (m == 0xDA) {
            if (!nf || L < 3) return jpegdec_fail(JPEGDEC_DAMAGED);
            const uint32_t ns = b[p + 4];
            if (ns < 1 || ns > 4 || L != 6 + 2 * ns) return jpegdec_fail(JPEGDEC_DAMAGED);
            if (ns != nf) return jpegdec_fail(JPEGDEC_UNSUPPORTED);   // one scan per component: several scans
            JpegDecHeader h{};
            for (uint32_t i = 0; i < ns; ++i) {
                if (b[p + 5 + 2 * i] != cid[i]) return jpegdec_fail(JPEGDEC_UNSUPPORTED);
                const uint32_t td = b[p + 6 + 2 * i] >> 4, ta = b[p + 6 + 2 * i] & 15;
                if (td > 3 || ta > 3 || !ht[0][td] || !ht[1][ta] || !qt[ctq[i]]) return jpegdec_fail(JPEGDEC_DAMAGED);
                h.dc_at[i] = ht[0][td];
                h.ac_at[i] = ht[1][ta];
                h.q_at[i] = qt[ctq[i]];
            }
            if (b[p + 5 + 2 * ns] != 0 || b[p + 6 + 2 * ns] != 63 || b[p + 7 + 2 * ns] != 0) return jpegdec_fail(JPEGDEC_UNSUPPORTED);
            const uint32_t mcus = ((columns + 7) / 8) * ((rows + 7) / 8);
            h.columns = columns;
            h.rows = rows;
            h.comps = ns;
            h.restart = ri;
            if ((uint64_t)mcus * ns > JPEGDEC_MAX_BLOCKS) {
                h.status = JPEGDEC_TOO_LARGE;
                return h;
            }
            const uint32_t per = ri ? ri : mcus;
            h.status = JPEGDEC_OK;
            h.scan = (uint32_t)end;
            h.blocks = mcus * ns;
            h.intervals = (mcus + per - 1) / per;
            return h;
        }
        p = end;
    }
}

// ---- Huffman tables ---------------------------------------------------------------------------------------------------------
struct JpegDecHuff {
    int32_t maxcode[18];            // [1 .. 16] the largest code of that length, -1: none; [17] ends every search
    int32_t valptr[17];             // symbol index = code + valptr[length]
    uint16_t look[1 << JPEGDEC_LOOKAHEAD];      // length << 8 | symbol for the codes of up to 8 bits, 0: longer or none
    uint8_t vals[256];
    uint32_t pad;
};
static_assert(sizeof(JpegDecHuff) == 912, "JpegDecHuff layout");

// from the 16 counts and the symbols behind them (a table that jpegdec_parse_header has accepted)
JPEG_HD void jpegdec_build_huff(const uint8_t *counts, JpegDecHuff &t)
{
    for (uint32_t i = 0; i < (1u << JPEGDEC_LOOKAHEAD); ++i) t.look[i] = 0;
    uint32_t code = 0, k = 0;
    t.maxcode[0] = -1;
    t.valptr[0] = 0;
    for (uint32_t l = 1; l <= 16; ++l) {
        const uint32_t cnt = counts[l - 1];
        t.valptr[l] = (int32_t)k - (int32_t)code;
        t.maxcode[l] = -1;
        if (cnt) {
            if (l <= JPEGDEC_LOOKAHEAD)
                for (uint32_t i = 0; i < cnt; ++i)
                    for (uint32_t fill = 0; fill < (1u << (JPEGDEC_LOOKAHEAD - l)); ++fill)
                        t.look[(code + i) << (JPEGDEC_LOOKAHEAD - l) | fill] = (uint16_t)(l << 8 | counts[16 + k + i]);
            code += cnt;
            k += cnt;
            t.maxcode[l] = (int32_t)code - 1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0xFFFFF;
    for (uint32_t i = 0; i < 256; ++i) t.vals[i] = i < k ? counts[16 + i] : 0;
    t.pad = 0;
}

// One code from a 16-bit window (the bits behind the stream's end are zero) of which `avail` are the stream's: the length
// and the symbol, or length 0 and the fault in `symbol`.
JPEG_HD uint32_t jpegdec_decode_step(const JpegDecHuff &t, uint32_t window, uint32_t avail, uint32_t &symbol)
{
    const uint32_t e = t.look[window >> (16 - JPEGDEC_LOOKAHEAD)];
    uint32_t l;
    if (e) {
        l = e >> 8;
        symbol = e & 255;
    } else {
        l = JPEGDEC_LOOKAHEAD + 1;
        while (l <= 16 && (int32_t)(window >> (16 - l)) > t.maxcode[l]) ++l;
        if (l > 16) {
            symbol = avail >= 16 ? JPEGDEC_BAD_CODE : JPEGDEC_SHORT;
            return 0;
        }
        symbol = t.vals[((int32_t)(window >> (16 - l)) + t.valptr[l]) & 255];
    }
    if (l > avail) {
        symbol = JPEGDEC_SHORT;
        return 0;
    }
    return l;
}

// ---- the entropy walk -------------------------------------------------------------------------------------------------------
// 32 bits from bit `bit` of src[0 .. nbytes), most significant first; the top 25 are the stream's, zeros behind its end
JPEG_HD uint32_t jpegdec_peek(const uint8_t *src, uint32_t nbytes, uint32_t bit)
{
    const uint32_t i = bit >> 3;
    const uint32_t b0 = i < nbytes ? src[i] : 0u, b1 = i + 1 < nbytes ? src[i + 1] : 0u, b2 = i + 2 < nbytes ? src[i + 2] : 0u,
                   b3 = i + 3 < nbytes ? src[i + 3] : 0u;
    return (b0 << 24 | b1 << 16 | b2 << 8 | b3) << (bit & 7);
}

struct JpegDecState {
    uint32_t p, c, z;               // the bit, the component in the MCU, the zigzag index (0: the DC symbol comes next)
};

// Symbols that begin in front of bit `end` of the interval src[0 .. nbytes), from state st, at most `limit` blocks.
// tabs: per component its DC table, then its AC table.  sink(block, zigzag index, value) takes what is decoded, the DC as its
// difference; block counts from 0.  -> the fault (st.p = JPEGDEC_DEAD then), `done` the blocks completed.
template <class Sink>
JPEG_HD uint32_t jpegdec_walk(const uint8_t *src, uint32_t nbytes, const JpegDecHuff *tabs, uint32_t comps, JpegDecState &st, uint32_t end,
                              uint32_t limit, uint32_t &done, Sink &&sink)
{
    done = 0;
    if (st.p == JPEGDEC_DEAD) return JPEGDEC_OK;
    const uint32_t nbits = nbytes * 8;
    uint32_t p = st.p, c = st.c, z = st.z, fault = JPEGDEC_OK;
    while (p < end && done < limit) {
        uint32_t sym, s;
        const uint32_t l = jpegdec_decode_step(tabs[2 * c + (z ? 1 : 0)], jpegdec_peek(src, nbytes, p) >> 16, nbits - p, sym);
        if (!l) {
            fault = sym;
            break;
        }
        p += l;
        if (z == 0) {
            s = sym;
        } else {
            const uint32_t r = sym >> 4;
            s = sym & 15;
            if (s == 0) {
                if (r == 15) {
                    if (z + 16 > 64) {
                        fault = JPEGDEC_INDEX;
                        break;
                    }
                    z += 16;
                } else {
                    z = 64;
                }
                if (z == 64) {
                    z = 0;
                    c = c + 1 == comps ? 0 : c + 1;
                    ++done;
                }
                continue;
            }
            z += r;
            if (z > 63) {
                fault = JPEGDEC_INDEX;
                break;
            }
        }
        if (p + s > nbits) {
            fault = JPEGDEC_SHORT;
            break;
        }
        int32_t v = s ? (int32_t)(jpegdec_peek(src, nbytes, p) >> (32 - s)) : 0;
        if (s && v < (1 << (s - 1))) v -= (1 << s) - 1;
        p += s;
        sink(done, z, v);
        if (++z == 64) {
            z = 0;
            c = c + 1 == comps ? 0 : c + 1;
            ++done;
        }
    }
    if (fault) {
        st.p = JPEGDEC_DEAD;
        st.c = st.z = 0;
        return fault;
    }
    st.p = p;
    st.c = c;
    st.z = z;
    return JPEGDEC_OK;
}

// ---- inverse DCT, range limit, colour -----------------------------------------------------------------------------------------
// One 1-D pass of jidctint over d[0 .. 8), in place; shift 11 for the column pass, 18 for the row pass
JPEG_HD void jpegdec_idct_pass(int32_t *d, int shift)
{
    typedef uint32_t U;
    const auto mul = [](U a, int32_t k) { return a * (U)k; };
    const U d0 = (U)d[0], d1 = (U)d[1], d2 = (U)d[2], d3 = (U)d[3], d4 = (U)d[4], d5 = (U)d[5], d6 = (U)d[6], d7 = (U)d[7];
    U z1 = mul(d2 + d6, 4433);
    const U e2 = z1 + mul(d6, -15137), e3 = z1 + mul(d2, 6270);
    const U e0 = (d0 + d4) << 13, e1 = (d0 - d4) << 13;
    const U t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    U t0 = d7, t1 = d5, t2 = d3, t3 = d1;
    z1 = t0 + t3;
    U z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const U z5 = mul(z3 + z4, 9633);
    t0 = mul(t0, 2446);
    t1 = mul(t1, 16819);
    t2 = mul(t2, 25172);
    t3 = mul(t3, 12299);
    z1 = mul(z1, -7373);
    z2 = mul(z2, -20995);
    z3 = mul(z3, -16069) + z5;
    z4 = mul(z4, -3196) + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    const U half = 1u << (shift - 1);
    const U o[8] = {t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3};
    for (int i = 0; i < 8; ++i) d[i] = (int32_t)(o[i] + half) >> shift;
}

// the sample of a value in front of the range limit: saturating
JPEG_HD uint32_t jpegdec_range_limit(int32_t v)
{
    const int32_t s = (int32_t)((uint32_t)v + 128u);
    return s < 0 ? 0u : s > 255 ? 255u : (uint32_t)s;
}

// jdcolor's four tables at sample value x: Cr -> R, Cb -> B, Cr -> G, Cb -> G (the last two in 16-bit fixed point)
JPEG_HD void jpegdec_colour_terms(int32_t x, int32_t &crr, int32_t &cbb, int32_t &crg, int32_t &cbg)
{
    x -= 128;
    crr = (91881 * x + 32768) >> 16;
    cbb = (116130 * x + 32768) >> 16;
    crg = -46802 * x;
    cbg = -22554 * x + 32768;
}

JPEG_HD void jpegdec_colour(int32_t y, int32_t cb, int32_t cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    int32_t crr, cbb, crg, cbg, unused;
    jpegdec_colour_terms(cr, crr, unused, crg, unused);
    jpegdec_colour_terms(cb, unused, cbb, unused, cbg);
    const int32_t rr = y + crr, gg = y + ((cbg + crg) >> 16), bb = y + cbb;
    r = rr < 0 ? 0 : rr > 255 ? 255 : rr;
    g = gg < 0 ? 0 : gg > 255 ? 255 : gg;
    b = bb < 0 ? 0 : bb > 255 ? 255 : bb;
}

}  // namespace xrit
