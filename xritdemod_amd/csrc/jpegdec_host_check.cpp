// jpegdec_host_check.cpp -- jpegdec_rule.h on the CPU under the address and undefined-behaviour sanitizers (make
// jpegdec-host-check): replays tests/golden/jpegdec_rule_table.txt, recorded from tests/jpegdec_spec.py, with exact equality.
// Lines of integers, the kind first.  0: an inverse-DCT pass (shift, 8 in, 8 out); 1: the range limit (the first value, n, the
// samples of n consecutive values); 2: the colour terms (the first x, n, four values per x); 3: a pixel (y, cb, cr, r, g, b);
// 4: a Huffman table (id, 16 counts, n, n symbols); 5: decode steps of a table (id, then window, avail, length, symbol or fault
// per step); 6: a stream (id, n, n bytes); 9: a stream that is stream 0 but for some bytes (id, then offset, value per byte);
// 7: the header of the first `cut` bytes of a stream for every cut of a range (id, first, last, xrit_jpegdec_info's eight
// fields); 8: a stream decoded with the serial walk (id, status, a checksum of its samples in block order).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "jpegdec_rule.h"

using namespace xrit;

static int failures = 0;
static void fail(size_t line, const char *what)
{
    if (++failures <= 20) fprintf(stderr, "line %zu: %s\n", line, what);
}

// the samples of a sound stream by the serial walk, one interval after the other, and their checksum
static uint32_t decode_stream(const std::vector<uint8_t> &f, uint32_t &sum)
{
    sum = 0;
    const JpegDecHeader h = jpegdec_parse_header(f.data(), f.size());
    if (h.status) return h.status;
    std::vector<JpegDecHuff> tabs(2 * h.comps);
    std::vector<uint8_t> q(64 * h.comps);
    for (uint32_t c = 0; c < h.comps; ++c) {
        jpegdec_build_huff(f.data() + h.dc_at[c], tabs[2 * c]);
        jpegdec_build_huff(f.data() + h.ac_at[c], tabs[2 * c + 1]);
        for (int k = 0; k < 64; ++k) q[64 * c + JPEG_ZIGZAG[k]] = f[h.q_at[c] + k];
    }
    // the scan cut at its markers
    std::vector<std::vector<uint8_t>> parts(1);
    std::vector<uint32_t> ms;
    bool other = false;
    for (size_t p = h.scan; p < f.size(); ++p) {
        if (f[p] != 0xFF) {
            parts.back().push_back(f[p]);
            continue;
        }
        const uint32_t n = p + 1 < f.size() ? f[p + 1] : 1u;
        if (n == 0) {
            parts.back().push_back(0xFF);
        } else if (n >= 0xD0 && n <= 0xD7) {
            ms.push_back(n & 7);
            parts.emplace_back();
        } else {
            other = p + 1 < f.size() && n != 0xD9;
            break;
        }
        ++p;
    }
    const uint32_t mcus = h.blocks / h.comps, per = h.restart ? h.restart : mcus;
    std::vector<int16_t> coef((size_t)h.blocks * 64, 0);
    for (uint32_t k = 0; k < h.intervals; ++k) {
        if (k >= parts.size()) return other ? JPEGDEC_MARKER : JPEGDEC_INTERVALS;
        const uint32_t m0 = k * per, m1 = m0 + per < mcus ? m0 + per : mcus, blocks = (m1 - m0) * h.comps;
        int16_t *at = coef.data() + (size_t)m0 * h.comps * 64;
        JpegDecState st{0, 0, 0};
        uint32_t done;
        const uint32_t fault = jpegdec_walk(parts[k].data(), (uint32_t)parts[k].size(), tabs.data(), h.comps, st, (uint32_t)parts[k].size() * 8, blocks, done,
                                            [&](uint32_t b, uint32_t z, int32_t v) { at[(size_t)b * 64 + z] = (int16_t)v; });
        if (fault) return fault;
        if (done < blocks) return JPEGDEC_SHORT;
        if (k + 1 < h.intervals && k < ms.size() && ms[k] != (k & 7)) return JPEGDEC_RST_ORDER;
    }
    if (parts.size() > h.intervals) return JPEGDEC_INTERVALS;
    if (other) return JPEGDEC_MARKER;
    uint32_t pred[3] = {0, 0, 0}, at = 0;
    for (uint32_t m = 0; m < mcus; ++m)
        for (uint32_t c = 0; c < h.comps; ++c) {
            int16_t *b = coef.data() + ((size_t)m * h.comps + c) * 64;
            if (m % per == 0) pred[c] = 0;
            pred[c] += (uint32_t)(int32_t)b[0];
            b[0] = (int16_t)(uint16_t)pred[c];
            int32_t ws[64];
            for (int col = 0; col < 8; ++col) {
                int32_t d[8];
                for (int i = 0; i < 8; ++i) {
                    int zz = 0;
                    while (JPEG_ZIGZAG[zz] != i * 8 + col) ++zz;
                    d[i] = (int32_t)((uint32_t)(int32_t)b[zz] * (uint32_t)q[64 * c + i * 8 + col]);
                }
                jpegdec_idct_pass(d, 11);
                for (int i = 0; i < 8; ++i) ws[i * 8 + col] = d[i];
            }
            for (int row = 0; row < 8; ++row) {
                jpegdec_idct_pass(ws + row * 8, 18);
                for (int i = 0; i < 8; ++i) sum += jpegdec_range_limit(ws[row * 8 + i]) * (++at);
            }
        }
    return JPEGDEC_OK;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s jpegdec_rule_table.txt\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    std::map<long long, std::vector<uint8_t>> tables, files;
    std::map<long long, JpegDecHuff> built;
    std::string text;
    size_t line = 0, rows[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, values = 0;
    while (std::getline(in, text)) {
        ++line;
        std::istringstream ss(text);
        std::vector<long long> v;
        for (long long x; ss >> x;) v.push_back(x);
        if (v.empty()) continue;
        const long long kind = v[0];
        if (kind < 0 || kind > 9) { fail(line, "unknown kind"); continue; }
        ++rows[kind];
        if (kind == 0 && v.size() == 18) {
            int32_t d[8];
            for (int i = 0; i < 8; ++i) d[i] = (int32_t)v[2 + i];
            jpegdec_idct_pass(d, (int)v[1]);
            for (int i = 0; i < 8; ++i)
                if (d[i] != v[10 + i]) { fail(line, "idct pass"); break; }
        } else if (kind == 1 && v.size() >= 3 && v.size() == 3 + (size_t)v[2]) {
            for (long long i = 0; i < v[2]; ++i)
                if (jpegdec_range_limit((int32_t)(v[1] + i)) != (uint32_t)v[3 + i]) { fail(line, "range limit"); break; }
            values += (size_t)v[2];
        } else if (kind == 2 && v.size() >= 3 && v.size() == 3 + 4 * (size_t)v[2]) {
            for (long long i = 0; i < v[2]; ++i) {
                int32_t a, b, c, d;
                const long long *w = &v[3 + 4 * i];
                jpegdec_colour_terms((int32_t)(v[1] + i), a, b, c, d);
                if (a != w[0] || b != w[1] || c != w[2] || d != w[3]) { fail(line, "colour terms"); break; }
            }
            values += (size_t)v[2];
        } else if (kind == 3 && v.size() == 7) {
            uint32_t r, g, b;
            jpegdec_colour((int32_t)v[1], (int32_t)v[2], (int32_t)v[3], r, g, b);
            if (r != v[4] || g != v[5] || b != v[6]) fail(line, "pixel");
        } else if (kind == 4 && v.size() >= 19 && v.size() == 19 + (size_t)v[18]) {
            std::vector<uint8_t> t;
            for (size_t i = 2; i < 18; ++i) t.push_back((uint8_t)v[i]);
            for (size_t i = 19; i < v.size(); ++i) t.push_back((uint8_t)v[i]);
            tables[v[1]] = t;
            jpegdec_build_huff(tables[v[1]].data(), built[v[1]]);
        } else if (kind == 5 && v.size() >= 6 && (v.size() - 2) % 4 == 0 && built.count(v[1])) {
            for (size_t i = 2; i < v.size(); i += 4) {
                uint32_t sym;
                const uint32_t l = jpegdec_decode_step(built[v[1]], (uint32_t)v[i], (uint32_t)v[i + 1], sym);
                if (l != v[i + 2] || sym != v[i + 3]) { fail(line, "decode step"); break; }
            }
            values += (v.size() - 2) / 4;
        } else if (kind == 9 && v.size() >= 2 && v.size() % 2 == 0 && files.count(0)) {
            std::vector<uint8_t> f = files[0];
            bool ok = true;
            for (size_t i = 2; i < v.size(); i += 2) {
                if (v[i] < 0 || (size_t)v[i] >= f.size()) { ok = false; break; }
                f[(size_t)v[i]] = (uint8_t)v[i + 1];
            }
            if (ok) files[v[1]] = f;
            else fail(line, "a byte outside stream 0");
        } else if (kind == 6 && v.size() >= 3 && v.size() == 3 + (size_t)v[2]) {
            std::vector<uint8_t> f;
            for (size_t i = 3; i < v.size(); ++i) f.push_back((uint8_t)v[i]);
            files[v[1]] = f;
        } else if (kind == 7 && v.size() == 12 && files.count(v[1]) && v[2] >= 0 && v[2] <= v[3] && (size_t)v[3] <= files[v[1]].size()) {
            for (long long n = v[2]; n <= v[3]; ++n) {
                // a copy of exactly `n` bytes: a read behind it is the sanitizer's to find
                const std::vector<uint8_t> cut(files[v[1]].begin(), files[v[1]].begin() + n);
                const JpegDecHeader h = jpegdec_parse_header(cut.data(), cut.size());
                const uint32_t got[8] = {h.columns, h.rows, h.comps, h.restart, h.status, h.scan, h.blocks, h.intervals};
                bool same = true;
                for (int i = 0; i < 8; ++i) same = same && got[i] == v[4 + i];
                if (!same) { fail(line, "header"); break; }
            }
            values += (size_t)(v[3] - v[2] + 1);
        } else if (kind == 8 && v.size() == 4 && files.count(v[1])) {
            uint32_t sum;
            const uint32_t status = decode_stream(files[v[1]], sum);
            if (status != v[2] || sum != v[3]) fail(line, "stream");
        } else {
            fail(line, "malformed row");
        }
    }
    size_t total = 0;
    for (int k = 0; k <= 9; ++k) {
        if (!rows[k]) { fprintf(stderr, "no row of kind %d\n", k); ++failures; }
        total += rows[k];
    }
    if (failures) {
        fprintf(stderr, "jpegdec-host-check: %d failures\n", failures);
        return 1;
    }
    printf("jpegdec-host-check: %zu rows, %zu values, decode steps and header cuts in them ok\n", total, values);
    return 0;
}
