// jpeg_host_check.cpp -- the JPEG stage's rule (jpeg_rule.h: jpeg_dct_pass, jpeg_quantise, jpeg_colour, jpeg_category,
// jpeg_quality_entry and the Huffman codes -- the functions the kernels of jpeg.hip call) replayed over a table recorded from
// tests/jpeg_spec.py (tests/golden/jpeg_rule_table.txt; tests/test_jpeg_spec.py holds the table to the specification).  A
// program of its own for the sanitizers: make jpeg-host-check.
// A row has 18 columns, zeros behind what a kind uses.  0 second, 8 in | 8 out: a transform pass.  1 c q | level: the
// quantiser.  2 r g b | y cb cr.  3 v | category, magnitude bits.  4 base quality | entry.  5 table symbol | code, length.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "jpeg_rule.h"

using namespace xrit;

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: jpeg_host_check TABLE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "jpeg_host_check: cannot read %s\n", argv[1]);
        return 2;
    }
    static constexpr JpegCodeTables codes = jpeg_make_code_tables();
    std::string text;
    size_t rows = 0, passes = 0, bad = 0, symbols = 0;
    while (std::getline(in, text)) {
        std::istringstream ss(text);
        std::vector<long long> v;
        for (long long x; ss >> x;) v.push_back(x);
        if (v.size() != 18 || v[0] < 0 || v[0] > 5) {
            std::fprintf(stderr, "jpeg_host_check: row %zu has %zu columns or an unknown kind\n", rows, v.size());
            return 1;
        }
        ++rows;
        bool ok = true;
        switch (v[0]) {
        case 0: {
            int32_t d[8];
            for (int i = 0; i < 8; ++i) {
                if (v[2 + i] < -5800 || v[2 + i] > 5800) return 1;
                d[i] = (int32_t)v[2 + i];
            }
            jpeg_dct_pass(d, v[1] != 0);
            for (int i = 0; i < 8; ++i) ok = ok && d[i] == v[10 + i];
            ++passes;
            break;
        }
        case 1:
            if (v[1] < -8192 || v[1] > 8191 || v[2] < 1 || v[2] > 255) return 1;
            ok = jpeg_quantise((int32_t)v[1], (uint32_t)v[2]) == v[3];
            break;
        case 2: {
            if (v[1] < 0 || v[1] > 255 || v[2] < 0 || v[2] > 255 || v[3] < 0 || v[3] > 255) return 1;
            int32_t y, cb, cr;
            jpeg_colour((int32_t)v[1], (int32_t)v[2], (int32_t)v[3], y, cb, cr);
            ok = y == v[4] && cb == v[5] && cr == v[6];
            break;
        }
        case 3: {
            if (v[1] < -32767 || v[1] > 32767) return 1;
            uint32_t bits;
            ok = jpeg_category((int32_t)v[1], bits) == v[2] && bits == v[3];
            break;
        }
        case 4:
            if (v[1] < 1 || v[1] > 255 || v[2] < 1 || v[2] > 100) return 1;
            ok = jpeg_quality_entry((uint32_t)v[1], (uint32_t)v[2]) == v[3];
            break;
        default:
            if (v[1] > 3 || v[2] < 0 || v[2] > 255) return 1;
            ok = codes.t[v[1]].e[v[2]] == ((uint32_t)v[3] << 8 | (uint32_t)v[4]);
            ++symbols;
            break;
        }
        if (!ok) {
            std::fprintf(stderr, "jpeg_host_check: row %zu differs: %s\n", rows - 1, text.c_str());
            ++bad;
        }
    }
    // a symbol that Annex K does not list has no code
    size_t listed = 0;
    for (int t = 0; t < 4; ++t)
        for (int s = 0; s < 256; ++s) listed += codes.t[t].e[s] != 0;
    if (bad || passes == 0 || symbols != listed || listed != 2 * (12 + 162)) {
        std::fprintf(stderr, "jpeg_host_check: %zu of %zu rows differ (%zu symbols recorded, %zu listed)\n", bad, rows, symbols, listed);
        return 1;
    }
    std::printf("jpeg_host_check: %zu rows, %zu transform passes, %zu Huffman codes, every one the specification's: ok\n", rows, passes, symbols);
    return 0;
}
