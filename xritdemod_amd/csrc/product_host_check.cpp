// product_host_check.cpp -- the product stage's rule (product_rule.h: product_decide, product_lut_entry, product_small_byte,
// product_reaches, product_is_lo, product_linear, product_clamp -- the functions the kernels of product.hip call) replayed
// over a table recorded from tests/product_spec.py (tests/golden/product_rule_table.txt; tests/test_product_spec.py holds
// the table to the specification).  A program of its own for the sanitizers: make product-host-check.
// A row has 12 columns.  0 tone bits N min_nz max_nz cmin lo hi | the tone in effect, fallback: a decision.  1 v c[v]
// table's entry | lut[v]: an entry under the last decision.  2 sum cnt | byte: a thumbnail's byte.  3 c p N | reaches,
// is_lo: a percentile test.  4 bits v maxv | linear of the clamped v, the clamped v.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "product_rule.h"

using namespace xrit;

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: product_host_check TABLE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "product_host_check: cannot read %s\n", argv[1]);
        return 2;
    }
    ProductTone t{};
    bool decided = false;
    std::string text;
    size_t rows = 0, entries = 0, bad = 0;
    while (std::getline(in, text)) {
        std::istringstream ss(text);
        std::vector<unsigned long long> v;
        for (unsigned long long x; ss >> x;) v.push_back(x);
        if (v.size() != 12 || v[0] > 4) {
            std::fprintf(stderr, "product_host_check: row %zu has %zu columns or an unknown kind\n", rows, v.size());
            return 1;
        }
        ++rows;
        bool ok = true;
        switch (v[0]) {
        case 0:
            if (v[1] > XRIT_TONE_STRETCH || v[2] < 1 || v[2] > 16) return 1;
            t = product_decide((uint32_t)v[1], (uint32_t)v[2], v[3], (uint32_t)v[4], (uint32_t)v[5], v[6], (uint32_t)v[7], (uint32_t)v[8]);
            decided = true;
            ok = t.tone == v[9] && t.fallback == v[10];
            break;
        case 1:
            if (!decided || v[1] > product_max(t.bits)) return 1;
            ++entries;
            ok = product_lut_entry(t, (uint32_t)v[1], v[2], (uint8_t)v[3]) == v[4];
            break;
        case 2:
            ok = product_small_byte((uint32_t)v[1], (uint32_t)v[2]) == v[3];
            break;
        case 3:
            ok = product_reaches(v[1], (uint32_t)v[2], v[3]) == (v[4] != 0) && product_is_lo(v[1], (uint32_t)v[2], v[3]) == (v[5] != 0);
            break;
        default:
            if (v[1] < 1 || v[1] > 16 || product_max((uint32_t)v[1]) != v[3]) return 1;
            ok = product_clamp((uint32_t)v[2], (uint32_t)v[3]) == v[5] && product_linear((uint32_t)v[1], (uint32_t)v[5]) == v[4];
            break;
        }
        if (!ok) {
            std::fprintf(stderr, "product_host_check: row %zu differs: %s\n", rows - 1, text.c_str());
            ++bad;
        }
    }
    if (bad || entries == 0) {
        std::fprintf(stderr, "product_host_check: %zu of %zu rows differ\n", bad, rows);
        return 1;
    }
    std::printf("product_host_check: %zu rows, %zu table entries, every one the specification's: ok\n", rows, entries);
    return 0;
}
