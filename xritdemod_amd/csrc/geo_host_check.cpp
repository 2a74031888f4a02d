// geo_host_check.cpp -- the projection stage's rule (geo_rule.h: geo_nav_of, geo_atan_small, geo_point, geo_sample -- the
// functions the kernels of geo.hip call) replayed over a table recorded from tests/geo_spec.py
// (tests/golden/geo_rule_table.txt; tests/test_geo_spec.py holds the table to the specification) with exact integer
// equality.  A program of its own for the sanitizers, built with -ffp-contract=off like the library: make geo-host-check.
// A row begins with its kind.  0 cfac lfac coff loff origin: a navigation.  1 A B C S qx qy (the doubles as their 64 bits
// in decimal): a map entry under the last navigation.  2 columns rows v ..: a source image, row by row.  3 qx qy mode out
// class: an output sample from the last image.  4 t r: geo_atan_small(t) = r, both as bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "geo_rule.h"

using namespace xrit;

static double from_bits(unsigned long long b)
{
    double d;
    static_assert(sizeof d == sizeof b, "a double has 64 bits");
    std::memcpy(&d, &b, sizeof d);
    return d;
}

static unsigned long long bits_of(double d)
{
    unsigned long long b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: geo_host_check TABLE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "geo_host_check: cannot read %s\n", argv[1]);
        return 2;
    }
    GeoNav nav{};
    bool have_nav = false;
    std::vector<uint32_t> image;
    uint32_t columns = 0, rows = 0;
    std::string text;
    size_t n_rows = 0, points = 0, samples = 0, bad = 0;
    while (std::getline(in, text)) {
        std::istringstream ss(text);
        std::vector<std::string> w;
        for (std::string x; ss >> x;) w.push_back(x);
        ++n_rows;
        if (w.empty()) return 1;
        const int kind = std::stoi(w[0]);
        auto s = [&](size_t k) { return std::stoll(w[k]); };
        auto u = [&](size_t k) { return std::stoull(w[k]); };
        bool ok = true;
        if (kind == 0 && w.size() == 6) {
            xrit_geo_nav n{(int32_t)s(1), (int32_t)s(2), (int32_t)s(3), (int32_t)s(4), (int32_t)s(5), 0, 0.0};
            nav = geo_nav_of(n);
            have_nav = true;
        } else if (kind == 1 && w.size() == 7 && have_nav) {
            const xrit_geo_point p = geo_point(from_bits(u(1)), from_bits(u(2)), from_bits(u(3)), from_bits(u(4)), nav);
            ++points;
            ok = p.qx == s(5) && p.qy == s(6) && geo_is_off(p) == (s(5) == GEO_OFF);
        } else if (kind == 2 && w.size() >= 3) {
            columns = (uint32_t)u(1);
            rows = (uint32_t)u(2);
            if (!columns || !rows || w.size() != 3 + (size_t)columns * rows) return 1;
            image.assign((size_t)columns * rows, 0);
            for (size_t k = 0; k < image.size(); ++k) image[k] = (uint32_t)u(3 + k);
        } else if (kind == 3 && w.size() == 6 && !image.empty()) {
            const xrit_geo_point p{(int32_t)s(1), (int32_t)s(2)};
            GeoClass cls = GEO_OFF_DISC;
            // .at(): a tap that the rule lets through outside the image ends the program
            const uint32_t out = geo_sample(p, (uint32_t)u(3), columns, rows, [&](uint32_t x, uint32_t y) {
                if (x >= columns || y >= rows) std::abort();
                return image.at((size_t)y * columns + x);
            }, cls);
            ++samples;
            ok = out == u(4) && (uint32_t)cls == u(5);
        } else if (kind == 4 && w.size() == 3) {
            ok = bits_of(geo_atan_small(from_bits(u(1)))) == u(2);
        } else {
            std::fprintf(stderr, "geo_host_check: row %zu is malformed: %s\n", n_rows - 1, text.c_str());
            return 1;
        }
        if (!ok) {
            std::fprintf(stderr, "geo_host_check: row %zu differs: %s\n", n_rows - 1, text.c_str());
            ++bad;
        }
    }
    if (bad || !points || !samples) {
        std::fprintf(stderr, "geo_host_check: %zu of %zu rows differ\n", bad, n_rows);
        return 1;
    }
    std::printf("geo_host_check: %zu rows, %zu map entries, %zu samples, every one the specification's: ok\n", n_rows, points, samples);
    return 0;
}
