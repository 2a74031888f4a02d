// acquire_host_check.cpp -- the plain host parts of the carrier acquisition stage (acquire_host.h: the parameter checks,
// the phase step from hertz, the segments of a call, the scratch sizes) held against a table recorded from
// tests/acquire_spec.py (tests/golden/acquire_host_table.txt; tests/test_acquire_spec.py holds the table to the
// specification).  A program of its own for the sanitizers: make acquire-host-check.
// Rows (floating-point values as C hexadecimal literals):
//   P sample_rate pre_sum segments min_ratio | ok pre_sum segments min_ratio     the parameters resolved (ok 0: refused)
//   I hz sample_rate | ok inc                                                    inc = llrint(ldexp(hz / sample_rate, 64))
//   M n pre_sum max_segments | segments
//   S segments | spectra_bytes power_bytes
//   T type | bytes                                                               of one complex sample, 0: refused
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "acquire_host.h"

using namespace xrit;

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: acquire_host_check TABLE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "acquire_host_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string text;
    size_t rows = 0, bad = 0;
    while (std::getline(in, text)) {
        std::istringstream ss(text);
        std::vector<std::string> w;
        for (std::string tok; ss >> tok;) w.push_back(tok);
        if (w.empty()) continue;
        ++rows;
        auto f = [&](size_t i) { return std::strtod(w.at(i).c_str(), nullptr); };
        auto u = [&](size_t i) { return std::strtoull(w.at(i).c_str(), nullptr, 10); };
        bool ok = false;
        if (w[0] == "P" && w.size() == 9) {
            xrit_acquire_params p{f(1), (uint32_t)u(2), (uint32_t)u(3), f(4)}, r{};
            const bool good = acquire_params_resolve(p, r);
            ok = good == (u(5) != 0) && (!good || (r.pre_sum == u(6) && r.segments == u(7) && r.min_ratio == f(8) && r.sample_rate == f(1)));
        } else if (w[0] == "I" && w.size() == 5) {
            int64_t inc = 0;
            const bool good = acquire_inc_from_hz(f(1), f(2), inc);
            ok = good == (u(3) != 0) && (!good || inc == (int64_t)std::strtoll(w[4].c_str(), nullptr, 10));
        } else if (w[0] == "M" && w.size() == 5) {
            ok = acquire_segments((size_t)u(1), (unsigned)u(2), (unsigned)u(3)) == u(4);
        } else if (w[0] == "S" && w.size() == 4) {
            ok = acquire_spectra_bytes((unsigned)u(1)) == u(2) && ACQ_POWER_BYTES == u(3);
        } else if (w[0] == "T" && w.size() == 3) {
            ok = acquire_sample_bytes((int)std::strtol(w[1].c_str(), nullptr, 10)) == u(2);
        }
        if (!ok) {
            ++bad;
            std::fprintf(stderr, "acquire_host_check: row %zu differs: %s\n", rows, text.c_str());
        }
    }
    if (bad || !rows) {
        std::fprintf(stderr, "acquire_host_check: %zu of %zu rows differ\n", bad, rows);
        return 1;
    }
    std::printf("acquire_host_check: %zu rows, the parameters, the phase steps, the segments and the sizes of each: ok\n", rows);
    return 0;
}
