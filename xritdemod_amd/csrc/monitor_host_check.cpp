// monitor_host_check.cpp -- the plain host parts of the link monitor (monitor_host.h: the argument checks, the plan of a push,
// xrit_monitor_derive) held against a table recorded from tests/monitor_spec.py (tests/golden/monitor_host_table.txt;
// tests/test_monitor_spec.py holds the table to the specification).  A program of its own for the sanitizers:
// make monitor-host-check.  Integers are compared exactly, the float64 fields to 1e-12 relative.
// Rows (floating-point values as C hexadecimal literals):
//   B block | ok                                                             a multiple of 64 in 64 .. 32768
//   T type | bytes                                                           of one symbol, 0: refused
//   G block open n | pieces rows open_after begin0 end0 begin_last end_last  the plan of a push of n symbols behind `open`
//                                                                            (call indices of the first and the last piece;
//                                                                            zeros when there is none)
//   D type n flips s1 s2 s4 sum sat neg | ok level dc flip_rate sat_rate neg_rate esn0_snv_db esn0_m2m4_db flags
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "monitor_host.h"

using namespace xrit;

static bool close_to(double got, double want) { return got == want || std::fabs(got - want) <= 1e-12 * std::fabs(want); }

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: monitor_host_check TABLE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "monitor_host_check: cannot read %s\n", argv[1]);
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
        auto s = [&](size_t i) { return std::strtoll(w.at(i).c_str(), nullptr, 10); };
        bool ok = false;
        if (w[0] == "B" && w.size() == 3) {
            ok = monitor_block_ok((uint32_t)u(1)) == (u(2) != 0);
        } else if (w[0] == "T" && w.size() == 3) {
            ok = monitor_symbol_bytes((int)s(1)) == u(2);
        } else if (w[0] == "G" && w.size() == 11) {
            const MonitorPlan p = monitor_plan((uint32_t)u(1), (uint32_t)u(2), (size_t)u(3));
            ok = p.pieces == u(4) && p.rows == u(5) && p.open_after == u(6);
            if (p.pieces) ok = ok && p.begin(0) == u(7) && p.end(0) == u(8) && p.begin(p.pieces - 1) == u(9) && p.end(p.pieces - 1) == u(10);
            else ok = ok && !u(7) && !u(8) && !u(9) && !u(10);
            // the pieces tile the call
            size_t at = 0;
            for (size_t k = 0; k < p.pieces && ok; ++k) {
                ok = p.begin(k) == at && p.end(k) > at;
                at = p.end(k);
            }
            ok = ok && at == p.n;
        } else if (w[0] == "D" && w.size() == 19) {
            xrit_monitor_block b{};
            b.n = (uint32_t)u(2);
            b.flips = (uint32_t)u(3);
            b.s1 = u(4);
            b.s2 = u(5);
            b.s4 = u(6);
            b.sum = s(7);
            b.sat = (uint32_t)u(8);
            b.neg = (uint32_t)u(9);
            xrit_monitor_quality q{};
            const int rc = monitor_derive(b, (int)s(1), q);
            ok = (rc == XRIT_OK) == (u(10) != 0);
            if (rc == XRIT_OK)
                ok = ok && close_to(q.level, f(11)) && close_to(q.dc, f(12)) && close_to(q.flip_rate, f(13)) && close_to(q.sat_rate, f(14)) &&
                     close_to(q.neg_rate, f(15)) && close_to(q.esn0_snv_db, f(16)) && close_to(q.esn0_m2m4_db, f(17)) && q.flags == u(18);
        }
        if (!ok) {
            ++bad;
            std::fprintf(stderr, "monitor_host_check: row %zu differs: %s\n", rows, text.c_str());
        }
    }
    if (bad || !rows) {
        std::fprintf(stderr, "monitor_host_check: %zu of %zu rows differ\n", bad, rows);
        return 1;
    }
    std::printf("monitor_host_check: %zu rows, the blocks, the symbol types, the plans and the derived records of each: ok\n", rows);
    return 0;
}
