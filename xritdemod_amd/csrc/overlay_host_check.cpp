// overlay_host_check.cpp -- the map overlay stage's rules (overlay_rule.h: overlay_setup, overlay_step_pixel,
// overlay_stamp, overlay_touches, overlay_mix, overlay_luma, overlay_blend_pixel -- the functions the kernels of overlay.hip
// call) replayed over a table recorded from tests/overlay_spec.py (tests/golden/overlay_rule_table.txt;
// tests/test_overlay_spec.py holds the table to the specification) with exact integer equality.  A program of its own for
// the sanitizers: make overlay-host-check.
// A row begins with its kind.  0 columns rows width max_jump: an image.  1 x0 y0 x1 y1 kind xmajor a0 b0 da db m0 line steps
// touched: a pair's set-up under the last image (touched: the specification walked every step; here it is overlay_touches).
// 2 x0 y0 x1 y1 k px py: the pixel of step k.  3 px py hit x0 x1 y0 y1: a stamp's part inside the last image.
// 4 src c alpha out.  5 r g b y.  6 cin cout m s0 s1 s2 o0 o1 o2: a pixel under the styles of the last row 7.  7 s0 .. s7.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "overlay_rule.h"

using namespace xrit;

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: overlay_host_check TABLE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "overlay_host_check: cannot read %s\n", argv[1]);
        return 2;
    }
    uint32_t columns = 0, rows = 0, width = 0, max_jump = 0, styles[8] = {0};
    bool have_styles = false;
    std::string text;
    size_t n_rows = 0, pairs = 0, steps = 0, stamps = 0, bytes = 0, bad = 0;
    while (std::getline(in, text)) {
        std::istringstream ss(text);
        std::vector<std::string> w;
        for (std::string x; ss >> x;) w.push_back(x);
        ++n_rows;
        if (w.empty()) return 1;
        const int kind = std::stoi(w[0]);
        auto s = [&](size_t k) { return std::stoll(w[k]); };
        auto u = [&](size_t k) { return (uint32_t)std::stoull(w[k]); };
        auto point = [&](size_t k) { return xrit_geo_point{(int32_t)s(k), (int32_t)s(k + 1)}; };
        bool ok = true;
        if (kind == 0 && w.size() == 5) {
            columns = u(1), rows = u(2), width = u(3), max_jump = u(4);
            if (columns < 1 || rows < 1 || columns > OVERLAY_MAX_DIM || rows > OVERLAY_MAX_DIM || width < 1 || width > OVERLAY_MAX_WIDTH) return 1;
        } else if (kind == 1 && w.size() == 15 && columns) {
            const OverlaySeg g = overlay_setup(point(1), point(3), width, max_jump, columns, rows);
            ++pairs;
            ok = g.kind == u(5);
            if (ok && g.kind == OVERLAY_DRAWN)
                ok = g.xmajor == u(6) && g.a0 == s(7) && g.b0 == s(8) && g.da == s(9) && g.db == s(10) && (!g.line || g.m0 == s(11)) &&
                     g.line == u(12) && g.steps == u(13) && overlay_touches(g, width, columns, rows) == (u(14) != 0);
        } else if (kind == 2 && w.size() == 8 && columns) {
            const OverlaySeg g = overlay_setup(point(1), point(3), width, max_jump, columns, rows);
            int64_t px = 0, py = 0;
            ok = g.kind == OVERLAY_DRAWN && u(5) < g.steps;
            if (ok) {
                overlay_step_pixel(g, u(5), px, py);
                ok = px == s(6) && py == s(7);
            }
            ++steps;
        } else if (kind == 3 && w.size() == 8 && columns) {
            OverlayStamp st{};
            const bool hit = overlay_stamp(s(1), s(2), width, columns, rows, st);
            ok = hit == (u(3) != 0);
            if (ok && hit) ok = st.x0 == u(4) && st.x1 == u(5) && st.y0 == u(6) && st.y1 == u(7) && st.x1 < columns && st.y1 < rows;
            ++stamps;
        } else if (kind == 4 && w.size() == 5) {
            ok = overlay_mix(u(1), u(2), u(3)) == u(4);
            ++bytes;
        } else if (kind == 5 && w.size() == 5) {
            ok = overlay_luma(u(1), u(2), u(3)) == u(4);
        } else if (kind == 6 && w.size() == 10 && have_styles) {
            const uint32_t cin = u(1), cout = u(2), src[3] = {u(4), u(5), u(6)};
            if ((cin != 1 && cin != 3) || (cout != 1 && cout != 3) || cin > cout) return 1;
            uint32_t out[3] = {0, 0, 0};
            overlay_blend_pixel(src, cin, u(3), styles, out, cout);
            ok = out[0] == u(7) && out[1] == u(8) && out[2] == u(9);
        } else if (kind == 7 && w.size() == 9) {
            for (size_t k = 0; k < 8; ++k) styles[k] = u(1 + k);
            have_styles = true;
        } else {
            std::fprintf(stderr, "overlay_host_check: row %zu is malformed: %s\n", n_rows - 1, text.c_str());
            return 1;
        }
        if (!ok) {
            std::fprintf(stderr, "overlay_host_check: row %zu differs: %s\n", n_rows - 1, text.c_str());
            ++bad;
        }
    }
    if (bad || !pairs || !steps || !stamps || !bytes) {
        std::fprintf(stderr, "overlay_host_check: %zu of %zu rows differ\n", bad, n_rows);
        return 1;
    }
    std::printf("overlay_host_check: %zu rows, %zu pairs, %zu steps, %zu stamps, every one the specification's: ok\n", n_rows, pairs, steps, stamps);
    return 0;
}
