// overlay_files.h -- the plain parts of --overlay / --graticule: the options on the command line, the text of a polyline
// file, the colours.  No library call: checked by `make host-program-check`.  (The image file is jpeg_files.h's binary PNM.)
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

// the fixed colours {r, g, b, alpha}: coastlines on layer 0 in opaque yellow, the graticule on layer 1 in cyan at 160 / 255
constexpr uint8_t OVERLAY_COAST_RGBA[4] = {255, 255, 0, 255};
constexpr uint8_t OVERLAY_GRATICULE_RGBA[4] = {0, 255, 255, 160};
constexpr double OVERLAY_DENSIFY_DEG = 0.05;        // polylines and graticule lines get a vertex at least this often

// the options: --overlay FILE, --graticule DEG, --overlay-width W.  flag(): 1 when `a` is one of them and `v` (the next
// token, or nullptr) was its value, 0 when `a` is another option, -1 when it is refused (*why says it); refused(): why the
// whole line is refused, or nullptr
struct OverlayOptions {
    std::string file;               // empty: no coastlines
    double graticule = 0.0;         // 0: none
    unsigned width = 1;
    bool width_given = false;
    bool on() const { return !file.empty() || graticule > 0.0; }
    int flag(const std::string &a, const char *v, std::string *why)
    {
        if (a != "--overlay" && a != "--graticule" && a != "--overlay-width") return 0;
        if (!v || (v[0] == '-' && v[1] == '-')) { *why = a + " needs a value\n"; return -1; }      // (the next option is no value)
        char *end = nullptr;
        if (a == "--overlay") {
            if (!*v) { *why = "--overlay needs a file name\n"; return -1; }
            file = v;
        } else if (a == "--graticule") {
            const double d = std::strtod(v, &end);
            if (end == v || *end != '\0' || !(d >= 0.1 && d <= 90.0)) { *why = std::string("--graticule ") + v + ": 0.1..90 degrees\n"; return -1; }
            graticule = d;
        } else {
            const long w = std::strtol(v, &end, 10);
            if (end == v || *end != '\0' || w < 1 || w > 8) { *why = std::string("--overlay-width ") + v + ": 1..8\n"; return -1; }
            width = (unsigned)w;
            width_given = true;
        }
        return 1;
    }
    const char *refused(bool products_given) const
    {
        if (on() && !products_given) return "--overlay / --graticule need --products\n";
        if (width_given && !on()) return "--overlay-width needs --overlay or --graticule\n";
        return nullptr;
    }
};

// GMT-style multi-segment text: one `lon lat` pair per line in degrees; a line that is blank or begins '>' or '#' is a break
// (NaN in both).  Returns 0, or the number (from 1) of the first line that is neither.
inline size_t parse_polylines(const std::string &text, std::vector<double> &lon, std::vector<double> &lat)
{
    lon.clear();
    lat.clear();
    size_t line = 0, at = 0;
    while (at <= text.size()) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        if (end == text.size() && at == end) break;                 // nothing behind the last newline
        ++line;
        std::string t = text.substr(at, end - at);
        at = end + 1;
        const size_t a = t.find_first_not_of(" \t\r"), b = t.find_last_not_of(" \t\r");
        if (a == std::string::npos || t[a] == '>' || t[a] == '#') {
            lon.push_back(NAN);
            lat.push_back(NAN);
            continue;
        }
        t = t.substr(a, b - a + 1);
        char *e1 = nullptr, *e2 = nullptr;
        const double x = std::strtod(t.c_str(), &e1);
        if (e1 == t.c_str() || (*e1 != ' ' && *e1 != '\t')) return line;
        const double y = std::strtod(e1, &e2);
        if (e2 == e1 || *e2 != '\0' || !std::isfinite(x) || !std::isfinite(y)) return line;
        lon.push_back(x);
        lat.push_back(y);
    }
    return 0;
}
