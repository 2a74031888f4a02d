// image_host_check.cpp -- the image stage's rule (image_rule.h: image_mark, image_next -- the functions the kernels of
// images.hip call) row by row against a table recorded from tests/image_spec.py (tests/golden/image_rule_table.txt;
// tests/test_abi_images.py holds the table to the specification).  A program of its own for the sanitizers:
// make images-host-check.
// A row: flags n_pieces key_serial header_length header_state file_type compression bits_per_pixel columns
// pixels_per_block | first piece's length, index_in_file | key before: open key_serial lines faults | rice continued
// n_lines first_row base_lines base_faults | padded | faults | key after: open key_serial lines faults
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "image_rule.h"

using namespace xrit;

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: image_host_check TABLE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "image_host_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::string text;
    size_t rows = 0, bad = 0;
    while (std::getline(in, text)) {
        std::istringstream ss(text);
        std::vector<unsigned long long> v;
        for (unsigned long long x; ss >> x;) v.push_back(x);
        if (v.size() != 28) {
            std::fprintf(stderr, "image_host_check: row %zu has %zu columns\n", rows, v.size());
            return 1;
        }
        xrit_file_record r{};
        r.flags = (uint8_t)v[0];
        r.n_pieces = (uint32_t)v[1];
        r.key_serial = (uint32_t)v[2];
        r.header_length = (uint32_t)v[3];
        r.header_state = (uint8_t)v[4];
        r.file_type = (uint8_t)v[5];
        r.compression = (uint8_t)v[6];
        r.bits_per_pixel = (uint8_t)v[7];
        r.columns = (uint16_t)v[8];
        r.pixels_per_block = (uint8_t)v[9];
        xrit_image_key k{};
        k.open = (uint8_t)v[12];
        k.key_serial = (uint32_t)v[13];
        k.lines = (uint32_t)v[14];
        k.faults = (uint32_t)v[15];
        const ImageMark m = image_mark(r, (uint32_t)v[10], (uint32_t)v[11], k);
        const xrit_image_key a = image_next(r, m, (uint32_t)v[23]);
        const unsigned long long got[12] = {m.rice, m.continued, m.n_lines, m.first_row, m.base_lines, m.base_faults, m.padded,
                                            v[23], a.open, a.key_serial, a.lines, a.faults};
        bool same = true;
        for (int i = 0; i < 12; ++i) same = same && got[i] == v[16 + i];
        // the events are the record's flags on a rice record
        const uint32_t ev = m.rice ? ((r.flags & XRIT_FILE_BEGINS) ? IMAGE_BEGUN : 0u) | ((r.flags & XRIT_FILE_ENDS) ? IMAGE_COMPLETED : 0u) |
                                         ((r.flags & XRIT_FILE_ABORTED) ? IMAGE_ABORTED : 0u)
                                   : 0u;
        same = same && m.events == ev && a.reserved[0] == 0 && a.reserved[1] == 0 && a.reserved[2] == 0;
        if (!same) {
            std::fprintf(stderr, "image_host_check: row %zu differs: %s\n", rows, text.c_str());
            ++bad;
        }
        ++rows;
    }
    if (bad || rows == 0) {
        std::fprintf(stderr, "image_host_check: %zu of %zu records differ\n", bad, rows);
        return 1;
    }
    std::printf("image_host_check: %zu records, the mark and the key after each: ok\n", rows);
    return 0;
}
