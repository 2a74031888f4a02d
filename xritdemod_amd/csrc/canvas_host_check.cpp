// canvas_host_check.cpp -- the canvas stage's rule (canvas_rule.h: canvas_check, canvas_same, canvas_rects_meet,
// canvas_begin, canvas_continues, canvas_key_of -- the functions the kernels of canvas.hip call) replayed over a table
// recorded from tests/canvas_spec.py (tests/golden/canvas_rule_table.txt; tests/test_abi_canvas.py holds the table to the
// specification).  A program of its own for the sanitizers: make canvas-host-check.
// A row has 18 columns.  0 slots slot_bytes: a fresh handle.  1 slot: that slot released.  2: a record the rule looked
// at: flags rice vcid apid key_serial bits_per_pixel columns lines | image_id segment start_column start_line max_segment
// max_column max_row (what the header walk found) | the reason and the slot + 1 the specification gave.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "canvas_rule.h"

using namespace xrit;

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: canvas_host_check TABLE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "canvas_host_check: cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<xrit_canvas_slot> slots(XRIT_CANVAS_MAX_SLOTS);
    std::vector<xrit_canvas_segment> segs((size_t)XRIT_CANVAS_MAX_SLOTS * XRIT_CANVAS_MAX_SEGMENTS);
    std::map<std::pair<unsigned, unsigned>, xrit_canvas_key_state> keys;
    uint32_t n_slots = 0;
    uint64_t slot_bytes = 0;
    std::string text;
    size_t rows = 0, records = 0, bad = 0;
    while (std::getline(in, text)) {
        std::istringstream ss(text);
        std::vector<unsigned long long> v;
        for (unsigned long long x; ss >> x;) v.push_back(x);
        if (v.size() != 18 || v[0] > 2) {
            std::fprintf(stderr, "canvas_host_check: row %zu has %zu columns or an unknown kind\n", rows, v.size());
            return 1;
        }
        ++rows;
        if (v[0] == 0) {
            if (v[1] < 1 || v[1] > XRIT_CANVAS_MAX_SLOTS) return 1;
            n_slots = (uint32_t)v[1];
            slot_bytes = v[2];
            std::memset(slots.data(), 0, slots.size() * sizeof slots[0]);
            std::memset(segs.data(), 0, segs.size() * sizeof segs[0]);
            keys.clear();
            continue;
        }
        if (v[0] == 1) {
            if (v[1] >= n_slots) return 1;
            const uint32_t g = slots[v[1]].generation + 1;
            std::memset(&slots[v[1]], 0, sizeof slots[0]);
            slots[v[1]].generation = g;
            std::memset(&segs[v[1] * XRIT_CANVAS_MAX_SEGMENTS], 0, XRIT_CANVAS_MAX_SEGMENTS * sizeof segs[0]);
            continue;
        }
        ++records;
        const bool begins = v[1] & XRIT_FILE_BEGINS, rice = v[2] != 0;
        const uint32_t vcid = (uint32_t)v[3], apid = (uint32_t)v[4], serial = (uint32_t)v[5];
        CanvasPlace pl{-1, XRIT_CANVAS_NOT_RICE, 0, 0, 0, 0};
        if (begins) {
            uint32_t generation = 0;
            if (rice) {
                CanvasHead h{};
                h.image_id = (uint32_t)v[9];
                h.segment = (uint32_t)v[10];
                h.start_column = (uint32_t)v[11];
                h.start_line = (uint32_t)v[12];
                h.max_segment = (uint32_t)v[13];
                h.max_column = (uint32_t)v[14];
                h.max_row = (uint32_t)v[15];
                bool born = false;
                pl = canvas_begin(slots.data(), segs.data(), n_slots, slot_bytes, vcid, apid, serial, (uint32_t)v[6], (uint32_t)v[7],
                                  (uint32_t)v[8], h, 0, &born);
                if (pl.reason == XRIT_CANVAS_PLACED) generation = slots[pl.slot].generation;
            }
            keys[{vcid, apid}] = canvas_key_of(serial, pl, generation);
        } else {
            const auto it = keys.find({vcid, apid});
            const xrit_canvas_key_state k = it == keys.end() ? xrit_canvas_key_state{} : it->second;
            if (canvas_continues(k, serial, slots.data(), n_slots))
                pl = CanvasPlace{(int32_t)k.slot, XRIT_CANVAS_PLACED, k.segment, k.start_line, k.start_column, k.lines};
            else
                pl.reason = XRIT_CANVAS_NO_PLACEMENT;
        }
        if (pl.reason != v[16] || (unsigned long long)(pl.slot + 1) != v[17]) {
            std::fprintf(stderr, "canvas_host_check: row %zu differs (reason %u, slot %d): %s\n", rows - 1, pl.reason, pl.slot, text.c_str());
            ++bad;
        }
    }
    if (bad || records == 0) {
        std::fprintf(stderr, "canvas_host_check: %zu of %zu records differ\n", bad, records);
        return 1;
    }
    std::printf("canvas_host_check: %zu rows, %zu records, the reason and the slot of each: ok\n", rows, records);
    return 0;
}
