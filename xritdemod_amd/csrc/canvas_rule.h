// canvas_rule.h -- the canvas stage's rule (include/xritdemod_amd.h, "Image canvases"; tests/canvas_spec.py states the
// same) as plain integer functions for the device (canvas.hip) and the host (canvas_host_check.cpp replays a table
// recorded from the specification through them).  The predicates are the kernels'; canvas_begin is their serial
// composition: the rule kernel evaluates the same predicates with a lane per slot and a lane per segment.
#pragma once

#include <cstdint>

#include "../../include/xritdemod_amd.h"

#if defined(__HIPCC__)
#define XRIT_HD __host__ __device__
#else
#define XRIT_HD
#endif

namespace xrit {

// what the header walk finds in a file's first piece
struct CanvasHead {
    uint32_t image_id, segment, start_column, start_line, max_segment, max_column, max_row;
    uint32_t name_len;              // bytes of the annotation text kept (0 .. 64) ...
    uint64_t name_off;              // ... and where they lie in the call's bytes
};

// a record's placement: what place and commit need of the rule's decision
struct CanvasPlace {
    int32_t slot;
    uint32_t reason, segment, start_line, start_column, lines;
};

XRIT_HD inline uint32_t canvas_be16(const unsigned char *p) { return (uint32_t)p[0] << 8 | p[1]; }
XRIT_HD inline uint32_t canvas_width(uint32_t bits) { return bits <= 8 ? 1u : 2u; }
XRIT_HD inline uint32_t canvas_pitch(uint32_t max_column, uint32_t bits) { return (max_column * canvas_width(bits) + 3u) & ~3u; }

// The headers in a first piece p[0 .. n) at offset `base` of the call's bytes, walked as the file stage walks them: the
// first record 128 of length 17 and the first annotation record.  Without record 128: one segment, the record's size.
XRIT_HD inline CanvasHead canvas_walk(const unsigned char *p, uint32_t n, uint64_t base, uint32_t columns, uint32_t lines)
{
    CanvasHead h{};
    bool seg = false, name = false;
    if (n >= 16 && p[0] == 0 && canvas_be16(p + 1) == 16) {
        const uint32_t H = canvas_be16(p + 4) << 16 | canvas_be16(p + 6);
        uint32_t q = 16;
        while (H <= n && q + 3 <= H) {
            const uint32_t t = p[q], l = canvas_be16(p + q + 1);
            if (l < 3 || q + l > H) break;
            if (t == 128 && l == 17 && !seg) {
                seg = true;
                h.image_id = canvas_be16(p + q + 3);
                h.segment = canvas_be16(p + q + 5);
                h.start_column = canvas_be16(p + q + 7);
                h.start_line = canvas_be16(p + q + 9);
                h.max_segment = canvas_be16(p + q + 11);
                h.max_column = canvas_be16(p + q + 13);
                h.max_row = canvas_be16(p + q + 15);
            }
            if (t == 4 && !name) {
                name = true;
                h.name_off = base + q + 3;
                h.name_len = l - 3 < 64u ? l - 3 : 64u;
            }
            q += l;
        }
    }
    if (!seg) {
        h.image_id = XRIT_CANVAS_NO_ID;
        h.segment = h.max_segment = 1;
        h.max_column = columns;
        h.max_row = lines;
    }
    return h;
}

// the checks on the segment alone: 0, BAD_SEGMENT or TOO_LARGE
XRIT_HD inline uint32_t canvas_check(const CanvasHead &h, uint32_t columns, uint32_t lines, uint32_t bits, uint64_t slot_bytes)
{
    if (h.max_segment == 0 || h.max_segment > XRIT_CANVAS_MAX_SEGMENTS || h.segment == 0 || h.segment > h.max_segment ||
        h.max_column == 0 || h.max_row == 0 || lines == 0 || h.start_column + columns > h.max_column || h.start_line + lines > h.max_row)
        return XRIT_CANVAS_BAD_SEGMENT;
    if ((uint64_t)canvas_pitch(h.max_column, bits) * h.max_row > slot_bytes) return XRIT_CANVAS_TOO_LARGE;
    return 0;
}

// the identity of a canvas: the apid is deliberately not part of it
XRIT_HD inline bool canvas_same(bool in_use, uint32_t s_vcid, uint32_t s_bits, uint32_t s_image_id, uint32_t s_max_column,
                                uint32_t s_max_row, uint32_t s_max_segment, uint32_t vcid, uint32_t bits, const CanvasHead &h)
{
    return in_use && h.image_id != XRIT_CANVAS_NO_ID && s_vcid == vcid && s_image_id == h.image_id && s_max_column == h.max_column &&
           s_max_row == h.max_row && s_max_segment == h.max_segment && s_bits == bits;
}

XRIT_HD inline bool canvas_rects_meet(const xrit_canvas_segment &g, uint32_t start_line, uint32_t lines, uint32_t start_column,
                                      uint32_t columns)
{
    return g.begun && start_line < g.start_line + g.lines && g.start_line < start_line + lines &&
           start_column < g.start_column + g.columns && g.start_column < start_column + columns;
}

// a rice record without BEGINS goes on where its key's state points, if that canvas is still the same
XRIT_HD inline bool canvas_continues(const xrit_canvas_key_state &k, uint32_t key_serial, const xrit_canvas_slot *slots, uint32_t n_slots)
{
    return k.placed && k.key_serial == key_serial && k.slot < n_slots && slots[k.slot].in_use && slots[k.slot].generation == k.generation;
}

// Whether a line of a placed record is copied, and where to: its row inside the segment's declared lines, its samples
// inside the image bytes, its end inside the canvas (the rule guarantees the last two for what the stages in front
// emit; they keep every access inside the buffers whatever is handed over).
XRIT_HD inline bool canvas_line_dst(uint64_t offset, uint32_t length, uint32_t row, const CanvasPlace &pl, uint32_t pitch,
                                    uint32_t max_row, uint32_t bits, uint64_t n_image_bytes, uint64_t &dst)
{
    if (row >= pl.lines || offset > n_image_bytes || length > n_image_bytes - offset) return false;
    dst = (uint64_t)(pl.start_line + row) * pitch + (uint64_t)pl.start_column * canvas_width(bits);
    return dst + length <= (uint64_t)pitch * max_row;
}

XRIT_HD inline xrit_canvas_key_state canvas_key_of(uint32_t key_serial, const CanvasPlace &pl, uint32_t generation)
{
    xrit_canvas_key_state k{};
    k.key_serial = key_serial;
    if (pl.reason == XRIT_CANVAS_PLACED) {
        k.slot = (uint32_t)pl.slot;
        k.generation = generation;
        k.segment = pl.segment;
        k.start_line = pl.start_line;
        k.start_column = pl.start_column;
        k.lines = pl.lines;
        k.placed = 1;
    }
    return k;
}

// The rule for a BEGINS rice record, serially over the slot table and the segment tables ([n_slots][64]).  On PLACED the
// slot's identity (if it is born: *born), begun_mask and the segment's entry are set; the name is the caller's.
XRIT_HD inline CanvasPlace canvas_begin(xrit_canvas_slot *slots, xrit_canvas_segment *segs, uint32_t n_slots, uint64_t slot_bytes,
                                        uint32_t vcid, uint32_t apid, uint32_t key_serial, uint32_t bits, uint32_t columns, uint32_t lines,
                                        const CanvasHead &h, uint32_t call, bool *born)
{
    CanvasPlace pl{-1, canvas_check(h, columns, lines, bits, slot_bytes), 0, 0, 0, 0};
    *born = false;
    if (pl.reason) return pl;
    int found = -1, free_slot = -1;
    for (uint32_t i = 0; i < n_slots; ++i) {
        const xrit_canvas_slot &s = slots[i];
        if (found < 0 && canvas_same(s.in_use, s.vcid, s.bits, s.image_id, s.max_column, s.max_row, s.max_segment, vcid, bits, h)) found = (int)i;
        if (free_slot < 0 && !s.in_use) free_slot = (int)i;
    }
    const uint64_t bit = 1ull << (h.segment - 1);
    if (found >= 0) {
        if (slots[found].begun_mask & bit) { pl.reason = XRIT_CANVAS_DUPLICATE; return pl; }
        for (uint32_t j = 0; j < XRIT_CANVAS_MAX_SEGMENTS; ++j)
            if (canvas_rects_meet(segs[(size_t)found * XRIT_CANVAS_MAX_SEGMENTS + j], h.start_line, lines, h.start_column, columns)) {
                pl.reason = XRIT_CANVAS_OVERLAP;
                return pl;
            }
    } else {
        if (free_slot < 0) { pl.reason = XRIT_CANVAS_NO_SLOT; return pl; }
        found = free_slot;
        xrit_canvas_slot &s = slots[found];
        s.in_use = 1;
        s.vcid = (uint8_t)vcid;
        s.bits = (uint8_t)bits;
        s.image_id = h.image_id;
        s.max_column = h.max_column;
        s.max_row = h.max_row;
        s.max_segment = h.max_segment;
        s.pitch = canvas_pitch(h.max_column, bits);
        s.born_call = call;
        *born = true;
    }
    slots[found].begun_mask |= bit;
    xrit_canvas_segment &g = segs[(size_t)found * XRIT_CANVAS_MAX_SEGMENTS + h.segment - 1];
    g.begun = 1;
    g.start_line = h.start_line;
    g.start_column = h.start_column;
    g.lines = lines;
    g.columns = columns;
    g.key_serial = key_serial;
    g.apid = (uint16_t)apid;
    pl = CanvasPlace{found, XRIT_CANVAS_PLACED, h.segment, h.start_line, h.start_column, lines};
    return pl;
}

}  // namespace xrit
