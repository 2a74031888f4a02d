"""Python specification of the canvas stage (xrit_canvas_*, ImageCanvas) on top of file_spec and
image_spec, and a generator of segmented images for it (test infrastructure).

One call takes one files call's outputs and the outputs of the images call made on them, and places every decoded line
into the canvas of the image its segment file belongs to: a pool of `slots` canvases of `slot_bytes` each.  `process` is
the serial statement, one record at a time, and the device must equal it byte for byte: per-record outputs, slot table,
segment tables, key states, counters and pixels.  The layout of the segment identification record (type 128) is our
reading; no recorded downlink was at hand."""
import numpy as np

import file_spec as fs
import image_spec as isp

NOT_RICE, PLACED, BAD_SEGMENT, TOO_LARGE, DUPLICATE, OVERLAP, NO_SLOT, NO_PLACEMENT = range(8)
REFUSALS = ("bad_segment", "too_large", "duplicate", "overlap", "no_slot", "no_placement")      # reasons 2 .. 7
NO_ID = 0xFFFFFFFF
MAX_SLOTS = MAX_SEGMENTS = 64
NAME_BYTES = 64

FILE_DTYPE = np.dtype([
    ("slot", np.int32), ("reason", np.uint32), ("segment", np.uint32), ("start_line", np.uint32), ("start_column", np.uint32),
    ("lines_placed", np.uint32), ("lines_clipped", np.uint32), ("faults", np.uint32)])
assert FILE_DTYPE.itemsize == 32
SLOT_DTYPE = np.dtype([
    ("begun_mask", np.uint64), ("done_mask", np.uint64), ("aborted_mask", np.uint64),
    ("image_id", np.uint32), ("max_column", np.uint32), ("max_row", np.uint32), ("max_segment", np.uint32), ("pitch", np.uint32),
    ("lines_placed", np.uint32), ("faults", np.uint32), ("generation", np.uint32), ("born_call", np.uint32),
    ("touched_call", np.uint32),
    ("in_use", np.uint8), ("complete", np.uint8), ("vcid", np.uint8), ("bits", np.uint8), ("reserved", np.uint8, (4,)),
    ("name", np.uint8, (NAME_BYTES,))])
assert SLOT_DTYPE.itemsize == 136
SEGMENT_DTYPE = np.dtype([
    ("start_line", np.uint32), ("start_column", np.uint32), ("lines", np.uint32), ("columns", np.uint32), ("placed", np.uint32),
    ("faults", np.uint32), ("key_serial", np.uint32), ("apid", np.uint16), ("begun", np.uint8), ("reserved", np.uint8)])
assert SEGMENT_DTYPE.itemsize == 32
KEY_DTYPE = np.dtype([
    ("key_serial", np.uint32), ("slot", np.uint32), ("generation", np.uint32), ("segment", np.uint32), ("start_line", np.uint32),
    ("start_column", np.uint32), ("lines", np.uint32), ("placed", np.uint8), ("reserved", np.uint8, (3,))])
assert KEY_DTYPE.itemsize == 32
COUNTERS = ("calls", "canvases_begun", "canvases_completed", "segments_begun", "segments_done", "segments_aborted",
            "lines_placed", "lines_clipped", "faults") + REFUSALS
CALL_COUNTS = ("placed", "call_lines_placed", "call_lines_clipped", "call_faults", "completed")

HEAD_FIELDS = ("image_id", "segment", "start_column", "start_line", "max_segment", "max_column", "max_row")


# ---- the serial statement ------------------------------------------------------------------------------------------
def walk_header(p, columns, lines):
    """The segment identification and the annotation of a file from its first piece's payload (which the link rule says
    is the headers alone, walked to their end): file_spec.parse_header's walk.  -> (dict of HEAD_FIELDS, name bytes)."""
    p = bytes(p)
    head, name = None, None
    n = len(p)
    if n >= 16 and p[0] == 0 and fs.be(p[1:3]) == 16 and fs.be(p[4:8]) <= n:
        H, q = fs.be(p[4:8]), 16
        while q + 3 <= H:
            t, l = p[q], fs.be(p[q + 1:q + 3])
            if l < 3 or q + l > H:
                break
            if t == 128 and l == 17 and head is None:
                head = {f: fs.be(p[q + 3 + 2 * i:q + 5 + 2 * i]) for i, f in enumerate(HEAD_FIELDS)}
            if t == 4 and name is None:
                name = p[q + 3:q + l][:NAME_BYTES]
            q += l
    if head is None:
        head = dict(image_id=NO_ID, segment=1, start_column=0, start_line=0, max_segment=1, max_column=int(columns),
                    max_row=int(lines))
    return head, (name or b"").ljust(NAME_BYTES, b"\0")


def width_of(bits):
    return 1 if bits <= 8 else 2


def pitch_of(max_column, bits):
    return (max_column * width_of(bits) + 3) & ~3


def check(h, columns, lines, bits, slot_bytes):
    """The checks on the segment alone -> 0, BAD_SEGMENT or TOO_LARGE."""
    if (h["max_segment"] == 0 or h["max_segment"] > MAX_SEGMENTS or h["segment"] == 0 or h["segment"] > h["max_segment"] or
            h["max_column"] == 0 or h["max_row"] == 0 or lines == 0 or h["start_column"] + columns > h["max_column"] or
            h["start_line"] + lines > h["max_row"]):
        return BAD_SEGMENT
    if pitch_of(h["max_column"], bits) * h["max_row"] > slot_bytes:
        return TOO_LARGE
    return 0


def rects_meet(a, b):
    """(start_line, lines, start_column, columns) twice."""
    return a[0] < b[0] + b[1] and b[0] < a[0] + a[1] and a[2] < b[2] + b[3] and b[2] < a[2] + a[3]


class State:
    def __init__(self, slots, slot_bytes):
        assert 1 <= slots <= MAX_SLOTS and slot_bytes % 16 == 0
        self.n_slots, self.slot_bytes = slots, slot_bytes
        self.reset()

    def reset(self):
        self.slots = np.zeros(self.n_slots, SLOT_DTYPE)
        self.segments = np.zeros((self.n_slots, MAX_SEGMENTS), SEGMENT_DTYPE)
        self.pixels = np.zeros((self.n_slots, self.slot_bytes), np.uint8)
        self.keys = {}
        for c in COUNTERS:
            setattr(self, c, 0)

    def key(self, v, a):
        return self.keys.get((v, a), np.zeros(1, KEY_DTYPE)[0])

    def read(self, slot):
        """The slot's pitch x max_row bytes."""
        s = self.slots[slot]
        return self.pixels[slot, :int(s["pitch"]) * int(s["max_row"])].copy()

    def image(self, slot):
        """The slot's canvas as samples (max_row, max_column)."""
        s = self.slots[slot]
        w = width_of(int(s["bits"]))
        rows = self.read(slot).reshape(int(s["max_row"]), int(s["pitch"]))[:, :int(s["max_column"]) * w]
        return (rows if w == 1 else np.ascontiguousarray(rows).view("<u2")).astype(np.int64)

    def release(self, slot):
        """The slot free again: all zero, but for the generation, which goes up by one."""
        g = int(self.slots[slot]["generation"])
        self.slots[slot] = np.zeros(1, SLOT_DTYPE)[0]
        self.slots[slot]["generation"] = (g + 1) & 0xFFFFFFFF
        self.segments[slot] = 0
        self.pixels[slot] = 0

    def counters(self):
        return {c: int(getattr(self, c)) for c in COUNTERS}


def begin(state, r, h, name, call):
    """The rule for a BEGINS rice record with the segment h -> (reason, slot).  On PLACED the slot's identity (if it is
    born), begun_mask and the segment's rectangle are set."""
    bits, columns, lines, vcid = int(r["bits_per_pixel"]), int(r["columns"]), int(r["lines"]), int(r["vcid"])
    reason = check(h, columns, lines, bits, state.slot_bytes)
    if reason:
        return reason, -1
    bit = 1 << (h["segment"] - 1)
    found = -1
    if h["image_id"] != NO_ID:
        for i, s in enumerate(state.slots):
            if (s["in_use"] and int(s["vcid"]) == vcid and int(s["image_id"]) == h["image_id"] and
                    int(s["max_column"]) == h["max_column"] and int(s["max_row"]) == h["max_row"] and
                    int(s["max_segment"]) == h["max_segment"] and int(s["bits"]) == bits):
                found = i
                break
    if found >= 0:
        s = state.slots[found]
        if int(s["begun_mask"]) & bit:
            return DUPLICATE, -1
        mine = (h["start_line"], lines, h["start_column"], columns)
        for g in state.segments[found]:
            if g["begun"] and rects_meet(mine, (int(g["start_line"]), int(g["lines"]), int(g["start_column"]), int(g["columns"]))):
                return OVERLAP, -1
    else:
        free = np.flatnonzero(state.slots["in_use"] == 0)
        if not len(free):
            return NO_SLOT, -1
        found = int(free[0])
        s = state.slots[found]
        s["in_use"], s["vcid"], s["bits"], s["image_id"] = 1, vcid, bits, h["image_id"]
        s["max_column"], s["max_row"], s["max_segment"] = h["max_column"], h["max_row"], h["max_segment"]
        s["pitch"], s["born_call"] = pitch_of(h["max_column"], bits), call
        s["name"] = np.frombuffer(name, np.uint8)
        state.canvases_begun += 1
    s["begun_mask"] = int(s["begun_mask"]) | bit
    g = state.segments[found][h["segment"] - 1]
    g["begun"], g["start_line"], g["start_column"], g["lines"], g["columns"] = 1, h["start_line"], h["start_column"], lines, columns
    g["key_serial"], g["apid"] = int(r["key_serial"]), int(r["apid"])
    state.segments_begun += 1
    return PLACED, found


def line_fits(ln, k, slot, n_image_bytes):
    """Whether a line of a placed record (key state k) is copied: its row inside the segment's declared lines, its
    samples inside the image bytes, and its end inside the canvas (the rule guarantees the last two for the outputs of
    the stages in front)."""
    off, length, row = int(ln["offset"]), int(ln["length"]), int(ln["row"])
    if row >= int(k["lines"]) or off + length > n_image_bytes:
        return None
    pitch = int(slot["pitch"])
    dst = (int(k["start_line"]) + row) * pitch + int(k["start_column"]) * width_of(int(slot["bits"]))
    return dst if dst + length <= pitch * int(slot["max_row"]) else None


def process(state, files_out, images_out, table=None):
    """One call on a files call's (bytes, pieces, records, ...) and the images call's (bytes, lines, image files, ...) on
    them.  Returns (canvas files FILE_DTYPE, one per record; the slot table after the call, SLOT_DTYPE; summary: a dict
    with the call's counts (CALL_COUNTS) and the state's counters after it).  table, a list: one row per record the
    rule looked at (the host check's table)."""
    data, pieces, files = files_out[:3]
    img, lines, ifiles = images_out[:3]
    raw = np.asarray(data, np.uint8).tobytes()
    img = np.asarray(img, np.uint8)
    out = np.zeros(len(files), FILE_DTYPE)
    state.calls += 1
    call = state.calls
    counts = dict.fromkeys(CALL_COUNTS, 0)
    was_complete = state.slots["complete"].copy()
    for f, r in enumerate(files):
        fl, key = ifiles[f], (int(r["vcid"]), int(r["apid"]))
        begins, rice = bool(int(r["flags"]) & fs.BEGINS), bool(fl["rice"])
        if not begins and not rice:
            continue
        k = np.zeros(1, KEY_DTYPE)[0]
        k["key_serial"] = r["key_serial"]
        h = dict.fromkeys(HEAD_FIELDS, 0)
        if begins:
            reason, slot = NOT_RICE, -1
            if rice:
                pc = pieces[int(r["first_piece"])]
                a, b = int(pc["offset"]), int(pc["offset"]) + int(pc["length"])
                h, name = walk_header(raw[a:b] if b <= len(raw) else b"", r["columns"], r["lines"])
                reason, slot = begin(state, r, h, name, call)
            if reason == PLACED:
                k["slot"], k["generation"], k["segment"], k["placed"] = slot, state.slots[slot]["generation"], h["segment"], 1
                k["start_line"], k["start_column"], k["lines"] = h["start_line"], h["start_column"], r["lines"]
            state.keys[key] = k
        else:
            k = state.key(*key)
            ok = (k["placed"] and int(k["key_serial"]) == int(r["key_serial"]) and int(k["slot"]) < state.n_slots and
                  state.slots[int(k["slot"])]["in_use"] and int(state.slots[int(k["slot"])]["generation"]) == int(k["generation"]))
            reason, slot = (PLACED, int(k["slot"])) if ok else (NO_PLACEMENT, -1)
        if table is not None:
            table.append([2, int(r["flags"]), int(rice), key[0], key[1], int(r["key_serial"]), int(r["bits_per_pixel"]), int(r["columns"]),
                          int(r["lines"])] + [h[c] for c in HEAD_FIELDS] + [reason, slot + 1])
        if not rice:
            continue
        o = out[f]
        o["reason"], o["slot"] = reason, slot
        if reason != PLACED:
            setattr(state, REFUSALS[reason - 2], getattr(state, REFUSALS[reason - 2]) + 1)
            continue
        s, g = state.slots[slot], state.segments[slot][int(k["segment"]) - 1]
        o["segment"], o["start_line"], o["start_column"] = k["segment"], k["start_line"], k["start_column"]
        placed = clipped = faults = 0
        for ln in lines[int(fl["first_line"]):int(fl["first_line"]) + int(fl["n_lines"])]:
            dst = line_fits(ln, k, s, len(img))
            if dst is None:
                clipped += 1
                continue
            a = int(ln["offset"])
            state.pixels[slot, dst:dst + int(ln["length"])] = img[a:a + int(ln["length"])]
            placed += 1
            faults += int(ln["status"]) != 0
        o["lines_placed"], o["lines_clipped"], o["faults"] = placed, clipped, faults
        g["placed"] += placed
        g["faults"] += faults
        s["touched_call"] = call
        bit = 1 << (int(k["segment"]) - 1)
        if int(r["flags"]) & fs.ENDS:
            s["done_mask"] = int(s["done_mask"]) | bit
            state.segments_done += 1
        if int(r["flags"]) & fs.ABORTED:
            s["aborted_mask"] = int(s["aborted_mask"]) | bit
            state.segments_aborted += 1
        counts["placed"] += 1
        counts["call_lines_placed"] += placed
        counts["call_lines_clipped"] += clipped
        counts["call_faults"] += faults
    for i, s in enumerate(state.slots):
        if not s["in_use"]:
            continue
        s["lines_placed"], s["faults"] = int(state.segments[i]["placed"].sum()), int(state.segments[i]["faults"].sum())
        s["complete"] = int(int(s["done_mask"]) == (1 << int(s["max_segment"])) - 1)
        counts["completed"] += int(s["complete"] and not was_complete[i])
    state.canvases_completed += counts["completed"]
    state.lines_placed += counts["call_lines_placed"]
    state.lines_clipped += counts["call_lines_clipped"]
    state.faults += counts["call_faults"]
    summary = dict(counts)
    summary.update(state.counters())
    return out, state.slots.copy(), summary


def table_reset(table, slots, slot_bytes):
    """The table's row for a fresh handle (or a reset)."""
    table.append([0, slots, slot_bytes] + [0] * 15)


def table_release(table, slot):
    table.append([1, slot] + [0] * 16)


# ---- generator ------------------------------------------------------------------------------------------------------
def segment_record(image_id, segment, start_column, start_line, max_segment, max_column, max_row):
    """The body of a segment identification record (type 128; fs.record makes it 17 bytes long)."""
    return b"".join(int(x).to_bytes(2, "big") for x in (image_id, segment, start_column, start_line, max_segment, max_column, max_row))


def segment_file(rng, part, n, J, ident=None, name=None, kinds=isp.rs.KINDS, spoil=None, declared_lines=None, extra=None):
    """A rice-coded file of the samples `part` (rows, cols) with the records `ident` (segment_record's arguments) and
    `name` in its headers -> (file bytes, cuts) as isp.image_file gives them: the headers alone in the first packet, one
    coded line in each packet behind it.  declared_lines: what the image structure record says instead of the rows."""
    rows, cols = part.shape
    coded = [isp.rs.encode(row, n, J) for row in part]
    if spoil is not None:
        coded = [spoil(rng, c) for c in coded]
    more = list(extra or [])
    if ident is not None:
        more.append((128, segment_record(*ident)))
    if name is not None:
        more.append((4, name))
    head = fs.lrit_file(b"", image=(n, cols, rows if declared_lines is None else declared_lines, 1), extra=more,
                        rice=(int(rng.integers(0, 65536)), J, 1), declared_data_bits=8 * sum(len(c) for c in coded))
    cuts = [int(c) for c in np.cumsum([len(head)] + [len(c) for c in coded])[:-1]]
    return head + b"".join(coded), cuts


def samples(rng, n, J, cols, rows, kinds=("uniform", "walk3")):
    return np.stack([isp.rs.samples(rng, kinds[int(rng.integers(0, len(kinds)))], n, J, cols) for _ in range(rows)])


def split_image(rng, img, n, J, image_id, keys, row_cuts, col_cuts=(), name=None, first_segment=1):
    """The image cut into a grid of segments at the given rows and columns, numbered row by row from first_segment, the
    segment files dealt over the keys in turn -> items for isp.stream_of."""
    R, Cc = img.shape
    re, ce = [0] + list(row_cuts) + [R], [0] + list(col_cuts) + [Cc]
    total = (len(re) - 1) * (len(ce) - 1)
    items, seg = [], first_segment
    for a, b in zip(re[:-1], re[1:]):
        for c, d in zip(ce[:-1], ce[1:]):
            data, cuts = segment_file(rng, img[a:b, c:d], n, J, ident=(image_id, seg, c, a, total, Cc, R), name=name)
            items.append((keys[(seg - 1) % len(keys)], data, cuts, 8190))
            seg += 1
    return items


def run_both(fst, ist, part):
    """The specification's files call and images call on a piece of stream -> (files_out, images_out)."""
    files_out = isp.run_files(fst, part)
    return files_out, isp.process(ist, *files_out[:3])
