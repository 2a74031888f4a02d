"""Constructed streams for the canvas stage's tests (test infrastructure on top of canvas_spec): each returns what a test
needs to drive the specification and the device alike.  The streams that go through the packet, file and image stages hold
images of at most 64 x 48 pixels for slots of 16 KiB, but for real_size_stream (2784 x 140 at 10 bit, 1051 x 130); the calls
built by hand (direct_call) go up to lines of 131070 bytes, records of 135 lines and images of 64 segments."""
import copy

import numpy as np

import canvas_spec as cs
import file_spec as fs
import image_spec as isp

SLOT_BYTES = 16384


def mixed_stream(seed=60):
    """An 8-bit image of three segments on one key (64 x 48, names its canvas), a 10-bit 2 x 2 image on two keys whose
    right half starts at column 13 (26 bytes: 2 mod 4), a one-column image of two segments, an 8-bit image cut at columns
    5 and 18 (odd and 2 mod 4 byte offsets, lengths 5, 13 and 15: the byte path and its tail), a rice file without
    record 128 and a file that is no image -> (stream, images {image_id: (vcid, bits, samples)})."""
    rng = np.random.default_rng(seed)
    a = cs.samples(rng, 8, 16, 64, 48)
    b = cs.samples(rng, 10, 32, 40, 20)
    c = cs.samples(rng, 8, 8, 1, 5)
    d = cs.samples(rng, 8, 8, 33, 6)
    items = cs.split_image(rng, a, 8, 16, 7, [(2, 100)], [16, 32], name=b"IMG A/8 bit.lrit")
    items += cs.split_image(rng, b, 10, 32, 9, [(2, 101), (2, 102)], [10], [13], name=b"B-10")
    items += cs.split_image(rng, c, 8, 8, 11, [(5, 100)], [2])
    items += cs.split_image(rng, d, 8, 8, 12, [(5, 101), (5, 102)], [], [5, 18], name=bytes(range(48, 48 + 70)))
    e, data, cuts = isp.image_file(rng, 12, 16, 9, 3)
    items.append(((5, 103), data, cuts, 8190))
    items.append(((2, 100), fs.lrit_file(rng.integers(0, 256, 300, dtype=np.uint8).tobytes(), file_type=2), None, 100))
    images = {7: (2, 8, a), 9: (2, 10, b), 11: (5, 8, c), 12: (5, 8, d), cs.NO_ID: (5, 12, e)}
    return isp.stream_of(rng, items, seq_start=16370), images


def one_key_three_segments(seed=61):
    rng = np.random.default_rng(seed)
    img = cs.samples(rng, 8, 16, 30, 12)
    return isp.stream_of(rng, cs.split_image(rng, img, 8, 16, 3, [(1, 7)], [4, 9], name=b"three")), img


def two_by_two_on_two_keys(seed=62):
    rng = np.random.default_rng(seed)
    img = cs.samples(rng, 11, 8, 21, 10)
    return isp.stream_of(rng, cs.split_image(rng, img, 11, 8, 4, [(1, 8), (1, 9)], [6], [9])), img


BAD_IDENTS = (          # (image_id, segment, start_column, start_line, max_segment, max_column, max_row), declared lines
    ((20, 1, 0, 0, 0, 8, 2), None), ((20, 1, 0, 0, 65, 8, 2), None), ((20, 0, 0, 0, 2, 8, 2), None), ((20, 3, 0, 0, 2, 8, 2), None),
    ((20, 1, 0, 0, 2, 0, 2), None), ((20, 1, 0, 0, 2, 8, 0), None), ((20, 1, 0, 0, 2, 8, 2), 0), ((20, 1, 1, 0, 2, 8, 2), None),
    ((20, 1, 0, 1, 2, 8, 2), None))


def reasons_stream(seed=63):
    """One file per key (1, 10 + i), so the records of a call lie in this order -> (stream, the reasons of the BEGINS
    records in that order): every clause of BAD_SEGMENT, TOO_LARGE, a segment placed, its DUPLICATE, an OVERLAP, a file
    without record 128, one whose record 128 has the wrong length, one with rows beyond its declared lines, and the
    segment that completes the image."""
    rng = np.random.default_rng(seed)
    files, want = [], []

    def add(part, ident, reason, **kw):
        files.append(cs.segment_file(rng, part, 8, 8, ident=ident, **kw))
        want.append(reason)

    small = lambda rows=2: cs.samples(rng, 8, 8, 8, rows)
    for ident, declared in BAD_IDENTS:
        add(small(), ident, cs.BAD_SEGMENT, declared_lines=declared)
    add(small(), (21, 1, 0, 0, 1, 200, 100), cs.TOO_LARGE)
    top, bottom = small(4), small(4)
    add(top, (50, 1, 0, 0, 2, 8, 8), cs.PLACED)
    add(small(4), (50, 1, 0, 0, 2, 8, 8), cs.DUPLICATE)
    add(small(4), (50, 2, 0, 2, 2, 8, 8), cs.OVERLAP)
    add(small(3), None, cs.PLACED)
    add(small(3), None, cs.PLACED, extra=[(128, bytes(12))])
    add(small(4), (51, 1, 0, 0, 1, 8, 2), cs.PLACED, declared_lines=2)
    add(bottom, (50, 2, 0, 4, 2, 8, 8), cs.PLACED)
    items = [((1, 10 + i), data, cuts, 8190) for i, (data, cuts) in enumerate(files)]
    return isp.stream_of(rng, items), want, np.concatenate([top, bottom])


def no_slot_stream(seed=64):
    """Three images of two segments each, their first segments only, on three keys: with two slots the third finds none."""
    rng = np.random.default_rng(seed)
    items = []
    for i in range(3):
        data, cuts = cs.segment_file(rng, cs.samples(rng, 8, 8, 8, 3), 8, 8, ident=(70 + i, 1, 0, 0, 2, 8, 6))
        items.append(((3, i), data, cuts, 8190))
    return isp.stream_of(rng, items)


def aborted_stream(seed=65):
    """Three segments on one key, a packet removed inside the second, then the second once more -> (stream, image, the
    rows of the second segment that were placed before the gap)."""
    rng = np.random.default_rng(seed)
    img = cs.samples(rng, 8, 16, 20, 12)
    items = cs.split_image(rng, img, 8, 16, 30, [(4, 40)], [4, 8])
    items.append(items[1])
    stream = isp.stream_of(rng, items)
    hit = [i for i, e in enumerate(stream) if e[2][2] == 1 and e[2][3] == 3][0]          # the second file's third packet: row 2
    return fs.remove(stream, hit), img, 2


def release_streams(seed=66):
    """(first call, second call, the new image): an image of two segments on two keys, begun in the first call and
    continued in the second, where a new one-segment image begins on a third key."""
    rng = np.random.default_rng(seed)
    old = cs.samples(rng, 8, 8, 16, 8)
    items = cs.split_image(rng, old, 8, 8, 40, [(6, 1), (6, 2)], [4])
    a1, a2 = isp.stream_of(rng, items[:1]), isp.stream_of(rng, items[1:])          # five packets each: the headers, four rows
    new = cs.samples(rng, 8, 8, 10, 3)
    data, cuts = cs.segment_file(rng, new, 8, 8, ident=(41, 1, 3, 1, 1, 16, 8))
    b = isp.stream_of(rng, [((6, 3), data, cuts, 8190)])
    return a1[:3] + a2[:3], a1[3:] + a2[3:] + b, new


def faulted_stream(seed=68):
    """A segment with a truncated line (status 1; the seed is one whose line keeps decoded blocks in front of the
    fault) -> stream."""
    rng = np.random.default_rng(seed)
    n = [0]

    def spoil(r, line):
        n[0] += 1
        return isp.rs.truncate(r, line) if n[0] == 2 else line

    data, cuts = cs.segment_file(rng, cs.samples(rng, 8, 16, 40, 4), 8, 16, ident=(60, 1, 0, 0, 1, 40, 4), spoil=spoil)
    return isp.stream_of(rng, [((7, 1), data, cuts, 8190)])


# ---- calls built by hand ----------------------------------------------------------------------------------------------
def seg(key, ident, bits, columns, lines, entries, key_serial=0, flags=fs.BEGINS | fs.ENDS, name=None, rice=True):
    """One record of a hand-built call.  ident: segment_record's arguments, or None for a file without record 128;
    columns, lines: what the image structure record declares; entries: the record's lines in the order they lie in the
    call, each (row, offset in the image bytes, the bytes there or None, length or None for len(bytes), status)."""
    return dict(key=key, ident=ident, bits=bits, columns=columns, lines=lines, entries=list(entries), key_serial=key_serial, flags=flags,
                name=name, rice=rice)


def direct_call(segments, n_image=None, fill=0xEE):
    """A canvas call made straight from its records, not by the packet, file and image stages -> (files_out, images_out)
    as canvas_spec.process and ImageCanvas.process take them.  The caller chooses what those stages never vary: the
    byte offset of every line (any residue mod 16), the order of the lines, a line's length and status, whether a record
    begins, ends or only continues its file.  What the stage relies on stays the caller's duty and is checked here: the
    records lie ordered by key, a record without BEGINS is its key's first, rows are unique within a record (the place
    kernel's "no two lines write one pixel" rests on it); `file` and the line ranges are consistent by construction.
    n_image: the size of the image bytes (the end of the last line by default); bytes no line covers are `fill`."""
    keys = [s["key"] for s in segments]
    assert keys == sorted(keys)
    for i, s in enumerate(segments):
        assert s["flags"] & fs.BEGINS or s["key"] not in keys[:i]
        rows = [e[0] for e in s["entries"]]
        assert len(rows) == len(set(rows))
    chunks, nbytes = [], 0
    pieces, records = np.zeros(len(segments), fs.PIECE_DTYPE), np.zeros(len(segments), fs.RECORD_DTYPE)
    ifiles = np.zeros(len(segments), isp.FILE_DTYPE)
    lines = np.zeros(sum(len(s["entries"]) for s in segments), isp.LINE_DTYPE)
    end = max([0] + [e[1] + len(e[2]) for s in segments for e in s["entries"] if e[2] is not None])
    img = np.full(end if n_image is None else n_image, fill, np.uint8)
    n_lines = 0
    for f, s in enumerate(segments):
        more = [(128, cs.segment_record(*s["ident"]))] if s["ident"] is not None else []
        if s["name"] is not None:
            more.append((4, s["name"]))
        head = fs.lrit_file(b"", image=(s["bits"], s["columns"], s["lines"], 1), rice=(0, 16, 1), extra=more)
        p, r, o = pieces[f], records[f], ifiles[f]
        p["offset"], p["length"], p["file"], p["apid"], p["vcid"], p["seq_flags"] = nbytes, len(head), f, s["key"][1], s["key"][0], 1
        r["offset"], r["length"], r["header_length"], r["first_piece"], r["n_pieces"] = nbytes, len(head), len(head), f, 1
        r["vcid"], r["apid"], r["key_serial"], r["flags"] = s["key"][0], s["key"][1], s["key_serial"], s["flags"]
        r["bits_per_pixel"], r["columns"], r["lines"] = s["bits"], s["columns"], s["lines"]
        r["header_state"], r["compression"], r["pixels_per_block"], r["lines_per_packet"] = 2, 1, 16, 1
        chunks.append(head)
        nbytes += len(head)
        o["rice"], o["first_line"], o["n_lines"], o["columns"], o["bits"] = int(s["rice"]), n_lines, len(s["entries"]), s["columns"], s["bits"]
        for row, offset, body, length, status in s["entries"]:
            ln = lines[n_lines]
            ln["offset"], ln["length"], ln["row"], ln["file"] = offset, len(body) if length is None else length, row, f
            ln["samples"], ln["bits"], ln["status"] = s["columns"], s["bits"], status
            if body is not None:
                img[offset:offset + len(body)] = np.frombuffer(bytes(body), np.uint8)
            n_lines += 1
    fsum = dict.fromkeys(fs.COUNTERS, 0)
    fsum.update(pieces=len(pieces), bytes=nbytes, files=len(records))
    isum = dict.fromkeys(isp.COUNTERS, 0)
    isum.update(lines=len(lines), bytes=len(img), images=len(records))
    return (np.frombuffer(b"".join(chunks), np.uint8), pieces, records, fsum), (img, lines, ifiles, isum)


def packed(rng, rows, length, residue=0, start=0, order=None, lo=1):
    """Entries for the rows, `length` random bytes (lo .. 255: never the zero of an untouched canvas) each, one behind the
    other in the image bytes from `start`, each at the next offset that is `residue` mod 16, in the given order of the
    rows -> (entries, the offset behind the last, {row: its bytes})."""
    entries, bodies, at = [], {}, start
    for row in (rows if order is None else order):
        at += (residue - at) % 16
        body = rng.integers(lo, 256, length, dtype=np.uint8).tobytes()
        entries.append((row, at, body, None, 0))
        bodies[row] = body
        at += length
    return entries, at, bodies


SOURCE_RESIDUES = (0, 4, 8, 12, 1, 2, 3)
FIRST_BYTES = (0, 4, 1, 2)
LINE_BYTES = (1051, 5568)               # 16 * 65 + 4 * 2 + 3; 2784 samples of two bytes
COPY_ROWS = 4
# pitches that are 12 mod 16: the rows' first bytes fall on 0, 12, 8 and 4 mod 16 in turn
COPY_MAX_BYTES = {1051: 1068, 5568: 5580}
COPY_SLOT_BYTES = 22528


def copy_path_call(seed=71):
    """One image of one segment of four rows per combination of where its lines lie in the image bytes (mod 16), where
    its first column lies in a canvas row (bytes, mod 16) and how long a line is: all 56 as 8-bit images, and eight of
    those with even offsets as 10-bit images, 64 canvases in all -> (the call, [(source residue, first byte, length,
    bits)] by record)."""
    rng = np.random.default_rng(seed)
    combos = [(s, d, n, 8) for n in LINE_BYTES for s in SOURCE_RESIDUES for d in FIRST_BYTES]
    combos += [(0, 0, 5568, 10), (4, 4, 5568, 10), (8, 2, 5568, 10), (4, 0, 5568, 10), (2, 4, 5568, 10), (12, 0, 1051, 10), (2, 2, 1051, 10),
               (0, 2, 1051, 10)]
    segments, at = [], 0
    for i, (s, d, n, bits) in enumerate(combos):
        w = cs.width_of(bits)
        entries, at, _ = packed(rng, range(COPY_ROWS), n, s, at, order=[int(r) for r in rng.permutation(COPY_ROWS)])
        ident = (100 + i, 1, d // w, 0, 1, COPY_MAX_BYTES[n] // w, COPY_ROWS)
        segments.append(seg((1, 100 + i), ident, bits, (n + w - 1) // w, COPY_ROWS, entries))
    return direct_call(segments), combos


def copy_paths(call, pixels_base=0, image_base=0):
    """How many lines of a call of one-segment images (start_line 0) each of the place kernel's four paths takes with more
    than 64 of its units, from the call's own numbers: {"16": .., "16, 4, 1": .., "4": .., "4 to bytes": .., "bytes": ..}.  The bases are
    the two buffers' addresses mod 16."""
    (data, pieces, files, _), (img, lines, ifiles, _) = call
    raw = data.tobytes()
    took = dict.fromkeys(("16", "16, 4, 1", "4", "4 to bytes", "bytes"), 0)
    for ln in lines:
        r, pc = files[int(ln["file"])], pieces[int(ln["file"])]
        h, _ = cs.walk_header(raw[int(pc["offset"]):int(pc["offset"]) + int(pc["length"])], r["columns"], r["lines"])
        bits = int(r["bits_per_pixel"])
        src = image_base + int(ln["offset"])
        dst = pixels_base + int(ln["row"]) * cs.pitch_of(h["max_column"], bits) + h["start_column"] * cs.width_of(bits)
        n = int(ln["length"])
        if (src | dst) % 16 == 0:
            took["16"] += n // 16 > 64
            took["16, 4, 1"] += n // 16 > 64 and n % 16 >= 4 and n % 4 > 0      # ... with dwords and a byte tail behind them
        elif (src | dst) % 4 == 0:
            took["4"] += n // 4 > 64
        elif src % 4 == 0:
            took["4 to bytes"] += n // 4 > 64
        else:
            took["bytes"] += n > 64
    return took


def widest_line_calls(seed=72):
    """A 16-bit image of 65535 columns and 2 rows (pitch 131072: 262144 bytes, lines of 131070 bytes, 128 trips of the
    16-byte loop) next to the same image declared with three rows -> (call, slot_bytes that hold it exactly)."""
    rng = np.random.default_rng(seed)
    entries, at, _ = packed(rng, range(2), 131070)
    more, at, _ = packed(rng, range(2), 16, start=at)            # (refused: its lines are never looked at)
    return direct_call([seg((2, 1), (7, 1, 0, 0, 1, 65535, 2), 16, 65535, 2, entries),
                        seg((2, 2), (8, 1, 0, 0, 1, 65535, 3), 16, 65535, 2, more)]), 262144


TALL_LINES = 129


def tall_entries(seed=73):
    """A record's lines for a segment that declares 129: rows 0 .. 128 in a permuted order with six entries beyond the
    declared lines among them (clipped), a status of 1 or 2 on some -> entries, 135 of them: the positions 0 .. 63, 64 .. 127
    and 128 .. 134 (the commit kernel's three trips) each hold placed lines, clipped ones and faulted ones."""
    rng = np.random.default_rng(seed)
    rows = [int(r) for r in rng.permutation(TALL_LINES)]
    for pos, row in ((3, 129), (40, 200), (66, 130), (100, 65535), (129, 131), (133, 1 << 31)):
        rows.insert(pos, row)
    entries, _, _ = packed(rng, rows, 20)
    status = lambda i: 1 if i % 9 == 0 else 2 if i % 7 == 4 or i == 66 else 0            # (66 is clipped: its status counts nowhere)
    return [(row, off, body, None, status(i)) for i, (row, off, body, _, _) in enumerate(entries)]


def tall_counts(entries):
    """(placed, clipped, faults) per trip of 64 lanes, as the rule words them."""
    out = []
    for lo in range(0, len(entries), 64):
        part = entries[lo:lo + 64]
        fits = [e[0] < TALL_LINES for e in part]
        out.append((sum(fits), len(part) - sum(fits), sum(ok and e[4] != 0 for ok, e in zip(fits, part))))
    return out


def tall_calls():
    """The tall record in one call, and the same file on another image and key cut in two: a BEGINS record with the first 65
    entries, then a record that only continues and ends with the other 70 -> (one call, [first call, second call])."""
    entries = tall_entries()
    one = direct_call([seg((3, 5), (9, 1, 0, 0, 1, 20, TALL_LINES), 8, 20, TALL_LINES, entries)])
    cut = [direct_call([seg((3, 6), (10, 1, 0, 0, 1, 20, TALL_LINES), 8, 20, TALL_LINES, entries[:65], key_serial=4, flags=fs.BEGINS)]),
           direct_call([seg((3, 6), (10, 1, 0, 0, 1, 20, TALL_LINES), 8, 20, TALL_LINES, entries[65:], key_serial=4, flags=fs.ENDS)])]
    return one, cut


def grid_segments(rng, image_id, count, keys, first=1, last=None, start=0):
    """Segments first .. last of an 8-bit image of 40 x 8 cut 8 x 8 (1 row by 5 columns each, `count` of them declared),
    dealt over the keys in turn and ordered by key -> (segments, the offset behind their lines, {segment: its bytes})."""
    out, bodies, at = [], {}, start
    serial = dict.fromkeys(keys, 0)
    for n in range(first, (count if last is None else last) + 1):
        key = keys[(n - 1) % len(keys)]
        entries, at, b = packed(rng, [0], 5, start=at)
        out.append(seg(key, (image_id, n, 5 * ((n - 1) % 8), (n - 1) // 8, count, 40, 8), 8, 5, 1, entries, key_serial=serial[key]))
        serial[key] += 1
        bodies[n] = b[0]
    return sorted(out, key=lambda s: s["key"]), at, bodies


def grid_image(bodies):
    img = np.zeros((8, 40), np.int64)
    for n, b in bodies.items():
        img[(n - 1) // 8, 5 * ((n - 1) % 8):5 * ((n - 1) % 8) + 5] = np.frombuffer(b, np.uint8)
    return img


def sixty_four_segment_calls(seed=74):
    """-> (calls, the full image, the image of 63).  Call 0: an image of 64 segments over four keys, whole; one of 63 segments
    alike; the first 61 segments of a second image of 64.  Calls 1 to 3: its segments 62, 63 and 64, one a call.  Call 4:
    segment 64 of the first image once more (DUPLICATE).  Call 5: a third image of 64 of which segments 33 and 64 alone
    begin (lanes 32 and 63 of the rectangle test), then a file numbered 1 across segment 64's rectangle alone, one
    numbered 2 across segment 33's alone (OVERLAP twice), and one numbered 3 that meets neither (PLACED)."""
    rng = np.random.default_rng(seed)
    keys = [(4, 0), (4, 10), (4, 11), (4, 2047)]                # (the channel is part of a canvas's identity, the apid is not)
    whole, at, full = grid_segments(rng, 300, 64, keys)
    most, at, part = grid_segments(rng, 301, 63, [(6, 1), (6, 2), (6, 3)], start=at)
    begun, at, late = grid_segments(rng, 302, 64, [(7, 1), (7, 2)], last=61, start=at)
    calls = [direct_call(sorted(whole + most + begun, key=lambda s: s["key"]))]
    for n in (62, 63, 64):
        one, _, b = grid_segments(rng, 302, 64, [(7, 1 + (n & 1))], first=n, last=n)
        one[0]["key_serial"] = 40 + n
        late.update(b)
        calls.append(direct_call(one))
    again, _, _ = grid_segments(rng, 300, 64, [(4, 12)], first=64, last=64)
    again[0]["key_serial"] = 99
    calls.append(direct_call(again))
    sparse, at = [], 0
    for apid, n, col, line, cols in ((1, 64, 35, 7, 5), (2, 33, 0, 4, 5), (3, 1, 33, 7, 4), (4, 2, 3, 4, 6), (5, 3, 5, 4, 30)):
        entries, at, _ = packed(rng, [0], cols, start=at)
        sparse.append(seg((8, apid), (303, n, col, line, 64, 40, 8), 8, cols, 1, entries))
    calls.append(direct_call(sparse))
    assert grid_image(full).all() and grid_image(late).all()
    return calls, (grid_image(full), grid_image(late)), grid_image(part)


def guard_calls(seed=75):
    """An 8-bit canvas of 16 x 4, its left half (segment 1, 8 columns) in call 0.  Call 1, the right half on image bytes of
    exactly n = 64: row 0 ends on the last image byte (placed); row 1 has offset + length = n + 1 (clipped); row 2 has
    offset = n and length 0 (in bounds: placed, nothing copied); row 3 has offset 2^63 (clipped).  Call 2, segment 1 of a
    second canvas alike, at columns 8 to 15, whose lines are 12 bytes long: rows 0 to 2 run on into the next row's first four
    pixels (copied, as the specification does); row 3, the canvas's last, would end behind the canvas (clipped).
    -> calls."""
    rng = np.random.default_rng(seed)
    left, _, _ = packed(rng, range(4), 8)
    body = lambda n: rng.integers(1, 256, n, dtype=np.uint8).tobytes()
    right = [(0, 56, body(8), None, 0), (1, 57, None, 8, 0), (2, 64, None, 0, 0), (3, 1 << 63, None, 8, 0)]
    long_lines, _, _ = packed(rng, range(4), 12)
    return [direct_call([seg((9, 1), (400, 1, 0, 0, 2, 16, 4), 8, 8, 4, left)]),
            direct_call([seg((9, 2), (400, 2, 8, 0, 2, 16, 4), 8, 8, 4, right)], n_image=64),
            direct_call([seg((9, 3), (401, 1, 8, 0, 2, 16, 4), 8, 8, 4, long_lines)])]


def real_size_stream(seed=76):
    """Through the stages in front: a 10-bit image of 2784 x 140 in two segments of 70 lines on two keys, named, and an 8-bit
    image of 1051 x 130 cut at row 65 and column 523 -> (stream, {image_id: samples})."""
    rng = np.random.default_rng(seed)
    a = cs.samples(rng, 10, 32, 2784, 140)
    b = cs.samples(rng, 8, 16, 1051, 130)
    items = cs.split_image(rng, a, 10, 32, 500, [(10, 1), (10, 2)], [70], name=b"full width, 10 bit")
    items += cs.split_image(rng, b, 8, 16, 501, [(11, 1), (11, 2)], [65], [523])
    return isp.stream_of(rng, items), {500: a, 501: b}


REAL_SLOT_BYTES = 5568 * 140


class Run:
    """The specification over the parts of a stream: per call the inputs, the outputs and a copy of the state behind it.
    actions {index of a call: [slots released in front of it]}; table: the host check's rows are appended to it.
    direct: the parts are calls already, (files_out, images_out) as direct_call makes them."""

    def __init__(self, parts, slots=4, slot_bytes=SLOT_BYTES, actions=None, table=None, direct=False):
        self.slots, self.slot_bytes, self.actions = slots, slot_bytes, actions or {}
        st, fst, ist = cs.State(slots, slot_bytes), fs.State(), isp.State()
        self.calls = []
        if table is not None:
            cs.table_reset(table, slots, slot_bytes)
        for i, part in enumerate(parts):
            for s in self.actions.get(i, ()):
                st.release(s)
                if table is not None:
                    cs.table_release(table, s)
            files_out, images_out = part if direct else cs.run_both(fst, ist, part)
            want = cs.process(st, files_out, images_out, table=table)
            self.calls.append((files_out, images_out, want, copy.deepcopy(st)))
        self.state = st
