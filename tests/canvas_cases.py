"""Constructed streams for the canvas stage's tests (test infrastructure on top of canvas_spec): each returns what a test
needs to drive the specification and the device alike.  Images are at most 64 x 48 pixels, handles have slots of 16 KiB."""
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


class Run:
    """The specification over the parts of a stream: per call the inputs, the outputs and a copy of the state behind it.
    actions {index of a call: [slots released in front of it]}; table: the host check's rows are appended to it."""

    def __init__(self, parts, slots=4, slot_bytes=SLOT_BYTES, actions=None, table=None):
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
            files_out, images_out = cs.run_both(fst, ist, part)
            want = cs.process(st, files_out, images_out, table=table)
            self.calls.append((files_out, images_out, want, copy.deepcopy(st)))
        self.state = st
