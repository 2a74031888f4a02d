"""CPU tier: the canvas stage's specification (tests/canvas_spec.py) against its own generator -- generated images are
reassembled exactly, the final state and pixels do not depend on how the stream is cut into calls, and every refusal
reason is reached by a constructed case."""
import numpy as np
import pytest

import canvas_cases as cc
import canvas_spec as cs
import file_spec as fs
import image_spec as isp


def same_final(a, b):
    """Two states after the same stream cut differently: everything but the call numbers."""
    sa, sb = a.slots.copy(), b.slots.copy()
    for s in (sa, sb):
        s["born_call"] = s["touched_call"] = 0
    assert sa.tobytes() == sb.tobytes()
    assert a.segments.tobytes() == b.segments.tobytes() and np.array_equal(a.pixels, b.pixels)
    assert {k: v.tobytes() for k, v in a.keys.items()} == {k: v.tobytes() for k, v in b.keys.items()}
    ca, cb = a.counters(), b.counters()
    ca.pop("calls"), cb.pop("calls")
    assert ca == cb


def test_three_segments_on_one_key():
    stream, img = cc.one_key_three_segments()
    run = cc.Run([stream])
    out, slots, summ = run.calls[0][2]
    assert [int(r) for r in out["reason"]] == [cs.PLACED] * 3 and [int(s) for s in out["segment"]] == [1, 2, 3]
    assert int(slots[0]["complete"]) == 1 and int(slots[0]["lines_placed"]) == 12 and summ["completed"] == 1
    assert bytes(slots[0]["name"]).rstrip(b"\0") == b"three" and not slots[1:]["in_use"].any()
    assert np.array_equal(run.state.image(0), img)
    assert summ["canvases_begun"] == 1 and summ["segments_begun"] == summ["segments_done"] == 3 and summ["lines_placed"] == 12


def test_two_by_two_with_start_column_on_two_keys():
    stream, img = cc.two_by_two_on_two_keys()
    run = cc.Run([stream])
    out, slots, summ = run.calls[0][2]
    assert sorted(int(s) for s in out["segment"]) == [1, 2, 3, 4] and set(int(c) for c in out["start_column"]) == {0, 9}
    assert int(slots[0]["complete"]) == 1 and int(slots[0]["pitch"]) == 44 and summ["canvases_begun"] == 1
    assert {int(g["apid"]) for g in run.state.segments[0][:4]} == {8, 9}
    assert np.array_equal(run.state.image(0), img)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cut_into_calls_gives_the_same_state_and_pixels(seed):
    stream, images = cc.mixed_stream()
    whole = cc.Run([stream], slots=6)
    assert whole.calls[0][2][2]["canvases_completed"] == 5 and whole.state.slots["complete"].sum() == 5
    for i in range(5):
        s = whole.state.slots[i]
        v, bits, img = images[int(s["image_id"])]
        assert (int(s["vcid"]), int(s["bits"])) == (v, bits) and np.array_equal(whole.state.image(i), img)
    rng = np.random.default_rng(seed)
    cut = cc.Run(list(fs.cut_calls(rng, stream, 5)), slots=6)
    assert len(cut.calls) > len(stream) // 5
    # (slots are born in record order within a call and in call order across calls: compare by image)
    by_id = lambda st: {int(s["image_id"]): i for i, s in enumerate(st.slots) if s["in_use"]}
    wa, cu = by_id(whole.state), by_id(cut.state)
    assert wa.keys() == cu.keys()
    for ident in wa:
        assert np.array_equal(whole.state.image(wa[ident]), cut.state.image(cu[ident]))
        assert whole.state.segments[wa[ident]].tobytes() == cut.state.segments[cu[ident]].tobytes()
    ca, cb = whole.state.counters(), cut.state.counters()
    ca.pop("calls"), cb.pop("calls")
    assert ca == cb


def test_one_key_cut_into_calls_is_the_one_call_exactly():
    stream, img = cc.one_key_three_segments()
    whole = cc.Run([stream])
    for seed in range(3):
        cut = cc.Run(list(fs.cut_calls(np.random.default_rng(seed), stream, 5)))
        same_final(whole.state, cut.state)
        assert np.array_equal(cut.state.image(0), img)


def test_every_reason():
    stream, want, img = cc.reasons_stream()
    run = cc.Run([stream], slots=8)
    out, slots, summ = run.calls[0][2]
    assert [int(r) for r in out["reason"]] == want
    assert (out["slot"][out["reason"] != cs.PLACED] == -1).all()
    for name, n in (("bad_segment", 9), ("too_large", 1), ("duplicate", 1), ("overlap", 1), ("no_slot", 0), ("no_placement", 0)):
        assert summ[name] == n, name
    # image 50 is complete and exact; the files without a usable record 128 are images of one segment; the clipped one
    # holds its two declared rows
    first = int(out["slot"][10])
    assert int(slots[first]["complete"]) == 1 and np.array_equal(run.state.image(first), img)
    for f in (13, 14):
        s = slots[int(out["slot"][f])]
        assert int(s["image_id"]) == cs.NO_ID and int(s["complete"]) == 1 and (int(s["max_row"]), int(s["max_column"])) == (3, 8)
    assert (int(out["lines_placed"][15]), int(out["lines_clipped"][15])) == (2, 2) and summ["lines_clipped"] == 2
    # cut in two: the records that go on after a refusal have no placement
    half = cc.Run([stream[:len(stream) // 2], stream[len(stream) // 2:]], slots=8)
    assert half.calls[1][2][2]["no_placement"] >= 2
    assert cs.NO_PLACEMENT in [int(r) for r in half.calls[1][2][0]["reason"]]
    # two slots, three images
    run = cc.Run([cc.no_slot_stream()], slots=2)
    assert [int(r) for r in run.calls[0][2][0]["reason"]] == [cs.PLACED, cs.PLACED, cs.NO_SLOT] and run.calls[0][2][2]["no_slot"] == 1


def test_a_call_built_by_hand_is_the_stages_call():
    """canvas_cases.direct_call against the packet, file and image stages: a 10-bit image of two segments on two keys, once
    through split_image, stream_of and Run, once from its rows by hand -> the same pixels, the same per-record outputs, the
    same masks and `complete`."""
    rng = np.random.default_rng(80)
    img = cs.samples(rng, 10, 32, 13, 7)
    items = cs.split_image(rng, img, 10, 32, 77, [(3, 20), (3, 21)], [4], name=b"by hand")
    staged = cc.Run([isp.stream_of(rng, items)])
    segments, at = [], 0
    for n, (key, (lo, hi)) in enumerate((((3, 20), (0, 4)), ((3, 21), (4, 7))), 1):
        entries = []
        for row in range(hi - lo):
            body = img[lo + row].astype("<u2").tobytes()
            entries.append((row, at, body, None, 0))
            at += (len(body) + 3) & ~3
        segments.append(cc.seg(key, (77, n, 0, lo, 2, 13, 7), 10, 13, hi - lo, entries, name=b"by hand"))
    direct = cc.Run([cc.direct_call(segments)], direct=True)
    (out_a, slots_a, sum_a), (out_b, slots_b, sum_b) = staged.calls[0][2], direct.calls[0][2]
    assert np.array_equal(staged.state.image(0), img) and np.array_equal(direct.state.image(0), img)
    assert np.array_equal(staged.state.pixels, direct.state.pixels)
    assert len(out_a) == len(out_b) == 2
    for f in ("reason", "slot", "segment", "start_line", "start_column", "lines_placed"):
        assert np.array_equal(out_a[f], out_b[f]), f
    assert [int(r) for r in out_b["reason"]] == [cs.PLACED] * 2 and [int(x) for x in out_b["lines_placed"]] == [4, 3]
    for f in ("begun_mask", "done_mask", "aborted_mask", "complete", "pitch", "lines_placed", "bits", "vcid", "image_id", "name"):
        assert np.array_equal(slots_a[f], slots_b[f]), f
    assert int(slots_b[0]["done_mask"]) == 3 and int(slots_b[0]["complete"]) == 1 and sum_a == sum_b
    # the image stage's own lines lie where the hand-built ones do: padded to 4 bytes, one behind the other
    assert np.array_equal(staged.calls[0][1][1]["offset"], direct.calls[0][1][1]["offset"])
    for a, b in zip(staged.calls[0][1][1], direct.calls[0][1][1]):
        lo, hi = int(a["offset"]), int(a["offset"]) + int(a["length"])
        assert a["length"] == b["length"] == 26 and np.array_equal(staged.calls[0][1][0][lo:hi], direct.calls[0][1][0][lo:hi])


def test_the_hand_built_cases_hold_what_they_are_for():
    """From the specification alone, without a device: every copy path with more than 64 of its units, the trips of the
    commit kernel's line loop, 64 segments, the guard's four lines."""
    call, combos = cc.copy_path_call()
    assert len(combos) == 64 and len(set(combos)) == 64
    took = cc.copy_paths(call)
    assert all(n >= 2 for n in took.values()), took
    run = cc.Run([call], slots=64, slot_bytes=cc.COPY_SLOT_BYTES, direct=True)
    out, slots, summ = run.calls[0][2]
    assert summ["canvases_completed"] == 64 and summ["call_lines_placed"] == 64 * cc.COPY_ROWS and summ["call_lines_clipped"] == 0
    assert {int(p) % 16 for p in slots["pitch"]} == {12}
    for trip in cc.tall_counts(cc.tall_entries()):
        assert all(n > 0 for n in trip), trip
    one, cut = cc.tall_calls()
    run = cc.Run([one], direct=True)
    want = [sum(t[i] for t in cc.tall_counts(cc.tall_entries())) for i in range(3)]
    o = run.calls[0][2][0][0]
    assert [int(o["lines_placed"]), int(o["lines_clipped"]), int(o["faults"])] == want and want[0] == cc.TALL_LINES
    run = cc.Run(cut, direct=True)
    assert [int(c[2][0][0]["reason"]) for c in run.calls] == [cs.PLACED] * 2 and int(run.state.slots[0]["complete"]) == 1
    assert int(run.state.slots[0]["lines_placed"]) == cc.TALL_LINES
    calls, (full, late), part = cc.sixty_four_segment_calls()
    run = cc.Run(calls, direct=True)
    st = run.state
    assert [int(s["done_mask"]) for s in st.slots] == [2 ** 64 - 1, 2 ** 63 - 1, 2 ** 64 - 1, 1 << 63 | 1 << 32 | 4]
    assert [int(s["complete"]) for s in st.slots] == [1, 1, 1, 0] and int(st.segments[0]["begun"].sum()) == 64
    assert np.array_equal(st.image(0), full) and np.array_equal(st.image(1), part) and np.array_equal(st.image(2), late)
    assert [int(s["complete"]) for s in run.calls[2][3].slots] == [1, 1, 0, 0]            # 63 of 64 done: not yet
    assert [int(r) for r in run.calls[4][2][0]["reason"]] == [cs.DUPLICATE]
    assert [int(r) for r in run.calls[5][2][0]["reason"]] == [cs.PLACED, cs.PLACED, cs.OVERLAP, cs.OVERLAP, cs.PLACED]
    run = cc.Run(cc.guard_calls(), direct=True)
    o = run.calls[1][2][0][0]
    assert (int(o["lines_placed"]), int(o["lines_clipped"])) == (2, 2)
    o = run.calls[2][2][0][0]
    assert (int(o["lines_placed"]), int(o["lines_clipped"])) == (3, 1)
    img = run.state.image(1)
    assert img[1:, :4].all() and not img[0, :8].any() and not img[3, 4:].any()            # the long lines ran on into the next rows
    call, slot_bytes = cc.widest_line_calls()
    run = cc.Run([call], slots=2, slot_bytes=slot_bytes, direct=True)
    assert [int(r) for r in run.calls[0][2][0]["reason"]] == [cs.PLACED, cs.TOO_LARGE]
    s = run.state.slots[0]
    assert int(s["pitch"]) * int(s["max_row"]) == slot_bytes and run.state.pixels[0, slot_bytes - 3] != 0 and int(s["complete"]) == 1
    run = cc.Run([call], slots=2, slot_bytes=slot_bytes - 16, direct=True)
    assert [int(r) for r in run.calls[0][2][0]["reason"]] == [cs.TOO_LARGE] * 2


def test_aborted_segment_and_release():
    stream, img, kept = cc.aborted_stream()
    run = cc.Run([stream])
    out, slots, summ = run.calls[0][2]
    assert [int(r) for r in out["reason"]] == [cs.PLACED, cs.PLACED, cs.PLACED, cs.DUPLICATE]
    assert int(slots[0]["aborted_mask"]) == 2 and int(slots[0]["done_mask"]) == 5 and not slots[0]["complete"] and summ["completed"] == 0
    got = run.state.image(0)
    assert np.array_equal(got[:4 + kept], img[:4 + kept]) and not got[4 + kept:8].any() and np.array_equal(got[8:], img[8:])
    first, second, new = cc.release_streams()
    run = cc.Run([first, second], actions={1: [0]})
    out = run.calls[1][2][0]
    assert sorted(int(r) for r in out["reason"]) == [cs.PLACED, cs.NO_PLACEMENT, cs.NO_PLACEMENT]
    s = run.state.slots[0]
    assert int(s["generation"]) == 1 and int(s["image_id"]) == 41 and int(s["complete"]) == 1
    want = np.zeros((8, 16), np.int64)
    want[1:4, 3:13] = new
    assert np.array_equal(run.state.image(0), want)
