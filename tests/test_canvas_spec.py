"""CPU tier: the canvas stage's specification (tests/canvas_spec.py) against its own generator -- generated images are
reassembled exactly, the final state and pixels do not depend on how the stream is cut into calls, and every refusal
reason is reached by a constructed case."""
import numpy as np
import pytest

import canvas_cases as cc
import canvas_spec as cs
import file_spec as fs


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
