"""CPU tier: the stream frame synchroniser's specification (tests/framer_spec.py) against itself and the oracle -- on an
aligned stream it is the fixed-window correlator and frame fix, its rows do not depend on how the stream is cut, the carry
and row bounds hold in every call, and on a stream whose sync word drifts across the fixed windows' boundary it takes
every frame once where the fixed-window pair does not."""
import numpy as np
import pytest

import framer_cases as fc
import framer_spec as fs

F = fs.FRAME


@pytest.fixture(scope="module")
def drifting(oracle_mod):
    """The issue's stream: 40 coded frames behind 16300 symbols, one symbol inserted after frames 10 and 20."""
    stream, frames, starts, _ = fc.drifting_stream(offset=16300)
    cache = {}
    rows, _, fr = fs.walk(stream, cache=cache)
    return dict(stream=stream, frames=frames, starts=starts, rows=rows, stats=fr.stats(), cache=cache)


def same_rows(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("frames", "valid", "hits", "start"))


def test_aligned_stream_is_the_fixed_window_pair(oracle_mod):
    o = oracle_mod
    rng = np.random.default_rng(2)
    frames, _ = fc.coded_frames(12, rng)
    stream = frames.reshape(-1).copy()
    stream[3 * F:4 * F] = 0                                    # one chunk of erasures: dropped by both
    stream[7 * F:] = (stream[7 * F:].view(np.uint8) ^ 0xFF).view(np.int8)      # the other phase from frame 7 on
    hits = o.sync_correlate(stream)
    want_frames, want_valid = o.sync_fix_frames(stream, hits)
    rows, _, fr = fs.walk(stream)
    assert len(rows) == 12 and np.array_equal(rows.hits[:, :3], hits) and not rows.hits[:, 3].any()
    assert np.array_equal(rows.valid, want_valid) and np.array_equal(rows.frames, want_frames)
    assert want_valid.tolist() == [1, 1, 1, 0] + [1] * 8 and hits[7:, 0].all() and not hits[:7, 0].any()
    assert np.array_equal(rows.start, np.arange(12, dtype=np.uint64) * F)
    assert np.array_equal(rows.frames[8], frames[8])            # inverted back
    assert fr.stats() == dict(symbols=12 * F, cursor=12 * F, rows=12, frames=11, dropped_chunks=1, resyncs=0, carry=0)
    # HRIT never inverts and keeps the raw word
    h_stream = fc.coded_frames(6, rng, hrit=True)[0].reshape(-1).copy()
    h_stream[3 * F:] = (h_stream[3 * F:].view(np.uint8) ^ 0xFF).view(np.int8)
    h_rows, _, _ = fs.walk(h_stream, hrit=True)
    raw = o.sync_correlate(h_stream, words=fs.HRIT_WORDS)
    assert set(raw[:, 0].tolist()) == {0, 1} and not raw[:, 1].any()        # NRZ-M: the word found follows the line level
    forced = raw.copy()
    forced[:, 0] = 0
    h_frames, h_valid = o.sync_fix_frames(h_stream, forced)
    assert np.array_equal(h_rows.hits[:, :3], raw) and np.array_equal(h_rows.frames, h_frames) and np.array_equal(h_rows.valid, h_valid)
    assert h_valid.all() and np.array_equal(h_rows.frames.reshape(-1), h_stream)


def test_rows_do_not_depend_on_the_cutting_and_bounds_hold(drifting):
    stream, whole = drifting["stream"], drifting["rows"]
    starts = drifting["starts"]
    for cuts in fc.cuttings(len(stream), F, int(starts[5]), int(starts[7]) + F):
        assert {0, 1, F - 1, F, int(starts[5]) + 31, int(starts[7]) + F - 1} <= set(cuts)
        fr = fs.Framer(cache=drifting["cache"])
        edges = [0] + cuts + [len(stream)]
        parts = []
        for a, b in zip(edges[:-1], edges[1:]):
            r = fr.push(stream[a:b])
            assert fr.carry <= 2 * F - 66 and fr.carry == fr.end - fr.cursor
            assert len(r) <= fs.rows_cap(b - a, F)
            parts.append(r)
        assert same_rows(fs.Rows.concat(parts, F), whole), cuts
        assert fr.stats() == drifting["stats"]
    # the bounds are tight: a hit at the last position, one symbol short of its frame, leaves 2 F - 66 symbols
    fr = fs.Framer()
    r = fr.push(np.concatenate([np.zeros(F - 65, np.int8), drifting["frames"][0][:F - 1]]))
    assert len(r) == 0 and fr.carry == 2 * F - 66 and fr.cursor == 0
    assert len(fr.push(drifting["frames"][0][F - 1:])) == 1 and fr.carry == 0
    assert fs.rows_cap(0) == 1 and fs.rows_cap(F) == 2 and fs.rows_cap(66, 65) == 2


def test_drifting_sync_word_every_frame_once(drifting, oracle_mod):
    """F = 16384, 40 coded frames from offset 16300, one symbol inserted after frame 10 and one after frame 20: the
    specification yields all 40 frames once each, in order.

    On this stream the fixed-window pair ALSO yields all 40: the word sits at 16300, 16301 and 16302 inside the windows,
    and positions up to F - 65 = 16319 are searched, so it never reaches the boundary.  The gap shows on the same stream
    begun at offset 16319, the last position a window searches: after the first inserted symbol the word straddles the
    boundary (16320), no window holds it whole, and the pair takes chance hits (47 .. 52 agreeing bits) instead."""
    o = oracle_mod
    rows = drifting["rows"]
    assert len(rows) == 40 and rows.valid.all()
    assert np.array_equal(rows.start, drifting["starts"]) and np.array_equal(rows.frames, drifting["frames"])
    assert rows.hits[:, 1].tolist() == [16300] + [0] * 10 + [1] + [0] * 9 + [1] + [0] * 18
    assert drifting["stats"]["resyncs"] == 3 and drifting["stats"]["carry"] == 0
    hits = o.sync_correlate(drifting["stream"])
    pair_frames, pair_valid = o.sync_fix_frames(drifting["stream"], hits)
    assert hits[:, 1].tolist() == [16300] * 11 + [16301] * 10 + [16302] * 19 and pair_valid.all()
    assert np.array_equal(pair_frames, drifting["frames"])
    # the same, begun at the last searched position: the word crosses the fixed windows' boundary
    stream, frames, starts, _ = fc.drifting_stream(offset=16319)
    rows, _, _ = fs.walk(stream)
    assert len(rows) == 40 and rows.valid.all() and np.array_equal(rows.start, starts) and np.array_equal(rows.frames, frames)
    hits = o.sync_correlate(stream)
    pair_frames, pair_valid = o.sync_fix_frames(stream, hits)
    got = [f for f in range(len(hits)) if pair_valid[f]]
    sent = {fr.tobytes(): i for i, fr in enumerate(frames)}
    taken = [sent.get(pair_frames[f].tobytes(), -1) for f in got]
    assert taken[:11] == list(range(11))                        # up to the first inserted symbol the two agree
    assert taken != list(range(40)) and set(range(11, 40)) - set(taken)       # then frames are lost
