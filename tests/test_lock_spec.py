"""CPU tier: the frame lock's specification (tests/lock_spec.py) -- the consequences DESIGN.md section 18 states, the table
of streams on which the flywheel shows, recheck = 1 against the framer's and the decoder's own specifications, the long
damaged stream of the GPU tier (that it reaches what it is there for, from the specification alone), and the state
machine alone on small frames with a cheap stand-in for the decoder."""
import numpy as np
import pytest

import ccsds
import framer_cases as fc
import framer_spec as fs
import lock_cases as lc
import lock_spec as ls

F = fs.FRAME
R1 = ls.FULL | ls.RECHECK                       # every chunk but the first under recheck = 1


def modes(rows):
    return [int(m) for m in rows.mode]


def decoded_like_the_decoder(rows, hrit, carry=None):
    """cadu, block and info of the rows against ccsds's stages run over all rows at once (the decoder's own spec)."""
    w, idx, _ = ccsds.windows(rows.frames, rows.valid, carry)
    cadu = np.zeros((len(rows), ccsds.CADU_BYTES), np.uint8)
    block = np.zeros((len(rows), ccsds.BLOCK_BYTES), np.uint8)
    info = np.array([ls.absent_info()] * len(rows), ls.INFO_DTYPE)
    if len(idx):
        bits, err = ccsds.viterbi_batch(w)
        cadu[idx] = ccsds.cadu_from_bits(bits, hrit)
        fixed, n, ok = ccsds.rs_decode_blocks(ccsds.derandomize(cadu[idx, 4:]))
        block[idx] = fixed
        scid, vcid, counter = ccsds.header_fields(fixed)
        info["valid"][idx], info["ok"][idx], info["viterbi_errors"][idx] = 1, ok, err
        info["rs_errors"][idx] = n
        info["scid"][idx], info["vcid"][idx], info["counter"][idx] = scid, vcid, counter
    return np.array_equal(rows.cadu, cadu) and np.array_equal(rows.block, block) and np.array_equal(rows.info, info)


# ---- the table ------------------------------------------------------------------------------------------------------
def test_plant_in_a_short_chunk_is_where_the_two_walks_differ(oracle_mod):
    a, b = lc.reference("plant2", 4), lc.reference("plant2", 1)
    ra, rb = a["rows"], b["rows"]
    assert not np.array_equal(ra.start, rb.start)                           # the case is not vacuous
    assert len(ra) == 12 and int(ra.info["ok"].sum()) == 12 and np.array_equal(ra.start, a["starts"])
    assert modes(ra) == [0, 1, 1, 1, 4, 1, 1, 1, 4, 1, 1, 1]
    assert ra.hits[2].tolist() == [0, 0, 49, 0] and a["stats"]["sensitive_chunks"] == 1 and a["stats"]["short_kept"] == 9
    assert len(rb) == 11 and int(rb.info["ok"].sum()) == 10
    assert int(rb.start[2]) == 38468 and rb.hits[2].tolist() == [0, 5000, 57, 0] and not rb.info["ok"][2]
    assert modes(rb) == [0] + [R1] * 10
    assert a["stats"]["frames_ok"] == 12 and (b["stats"]["frames_ok"], b["stats"]["frames_bad"]) == (10, 1)


@pytest.mark.parametrize("name", ["plant4", "bad5_plant6", "slip1_plant4"])
def test_streams_on_which_the_flywheel_changes_no_row(oracle_mod, name):
    a, b = lc.reference(name, 4), lc.reference(name, 1)
    ra, rb = a["rows"], b["rows"]
    for f in ls.FIELDS:
        if f != "mode":
            assert np.array_equal(getattr(ra, f), getattr(rb, f)), f
    assert len(ra) == 11 and modes(rb) == [0] + [R1] * 10
    if name == "plant4":                        # fc == 4 at the entry of frame 4: correlated in full, follows the plant
        assert modes(ra) == [0, 1, 1, 1, 4, 0, 1, 1, 4, 1, 1] and ra.hits[4, 1] == lc.PLANT_AT and not ra.info["ok"][4]
        assert a["stats"]["sensitive_chunks"] == 0
    if name == "bad5_plant6":                   # frame 5 fails RS: frame 6 is correlated in full and follows the plant
        assert modes(ra) == [0, 1, 1, 1, 4, 1, 0, 0, 4, 1, 1] and not ra.info["ok"][5] and ra.hits[6, 1] == lc.PLANT_AT
        assert a["stats"]["sensitive_chunks"] == 1 and a["stats"]["frames_bad"] == 2
    if name == "slip1_plant4":                  # frame 2 begins a symbol early: nothing at 0 in the short range
        assert modes(ra)[2] == ls.MISS and ra.hits[2, 1] != 0 and a["stats"]["short_missed"] == 1


def test_hrit_version_of_the_first_stream(oracle_mod):
    a, b = lc.reference("plant2_hrit", 4), lc.reference("plant2_hrit", 1)
    assert len(a["rows"]) == 12 and int(a["rows"].info["ok"].sum()) == 12 and modes(a["rows"])[2] == ls.SHORT
    assert len(b["rows"]) == 11 and int(b["rows"].info["ok"].sum()) == 10


def test_short_hit_at_position_0_below_the_acceptance_drops_the_chunk_and_keeps_ok(oracle_mod):
    a, b = lc.reference("weak2", 4), lc.reference("weak2", 1)
    ra = a["rows"]
    assert modes(ra)[:4] == [0, 1, 1, 1] and ra.hits[2].tolist() == [0, 0, 45, 0] and not ra.valid[2]
    assert int(ra.start[2]) == int(a["starts"][2]) and int(ra.start[3]) == int(a["starts"][3])     # c += F: frame 3 at 0
    assert ra.hits[3, 1] == 0 and ra.valid[3]                           # ... and still in the short range: ok was kept
    assert len(ra) == 12 and a["stats"]["dropped_chunks"] == 1 and a["stats"]["frames_ok"] == 11
    assert b["rows"].hits[2].tolist() == [1, 4456, 51, 0]                # recheck 1 takes the chance hit of the whole chunk


# ---- consequences ---------------------------------------------------------------------------------------------------
def check_cutting(ref, recheck, cuts):
    rows, per_call, lk = ls.walk(ref["stream"], cuts, recheck=recheck, hrit=ref["hrit"], cache=ref["cache"])
    assert rows.same_as(ref["rows"]), cuts
    assert lk.stats() == ref["stats"], cuts
    return per_call, lk


def test_rows_do_not_depend_on_the_cutting(oracle_mod):
    ref = lc.reference("plant2", 4)
    stream, starts = ref["stream"], ref["starts"]
    for cuts in fc.cuttings(len(stream), F, int(starts[5]), int(starts[7]) + F, count=8):
        check_cutting(ref, 4, cuts)
    # the sensitive chunk (frame 2) with the frame that governs it (frame 1) in the call before
    per_call, _ = check_cutting(ref, 4, [int(starts[2])])
    assert len(per_call[0]) == 2 and modes(per_call[1])[0] == ls.SHORT
    check_cutting(ref, 4, [int(starts[2]) + 1, int(starts[2]) + F - 1])


def test_stop_for_want_of_symbols_restores_ok_and_fc(oracle_mod):
    """plant4: frame 4 is entered with fc == 4, step 1 fires, the whole-chunk hit is the plant at 5000 -- and the call ends
    100 symbols behind the chunk, so step 5 stops.  The next call walks the chunk again: one recheck, not two."""
    ref = lc.reference("plant4", 4)
    cut = int(ref["starts"][4]) + F + 100
    per_call, lk = check_cutting(ref, 4, [cut])
    assert len(per_call[0]) == 4 and modes(per_call[1])[0] == R1 and lk.stats()["rechecks"] == 2
    # ... and the same on the sensitive chunk of plant2 (SHORT at position 0 fits where the plant would not)
    ref = lc.reference("plant2", 4)
    per_call, _ = check_cutting(ref, 4, [int(ref["starts"][2]) + F + 100])
    assert len(per_call[0]) == 3


def test_recheck_1_is_the_framer_then_the_decoder(oracle_mod):
    stream, _, _, _ = fc.drifting_stream(offset=16300, n=12, inserts=(3, 7))
    rows, _, lk = ls.walk(stream, recheck=1)
    want, _, fr = fs.walk(stream)
    assert len(rows) == len(want) == 12
    for f in ("frames", "valid", "hits", "start"):
        assert np.array_equal(getattr(rows, f), getattr(want, f)), f
    assert decoded_like_the_decoder(rows, False)
    assert {k: lk.stats()[k] for k in fs.STATS} == fr.stats()
    assert modes(rows) == [0] + [R1] * 11


# ---- the long damaged stream of the GPU tier: does it reach what it is there for? --------------------------------------
@pytest.mark.parametrize("recheck", [2, 3, 4, 5, 255])
def test_long_stream_earns_its_place(oracle_mod, recheck):
    """Conditions on lock_cases.long_stream() pushed whole, from the specification alone: enough chunks of every kind, more
    rows than two batches of 64, and at least four rounds that no device can avoid (round_bounds' lower bound)."""
    ref = lc.long_reference(recheck)
    rows, st, cache = ref["rows"], ref["stats"], ref["cache"]
    fck0 = lc.fck0_rows(rows, cache)
    print("recheck", recheck, "rows", len(rows), {k: st[k] for k in ls.STATS}, "bounds", ref["bounds"], "fck0", fck0)
    assert st["sensitive_chunks"] >= 4 and st["short_missed"] >= 4 and st["frames_bad"] >= 6
    assert st["dropped_chunks"] >= 3 and st["resyncs"] >= 15 and len(rows) > 128
    lower, upper = ref["bounds"]
    assert 4 <= lower <= upper
    assert {ls.FULL, ls.SHORT, ls.MISS} <= set(m & 3 for m in modes(rows))
    if recheck == 4:
        assert len(fck0) >= 2                   # fc not known at a chunk that hangs on it, twice at the least
        plain = lc.long_reference(1)            # ... and the flywheel shows: other rows, more good frames
        assert not np.array_equal(rows.start[:len(plain["rows"])], plain["rows"].start[:len(rows)])
        assert st["frames_ok"] > plain["stats"]["frames_ok"] and plain["bounds"][0] == 1


def test_long_stream_memoised_decode_is_the_decoder(oracle_mod):
    """The rows of the long stream are decoded through lock_cases.memo_decode; the 30 rows up to two behind the first dropped
    chunk (frames that fail RS among them) against the decoder's stages run over them at once, behind the carry of the row
    before them."""
    rows = lc.long_reference(4)["rows"]
    b = int(np.flatnonzero(rows.valid == 0)[0]) + 3
    part = ls.Rows(F, **{f: getattr(rows, f)[b - 30:b] for f in ls.FIELDS})
    assert rows.valid[b - 31] and not part.info["ok"][part.valid != 0].all()
    assert decoded_like_the_decoder(part, False, rows.frames[b - 31][-ccsds.CARRY:])


@pytest.mark.parametrize("recheck", [4, 3])
def test_long_stream_rows_do_not_depend_on_the_cutting(oracle_mod, recheck):
    ref = lc.long_reference(recheck)
    for cuts in lc.long_cuttings(len(ref["stream"])):
        spec = lc.long_lock(ref, recheck)
        per_call = [spec.push(p) for p in lc.pieces_of(ref["stream"], cuts)]
        assert ls.Rows.concat(per_call, F).same_as(ref["rows"]), cuts
        assert spec.stats() == ref["stats"], cuts
        assert all(1 <= lo <= hi for lo, hi in (lc.round_bounds(r, ref["cache"]) for r in per_call))


@pytest.mark.parametrize("recheck,at,due", [(4, 64, True), (3, 66, True), (3, 64, False), (255, 64, False)])
def test_planted_chunk_behind_64_frames_in_lock(oracle_mod, recheck, at, due):
    """lock_cases.batch_reference: 64 good frames at position 0, then a planted chunk entered with fc == recheck (step 1
    fires, the whole chunk is correlated, the plant is followed) or not (SHORT at position 0, and only ok decides it)."""
    ref = lc.batch_reference(recheck, at)
    rows = ref["rows"]
    assert rows.valid[:at].all() and rows.info["ok"][:at].all() and not rows.hits[:at, 1].any()
    assert modes(rows)[:at] == [4 if i and (i - 1) % recheck + 1 == recheck else (1 if i else 0) for i in range(at)]
    if due:
        assert modes(rows)[at] == R1 and rows.hits[at, 1] == lc.PLANT_AT and not rows.info["ok"][at]
        assert ref["stats"]["sensitive_chunks"] == 0 and ref["bounds"] == (1, 2)
    else:
        assert modes(rows)[at] == ls.SHORT and rows.hits[at, 1] == 0 and rows.info["ok"].all() and len(rows) == at + 6
        assert ref["stats"]["sensitive_chunks"] == 1 and ref["bounds"] == (2, 2)


# ---- the state machine alone: frames of 2048 symbols, a stand-in for the decoder --------------------------------------
SMALL = 2048                                    # frame // 16 = 128: the short range is positions 0 .. 63


def fake_decode(frame, carry):
    """ok from one symbol of the frame; the carry reaches the outputs so that its handling shows."""
    info = np.zeros((), ls.INFO_DTYPE)
    info["valid"], info["ok"] = 1, int(frame[100] >= 0)
    info["viterbi_errors"] = int(np.abs(carry.astype(np.int64)).sum())
    return np.zeros(ccsds.CADU_BYTES, np.uint8), np.zeros(ccsds.BLOCK_BYTES, np.uint8), info


def small_stream(seed, n=60):
    """n frames of SMALL symbols: the sync word, noise behind it; some words weakened, some planted 300 symbols in, some
    frames marked bad, a symbol deleted or inserted now and then."""
    rng = np.random.default_rng(seed)
    word = np.array([100 if (fs.LRIT_WORDS[0] >> (63 - i)) & 1 else -100 for i in range(64)], np.int8)
    parts = [rng.integers(-50, 51, int(rng.integers(0, 400))).astype(np.int8)]
    for _ in range(n):
        fr = rng.integers(-100, 101, SMALL).astype(np.int8)
        fr[:64] = word
        kind = int(rng.integers(0, 10))
        if kind == 0:                                            # plant
            fr[300:364] = word
            fr[rng.choice(64, 10, replace=False)] *= -1
        elif kind == 1:                                          # weak
            fr[rng.choice(64, int(rng.integers(12, 24)), replace=False)] *= -1
        fr[100] = -50 if int(rng.integers(0, 4)) == 0 else 50    # the stand-in's ok
        if kind == 2:
            fr = fr[:-1]
        elif kind == 3:
            fr = np.concatenate([fr, fr[-1:]])
        parts.append(fr)
    return np.concatenate(parts)


@pytest.mark.parametrize("recheck", [1, 2, 4, 255])
def test_state_machine_on_small_frames(oracle_mod, recheck):
    seen = set()
    for seed in range(6):
        stream = small_stream(seed)
        cache = {}
        kw = dict(recheck=recheck, frame=SMALL, decode=fake_decode, cache=cache)
        rows, _, lk = ls.walk(stream, **kw)
        seen |= set(modes(rows))
        rng = np.random.default_rng(100 + seed)
        cuttings = [sorted(int(v) for v in rng.integers(0, len(stream) + 1, 12)) for _ in range(10)]
        cuttings.append(list(range(0, len(stream), 97)))        # stops of step 5 at every kind of chunk
        for cuts in cuttings:
            lk2 = ls.Lock(**kw)
            edges = [0] + cuts + [len(stream)]
            parts = []
            for a, b in zip(edges[:-1], edges[1:]):
                got = lk2.push(stream[a:b])
                assert len(got) <= fs.rows_cap(b - a, SMALL) and lk2.carry <= 2 * SMALL - 66
                parts.append(got)
            assert ls.Rows.concat(parts, SMALL).same_as(rows) and lk2.stats() == lk.stats(), (seed, cuts)
        if recheck == 1:
            want, _, fr = fs.walk(stream, frame=SMALL)
            for f in ("frames", "valid", "hits", "start"):
                assert np.array_equal(getattr(rows, f), getattr(want, f)), f
            assert modes(rows)[1:] == [R1] * (len(rows) - 1)
    if recheck == 4:
        assert seen >= {ls.FULL, ls.SHORT, ls.MISS, ls.FULL | ls.RECHECK}


def test_arguments(oracle_mod):
    for r in (0, 256):
        with pytest.raises(ValueError):
            ls.Lock(recheck=r)
    with pytest.raises(ValueError):
        ls.Lock(frame=1039, decode=fake_decode)
