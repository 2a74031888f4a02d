"""Streams the frame lock's tests share (tests/test_lock_spec.py, tests/test_gpu_lock.py, tests/test_gpu_lock_host.py):
12 coded frames behind 700 symbols of noise, with the two things the flywheel is about -- a frame whose sync word is
weakened while a clean copy of it stands 5000 symbols in (a *plant*), and a frame that Reed-Solomon rejects (*bad*).
Behind them a long damaged stream (long_stream: 192 frames, a damage every few frames, many rounds in a call) with the
bounds its rows set on the device's rounds, and streams with a whole batch of 64 frames in lock in front of a plant."""
import numpy as np

import framer_cases as fc

F = fc.F
LEAD = 700
PLANT_AT = 5000
NFRAMES = 12


def plant(frames, i):
    """Frame i: 8 of the 64 sync symbols negated, the original 64 copied to PLANT_AT."""
    word = frames[i][:64].copy()
    for k in range(8):
        frames[i][12 + 6 * k] = -frames[i][12 + 6 * k]
    frames[i][PLANT_AT:PLANT_AT + 64] = word


def bad(frames, i, rng):
    """Frame i: everything behind the sync symbols replaced by uniform noise."""
    frames[i][64:] = rng.integers(-100, 101, F - 64).astype(np.int8)


def weak(frames, i, flips=18):
    """Frame i: `flips` of the 64 sync symbols negated, no copy anywhere.  With seed 11 and 18 flips frame 2 keeps 45
    agreeing bits at position 0, still the best of the first F / 16 positions (found by a search over seeds with the
    specification; the whole chunk's best is a chance hit of 51 bits at 4456)."""
    idx = (np.arange(flips) * 5 + 1) % 64
    frames[i][idx] = -frames[i][idx]


def sent_vcdus(hrit=False, seed=11, n=NFRAMES):
    """The VCDUs inside stream_a's frames, (n, 892)."""
    import ccsds
    _, cadus = fc.coded_frames(n, np.random.default_rng(seed), hrit=hrit)
    return np.stack([ccsds.derandomize(np.asarray(c[4:], np.uint8))[:ccsds.VCDU_BYTES] for c in cadus])


def stream_a(plants=(), bads=(), weaks=(), delete_last_of=None, hrit=False, seed=11, n=NFRAMES):
    """(stream, offsets at which the frames begin)."""
    rng = np.random.default_rng(seed)
    frames, _ = fc.coded_frames(n, rng, hrit=hrit)
    frames = frames.copy()
    lead = rng.integers(-20, 21, LEAD).astype(np.int8)
    for i in bads:
        bad(frames, i, rng)
    for i in plants:
        plant(frames, i)
    for i in weaks:
        weak(frames, i)
    parts, starts, at = [lead], [], LEAD
    for i in range(n):
        part = frames[i][:-1] if i == delete_last_of else frames[i]
        starts.append(at)
        parts.append(part)
        at += len(part)
    return np.concatenate(parts), np.array(starts, np.int64)


# name -> arguments of stream_a; the table of DESIGN.md section 18
TABLE = {
    "plant2": dict(plants=(2,)),
    "plant4": dict(plants=(4,)),
    "bad5_plant6": dict(plants=(6,), bads=(5,)),
    "slip1_plant4": dict(plants=(4,), delete_last_of=1),
}
# ... the first stream as HRIT, and a SHORT hit at position 0 below the acceptance
MORE = {
    "plant2_hrit": dict(plants=(2,), hrit=True),
    "weak2": dict(weaks=(2,)),
}

_REFERENCE = {}

# ---- a long damaged stream: many rounds in a call, whole batches of records between them ------------------------------
KINDS = ("plant", "plant", "plant", "bad", "weak", "delete", "insert", "zero", "bad_plant", "slip_plant")
MEMO = {}                                       # memo_decode's, shared by every test of a process


def long_stream(n=192, seed=9, hrit=False):
    """(stream, [(frame, kind)]): 8 coded frames tiled to n behind LEAD symbols of noise, and about every 2 to 13 frames a
    damage of KINDS (a plant three times as likely as each other kind): plant, bad and weak as above; `delete` removes the
    frame's last symbol, `insert` puts three noise symbols behind the frame, `zero` zeroes it; `bad_plant` is a bad frame
    with a plant in the next, `slip_plant` a delete with a plant two frames on.  Frames 0 to 4 and the last three are
    clean.  The damages come from a second generator, so that the frames are those of coded_frames(8, default_rng(seed)).
    Seed 9 is the first of 3 .. 15 at which the walk meets every condition of
    test_lock_spec.py::test_long_stream_earns_its_place at every recheck (seed 3 has 3 sensitive chunks at recheck 2)."""
    tile, _ = fc.coded_frames(8, np.random.default_rng(seed), hrit=hrit)
    frames = [tile[i % 8].copy() for i in range(n)]
    rng = np.random.default_rng([seed, 1])
    lead = rng.integers(-20, 21, LEAD).astype(np.int8)
    tails, cut, kinds = {}, set(), []
    i = 5 + int(rng.integers(0, 4))
    while i + 2 < n - 3:
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        kinds.append((i, kind))
        last = i
        if kind == "plant":
            plant(frames, i)
        elif kind in ("bad", "bad_plant"):
            bad(frames, i, rng)
            if kind == "bad_plant":
                plant(frames, i + 1)
                last = i + 1
        elif kind == "weak":
            weak(frames, i)
        elif kind in ("delete", "slip_plant"):
            cut.add(i)
            if kind == "slip_plant":
                plant(frames, i + 2)
                last = i + 2
        elif kind == "insert":
            tails[i] = rng.integers(-20, 21, 3).astype(np.int8)
        elif kind == "zero":
            frames[i][:] = 0
        i = last + int(rng.integers(2, 14))
    parts = [lead]
    for i in range(n):
        parts.append(frames[i][:-1] if i in cut else frames[i])
        if i in tails:
            parts.append(tails[i])
    return np.concatenate(parts), kinds


def memo_decode(hrit, memo):
    """lock_spec.make_ccsds_decode(hrit), memoised in `memo` on the frame and the carry: a cache of the specification's own
    function.  On a stream of tiled frames only the damaged ones and their neighbours cost a decode."""
    import lock_spec as ls
    decode = ls.make_ccsds_decode(hrit)

    def memoised(frame, carry):
        key = (bool(hrit), frame.tobytes(), carry.tobytes())
        if key not in memo:
            memo[key] = decode(frame, carry)
        return memo[key]
    return memoised


def long_lock(ref, recheck):
    """A fresh specification for the stream of a long_reference, on its caches."""
    import lock_spec as ls
    return ls.Lock(hrit=ref["hrit"], recheck=recheck, decode=memo_decode(ref["hrit"], MEMO), cache=ref["cache"])


def chunk_of(rows, i):
    """The cursor at which row i's chunk begins."""
    return int(rows.start[i]) - (int(rows.hits[i][1]) if rows.valid[i] else 0)


def fill_short_hits(ref, cursors):
    """The specification asks for a chunk's short hit only where step 2 or its sensitive_chunks counter reads it; for
    round_bounds every chunk whose whole-chunk position is not 0 needs one, so the missing ones are added to the cache,
    by the correlator the specification uses."""
    import framer_spec as fs
    import oracle
    stream, cache, span = ref["stream"], ref["cache"], F // 16
    words = fs.HRIT_WORDS if ref["hrit"] else fs.LRIT_WORDS
    for c in cursors:
        if cache[(c, F)][1] != 0 and (c, span) not in cache:
            cache[(c, span)] = tuple(int(v) for v in oracle.sync_correlate(stream[c:c + span], words, span)[0])


def nz_s0(rows, cache):
    """Per row: (the whole-chunk position is not 0, the short position is 0)."""
    out = []
    for i in range(len(rows)):
        c = chunk_of(rows, i)
        nz = cache[(c, F)][1] != 0
        out.append((nz, cache[(c, F // 16)][1] == 0 if nz else True))
    return out


def round_bounds(rows_of_a_call, cache, stop=None):
    """(lower, upper) for the rounds a call takes, from the specification's rows of that call and its hit cache alone.
    A round begins with ok and fc known and stops only at a chunk that hangs on them: whole-chunk position not 0 (nz), short
    position 0 (s0).  That chunk is the first row of the next round, so upper = 1 + the rows that are nz and s0.  Such a
    row whose mode is SHORT behind a valid row of its call cannot have been decided in that row's round (ok is not known
    behind it), so it is the first row of a round of its own: lower = 1 + those rows.  `stop`: the cursor of the chunk at
    which the call stopped for want of symbols (step 5), if it did; a round may have stopped at that chunk as well, and
    the round behind it then emits no row."""
    import lock_spec as ls
    rows = rows_of_a_call
    flags = nz_s0(rows, cache)
    lower = upper = 1
    for i, (nz, s0) in enumerate(flags):
        if nz and s0:
            upper += 1
            if (int(rows.mode[i]) & 3) == ls.SHORT and i > 0 and rows.valid[i - 1]:
                lower += 1
    if stop is not None and cache[(stop, F)][1] != 0 and cache[(stop, F // 16)][1] == 0:
        upper += 1
    return lower, upper


def fck0_rows(rows_of_a_call, cache):
    """The nz and s0 rows that the device reaches with fc not known: between the nz and s0 row before (or the call's
    start) and this one a valid row is directly followed by a row that is nz and not s0 -- MISS if the valid row's frame
    was good, FULL if not, so fc is 0 or what it was."""
    rows = rows_of_a_call
    flags = nz_s0(rows, cache)
    out, lost = [], False
    for i, (nz, s0) in enumerate(flags):
        if nz and s0:
            if lost:
                out.append(i)
            lost = False
        elif nz and i > 0 and rows.valid[i - 1]:
            lost = True
    return out


def long_reference(recheck, n=192, hrit=False):
    """The specification's walk of long_stream(n, hrit=hrit) pushed whole, once per process and not to be changed:
    dict(stream, kinds, hrit, rows, stats, cache, bounds); the cache holds the short hit of every row that is nz."""
    import lock_spec as ls
    skey = ("long", n, hrit)
    if skey not in _REFERENCE:
        _REFERENCE[skey] = long_stream(n=n, hrit=hrit) + ({},)
    stream, kinds, cache = _REFERENCE[skey]
    key = skey + (recheck,)
    if key not in _REFERENCE:
        ref = dict(stream=stream, kinds=kinds, hrit=hrit, cache=cache)
        rows, _, lk = ls.walk(stream, recheck=recheck, hrit=hrit, decode=memo_decode(hrit, MEMO), cache=cache)
        fill_short_hits(ref, [chunk_of(rows, i) for i in range(len(rows))])
        ref.update(rows=rows, stats=lk.stats(), bounds=round_bounds(rows, cache))
        _REFERENCE[key] = ref
    return _REFERENCE[key]


def pieces_of(stream, cuts):
    edges = [0] + list(cuts) + [len(stream)]
    return [stream[a:b] for a, b in zip(edges[:-1], edges[1:])]


def long_cuttings(length):
    """The cuttings both tiers run the long stream in: three of framer_cases.cuttings (each with calls of 0, 1, F - 1 and F
    symbols, a cut inside frame 3's sync word and one at frame 3's last symbol) and one every 40 000 symbols."""
    return fc.cuttings(length, F, LEAD + 3 * F, LEAD + 4 * F, count=3) + [list(range(40000, length, 40000))]


def batch_reference(recheck, at, seed=9):
    """long_stream's frames with no noise in front, tiled to at + 6 frames, and a plant in frame `at` (at >= 64): chunk i is
    frame i, entered with fc = (i - 1) % recheck + 1, and with walker segments of 128 chunks the first 64 rows are a whole
    batch in lock.  The specification's walk, once per process: dict(stream, hrit, rows, stats, cache, bounds)."""
    import lock_spec as ls
    skey = ("batch", at, seed)
    if skey not in _REFERENCE:
        tile, _ = fc.coded_frames(8, np.random.default_rng(seed))
        frames = [tile[i % 8].copy() for i in range(at + 6)]
        plant(frames, at)
        _REFERENCE[skey] = (np.concatenate(frames), {})
    stream, cache = _REFERENCE[skey]
    key = skey + (recheck,)
    if key not in _REFERENCE:
        ref = dict(stream=stream, hrit=False, cache=cache)
        rows, _, lk = ls.walk(stream, recheck=recheck, decode=memo_decode(False, MEMO), cache=cache)
        fill_short_hits(ref, [chunk_of(rows, i) for i in range(len(rows))])
        ref.update(rows=rows, stats=lk.stats(), bounds=round_bounds(rows, cache))
        _REFERENCE[key] = ref
    return _REFERENCE[key]


def stop_of(spec):
    """The chunk at which the specification's last call stopped for want of symbols, or None."""
    return spec.cursor if spec.cursor + F <= spec.end else None


def reference(name, recheck):
    """The specification's walk of a named stream pushed whole, computed once per process and not to be changed:
    dict(stream, starts, hrit, rows, stats, cache); `cache` is for further walks of the same stream."""
    import lock_spec as ls
    kw = {**TABLE, **MORE}[name]
    key = (name, recheck)
    if key not in _REFERENCE:
        if ("stream", name) not in _REFERENCE:
            _REFERENCE[("stream", name)] = stream_a(**kw) + ({},)
        stream, starts, cache = _REFERENCE[("stream", name)]
        hrit = bool(kw.get("hrit", False))
        rows, _, lk = ls.walk(stream, recheck=recheck, hrit=hrit, cache=cache)
        _REFERENCE[key] = dict(stream=stream, starts=starts, hrit=hrit, rows=rows, stats=lk.stats(), cache=cache)
    return _REFERENCE[key]
