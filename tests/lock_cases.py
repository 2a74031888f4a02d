"""Streams the frame lock's tests share (tests/test_lock_spec.py, tests/test_gpu_lock.py, tests/test_gpu_lock_host.py):
12 coded frames behind 700 symbols of noise, with the two things the flywheel is about -- a frame whose sync word is
weakened while a clean copy of it stands 5000 symbols in (a *plant*), and a frame that Reed-Solomon rejects (*bad*)."""
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
