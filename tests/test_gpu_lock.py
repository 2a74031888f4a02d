"""GPU tier: the frame lock (xrit_lock_*, FrameLock) against the specification of tests/lock_spec.py -- all eight outputs,
the count and the counters of every call compared exactly: the table of streams on which the flywheel shows, pushed whole
(a stop for an RS outcome and a second round) and cut (the outcome comes from the committed state), HRIT, a short hit
below the acceptance, empty and tiny calls, segment lengths and resident windows, reset, recheck = 1 against
FrameSynchroniser followed by FrameDecoder, the device path with the demultiplexer behind it, the error paths; and a long
damaged stream (192 frames, up to 10 rounds in a call) at recheck 2, 3, 4, 5, 255 and 1, whole, with other segments, cut
into calls, as HRIT and on the device path, its rounds within the bounds the specification's rows set; whole batches of 64
frames in lock at eight rechecks, and in front of a planted chunk that shows the fc they left."""
import ctypes as C

import numpy as np
import pytest

import framer_cases as fc
import framer_spec as fs
import lock_cases as lc
import lock_spec as ls

pytestmark = pytest.mark.gpu

F = fs.FRAME
# The counters the specification has are compared with it, every one.  `rounds`, `rewalked_chunks`, `adopted_chunks` and
# `calls` say how the device went about it; the specification has none of them and the tests assert them one by one.
COUNTERS = ls.STATS


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


def pieces_of(stream, cuts):
    edges = [0] + list(cuts) + [len(stream)]
    return [stream[a:b] for a, b in zip(edges[:-1], edges[1:])]


def check_stats(lock, spec):
    got, want = lock.stats(), spec.stats()
    print("stats", {k: int(got[k]) for k in got.dtype.names})
    assert [int(got[k]) for k in COUNTERS] == [want[k] for k in COUNTERS]
    return got


def push_and_compare(lock, spec, pieces):
    """Every piece through the host path and through the specification: the call's rows, the absent rows behind them and
    the count must agree; returns all rows of the device."""
    parts = []
    for piece in pieces:
        want = spec.push(piece)
        *out, count = lock.push(piece, trim=False)
        cap = fs.rows_cap(len(piece), F)
        assert len(out[1]) == cap == lock.rows(len(piece))
        assert count == len(want), (count, len(want), len(piece))
        got = ls.Rows(F, **{f: a[:count] for f, a in zip(ls.FIELDS, out)})
        got.info = got.info.view(ls.INFO_DTYPE)
        for f in ls.FIELDS:
            assert np.array_equal(getattr(got, f), getattr(want, f)), (f, len(piece))
        rest = dict(zip(ls.FIELDS, (a[count:] for a in out)))
        assert not any(rest[f].any() for f in ls.FIELDS if f != "info")
        absent = rest["info"].view(ls.INFO_DTYPE)
        assert (absent["rs_errors"] == -1).all() and not any(absent[f].any() for f in absent.dtype.names if f != "rs_errors")
        parts.append(got)
    return ls.Rows.concat(parts, F)


def spec_for(ref, recheck):
    return ls.Lock(hrit=ref["hrit"], recheck=recheck, cache=ref["cache"])


@pytest.mark.parametrize("recheck", [4, 1])
@pytest.mark.parametrize("name", list(lc.TABLE) + list(lc.MORE))
def test_streams_pushed_whole(xa, oracle_mod, name, recheck):
    ref = lc.reference(name, recheck)
    lock = xa.FrameLock("hrit" if ref["hrit"] else "lrit", flywheel=recheck)
    spec = spec_for(ref, recheck)
    got = push_and_compare(lock, spec, [ref["stream"]])
    assert got.same_as(ref["rows"])
    st = check_stats(lock, spec)
    # a second round exactly where a chunk hangs on the RS outcome of a frame of the same call
    sensitive = {"plant2": 1, "plant2_hrit": 1, "bad5_plant6": 1, "weak2": 1}.get(name, 0) if recheck == 4 else 0
    assert int(st["sensitive_chunks"]) == sensitive and int(st["rounds"]) == 1 + sensitive and int(st["calls"]) == 1
    lock.close()


def test_the_flywheel_keeps_the_frames_the_plain_walk_loses(xa, oracle_mod):
    a, b = lc.reference("plant2", 4), lc.reference("plant2", 1)
    out = {}
    for recheck in (4, 1):
        lock = xa.FrameLock("lrit", flywheel=recheck)
        out[recheck] = lock.push(a["stream"])
        lock.close()
    assert len(out[4][1]) == 12 and int(out[4][7]["ok"].sum()) == 12 and out[4][4][2] == xa.LOCK_SHORT
    assert len(out[1][1]) == 11 and int(out[1][7]["ok"].sum()) == 10 and int(out[1][3][2]) == 38468
    assert np.array_equal(out[4][6][:, :892], lc.sent_vcdus()) and len(b["rows"]) == 11


def test_outcome_from_the_committed_state_when_the_governing_frame_is_a_call_back(xa, oracle_mod):
    ref = lc.reference("plant2", 4)
    lock, spec = xa.FrameLock("lrit"), spec_for(ref, 4)                 # the default is 4
    for i, piece in enumerate(pieces_of(ref["stream"], [int(ref["starts"][2])])):
        push_and_compare(lock, spec, [piece])
        assert int(lock.stats()["rounds"]) == i + 1                     # one round per call: nothing to wait for
    st = check_stats(lock, spec)
    assert int(st["sensitive_chunks"]) == 1 and int(st["short_kept"]) == 9 and int(st["frames_ok"]) == 12
    lock.close()


def test_cuttings_with_empty_tiny_and_frame_sized_calls(xa, oracle_mod):
    ref = lc.reference("plant2", 4)
    stream, starts = ref["stream"], ref["starts"]
    lock = xa.FrameLock("lrit")
    fixed = [0, 1, F, 2 * F, int(starts[3]) + 31, int(starts[7]) + F - 1]       # calls of 0, 1, F - 1 and F symbols
    assert [len(p) for p in pieces_of(stream, fixed)[:4]] == [0, 1, F - 1, F]
    cuttings = [fixed, [int(starts[2]) + F + 100], [int(starts[2]) + 1, int(starts[2]) + F - 1]]
    cuttings += fc.cuttings(len(stream), F, int(starts[5]), int(starts[7]) + F, count=3)
    for cuts in cuttings:
        lock.reset()
        spec = spec_for(ref, 4)
        got = push_and_compare(lock, spec, pieces_of(stream, cuts))
        assert got.same_as(ref["rows"]), cuts
        check_stats(lock, spec)
    lock.close()


def test_stop_for_want_of_symbols_on_a_recheck_chunk(xa, oracle_mod):
    ref = lc.reference("plant4", 4)
    lock, spec = xa.FrameLock("lrit"), spec_for(ref, 4)
    got = push_and_compare(lock, spec, pieces_of(ref["stream"], [int(ref["starts"][4]) + F + 100]))
    assert got.same_as(ref["rows"]) and int(check_stats(lock, spec)["rechecks"]) == 2
    lock.close()


def test_segment_length_and_resident_windows_do_not_show(xa, oracle_mod):
    ref = lc.reference("slip1_plant4", 4)
    for kw in (dict(segment=1), dict(segment=2), dict(segment=7), dict(), dict(windows=1)):
        lock, spec = xa.FrameLock("lrit", **kw), spec_for(ref, 4)
        got = push_and_compare(lock, spec, pieces_of(ref["stream"], [100000]))
        assert got.same_as(ref["rows"]), kw
        check_stats(lock, spec)
        lock.close()
    ref = lc.reference("plant2", 4)                                      # ... nor where the walk leaves a walker's record
    for segment in (1, 2, 7):
        lock, spec = xa.FrameLock("lrit", segment=segment), spec_for(ref, 4)
        assert push_and_compare(lock, spec, [ref["stream"]]).same_as(ref["rows"]), segment
        lock.close()


def test_reset_in_mid_stream(xa, oracle_mod):
    ref = lc.reference("plant2", 4)
    lock = xa.FrameLock("lrit")
    lock.push(ref["stream"][:100001])
    st = lock.stats()
    assert int(st["carry"]) > 0 and int(st["frames_ok"]) > 0
    lock.reset()
    assert not any(int(v) for v in lock.stats())
    spec = spec_for(ref, 4)
    assert push_and_compare(lock, spec, [ref["stream"]]).same_as(ref["rows"])       # ok, fc and the decoder's carry too
    check_stats(lock, spec)
    lock.close()


def test_recheck_1_is_the_synchroniser_then_the_decoder(xa, oracle_mod):
    stream, _, _, _ = fc.drifting_stream(offset=16300, n=14, inserts=(3, 8))
    lock, sync, dec = xa.FrameLock("lrit", flywheel=1), xa.FrameSynchroniser("lrit"), xa.FrameDecoder("lrit")
    total = 0
    for piece in pieces_of(stream, [70000, 70001, 150000]):
        frames, valid, hits, start, mode, cadu, block, info, count = lock.push(piece, trim=False)
        w_frames, w_valid, w_hits, w_start, w_count = sync.push(piece, trim=False)
        w_cadu, w_block, w_info = dec.decode(w_frames, w_valid)
        assert count == w_count
        for got, want in ((frames, w_frames), (valid, w_valid), (hits, w_hits), (start, w_start), (cadu, w_cadu), (block, w_block)):
            assert np.array_equal(got, want)
        assert info.tobytes() == w_info.tobytes()
        total += count
    assert total == 14
    a, b = lock.stats(), sync.stats()
    assert [int(a[k]) for k in b.dtype.names] == [int(b[k]) for k in b.dtype.names]
    for h in (lock, sync, dec):
        h.close()


def test_device_path_with_the_demultiplexer_behind_it(xa, oracle_mod):
    """push_device on a side stream into poisoned buffers, xrit_demux_process_device on its outputs as they are."""
    torch = pytest.importorskip("torch")
    ref = lc.reference("plant2", 4)
    stream = ref["stream"]
    dev = torch.device("cuda:0")
    lock, dm, dm2 = xa.FrameLock("lrit"), xa.ChannelDemux(), xa.ChannelDemux()
    host = xa.FrameLock("lrit")
    s = torch.cuda.Stream(device=dev)
    d_sym = torch.from_numpy(stream.view(np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    n, cap = len(stream), lock.rows(len(stream))
    sizes = dict(frames=cap * F, valid=cap, hits=cap * 16, start=cap * 8, mode=cap, cadu=cap * 1024, block=cap * 1020,
                 info=cap * 40, count=4, vcdu=cap * 892, off=65 * 4, rec=cap * 88)
    b = {k: torch.full((v,), 0xAB, dtype=torch.uint8, device=dev) for k, v in sizes.items()}
    with torch.cuda.stream(s):
        lock.push_device(d_sym.data_ptr(), n, *(b[k].data_ptr() for k in ("frames", "valid", "hits", "start", "mode", "cadu",
                                                                          "block", "info", "count")), stream=s.cuda_stream)
        dm.process_device(b["hits"].data_ptr(), b["cadu"].data_ptr(), b["block"].data_ptr(), b["info"].data_ptr(), cap,
                          b["vcdu"].data_ptr(), b["off"].data_ptr(), b["rec"].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    want = host.push(stream, trim=False)
    dtypes = dict(frames=np.int8, hits=np.uint32, start=np.uint64, info=xa.FRAME_INFO_DTYPE)
    for k, w in zip(ls.FIELDS, want):
        assert b[k].cpu().numpy().view(dtypes.get(k, np.uint8)).reshape(w.shape).tobytes() == w.tobytes(), k
    assert int(b["count"].cpu().numpy().view(np.uint32)[0]) == want[8] == 12
    w_vcdu, w_off, w_rec = dm2.process(want[2], want[5], want[6], want[7])[:3]
    off = b["off"].cpu().numpy().view(np.uint32)
    assert np.array_equal(off, w_off) and int(off[64]) == 12
    assert np.array_equal(b["vcdu"].cpu().numpy()[:12 * 892].reshape(12, 892), np.asarray(w_vcdu).reshape(-1, 892)[:12])
    for h in (lock, host, dm, dm2):
        h.close()


def test_error_paths(xa, oracle_mod):
    L = xa.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.xrit_lock_push_device(None, p, 1, p, p, p, p, p, p, p, p, p, None) == -1
    assert L.xrit_lock_push(None, p, 1, p, p, p, p, p, p, p, p) == -1 and L.xrit_lock_stats(None, p) == -1
    assert L.xrit_lock_reset(None) == -1 and L.xrit_lock_set_flywheel(None, 4) == -1 and L.xrit_lock_rows(None, 9) == 0
    assert L.xrit_lock_set_segment(None, 4) == -1 and L.xrit_lock_set_windows(None, 4) == -1
    assert L.xrit_lock_create(None, 0, 0) == -1
    lock = xa.FrameLock("lrit")
    for recheck in (0, 256):
        with pytest.raises(xa.XritError) as ei:
            lock.set_flywheel(recheck)
        assert ei.value.code == -1 and "1..255" in str(ei.value)
    assert L.xrit_lock_push_device(lock._h, p, (1 << 30) + 1, p, p, p, p, p, p, p, p, p, None) == -1     # before anything is read
    assert L.xrit_lock_push_device(lock._h, None, 5, p, p, p, p, p, p, p, p, p, None) == -1
    assert L.xrit_lock_push_device(lock._h, p, 5, p, p, p, p, None, p, p, p, p, None) == -1
    lock.set_flywheel(255)                                       # still allowed: nothing has been pushed
    lock.set_flywheel(4)
    ref = lc.reference("plant2", 4)
    assert len(lock.push(ref["stream"][:100])[1]) == 0
    with pytest.raises(xa.XritError) as ei:
        lock.set_flywheel(4)
    assert ei.value.code == -1 and "before the first push" in str(ei.value)
    lock.set_segment(3)                                          # segment and windows may change between calls
    lock.set_windows(2)
    got = lock.push(ref["stream"][100:])
    assert np.array_equal(got[3], ref["rows"].start)
    with pytest.raises(ValueError):
        xa.FrameLock("xrit")
    lock.close()


def test_hundreds_of_frames_in_lock_with_whole_waves_of_records(xa, oracle_mod):
    """600 aligned frames (8 coded frames tiled) with walker segments of 128 chunks, so that joints and commit take 64
    rows at a time: recheck 1 against FrameSynchroniser followed by FrameDecoder, every other recheck with the same rows
    and the modes of a stream in lock."""
    frames, _ = fc.coded_frames(8, np.random.default_rng(3))
    n = 600
    stream = np.tile(frames.reshape(-1), n // 8)
    sync, dec = xa.FrameSynchroniser("lrit", segment=128), xa.FrameDecoder("lrit")
    w = sync.push(stream, trim=False)
    w_cadu, w_block, w_info = dec.decode(w[0], w[1])
    assert w[4] == n and int(w_info["ok"].sum()) == n
    # 3, 5, 7: a whole batch of 64 does not return fc to where it was; 255: fc == recheck falls once, inside a batch; 64: on
    # a batch's edge
    for recheck in (1, 2, 3, 4, 5, 7, 64, 255):
        lock = xa.FrameLock("lrit", flywheel=recheck, segment=128)
        frames_, valid, hits, start, mode, cadu, block, info, count = lock.push(stream, trim=False)
        st = lock.stats()
        print("recheck", recheck, {k: int(st[k]) for k in st.dtype.names})
        assert count == n
        for name, got, want in (("frames", frames_, w[0]), ("valid", valid, w[1]), ("hits", hits, w[2]), ("start", start, w[3]),
                                ("cadu", cadu, w_cadu), ("block", block, w_block)):
            assert np.array_equal(got, want), name
        assert info.tobytes() == w_info.tobytes()
        fc_entry = [0] + [(i - 1) % recheck + 1 for i in range(1, n)]              # fc at the entry of chunk i
        want_mode = [4 if f == recheck else (1 if i else 0) for i, f in enumerate(fc_entry)]
        assert mode[:n].tolist() == want_mode and not mode[n:].any()
        assert int(st["frames_ok"]) == n and int(st["frames_bad"]) == 0 and int(st["frames"]) == n
        assert int(st["rechecks"]) == sum(m == 4 for m in want_mode) and int(st["short_kept"]) == sum(m == 1 for m in want_mode)
        assert int(st["short_missed"]) == 0 and int(st["sensitive_chunks"]) == 0 and int(st["rounds"]) == 1
        assert int(st["rewalked_chunks"]) == 0 and int(st["adopted_chunks"]) == n
        lock.close()
    sync.close()
    dec.close()


def test_recheck_1_adopts_batches_out_of_lock_in_parallel(xa, oracle_mod):
    """200 frames (8 coded frames tiled) with the last symbol of every 50th frame deleted and one chunk zeroed, walker
    segments of 128 chunks, two calls cut in mid-frame: with flywheel = 1 the joints copy a walker's record, longer than a
    wave and not all in lock, batch by batch.  The synchroniser against the specification first, then the lock against
    the synchroniser followed by the decoder; once more with segments of 7 chunks, real steps and adoption in one call."""
    frames, _ = fc.coded_frames(8, np.random.default_rng(3))
    sent = np.tile(frames, (25, 1))
    sent[20] = 0
    stream = np.concatenate([f[:-1] if i % 50 == 49 else f for i, f in enumerate(sent)])
    cuts = [140 * F + 5000]
    assert len(stream) == 200 * F - 4
    want_rows, per_call, spec = fs.walk(stream, cuts)
    assert spec.resyncs >= 3 and spec.dropped >= 1 and len(want_rows) > 128 and len(per_call[0]) > 128
    assert int(want_rows.hits[0][1]) == 0                               # the stream's first chunk is a frame at position 0

    sync, dec = xa.FrameSynchroniser("lrit", segment=128), xa.FrameDecoder("lrit")
    want = []
    for piece, rows in zip(pieces_of(stream, cuts), per_call):
        w = sync.push(piece, trim=False)
        assert w[4] == len(rows)
        for name, got in zip(("frames", "valid", "hits", "start"), w):
            assert np.array_equal(got[:w[4]], getattr(rows, name)), name
            assert not got[w[4]:].any(), name
        want.append(w + dec.decode(w[0], w[1]))
    b = sync.stats()
    assert [int(b[k]) for k in fs.STATS] == [spec.stats()[k] for k in fs.STATS]

    for segment in (128, 7):
        lock = xa.FrameLock("lrit", flywheel=1, segment=segment)
        first = True
        for piece, w in zip(pieces_of(stream, cuts), want):
            *out, count = lock.push(piece, trim=False)
            assert count == w[4]
            for name, got, wanted in zip(ls.FIELDS, out, w[:4] + (None,) + w[5:]):
                if name == "mode":
                    want_mode = [xa.LOCK_FULL | xa.LOCK_RECHECK] * count + [0] * (len(got) - count)
                    if first:
                        want_mode[0] = xa.LOCK_FULL
                    assert got.tolist() == want_mode
                elif name == "info":
                    assert got.tobytes() == wanted.tobytes()
                else:
                    assert np.array_equal(got, wanted), (name, segment)
            first = False
        a = lock.stats()
        print("segment", segment, {k: int(a[k]) for k in a.dtype.names})
        if segment == 128:
            assert [int(a[k]) for k in b.dtype.names] == [int(b[k]) for k in b.dtype.names]
            assert int(a["adopted_chunks"]) > 64
            assert int(a["short_kept"]) == int(a["short_missed"]) == int(a["sensitive_chunks"]) == 0
            assert int(a["rounds"]) == int(a["calls"]) == 2
        lock.close()
    sync.close()
    dec.close()


def test_recheck_1_counts_the_first_chunk_behind_a_reset_sensitive(xa, oracle_mod):
    """A plant in frame 0 and nothing in front of it: the stream's first chunk is entered with fc = 0 != recheck, its
    whole-chunk hit is the plant and its short hit is at position 0.  With flywheel = 1 the chunk is FULL and follows the
    plant, and it is the one chunk that sensitive_chunks can count: whether the first call emits a row or none, and not
    again behind it or in the calls that follow."""
    stream, starts = lc.stream_a(plants=(0,))
    stream = stream[int(starts[0]):]
    for cuts in ([], [100, 5 * F]):
        lock, spec = xa.FrameLock("lrit", flywheel=1), ls.Lock(recheck=1)
        got = push_and_compare(lock, spec, pieces_of(stream, cuts))
        assert int(got.hits[0][1]) == lc.PLANT_AT and int(got.mode[0]) == xa.LOCK_FULL
        st = check_stats(lock, spec)
        assert int(st["sensitive_chunks"]) == 1 and int(st["rounds"]) == int(st["calls"]) == len(cuts) + 1
        lock.close()


# ---- the long damaged stream (lock_cases.long_stream): many rounds in a call, whole batches of records between them ----
def long_pair(xa, ref, recheck, **kw):
    return xa.FrameLock("hrit" if ref["hrit"] else "lrit", flywheel=recheck, **kw), lc.long_lock(ref, recheck)


def check_how_it_went(st, rows, bounds, recheck, calls=1):
    """The device's own counters: rounds within the bounds the specification's rows give, every row walked or adopted."""
    rounds, rewalked, adopted = int(st["rounds"]), int(st["rewalked_chunks"]), int(st["adopted_chunks"])
    print("recheck", recheck, "rounds", rounds, "bounds", bounds, "rewalked", rewalked, "adopted", adopted, "rows", len(rows))
    if recheck == 1:
        assert rounds == calls
    else:
        assert bounds[0] <= rounds <= bounds[1]
    assert rewalked + adopted == len(rows) and int(st["calls"]) == calls


@pytest.mark.parametrize("recheck", [2, 3, 4, 5, 255, 1])
def test_long_damaged_stream_pushed_whole(xa, oracle_mod, recheck):
    ref = lc.long_reference(recheck)
    lock, spec = long_pair(xa, ref, recheck)
    got = push_and_compare(lock, spec, [ref["stream"]])
    assert got.same_as(ref["rows"])
    st = check_stats(lock, spec)
    check_how_it_went(st, got, ref["bounds"], recheck)
    assert int(st["rewalked_chunks"]) > 0 and int(st["adopted_chunks"]) > 64
    lock.close()


@pytest.mark.parametrize("kw", [dict(segment=1), dict(segment=7), dict(segment=128), dict(windows=1)], ids=str)
@pytest.mark.parametrize("recheck", [4, 3])
def test_long_damaged_stream_whatever_the_walkers_segments(xa, oracle_mod, recheck, kw):
    """Segments of 1 chunk (every record a single step), of 7 (records entered in their middle behind a rewalk), of 128
    (batches of 64 records that mix good, bad and dropped frames, MISS and SHORT chunks), and one resident window."""
    ref = lc.long_reference(recheck)
    lock, spec = long_pair(xa, ref, recheck, **kw)
    got = push_and_compare(lock, spec, [ref["stream"]])
    assert got.same_as(ref["rows"])
    check_how_it_went(check_stats(lock, spec), got, ref["bounds"], recheck)
    lock.close()


def sensitive_cuttings(ref):
    """Cuts at rows that only a known ok = true decides (SHORT at position 0 against a whole-chunk hit elsewhere, behind
    a valid row): 100 symbols behind the row's chunk, on the chunk's first symbol, in the middle of the frame before it --
    each alone at one such row, and the three in one cutting at three such rows."""
    rows, flags = ref["rows"], lc.nz_s0(ref["rows"], ref["cache"])
    at = [i for i, (nz, s0) in enumerate(flags) if nz and s0 and (int(rows.mode[i]) & 3) == ls.SHORT and rows.valid[i - 1]]
    a, b, c = (lc.chunk_of(rows, i) for i in (at[0], at[len(at) // 2], at[-1]))
    assert a + 2 * F < b < c - 2 * F
    return [[b + F + 100], [b], [b - F // 2], [a + F + 100, b, c - F // 2]]


@pytest.mark.parametrize("recheck", [4, 5])
def test_long_damaged_stream_cut_into_calls(xa, oracle_mod, recheck):
    ref = lc.long_reference(recheck)
    stream = ref["stream"]
    lock = xa.FrameLock("lrit", flywheel=recheck)
    for cuts in lc.long_cuttings(len(stream)) + sensitive_cuttings(ref):
        lock.reset()
        spec = lc.long_lock(ref, recheck)
        pieces, parts, lower, upper, rounds = pieces_of(stream, cuts), [], 0, 0, 0
        for piece in pieces:
            parts.append(push_and_compare(lock, spec, [piece]))
            st = check_stats(lock, spec)
            stop = lc.stop_of(spec)
            lc.fill_short_hits(ref, [] if stop is None else [stop])
            lo, hi = lc.round_bounds(parts[-1], ref["cache"], stop)
            assert lo <= int(st["rounds"]) - rounds <= hi, (cuts, len(parts))
            lower, upper, rounds = lower + lo, upper + hi, int(st["rounds"])
        got = ls.Rows.concat(parts, F)
        assert got.same_as(ref["rows"]), cuts
        print("cuts", len(cuts), "rounds", rounds, "bounds", (lower, upper))
        assert lower <= rounds <= upper and int(st["calls"]) == len(pieces)
        assert int(st["rewalked_chunks"]) + int(st["adopted_chunks"]) == len(got)
    lock.close()


def test_long_damaged_stream_hrit(xa, oracle_mod):
    ref = lc.long_reference(4, n=96, hrit=True)
    stream = ref["stream"]
    assert ref["stats"]["sensitive_chunks"] >= 2 and ref["stats"]["short_missed"] >= 2 and ref["bounds"][0] >= 2
    for cuts in ([], [len(stream) // 2 + 4321]):
        lock, spec = long_pair(xa, ref, 4)
        pieces = pieces_of(stream, cuts)
        got = push_and_compare(lock, spec, pieces)
        assert got.same_as(ref["rows"])
        st = check_stats(lock, spec)
        assert int(st["calls"]) == len(pieces) and int(st["rewalked_chunks"]) + int(st["adopted_chunks"]) == len(got)
        if not cuts:
            check_how_it_went(st, got, ref["bounds"], 4)
        lock.close()


def test_long_damaged_stream_on_the_device_path_with_the_demultiplexer_behind_it(xa, oracle_mod):
    """Many rounds with a stage waiting behind them: push_device at recheck 4 on a side stream into poisoned buffers,
    xrit_demux_process_device queued behind it on all rows_cap rows; the demultiplexer's outputs against those it gives
    on the host path's rows."""
    torch = pytest.importorskip("torch")
    ref = lc.long_reference(4)
    stream = ref["stream"]
    dev = torch.device("cuda:0")
    lock, dm, dm2 = xa.FrameLock("lrit", flywheel=4), xa.ChannelDemux(), xa.ChannelDemux()
    host = xa.FrameLock("lrit", flywheel=4)
    s = torch.cuda.Stream(device=dev)
    d_sym = torch.from_numpy(stream.view(np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    n, cap = len(stream), lock.rows(len(stream))
    sizes = dict(frames=cap * F, valid=cap, hits=cap * 16, start=cap * 8, mode=cap, cadu=cap * 1024, block=cap * 1020,
                 info=cap * 40, count=4, vcdu=cap * 892, off=65 * 4, rec=cap * 88)
    b = {k: torch.full((v,), 0xAB, dtype=torch.uint8, device=dev) for k, v in sizes.items()}
    with torch.cuda.stream(s):
        lock.push_device(d_sym.data_ptr(), n, *(b[k].data_ptr() for k in ("frames", "valid", "hits", "start", "mode", "cadu",
                                                                          "block", "info", "count")), stream=s.cuda_stream)
        dm.process_device(b["hits"].data_ptr(), b["cadu"].data_ptr(), b["block"].data_ptr(), b["info"].data_ptr(), cap,
                          b["vcdu"].data_ptr(), b["off"].data_ptr(), b["rec"].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    want = host.push(stream, trim=False)
    rows = ref["rows"]
    assert want[8] == len(rows) and all(np.array_equal(w[:len(rows)], getattr(rows, f)) for f, w in zip(ls.FIELDS[:7], want))
    dtypes = dict(frames=np.int8, hits=np.uint32, start=np.uint64, info=xa.FRAME_INFO_DTYPE)
    for k, w in zip(ls.FIELDS, want):
        assert b[k].cpu().numpy().view(dtypes.get(k, np.uint8)).reshape(w.shape).tobytes() == w.tobytes(), k
    assert int(b["count"].cpu().numpy().view(np.uint32)[0]) == want[8]
    st = lock.stats()
    assert ref["bounds"][0] <= int(st["rounds"]) <= ref["bounds"][1] and int(st["rounds"]) == int(host.stats()["rounds"])
    w_vcdu, w_off, w_rec = dm2.process(want[2], want[5], want[6], want[7])
    good = ref["stats"]["frames_ok"]
    off = b["off"].cpu().numpy().view(np.uint32)
    assert np.array_equal(off, w_off) and int(off[64]) == good == len(w_vcdu)
    assert np.array_equal(b["vcdu"].cpu().numpy()[:good * 892].reshape(good, 892), w_vcdu)
    rec = b["rec"].cpu().numpy().view(xa.FRAME_STATS_DTYPE)
    for f in rec.dtype.names:
        if f != "reserved":
            assert np.array_equal(rec[f], w_rec[f]), f
    a, c = dm.stats(), dm2.stats()
    for f in a.dtype.names:
        if f not in ("start_time", "reserved"):              # start_time: when each handle was made
            assert np.array_equal(a[f], c[f]), f
    for h in (lock, host, dm, dm2):
        h.close()


# a whole batch of 64 records in lock, then a planted chunk: (recheck, the planted frame, whether fc == recheck at its entry)
BATCH_CASES = [(2, 64, True), (4, 64, True), (64, 64, True), (3, 66, True), (5, 65, True), (7, 70, True),
               (3, 64, False), (5, 64, False), (255, 64, False), (4, 65, False), (64, 65, False)]


@pytest.mark.parametrize("recheck,at,due", BATCH_CASES)
def test_fc_behind_a_whole_batch_in_lock_decides_a_planted_chunk(xa, oracle_mod, recheck, at, due):
    """Walker segments of 128 chunks: the first 64 rows are adopted as a whole batch with fc in closed form, in the joints
    and in the commit.  The planted chunk behind them shows what fc the joints came out with.  Where fc == recheck at its
    entry, step 1 clears ok: the chunk is decided without the RS outcome of the row before it and the call is ONE round
    (fc is known: no chunk before it has a whole-chunk hit off position 0) -- a joints' fc that is not recheck there stops
    the round.  Everywhere else the chunk hangs on that RS outcome and the call is TWO rounds (round_bounds gives 2, 2) -- a
    joints' fc that is recheck there takes the plant, and the commit's replay refuses the round."""
    ref = lc.batch_reference(recheck, at)
    lock, spec = long_pair(xa, ref, recheck, segment=128)
    got = push_and_compare(lock, spec, [ref["stream"]])
    assert got.same_as(ref["rows"])
    st = check_stats(lock, spec)
    want_mode = (ls.FULL | ls.RECHECK) if due else ls.SHORT
    assert int(got.mode[at]) == want_mode and int(got.hits[at][1]) == (lc.PLANT_AT if due else 0)
    assert ref["bounds"] == ((1, 2) if due else (2, 2)) and int(st["rounds"]) == (1 if due else 2)
    assert int(st["rewalked_chunks"]) + int(st["adopted_chunks"]) == len(got) and int(st["adopted_chunks"]) >= 64
    lock.close()
