"""GPU tier: the stream frame synchroniser (xrit_framer_*, FrameSynchroniser) against the specification of
tests/framer_spec.py -- rows, frames, valid, hits, starts, count and the counters of every call compared exactly: a stream
whose sync word drifts, pushed whole and cut at random with empty and one-symbol calls between; the other phase; HRIT;
erasures; noise alone; tiny frames with many walker segments and joints; reset; two handles; the chain on the device
behind it with no read-back; the error paths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ccsds
import demux_spec as ds
import framer_cases as fc
import framer_spec as fs
import synth

pytestmark = pytest.mark.gpu

F = fs.FRAME
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


@pytest.fixture(scope="module")
def drifting(oracle_mod):
    stream, frames, starts, cadus = fc.drifting_stream(offset=16300)
    cache = {}
    rows, _, fr = fs.walk(stream, cache=cache)
    assert len(rows) == 40 and np.array_equal(rows.start, starts)
    return dict(stream=stream, frames=frames, starts=starts, cadus=cadus, rows=rows, cache=cache)


def check_stats(sync, spec):
    got = sync.stats()
    want = spec.stats()
    print("stats", {k: int(got[k]) for k in got.dtype.names})
    assert [int(got[k]) for k in fs.STATS] == [want[k] for k in fs.STATS]
    return got


def push_and_compare(sync, spec, pieces):
    """Every piece through the host path and through the specification: the call's rows, the zero rows behind them and the
    count must agree; returns all rows of the device."""
    parts = []
    for piece in pieces:
        want = spec.push(piece)
        frames, valid, hits, start, count = sync.push(piece, trim=False)
        cap = fs.rows_cap(len(piece), spec.frame)
        assert len(valid) == cap == sync.rows(len(piece))
        assert count == len(want), (count, len(want), len(piece))
        assert np.array_equal(valid[:count], want.valid) and np.array_equal(hits[:count], want.hits)
        assert np.array_equal(start[:count], want.start)
        assert np.array_equal(frames[:count], want.frames)
        assert not frames[count:].any() and not valid[count:].any() and not hits[count:].any() and not start[count:].any()
        parts.append(fs.Rows(spec.frame, frames[:count], valid[:count], hits[:count], start[:count]))
    return fs.Rows.concat(parts, spec.frame)


def pieces_of(stream, cuts):
    edges = [0] + list(cuts) + [len(stream)]
    return [stream[a:b] for a, b in zip(edges[:-1], edges[1:])]


def test_drifting_stream_whole_and_in_cuttings(xa, drifting):
    stream, starts = drifting["stream"], drifting["starts"]
    sync = xa.FrameSynchroniser("lrit")
    got = push_and_compare(sync, fs.Framer(cache=drifting["cache"]), [stream])
    assert len(got) == 40 and np.array_equal(got.frames, drifting["frames"])
    st = sync.stats()
    assert int(st["frames"]) == 40 and int(st["resyncs"]) == 3 and int(st["carry"]) == 0 and int(st["calls"]) == 1
    for i, cuts in enumerate(fc.cuttings(len(stream), F, int(starts[5]), int(starts[7]) + F)):
        pieces = pieces_of(stream, cuts)
        if i == 0:                                   # empty calls between
            pieces = [q for p in pieces for q in (p, p[:0])]
        if i == 1:                                   # one-symbol calls between
            pieces = [q for p in pieces for q in ((p[:1], p[1:]) if len(p) > 1 else (p,))]
        sync.reset()
        spec = fs.Framer(cache=drifting["cache"])
        got = push_and_compare(sync, spec, pieces)
        assert len(got) == 40 and np.array_equal(got.start, starts), cuts
        check_stats(sync, spec)
    sync.close()


def test_word_across_the_fixed_windows_boundary(xa, oracle_mod):
    """The stream begun at the last position a fixed window searches: every frame once (the fixed-window pair loses them,
    tests/test_framer_spec.py)."""
    stream, frames, starts, _ = fc.drifting_stream(offset=16319)
    sync, spec = xa.FrameSynchroniser("lrit"), fs.Framer()
    got = push_and_compare(sync, spec, pieces_of(stream, [100000, 300001]))
    assert np.array_equal(got.start, starts) and np.array_equal(got.frames, frames)
    check_stats(sync, spec)
    sync.close()


def test_lrit_phase_inverted_from_frame_15_on(xa, oracle_mod):
    rng = np.random.default_rng(4)
    frames, _ = fc.coded_frames(24, rng)
    stream = np.concatenate([rng.integers(-20, 21, 777).astype(np.int8), frames.reshape(-1)])
    at = 777 + 15 * F
    stream[at:] = (stream[at:].view(np.uint8) ^ 0xFF).view(np.int8)
    sync, spec = xa.FrameSynchroniser("lrit"), fs.Framer()
    got = push_and_compare(sync, spec, pieces_of(stream, [at + 5]))
    assert len(got) == 24 and got.hits[:15, 0].tolist() == [0] * 15 and got.hits[15:, 0].tolist() == [1] * 9
    assert np.array_equal(got.frames, frames)                   # inverted back
    check_stats(sync, spec)
    sync.close()


def test_hrit_words_never_invert(xa, oracle_mod):
    rng = np.random.default_rng(5)
    frames, _ = fc.coded_frames(10, rng, hrit=True)
    stream = np.concatenate([rng.integers(-20, 21, 33).astype(np.int8), frames.reshape(-1)])
    at = 33 + 4 * F
    stream[at:] = (stream[at:].view(np.uint8) ^ 0xFF).view(np.int8)
    sync, spec = xa.FrameSynchroniser("hrit"), fs.Framer(hrit=True)
    got = push_and_compare(sync, spec, [stream])
    assert len(got) == 10 and set(got.hits[:, 0].tolist()) == {0, 1}        # the raw word is kept
    assert np.array_equal(got.frames.reshape(-1), stream[33:])              # ... and nothing is inverted
    check_stats(sync, spec)
    sync.close()


def test_erased_chunk_is_dropped_and_the_walk_goes_on(xa, oracle_mod):
    rng = np.random.default_rng(6)
    frames, _ = fc.coded_frames(9, rng)
    stream = frames.reshape(-1).copy()
    stream[4 * F:5 * F] = 0
    sync, spec = xa.FrameSynchroniser("lrit"), fs.Framer()
    got = push_and_compare(sync, spec, pieces_of(stream, [4 * F + 9]))
    assert got.valid.tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1] and not got.frames[4].any() and int(got.start[4]) == 4 * F
    assert int(check_stats(sync, spec)["dropped_chunks"]) == 1
    sync.close()


def test_noise_alone_follows_the_chance_hits(xa, oracle_mod):
    stream = np.random.default_rng(7).integers(-128, 128, 64 * 1024).astype(np.int8)
    whole, _, _ = fs.walk(stream)
    assert len(whole) and (whole.hits[:, 2] >= 46).any()        # hits of 46 and more occur by chance
    for cuts in ([], [1, 20000, 40001]):
        sync, spec = xa.FrameSynchroniser("lrit"), fs.Framer()
        got = push_and_compare(sync, spec, pieces_of(stream, cuts))
        assert np.array_equal(got.hits, whole.hits) and np.array_equal(got.frames, whole.frames)
        check_stats(sync, spec)
        sync.close()


@pytest.fixture(scope="module")
def tiny(oracle_mod):
    """frame = 320: 3000 frames of random payload behind the LRIT word, a symbol deleted every 97 frames."""
    rng = np.random.default_rng(8)
    frame, n = 320, 3000
    word = np.array([60 if (fs.LRIT_WORDS[0] >> (63 - k)) & 1 else -60 for k in range(64)], np.int8)
    body = rng.choice(np.array([-60, 60], np.int8), (n, frame))
    body[:, :64] = word
    keep = np.ones(n * frame, bool)
    keep[np.arange(96, n, 97) * frame + frame - 1] = False
    stream = body.reshape(-1)[keep]
    cache = {}
    rows, _, spec = fs.walk(stream, frame=frame, cache=cache)
    assert len(rows) > 2500 and spec.stats()["resyncs"] > 10 and spec.stats()["dropped_chunks"] > 10
    return dict(stream=stream, frame=frame, rows=rows, cache=cache)


@pytest.mark.parametrize("segment", [1, 2, 7, 64, 0])
def test_tiny_frames_joints_and_rewalk(xa, tiny, segment):
    sync = xa.FrameSynchroniser("lrit", frame=tiny["frame"], segment=segment)
    spec = fs.Framer(frame=tiny["frame"], cache=tiny["cache"])
    cuts = [] if segment in (1, 64) else [123457, 500000]
    got = push_and_compare(sync, spec, pieces_of(tiny["stream"], cuts))
    assert len(got) == len(tiny["rows"]) and np.array_equal(got.start, tiny["rows"].start)
    st = check_stats(sync, spec)
    assert int(st["rewalked_chunks"]) + int(st["adopted_chunks"]) >= int(st["rows"])       # (a step that must wait emits no row)
    if segment in (1, 2, 7):
        assert int(st["rewalked_chunks"]) > 0                   # the nominal starts miss: joints walked again
    sync.close()


def test_rewalked_chunks_counts_a_chunk_once_when_it_is_consumed(xa, oracle_mod):
    """frame = 320, segments of one chunk, 10 frames behind 100 symbols of noise with one symbol inserted in front of
    frame 6: behind chunk 0 the chain never stands on a walker's start, so every step is a real one.  The first call ends
    one symbol short of frame 6: its real step must wait and is walked again in the second call.  It is counted there,
    once: rewalked_chunks + adopted_chunks is the number of rows after either call."""
    rng = np.random.default_rng(5)
    frame, n, offset = 320, 10, 100
    word = np.array([60 if (fs.LRIT_WORDS[0] >> (63 - k)) & 1 else -60 for k in range(64)], np.int8)
    body = rng.choice(np.array([-60, 60], np.int8), (n, frame))
    body[:, :64] = word
    noise = rng.integers(-20, 21, offset).astype(np.int8)
    stream = np.concatenate([noise, body[:6].reshape(-1), noise[:1], body[6:].reshape(-1)])
    cut = offset + 7 * frame                                    # frame 6 begins at offset + 6 * frame + 1
    sync, spec = xa.FrameSynchroniser("lrit", frame=frame, segment=1), fs.Framer(frame=frame)
    first = push_and_compare(sync, spec, [stream[:cut]])
    assert len(first) == 6 and spec.carry == frame              # the chunk at the cursor is whole, its frame is not
    st = check_stats(sync, spec)
    assert int(st["adopted_chunks"]) == 1 and int(st["rewalked_chunks"]) == 5
    rest = push_and_compare(sync, spec, [stream[cut:]])
    assert len(rest) == 4 and int(rest.hits[0][1]) == 1
    st = check_stats(sync, spec)
    assert int(st["rewalked_chunks"]) + int(st["adopted_chunks"]) == int(st["rows"]) == 10
    sync.close()


def test_reset_in_mid_stream(xa, drifting):
    stream = drifting["stream"]
    sync = xa.FrameSynchroniser("lrit")
    sync.push(stream[:200001])
    assert int(sync.stats()["carry"]) > 0
    sync.reset()
    assert not any(int(v) for v in sync.stats())
    got = push_and_compare(sync, fs.Framer(cache=drifting["cache"]), pieces_of(stream, [300000]))
    assert np.array_equal(got.start, drifting["starts"]) and np.array_equal(got.frames, drifting["frames"])
    sync.close()


def test_two_handles_do_not_disturb_each_other(xa, drifting, tiny):
    a, b = xa.FrameSynchroniser("lrit"), xa.FrameSynchroniser("lrit", frame=tiny["frame"])
    sa, sb = fs.Framer(cache=drifting["cache"]), fs.Framer(frame=tiny["frame"], cache=tiny["cache"])
    pa, pb = pieces_of(drifting["stream"], [70000, 400000]), pieces_of(tiny["stream"][:200000], [1000, 99999])
    ra, rb = [], []
    for x, y in zip(pa, pb):                                    # interleaved
        ra.append(push_and_compare(a, sa, [x]))
        rb.append(push_and_compare(b, sb, [y]))
    assert np.array_equal(fs.Rows.concat(ra, F).start, drifting["starts"])
    assert len(fs.Rows.concat(rb, tiny["frame"])) > 500
    check_stats(a, sa)
    check_stats(b, sb)
    a.close()
    b.close()


def test_chain_on_the_device_without_read_back(xa, drifting):
    """push_device -> xrit_decoder_decode_device -> xrit_demux_process_device on one stream with nf = rows(n), the
    inserted-symbol stream in three calls; VCDUs and records against tests/ccsds.py and tests/demux_spec.py on the
    specification's frames."""
    torch = pytest.importorskip("torch")
    stream = drifting["stream"]
    pieces = pieces_of(stream, [250000, 250001 + 9 * F])
    dev = torch.device("cuda:0")
    sync, dec, dm = xa.FrameSynchroniser("lrit"), xa.FrameDecoder("lrit"), xa.ChannelDemux()
    start_time = int(dm.stats()["start_time"])
    s = torch.cuda.Stream(device=dev)
    d_sym = torch.from_numpy(stream.view(np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    bufs, at = [], 0

    def poisoned(n):
        return torch.full((max(n, 1),), 0xAB, dtype=torch.uint8, device=dev)

    with torch.cuda.stream(s):
        for p in pieces:
            n, cap = len(p), sync.rows(len(p))
            b = dict(frames=poisoned(cap * F), valid=poisoned(cap), hits=poisoned(cap * 16), start=poisoned(cap * 8),
                     count=poisoned(4), cadu=poisoned(cap * 1024), block=poisoned(cap * 1020), info=poisoned(cap * 40),
                     vcdu=poisoned(cap * 892), off=poisoned(65 * 4), rec=poisoned(cap * 88), cap=cap)
            sync.push_device(d_sym[at:].data_ptr() if n else 0, n, b["frames"].data_ptr(), b["valid"].data_ptr(),
                             b["hits"].data_ptr(), b["start"].data_ptr(), b["count"].data_ptr(), stream=s.cuda_stream)
            dec.decode_device(b["frames"].data_ptr(), b["valid"].data_ptr(), cap, b["cadu"].data_ptr(), b["block"].data_ptr(),
                              b["info"].data_ptr(), stream=s.cuda_stream)
            dm.process_device(b["hits"].data_ptr(), b["cadu"].data_ptr(), b["block"].data_ptr(), b["info"].data_ptr(), cap,
                              b["vcdu"].data_ptr(), b["off"].data_ptr(), b["rec"].data_ptr(), stream=s.cuda_stream)
            bufs.append(b)
            at += n
    s.synchronize()
    # the specification: the framer's rows, the NumPy Viterbi on their windows (one batch for the three calls), the demux
    spec, state, carry = fs.Framer(cache=drifting["cache"]), ds.State(start_time=start_time), None
    calls = []
    for p, b in zip(pieces, bufs):
        want, cap = spec.push(p), b["cap"]
        k = len(want)
        pad = lambda a, shape, dt: np.concatenate([a, np.zeros((cap - k,) + shape, dt)])        # noqa: E731
        c = dict(k=k, frames=pad(want.frames, (F,), np.int8), valid=pad(want.valid, (), np.uint8),
                 hits=pad(want.hits, (4,), np.uint32), start=pad(want.start, (), np.uint64))
        c["windows"], c["idx"], carry = ccsds.windows(c["frames"], c["valid"], carry)
        calls.append(c)
    bits, err = ccsds.viterbi_batch(np.concatenate([c["windows"] for c in calls]))
    total = 0
    for c, b in zip(calls, bufs):
        cap, k, idx = b["cap"], c["k"], c["idx"]
        assert int(b["count"].cpu().numpy().view(np.uint32)[0]) == k
        assert np.array_equal(b["frames"].cpu().numpy().view(np.int8).reshape(cap, F), c["frames"])
        assert np.array_equal(b["valid"].cpu().numpy()[:cap], c["valid"])
        assert np.array_equal(b["hits"].cpu().numpy().view(np.uint32).reshape(cap, 4), c["hits"])
        assert np.array_equal(b["start"].cpu().numpy().view(np.uint64)[:cap], c["start"])
        cadu, block = np.zeros((cap, 1024), np.uint8), np.zeros((cap, 1020), np.uint8)
        info = np.zeros(cap, xa.FRAME_INFO_DTYPE)
        info["rs_errors"] = -1
        cadu[idx] = ccsds.cadu_from_bits(bits[total:total + k])
        for j, f in enumerate(idx):
            block[f] = ccsds.derandomize(cadu[f, 4:])
            assert not any(ccsds.syndromes(block[f, q::4]).any() for q in range(4))      # clean: nothing to correct
            info[f] = (1, 1, err[total + j], [0] * 4, (int(block[f, 0]) & 0x3F) << 2 | int(block[f, 1]) >> 6,
                       int(block[f, 1]) & 0x3F, int(block[f, 2]) << 16 | int(block[f, 3]) << 8 | int(block[f, 4]))
        assert np.array_equal(b["cadu"].cpu().numpy()[:cap * 1024].reshape(cap, 1024), cadu)
        assert b["info"].cpu().numpy()[:cap * 40].view(xa.FRAME_INFO_DTYPE).tobytes() == info.tobytes()
        want_vcdu, want_off, want_rec, _ = ds.process(state, c["hits"], cadu, block, info, wire=False)
        off = b["off"].cpu().numpy().view(np.uint32)
        assert np.array_equal(off, want_off) and int(off[64]) == k
        assert np.array_equal(b["vcdu"].cpu().numpy()[:k * 892].reshape(k, 892), want_vcdu)
        assert b["rec"].cpu().numpy()[:cap * 88].tobytes() == want_rec.tobytes()
        total += k
    assert total == 40
    sent = np.stack([ccsds.derandomize(np.asarray(c[4:], np.uint8))[:892] for c in drifting["cadus"]])
    got = np.concatenate([b["block"].cpu().numpy()[:b["cap"] * 1020].reshape(b["cap"], 1020)[:, :892] for b in bufs])
    assert np.array_equal(got[got.any(axis=1)], sent)           # every VCDU sent, once, in order
    for h in (sync, dec, dm):
        h.close()


def test_error_paths(xa, drifting):
    L = xa.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.xrit_framer_push_device(None, p, 1, p, p, p, p, p, None) == -1
    assert L.xrit_framer_push(None, p, 1, p, p, p, p) == -1 and L.xrit_framer_stats(None, p) == -1
    assert L.xrit_framer_reset(None) == -1 and L.xrit_framer_set_frame(None, 320, 46) == -1 and L.xrit_framer_rows(None, 9) == 0
    assert L.xrit_framer_create(None, 0, 0) == -1
    sync = xa.FrameSynchroniser("lrit")
    for frame, minc in ((64, 46), ((1 << 20) + 1, 46), (320, 65)):
        with pytest.raises(xa.XritError) as ei:
            sync.set_frame(frame, minc)
        assert ei.value.code == -1
    assert L.xrit_framer_push_device(sync._h, p, (1 << 30) + 1, p, p, p, p, p, None) == -1      # refused before anything is read
    assert b"2^30" in L.xrit_last_error()
    assert L.xrit_framer_push_device(sync._h, None, 5, p, p, p, p, p, None) == -1
    sync.set_frame(320, 40)                                     # still allowed: nothing has been pushed
    sync.set_frame(F, 46)
    assert len(sync.push(drifting["stream"][:100])[1]) == 0
    with pytest.raises(xa.XritError) as ei:
        sync.set_frame(320, 46)
    assert ei.value.code == -1 and "before the first push" in str(ei.value)
    sync.set_segment(3)                                         # the segment length may change between calls
    got = sync.push(drifting["stream"][100:])
    assert np.array_equal(got[3], drifting["starts"])
    with pytest.raises(ValueError):
        xa.FrameSynchroniser("xrit")
    sync.close()


def test_host_program_stream_sync(xa, tmp_path):
    """--stream-sync puts the framer in front of the frame decoder; on a clean capture it decodes what the fixed windows
    decode, and says what it did."""
    rng = np.random.default_rng(13)
    n = 14
    blocks = np.stack([ccsds.make_block(0x8C, (0, 5, 63)[i % 3], 500 + i // 3, rng) for i in range(n)])
    sym = ccsds.coded_symbols([ccsds.cadu_from_block(b) for b in blocks], amplitude=1).astype(np.float64)
    p = synth.SynthParams(fs_in=1.25e6, seed=13)
    synth.generate(p, int((len(sym) + 64) * p.sps_in), symbols=sym).tofile(tmp_path / "iq.cf32")
    host_bin = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
    out = {}
    for tag, extra in (("windows", []), ("stream", ["--stream-sync"])):
        r = subprocess.run([host_bin, "--input", str(tmp_path / "iq.cf32"), "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null",
                            "--block", "200000", "--decode", str(tmp_path / (tag + ".bin"))] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, (tag, r.stderr)
        out[tag] = (np.fromfile(tmp_path / (tag + ".bin"), np.uint8).reshape(-1, 892), r.stderr)
    assert "sync:" not in out["windows"][1]
    line = [ln for ln in out["stream"][1].splitlines() if ln.startswith("sync:")]
    assert len(line) == 1 and "resynchronisations" in line[0]
    got, ref = out["stream"][0], out["windows"][0]
    assert len(got) >= n - 4 and len(got) >= len(ref) - 1
    sent = {b[:892].tobytes(): i for i, b in enumerate(blocks)}
    tail = got[3:]                                              # after acquisition (a frame with one good codeword of four counts as ok)
    order = [sent[v.tobytes()] for v in tail]                   # every VCDU is one that was sent ...
    assert order == list(range(order[0], order[0] + len(tail))) and order[-1] >= n - 2      # ... each once, in order, none skipped
    assert np.array_equal(got[-8:], ref[-8:])
