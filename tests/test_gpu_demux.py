"""GPU tier: the channel demultiplexer and packet accounting (xrit_demux_*, ChannelDemux) against the specification of
tests/demux_spec.py -- synthetic decoder outputs with gaps, repeats, wraps, corrupted and invalid frames at tile-edge
sizes and VCID mixes, calls cut at random, several handles, the device path behind the frame decoder, the wire
records, the chain from IQ and the host program.  Every comparison is exact (startTime aside)."""
import os
import subprocess

import numpy as np
import pytest

import ccsds
import demux_spec as ds
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


def synthetic(xa, rng, nf, mix, with_block=True):
    """Decoder outputs: (hits, cadu, block, info).  Counters advance per VCID with gaps, repeats and 24-bit wraps;
    about 3 % of the frames are corrupted and 2 % invalid."""
    if mix == "one":
        vc = np.full(nf, 5)
    elif mix == "all":
        vc = rng.integers(0, 64, nf)
    else:                                    # most frames on one channel, a few on 20 others (fill included)
        others = np.array([0, 1, 2, 3, 4, 6, 7, 9, 13, 20, 21, 30, 31, 32, 40, 41, 50, 60, 62, 63])
        vc = np.where(rng.random(nf) < 0.9, 5, others[rng.integers(0, len(others), nf)])
    step = rng.choice([1, 1, 1, 1, 1, 1, 1, 0, 2, 4, 1 << 23], nf)
    start = rng.integers(0, 1 << 24, 64)
    start[5] = (1 << 24) - 3                 # the busy channel wraps early
    counter = np.zeros(nf, np.int64)
    cur = start.copy()
    for v in np.unique(vc):
        idx = np.nonzero(vc == v)[0]
        c = (cur[v] + np.cumsum(step[idx])) & 0xFFFFFF
        counter[idx] = c
    info = np.zeros(nf, xa.FRAME_INFO_DTYPE)
    u = rng.random(nf)
    valid = u >= 0.02
    corrupted = valid & (u < 0.05)
    rs = rng.integers(-1, 17, (nf, 4))
    rs[corrupted] = -1
    rs[~valid] = -1
    allbad = (rs == -1).all(1) & valid & ~corrupted
    rs[allbad, 0] = 3                          # "good" frames keep at least one codeword
    info["valid"] = valid
    info["ok"] = valid & ~corrupted
    info["viterbi_errors"] = np.where(valid, rng.choice([0, 1, 83, 500, 900, 16448], nf), 0)
    info["rs_errors"] = rs
    info["scid"] = np.where(valid, 0x8C, 0)
    info["vcid"] = np.where(valid, vc, 0)
    info["counter"] = np.where(valid, counter, 0)
    hits = np.zeros((nf, 4), np.uint32)
    hits[:, 0] = rng.integers(0, 2, nf)
    hits[:, 1] = rng.integers(0, 16384, nf)
    hits[:, 2] = rng.integers(0, 65, nf)
    cadu = np.zeros((nf, 1024), np.uint8)
    cadu[:, :4] = rng.integers(0, 256, (nf, 4))
    block = rng.integers(0, 256, (nf, 1020), dtype=np.uint8) if with_block else None
    return hits, cadu, block, info


def masked(st):
    a = np.array(st).copy()
    a["start_time"] = 0
    return a.tobytes()


def spec_stats_bytes(xa, s):
    a = np.zeros(1, xa.DECODER_STATS_DTYPE)[0]
    a["total_packets"], a["dropped_packets"], a["lost_packets"] = s.frames, s.dropped, s.lost
    a["sum_viterbi_errors"], a["sum_rs_corrections"] = s.sum_vit, s.sum_rs
    a["received"], a["lost"], a["last_counter"] = s.received, s.lost_vc, s.last
    return masked(a)


@pytest.mark.parametrize("mix", ["one", "all", "skewed"])
@pytest.mark.parametrize("nf", [1, 63, 64, 65, 1023, 1024, 1025, 100000])
def test_one_call_matches_spec(xa, nf, mix):
    rng = np.random.default_rng(nf * 3 + len(mix))
    hits, cadu, block, info = synthetic(xa, rng, nf, mix)
    dm = xa.ChannelDemux()
    start = dm.stats()
    vcdu, off, rec = dm.process(hits, cadu, block, info)
    st = ds.State(start_time=int(start["start_time"]))
    want_vcdu, want_off, want_rec, want_wire = ds.process(st, hits, cadu, block, info, wire=nf <= 1025)
    assert np.array_equal(off, want_off)
    assert np.array_equal(vcdu, want_vcdu)
    assert rec.tobytes() == want_rec.tobytes()
    assert masked(dm.stats()) == spec_stats_bytes(xa, st)
    if nf <= 1025:
        assert dm.wire_records(start, rec) == b"".join(want_wire)


def test_2_pow_20_frames_on_the_device(xa):
    torch = pytest.importorskip("torch")
    nf = 1 << 20
    rng = np.random.default_rng(20)
    hits, cadu, _, info = synthetic(xa, rng, nf, "skewed", with_block=False)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(20)
    d_block = torch.randint(0, 256, (nf, 1020), dtype=torch.uint8, device=dev, generator=g)
    d_hits = torch.from_numpy(hits.view(np.uint8)).to(dev)
    d_cadu = torch.from_numpy(cadu).to(dev)
    d_info = torch.from_numpy(info.view(np.uint8)).to(dev)
    d_vcdu = torch.zeros((nf, 892), dtype=torch.uint8, device=dev)
    d_off = torch.zeros(65 * 4, dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(nf * 88, dtype=torch.uint8, device=dev)
    dm = xa.ChannelDemux()
    s = torch.cuda.current_stream(dev)
    dm.process_device(d_hits.data_ptr(), d_cadu.data_ptr(), d_block.data_ptr(), d_info.data_ptr(), nf,
                      d_vcdu.data_ptr(), d_off.data_ptr(), d_rec.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    st = ds.State()
    _, want_off, want_rec, _ = ds.process(st, hits, cadu, np.zeros((nf, 0), np.uint8), info, wire=False)
    off = d_off.cpu().numpy().view(np.uint32)
    assert np.array_equal(off, want_off)
    assert d_rec.cpu().numpy().tobytes() == want_rec.tobytes()
    good = np.nonzero((info["valid"] != 0) & (info["ok"] != 0))[0]
    order = good[np.argsort(info["vcid"][good], kind="stable")]
    want = d_block[torch.from_numpy(order).to(dev), :892]
    assert torch.equal(d_vcdu[:len(order)], want)
    assert masked(dm.stats()) == spec_stats_bytes(xa, st)
    # hand the 3 GB of this test back (the tests after it run on the same device) and destroy the handle here
    dm.close()
    del d_block, d_hits, d_cadu, d_info, d_vcdu, d_off, d_rec, want
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mix", ["all", "skewed"])
def test_random_calls_equal_one_call(xa, mix):
    rng = np.random.default_rng(11)
    nf = 5000
    hits, cadu, block, info = synthetic(xa, rng, nf, mix)
    one = xa.ChannelDemux()
    v1, o1, r1 = one.process(hits, cadu, block, info)
    cuts = np.sort(rng.choice(np.arange(1, nf), 12, replace=False))
    cuts = np.concatenate([[0], cuts, [nf]])
    many = xa.ChannelDemux()
    per_vc = [[] for _ in range(64)]
    recs, wire = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s0 = many.stats()
        v, o, r = many.process(hits[a:b], cadu[a:b], block[a:b], info[a:b])
        for c in range(64):
            per_vc[c].append(v[o[c]:o[c + 1]])
        recs.append(r)
        wire.append(many.wire_records(s0, r))
    many.process(hits[:0], cadu[:0], block[:0], info[:0])          # an empty call changes nothing
    for c in range(64):
        assert np.array_equal(np.concatenate(per_vc[c]), v1[o1[c]:o1[c + 1]]), c
    assert np.concatenate(recs).tobytes() == r1.tobytes()
    assert masked(many.stats()) == masked(one.stats())
    st = ds.State(start_time=int(many.stats()["start_time"]))
    assert b"".join(wire) == b"".join(ds.process(st, hits, cadu, block, info)[3])


def test_reset_and_several_handles(xa):
    rng = np.random.default_rng(5)
    hits, cadu, block, info = synthetic(xa, rng, 3000, "all")
    a, b = xa.ChannelDemux(), xa.ChannelDemux()
    ra = a.process(hits[:1500], cadu[:1500], block[:1500], info[:1500])
    rb = b.process(hits[1500:], cadu[1500:], block[1500:], info[1500:])       # interleaved with a
    ra2 = a.process(hits[1500:], cadu[1500:], block[1500:], info[1500:])
    assert not np.array_equal(ra2[2], rb[2])                                  # a carries its counters
    fresh = xa.ChannelDemux().stats()
    a.reset()
    assert masked(a.stats()) == masked(fresh)
    again = a.process(hits[1500:], cadu[1500:], block[1500:], info[1500:])
    assert all(np.array_equal(x, y) for x, y in zip(again, rb))
    whole = xa.ChannelDemux().process(hits, cadu, block, info)
    assert np.concatenate([ra[2], ra2[2]]).tobytes() == whole[2].tobytes()


def make_cadus(rng, vcids, counters):
    blocks = np.stack([ccsds.make_block(0x8C, v, c, rng) for v, c in zip(vcids, counters)])
    cadus = np.stack([ccsds.cadu_from_block(b) for b in blocks])
    return blocks, cadus


def test_device_path_behind_the_decoder_on_a_side_stream(xa):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(8)
    n = 48
    vcids = [(0, 7, 63)[i % 3] for i in range(n)]
    counters = [100 + i // 3 + (5 if i > 20 else 0) for i in range(n)]
    blocks, cadus = make_cadus(rng, vcids, counters)
    clean = ccsds.coded_symbols(cadus).reshape(n, ccsds.FRAME_SYMBOLS).astype(np.int16)
    frames = np.clip(clean + rng.normal(0, 70, clean.shape).round(), -128, 127).astype(np.int8)
    frames[10] = rng.integers(-128, 128, ccsds.FRAME_SYMBOLS)             # a corrupted frame
    valid = np.ones(n, np.uint8)
    valid[[4, 30]] = 0
    hits = np.zeros((n, 4), np.uint32)
    hits[:, 0] = np.arange(n) % 2
    hits[:, 2] = 50 + np.arange(n) % 15
    cadu, block, info = xa.FrameDecoder("lrit").decode(frames, valid)
    want = xa.ChannelDemux().process(hits, cadu, block, info)
    assert want[2]["frame_lock"][10] == 0 and want[2]["valid"][4] == 0
    dev = torch.device("cuda:0")
    d_frames = torch.from_numpy(frames.view(np.uint8)).to(dev)
    d_valid = torch.from_numpy(valid).to(dev)
    d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1)).to(dev)
    d_cadu = torch.zeros((n, 1024), dtype=torch.uint8, device=dev)
    d_block = torch.zeros((n, 1020), dtype=torch.uint8, device=dev)
    d_info = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    d_vcdu = torch.zeros((n, 892), dtype=torch.uint8, device=dev)
    d_off = torch.zeros(2 * 65 * 4, dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(n * 88, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    dec, dm = xa.FrameDecoder("lrit"), xa.ChannelDemux()
    h = n // 2
    with torch.cuda.stream(s):
        for k, (a, b) in enumerate(((0, h), (h, n))):
            dec.decode_device(d_frames[a:].data_ptr(), d_valid[a:].data_ptr(), b - a, d_cadu[a:].data_ptr(),
                              d_block[a:].data_ptr(), d_info[a * 40:].data_ptr(), stream=s.cuda_stream)
            dm.process_device(d_hits[a * 16:].data_ptr(), d_cadu[a:].data_ptr(), d_block[a:].data_ptr(),
                              d_info[a * 40:].data_ptr(), b - a, d_vcdu[a:].data_ptr(), d_off[k * 260:].data_ptr(),
                              d_rec[a * 88:].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert d_rec.cpu().numpy().tobytes() == want[2].tobytes()
    off = d_off.cpu().numpy().view(np.uint32).reshape(2, 65)
    vc = d_vcdu.cpu().numpy()
    for c in range(64):
        parts = [vc[0:][off[0, c]:off[0, c + 1]], vc[h:][off[1, c]:off[1, c + 1]]]
        assert np.array_equal(np.concatenate(parts), want[0][want[1][c]:want[1][c + 1]]), c
    assert want[1][64] >= n - 6
    dec.close()
    dm.close()


def test_chain_from_iq_counts_the_skipped_counter(xa):
    rng = np.random.default_rng(9)
    n = 18
    vcids = [(2, 5, 63)[i % 3] for i in range(n)]
    skip = 10                                # vcid 5: one counter deliberately skipped from frame 10 on
    counters = [40 + i // 3 + (1 if (i >= skip and vcids[i] == 5) else 0) for i in range(n)]
    blocks, cadus = make_cadus(rng, vcids, counters)
    sym = ccsds.coded_symbols(cadus, amplitude=1).astype(np.float64)
    p = synth.SynthParams(fs_in=1.25e6, seed=9, esn0_db=12.0)
    x = synth.generate(p, int((len(sym) + 64) * p.sps_in), symbols=sym)
    q = xa.Demodulator(xa.Demodulator.config("lrit", 1.25e6, 1))
    s8 = q.quantize_i8(q.process(x))
    hits = np.asarray(xa.sync_correlate(s8))
    frames, valid = xa.sync_fix_frames(s8, hits)
    cadu, block, info = xa.FrameDecoder("lrit").decode(frames, valid)
    a = 3                                    # after acquisition
    assert (info["ok"][a:] == 1).all()
    dm = xa.ChannelDemux()
    vcdu, off, rec = dm.process(hits[a:], cadu[a:], block[a:], info[a:])
    first = next(i for i in range(n) if np.array_equal(blocks[i, :892], block[a, :892]))
    assert first <= a and skip > first + 3
    for v in (2, 5, 63):
        sent = np.stack([blocks[i, :892] for i in range(first, n) if vcids[i] == v])
        got = vcdu[off[v]:off[v + 1]]
        assert len(sent) - 1 <= len(got) <= len(sent) and np.array_equal(got, sent[:len(got)]), v
    st = dm.stats()
    assert int(st["lost_packets"]) == 1 and int(st["lost"][5]) == 1
    assert int(st["lost"][2]) == 0 and int(st["lost"][63]) == 0
    assert (rec["frame_lock"] == 1).all() and (rec["sync_word"] == np.frombuffer(ccsds.ASM, np.uint8)).all()


def run_host(xa, tmp_path, extra, tag):
    host_bin = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
    r = subprocess.run([host_bin, "--input", str(tmp_path / "iq.cf32"), "--mode", "lrit", "--sample-rate", "1250000",
                        "--sink", "null", "--block", "200000"] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (tag, r.stderr)
    return r.stderr


def test_host_program_channels_and_statistics(xa, tmp_path):
    rng = np.random.default_rng(12)
    n = 18
    vcids = [(0, 5, 63)[i % 3] for i in range(n)]
    counters = [7000 + i // 3 + (2 if (vcids[i] == 0 and i > 9) else 0) for i in range(n)]
    blocks, cadus = make_cadus(rng, vcids, counters)
    sym = ccsds.coded_symbols(cadus, amplitude=1).astype(np.float64)
    p = synth.SynthParams(fs_in=1.25e6, seed=12)
    x = synth.generate(p, int((len(sym) + 64) * p.sps_in), symbols=sym)
    x.tofile(tmp_path / "iq.cf32")
    plain = run_host(xa, tmp_path, ["--decode", str(tmp_path / "a.bin")], "plain")
    both = run_host(xa, tmp_path, ["--decode", str(tmp_path / "b.bin"), "--channels", str(tmp_path / "ch"),
                                   "--decoder-stats", str(tmp_path / "st.bin")], "both")
    only = run_host(xa, tmp_path, ["--channels", str(tmp_path / "ch2")], "channels only")
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes()
    dline = [ln for ln in plain.splitlines() if ln.startswith("decode:")]
    assert dline and dline == [ln for ln in both.splitlines() if ln.startswith("decode:")]
    assert "demux: lost packets" in both and "demux: lost packets" in only
    good = np.fromfile(tmp_path / "a.bin", np.uint8).reshape(-1, 892)
    raw = (tmp_path / "st.bin").read_bytes()
    assert len(raw) % 4167 == 0 and len(raw) >= 4167 * len(good)
    recs = [ds.unpack(raw[i:i + 4167]) for i in range(0, len(raw), 4167)]
    # the same run's decoded frames, rebuilt from its outputs: the good frames' VCDUs (--decode) and each valid frame's
    # fields the decoder produced (header, errors, hit, sync word); the spec then derives the accounting
    nv = len(recs)
    info = np.zeros(nv, xa.FRAME_INFO_DTYPE)
    hits = np.zeros((nv, 4), np.uint32)
    cadu = np.zeros((nv, 1024), np.uint8)
    block = np.zeros((nv, 1020), np.uint8)
    g = 0
    for f, d in enumerate(recs):
        lock = d["frameLock"]
        info[f] = (1, lock, d["vitErrors"], d["rsErrors"], d["scid"], d["vcid"], d["packetNumber"])
        hits[f] = (1 if d["phaseCorrection"] == 180 else 0, 0, d["syncCorrelation"], 0)
        cadu[f, :4] = np.frombuffer(d["syncWord"], np.uint8)
        if lock:
            block[f, :892] = good[g]
            g += 1
    assert g == len(good)
    st = ds.State(start_time=recs[0]["startTime"])
    vcdu, off, _, wire = ds.process(st, hits, cadu, block, info)
    assert b"".join(wire) == raw
    for v in range(64):
        for d in ("ch", "ch2"):
            path = tmp_path / d / f"channel_{v}.bin"
            if off[v + 1] == off[v]:
                assert not path.exists(), (d, v)
            else:
                assert path.read_bytes() == vcdu[off[v]:off[v + 1]].tobytes(), (d, v)
    assert st.lost_vc[0] >= 2                                                  # the skipped counters of vcid 0
