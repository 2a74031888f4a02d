"""GPU tier: the frame decoder (xrit_decoder_*, FrameDecoder) against the NumPy specification of tests/ccsds.py --
Viterbi bit for bit on arbitrary soft frames, clean round trips of CADUs, RS correction up to and past 16 errors,
the carry across calls, and the whole chain from IQ to VCDUs, in the library and in the host program; the RS kernel
codeword for codeword against the reference decoder of tests/ccsds.py on constructed error patterns, and calls of more
frames than there are resident Viterbi windows (set_windows, and the default geometry).  Every assertion is exact."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import ccsds
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR = ccsds.FRAME_SYMBOLS


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


def spec_decode(frames, valid, hrit, carry=None):
    """What the decoder's cadu rows and viterbi_errors must be (zero rows for valid = 0)."""
    w, idx, carry = ccsds.windows(frames, valid, carry)
    cadu = np.zeros((len(frames), ccsds.CADU_BYTES), np.uint8)
    verr = np.zeros(len(frames), np.int64)
    if len(idx):
        bits, err = ccsds.viterbi_batch(w)
        cadu[idx] = ccsds.cadu_from_bits(bits, hrit)
        verr[idx] = err
    return cadu, verr, carry


def check_block_against_rs(block, cadu, info, valid):
    """Every codeword either decoded to a codeword (syndromes zero, <= 16 corrections) or is -1 and passed through."""
    for f in range(len(block)):
        if not valid[f]:
            assert not block[f].any() and info["rs_errors"][f].tolist() == [-1] * 4 and info["ok"][f] == 0
            continue
        derand = ccsds.derandomize(cadu[f, 4:])
        for k in range(4):
            e = int(info["rs_errors"][f, k])
            if e == -1:
                assert np.array_equal(block[f, k::4], derand[k::4]), (f, k)
            else:
                assert 0 <= e <= 16 and not ccsds.syndromes(block[f, k::4]).any(), (f, k, e)
                assert int((block[f, k::4] != derand[k::4]).sum()) == e, (f, k, e)
        assert info["ok"][f] == (0 if (info["rs_errors"][f] == -1).all() else 1)


def random_frames(rng, n):
    kinds = [lambda: rng.integers(-128, 128, FR), lambda: rng.integers(-2, 3, FR), lambda: np.zeros(FR, np.int64),
             lambda: rng.choice([-127, 127], FR)]
    return np.stack([kinds[i % 4]() for i in range(n)]).astype(np.int8)


@pytest.mark.parametrize("mode", ["lrit", "hrit"])
def test_viterbi_bit_for_bit_on_arbitrary_frames(xa, mode):
    rng = np.random.default_rng(11)
    frames = random_frames(rng, 48)
    valid = (rng.random(48) > 0.3).astype(np.uint8)
    valid[[0, 5, 6, 7, 30]] = [0, 1, 0, 0, 1]
    cadu, block, info = xa.FrameDecoder(mode).decode(frames, valid)
    want, verr, _ = spec_decode(frames, valid, mode == "hrit")
    assert np.array_equal(cadu, want)
    assert np.array_equal(info["viterbi_errors"].astype(np.int64), verr)
    assert np.array_equal(info["valid"], valid)
    check_block_against_rs(block, cadu, info, valid)
    assert not info["scid"][valid == 0].any() and not info["counter"][valid == 0].any()


def make_stream(n, rng, counter0=100, scid=0x8C):
    blocks = np.stack([ccsds.make_block(scid, (0, 63)[i % 2], counter0 + i, rng) for i in range(n)])
    cadus = np.stack([ccsds.cadu_from_block(b) for b in blocks])
    return blocks, cadus


@pytest.mark.parametrize("mode,invert", [("lrit", False), ("hrit", False), ("hrit", True)])
def test_clean_round_trip(xa, mode, invert):
    rng = np.random.default_rng(2)
    blocks, cadus = make_stream(24, rng)
    sym = ccsds.coded_symbols(cadus, hrit=mode == "hrit")
    frames = (-sym if invert else sym).reshape(24, FR)
    cadu, block, info = xa.FrameDecoder(mode).decode(frames, np.ones(24, np.uint8))
    assert (cadu[:, :4] == np.frombuffer(ccsds.ASM, np.uint8)).all()
    assert np.array_equal(cadu, cadus)
    assert np.array_equal(block, blocks)
    assert (info["rs_errors"] == 0).all() and (info["ok"] == 1).all() and (info["viterbi_errors"] == 0).all()
    assert (info["scid"] == 0x8C).all() and info["vcid"].tolist() == [(0, 63)[i % 2] for i in range(24)]
    assert info["counter"].tolist() == list(range(100, 124))


def test_rs_corrects_up_to_16_errors_per_codeword(xa):
    rng = np.random.default_rng(3)
    ks = [1, 2, 8, 15, 16, 17, 24, 60]
    n = len(ks) + 2
    blocks, _ = make_stream(n, rng)
    sent = blocks.copy()
    for f in range(n):
        for k in range(4):
            if f < len(ks):
                e = ks[f]
            else:
                e = 60 if (f == len(ks) + 1 or k == 2) else 0          # one bad codeword / all four bad
            pos = rng.choice(255, e, replace=False)
            if e and f % 2 == 0:                                      # parity, and the block's last byte
                forced = 254 if k == 3 else 230
                pos = np.append(rng.choice(np.setdiff1d(np.arange(255), [forced]), e - 1, replace=False), forced)
            blocks[f, 4 * pos + k] ^= rng.integers(1, 256, e).astype(np.uint8)
    cadus = np.stack([ccsds.cadu_from_block(b) for b in blocks])
    frames = ccsds.coded_symbols(cadus).reshape(n, FR)
    cadu, block, info = xa.FrameDecoder("lrit").decode(frames, np.ones(n, np.uint8))
    assert np.array_equal(cadu, cadus) and (info["viterbi_errors"] == 0).all()
    check_block_against_rs(block, cadu, info, np.ones(n, np.uint8))
    for f, e in enumerate(ks):
        if e <= 16:
            assert info["rs_errors"][f].tolist() == [e] * 4, (e, info["rs_errors"][f])
            assert np.array_equal(block[f], sent[f])
    one_bad, all_bad = info[len(ks)], info[len(ks) + 1]
    assert one_bad["rs_errors"].tolist() == [0, 0, -1, 0] and one_bad["ok"] == 1
    good = np.arange(1020) % 4 != 2
    assert np.array_equal(block[len(ks)][good], sent[len(ks)][good])
    assert all_bad["rs_errors"].tolist() == [-1] * 4 and all_bad["ok"] == 0


def streaming_input(rng):
    _, cadus = make_stream(20, rng)
    clean = ccsds.coded_symbols(cadus).reshape(20, FR).astype(np.int16)
    noisy = np.clip(clean + rng.normal(0, 60, clean.shape).round(), -128, 127).astype(np.int8)
    frames = np.concatenate([random_frames(rng, 20), noisy])
    valid = np.ones(40, np.uint8)
    valid[[3, 4, 17, 25]] = 0
    return frames, valid


def test_streaming_carry_across_calls(xa):
    rng = np.random.default_rng(4)
    frames, valid = streaming_input(rng)
    whole = xa.FrameDecoder("lrit").decode(frames, valid)
    want, verr, _ = spec_decode(frames, valid, False)
    assert np.array_equal(whole[0], want) and np.array_equal(whole[2]["viterbi_errors"].astype(np.int64), verr)
    dec = xa.FrameDecoder("lrit")
    parts, a = [], 0
    for n in (1, 2, 5, 13, 19):
        parts.append(dec.decode(frames[a:a + n], valid[a:a + n]))
        a += n
    for i in range(3):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), whole[i]), i
    # a valid = 0 frame leaves the carry alone; an empty call too
    d2 = xa.FrameDecoder("lrit")
    d2.decode(frames[:3], valid[:3])
    d2.decode(frames[3:5], valid[3:5])
    d2.decode(frames[:0], valid[:0])
    assert all(np.array_equal(x, y) for x, y in zip(d2.decode(frames[5:9], valid[5:9]), [w[5:9] for w in whole]))
    # reset: the erasure carry again
    d2.reset()
    fresh = xa.FrameDecoder("lrit").decode(frames[10:14], valid[10:14])
    assert all(np.array_equal(x, y) for x, y in zip(d2.decode(frames[10:14], valid[10:14]), fresh))
    assert not np.array_equal(fresh[2]["viterbi_errors"], whole[2]["viterbi_errors"][10:14])     # the carry matters here


def test_device_path_on_a_side_stream(xa):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(4)
    frames, valid = streaming_input(rng)
    want = xa.FrameDecoder("lrit").decode(frames, valid)
    dev = torch.device("cuda:0")
    d_frames = torch.from_numpy(frames.view(np.uint8)).to(dev)
    d_valid = torch.from_numpy(valid).to(dev)
    d_cadu = torch.zeros((40, 1024), dtype=torch.uint8, device=dev)
    d_block = torch.zeros((40, 1020), dtype=torch.uint8, device=dev)
    d_info = torch.zeros(40 * xa.FRAME_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    dec = xa.FrameDecoder("lrit")
    with torch.cuda.stream(s):
        dec.decode_device(d_frames.data_ptr(), d_valid.data_ptr(), 20, d_cadu.data_ptr(), d_block.data_ptr(),
                          d_info.data_ptr(), stream=s.cuda_stream)
        dec.decode_device(d_frames[20:].data_ptr(), d_valid[20:].data_ptr(), 20, d_cadu[20:].data_ptr(),
                          d_block[20:].data_ptr(), d_info[20 * xa.FRAME_INFO_DTYPE.itemsize:].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_cadu.cpu().numpy(), want[0])
    assert np.array_equal(d_block.cpu().numpy(), want[1])
    assert d_info.cpu().numpy().view(xa.FRAME_INFO_DTYPE).tobytes() == want[2].tobytes()


def chain_frames(xa, mode, fs, D, esn0, n_frames=12, seed=3):
    """CADUs -> coded symbols -> IQ (synth) -> Demodulator -> int8 -> correlator -> frame fix: (frames, valid, sent
    blocks)."""
    rng = np.random.default_rng(seed)
    blocks, cadus = make_stream(n_frames, rng, counter0=1000)
    hrit = mode == "hrit"
    sym = ccsds.coded_symbols(cadus, hrit=hrit, amplitude=1).astype(np.float64)
    kw = dict(symbol_rate=927000.0, alpha=0.3) if hrit else {}
    p = synth.SynthParams(fs_in=fs, seed=seed, esn0_db=esn0, **kw)
    x = synth.generate(p, int((len(sym) + 64) * p.sps_in), symbols=sym)
    q = xa.Demodulator(xa.Demodulator.config(mode, fs, D))
    s8 = q.quantize_i8(q.process(x))
    words = (xa.HRIT_UW0, xa.HRIT_UW2) if hrit else (xa.LRIT_UW0, xa.LRIT_UW2)
    hits = np.asarray(xa.sync_correlate(s8, words=words))
    if hrit:
        hits[:, 0] = 0                       # NRZ-M: the phase does not matter (newdecoder.cpp:265)
    frames, valid = xa.sync_fix_frames(s8, hits)
    return frames, valid, blocks


def check_vcdus(block, info, sent, first=3):
    """From the fourth frame on: ok, VCDU as sent, counters consecutive."""
    assert (info["ok"][first:] == 1).all(), info["rs_errors"]
    c = info["counter"][first:].astype(np.int64)
    assert (np.diff(c) == 1).all(), c
    for f in range(first, len(block)):
        i = int(info["counter"][f]) - 1000
        assert 0 <= i < len(sent) and np.array_equal(block[f, :892], sent[i, :892]), f


@pytest.mark.parametrize("mode,fs,D,esn0", [("lrit", 1.25e6, 1, 12.0), ("lrit", 1.25e6, 1, 4.0), ("lrit", 6.25e6, 5, 12.0),
                                            ("lrit", 6.25e6, 5, 4.0), ("hrit", 2.5e6, 1, 12.0)])
def test_chain_from_iq_to_vcdus(xa, mode, fs, D, esn0):
    frames, valid, sent = chain_frames(xa, mode, fs, D, esn0)
    assert valid[3:].all()
    cadu, block, info = xa.FrameDecoder(mode).decode(frames, valid)
    check_vcdus(block, info, sent)
    if esn0 < 10:
        assert info["viterbi_errors"][3:].max() > 0
    # the decoder's Viterbi is the specification's on these frames too
    want, verr, _ = spec_decode(frames[:6], valid[:6], mode == "hrit")
    assert np.array_equal(cadu[:6], want) and np.array_equal(info["viterbi_errors"][:6].astype(np.int64), verr)


def test_host_program_decodes_vcdus(xa, tmp_path):
    host_bin = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
    rng = np.random.default_rng(7)
    blocks, cadus = make_stream(16, rng, counter0=5000)
    sym = ccsds.coded_symbols(cadus, amplitude=1).astype(np.float64)
    p = synth.SynthParams(fs_in=1.25e6, seed=7)
    x = synth.generate(p, int((len(sym) + 64) * p.sps_in), symbols=sym)
    f, out = tmp_path / "frames.cf32", tmp_path / "vcdu.bin"
    x.tofile(f)
    r = subprocess.run([host_bin, "--input", str(f), "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null",
                        "--decode", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "decode:" in r.stderr, r.stderr
    got = np.fromfile(out, np.uint8)
    assert len(got) % 892 == 0 and len(got) >= 10 * 892, (len(got), r.stderr)
    v = got.reshape(-1, 892)
    # the first frames fall in the demodulator's acquisition: a frame there may come out with some codewords good and
    # some not (ok, as the reference dispatches it) -- the check starts, as in the library's chain test, at most three in
    match = [next((i for i in range(16) if np.array_equal(blocks[i, :892], row)), -1) for row in v]
    j0 = next(j for j in range(len(v)) if match[j] >= 0)
    assert j0 <= 3, match
    i0 = match[j0]
    assert match[j0:] == list(range(i0, i0 + len(v) - j0)), match
    assert i0 <= 3 and i0 + len(v) - j0 >= 15, (match, r.stderr)      # up to the last complete frame


# ---- the RS kernel against the reference decoder (ccsds.rs_decode_many), codeword for codeword -----------------------
def wire_pattern(positions, values):
    e = np.zeros(255, np.uint8)
    e[np.asarray(positions, np.int64)] = np.asarray(values, np.uint8)
    return e


def random_pattern(rng, v, positions=None):
    pos = rng.choice(255, v, replace=False) if positions is None else positions
    return wire_pattern(pos, rng.integers(1, 256, v))


def rs_case_frames():
    """Error patterns on two sent blocks (the code is linear), every frame with all four codewords in use and the
    classes rotated over the interleave slots: a dict with the sent and the damaged blocks, the counts and blocks that
    are true by construction, and the frame range of every class."""
    rng = np.random.default_rng(31)
    base = [ccsds.make_block(0x8C, 21, 0x0A0B0C, rng), ccsds.make_block(0x35, 42, 0xFEDCBA, rng)]
    err, want_err, counts, cls = [], [], [], {}

    def add(patterns, n, other=None):
        """patterns: four (255,) wire patterns, slot by slot; n: the four counts; other: the codewords (or None) that
        the decoder must add to the sent ones."""
        err.append(ccsds.interleave(np.stack(patterns)))
        want_err.append(ccsds.interleave(np.stack([np.zeros(255, np.uint8) if g is None else g for g in other or [None] * 4])))
        counts.append(list(n))

    def rotate(items, by):
        return [items[(k - by) % 4] for k in range(4)]         # item q goes to slot (q + by) % 4

    # 1. a single error at every position of every slot, every non-zero wire byte as its value
    start = len(err)
    for i in range(255):
        add([wire_pattern([(i + 64 * k) % 255], [(4 * i + k) % 255 + 1]) for k in range(4)], [1] * 4)
    cls["position"] = (start, len(err))
    seen = np.stack(err[start:]).reshape(255, 255, 4)
    assert (np.count_nonzero(seen, axis=0) == 1).all() and len(np.unique(seen)) == 256

    # 2. every count 1 .. 16: consecutive symbols, parity only, both ends, the data/parity seam, four random ones, and
    #    a burst of 4 v consecutive block bytes
    start = len(err)
    for v in range(1, 17):
        a = int(rng.integers(0, 256 - v))
        ends = np.concatenate([[0, 254][:v], rng.choice(np.arange(1, 222), max(v - 2, 0), replace=False)])
        seam = np.concatenate([[222, 223][:v], rng.choice(np.arange(1, 222), max(v - 2, 0), replace=False)])
        first = [random_pattern(rng, v, np.arange(a, a + v)), random_pattern(rng, v, 223 + rng.choice(32, v, replace=False)),
                 random_pattern(rng, v, ends), random_pattern(rng, v, seam)]
        add(rotate(first, v), [v] * 4)
        add(rotate([random_pattern(rng, v) for _ in range(4)], v), [v] * 4)
        burst = np.zeros(1020, np.uint8)
        b0 = int(rng.integers(0, 1020 - 4 * v + 1))
        burst[b0:b0 + 4 * v] = rng.integers(1, 256, 4 * v)
        add(list(ccsds.deinterleave(burst)), [v] * 4)
    cls["count"] = (start, len(err))

    # 3. error values solved so that chosen syndromes vanish (zero discrepancies in Berlekamp-Massey)
    start = len(err)
    zero_cases = [(v, z) for v in (2, 3, 8, 16) for z in ((0,), (0, 1), (15,), (31,), (0, 31)) if len(z) < v]
    zero_cases = (zero_cases + [(16, (16,)), (3, (1,)), (8, (0, 1))])[:20]
    for fr in range(5):
        group = zero_cases[4 * fr:4 * fr + 4]
        pats = [ccsds.zero_syndrome_errors(rng.choice(255, v, replace=False), z, rng) for v, z in group]
        for (v, z), e in zip(group, pats):
            assert int((e != 0).sum()) == v and not ccsds.syndromes(e)[list(z)].any()
        add(rotate(pats, fr), rotate([v for v, _ in group], fr))
    cls["zero"] = (start, len(err))

    # 4. 33 - j symbols of a shifted, scaled g(x): j from sent + that codeword (j <= 16), or 16 from sent (j = 17)
    start = len(err)
    for si, (shift, scale) in enumerate([(222, 1), (0, 255), (91, 0x53), (222, 0xB7)]):
        pats, n, other = [], [], []
        for j in (1, 8, 16, 17):
            e, g = ccsds.near_codeword_error(shift, scale, j, rng)
            pats.append(e)
            n.append(j if j <= 16 else 16)
            other.append(g if j <= 16 else None)
        add(rotate(pats, si), rotate(n, si), rotate(other, si))
    cls["near"] = (start, len(err))

    # 5. beyond the capability: -1 and pass-through; frames with one, two and three such codewords
    start = len(err)
    for fr, vs in enumerate([(17, 18, 24, 32), (100, 255, 17, 18), (32, 100, 255, 24), (24, 17, 18, 255),
                             (17, 3, 0, 16), (5, 24, 30, 0), (18, 100, 1, 255)]):
        add(rotate([random_pattern(rng, v) for v in vs], fr), rotate([v if v <= 16 else -1 for v in vs], fr))
    cls["beyond"] = (start, len(err))

    # 6. the header: correctable errors on block bytes 0 .. 4, and codeword 1 beyond repair with a damaged vcid byte
    start = len(err)
    head = np.zeros(1020, np.uint8)
    head[:5] = (0x3F, 0xFF, 0x80, 0x01, 0x7E)
    add(list(ccsds.deinterleave(head)), [2, 1, 1, 1])
    lost = random_pattern(rng, 20, np.concatenate([[0], rng.choice(np.arange(1, 255), 19, replace=False)]))
    lost[0] = 0x2A                                              # block byte 1: vcid 42 -> 0
    add([random_pattern(rng, 4, [0, 1, 2, 3]), lost, random_pattern(rng, 1, [0]), np.zeros(255, np.uint8)], [4, -1, 1, 0])
    cls["header"] = (start, len(err))

    err, want_err, counts = np.stack(err), np.stack(want_err), np.array(counts, np.int64)
    sent = np.stack([base[f % 2] for f in range(len(err))])
    truth = sent ^ want_err
    damaged = sent ^ err
    bad = np.tile(counts == -1, (1, 255))                        # byte j belongs to codeword j % 4
    truth[bad] = damaged[bad]                                    # a -1 codeword passes through
    return dict(sent=sent, blocks=damaged, truth=truth, counts=counts, cls=cls)


@pytest.fixture(scope="module")
def rs_run(xa):
    """The constructed frames through clean coded symbols and one decoder call, with the reference's answer."""
    case = rs_case_frames()
    n = len(case["blocks"])
    cadus = np.stack([ccsds.cadu_from_block(b) for b in case["blocks"]])
    frames = ccsds.coded_symbols(cadus).reshape(n, FR)
    cadu, block, info = xa.FrameDecoder("lrit").decode(frames, np.ones(n, np.uint8))
    assert np.array_equal(cadu, cadus) and (info["viterbi_errors"] == 0).all()          # what fails below is the RS stage's
    ref_block, ref_n, ref_ok = ccsds.rs_decode_blocks(case["blocks"])
    return dict(case, block=block, info=info, ref_block=ref_block, ref_n=ref_n, ref_ok=ref_ok)


def test_rs_every_frame_equals_the_reference_decoder(rs_run):
    r = rs_run
    assert 300 <= len(r["blocks"]) <= 400
    # the reference gives what the construction says, so the comparison below is with the truth
    assert np.array_equal(r["ref_n"], r["counts"])
    assert np.array_equal(r["ref_block"], r["truth"])
    info, block = r["info"], r["block"]
    mism = np.argwhere(info["rs_errors"] != r["ref_n"])
    assert not len(mism), [(f, k, int(info["rs_errors"][f, k]), int(r["ref_n"][f, k])) for f, k in mism[:8]]
    for k in range(4):
        rows = np.nonzero((block[:, k::4] != r["ref_block"][:, k::4]).any(axis=1))[0]
        assert not len(rows), (k, rows[:8])
    assert np.array_equal(info["ok"], r["ref_ok"]) and (info["valid"] == 1).all()
    scid, vcid, counter = ccsds.header_fields(block)
    assert np.array_equal(info["scid"], scid) and np.array_equal(info["vcid"], vcid) and np.array_equal(info["counter"], counter)


@pytest.mark.parametrize("name", ["position", "count", "zero"])
def test_rs_restores_the_sent_block(rs_run, name):
    a, b = rs_run["cls"][name]
    assert np.array_equal(rs_run["info"]["rs_errors"][a:b], rs_run["counts"][a:b])
    assert (rs_run["counts"][a:b] >= 1).all() and (rs_run["counts"][a:b] <= 16).all()
    assert np.array_equal(rs_run["block"][a:b], rs_run["sent"][a:b])
    assert (rs_run["info"]["ok"][a:b] == 1).all()
    if name == "count":
        assert sorted(set(rs_run["counts"][a:b].ravel().tolist())) == list(range(1, 17))


def test_rs_corrects_to_the_other_codeword_within_16(rs_run):
    a, b = rs_run["cls"]["near"]
    got, info = rs_run["block"][a:b], rs_run["info"][a:b]
    assert sorted(info["rs_errors"].ravel().tolist()) == sorted([1, 8, 16, 16] * (b - a))
    assert np.array_equal(info["rs_errors"], rs_run["counts"][a:b])
    assert np.array_equal(got, rs_run["truth"][a:b])
    moved = (got != rs_run["sent"][a:b]).reshape(b - a, 255, 4).sum(axis=1)
    assert sorted(moved.ravel().tolist()) == sorted([33, 33, 33, 0] * (b - a))          # j = 17 goes back to the sent one
    # shift 222 puts the other codeword on the header bytes: the fields are the returned block's, not the sent one's
    scid, vcid, counter = ccsds.header_fields(got)
    sent_fields = ccsds.header_fields(rs_run["sent"][a:b])
    assert np.array_equal(info["scid"], scid) and np.array_equal(info["vcid"], vcid) and np.array_equal(info["counter"], counter)
    assert any((x != y).any() for x, y in zip((scid, vcid, counter), sent_fields))


def test_rs_passes_uncorrectable_codewords_through(rs_run):
    a, b = rs_run["cls"]["beyond"]
    info, got = rs_run["info"][a:b], rs_run["block"][a:b]
    assert np.array_equal(info["rs_errors"], rs_run["counts"][a:b])
    assert ((info["rs_errors"] == -1).sum(axis=1)).tolist() == [4, 4, 4, 4, 1, 2, 3]
    assert info["ok"].tolist() == [0, 0, 0, 0, 1, 1, 1]
    for f in range(b - a):
        for k in range(4):
            want = rs_run["blocks" if info["rs_errors"][f, k] == -1 else "sent"][a + f, k::4]
            assert np.array_equal(got[f, k::4], want), (f, k)


def test_rs_header_fields_come_from_the_returned_block(rs_run):
    a, _ = rs_run["cls"]["header"]
    info, got, sent = rs_run["info"], rs_run["block"], rs_run["sent"]
    scid, vcid, counter = (x.tolist() for x in ccsds.header_fields(sent[a:a + 2]))
    # corrected header bytes: the sent fields, though every one of bytes 0 .. 4 came in damaged
    assert info["rs_errors"][a].tolist() == [2, 1, 1, 1] and np.array_equal(got[a], sent[a])
    assert (int(info["scid"][a]), int(info["vcid"][a]), int(info["counter"][a])) == (scid[0], vcid[0], counter[0])
    assert ccsds.header_fields(rs_run["blocks"][a])[2][0] != counter[0]
    # codeword 1 is not corrected: byte 1 stays damaged, vcid is read from it; bytes 0, 2, 3, 4 are corrected
    assert info["rs_errors"][a + 1].tolist() == [4, -1, 1, 0] and info["ok"][a + 1] == 1
    assert got[a + 1, 1] == rs_run["blocks"][a + 1, 1] == sent[a + 1, 1] ^ 0x2A
    assert int(info["vcid"][a + 1]) == (int(sent[a + 1, 1]) ^ 0x2A) & 0x3F != vcid[1]
    assert (int(info["scid"][a + 1]) >> 2, int(info["counter"][a + 1])) == (scid[1] >> 2, counter[1])


# ---- calls of more frames than resident windows ---------------------------------------------------------------------
_VITERBI_CACHE = {}


def viterbi_cached(windows):
    """ccsds.viterbi_batch, run once per distinct window of the module."""
    keys = [hashlib.sha1(w.tobytes()).digest() for w in windows]
    todo = sorted(set(k for k in keys if k not in _VITERBI_CACHE))
    if todo:
        first = {k: i for i, k in reversed(list(enumerate(keys)))}
        bits, err = ccsds.viterbi_batch(np.stack([windows[first[k]] for k in todo]))
        for i, k in enumerate(todo):
            _VITERBI_CACHE[k] = (bits[i], int(err[i]))
    return np.stack([_VITERBI_CACHE[k][0] for k in keys]), np.array([_VITERBI_CACHE[k][1] for k in keys], np.int64)


class Pool:
    """Six frames -- two uniform random (with -128), one of -2 .. 2 (ties), one of zeros, two noisy coded frames of known
    blocks -- and what the decoder must give for each of them behind each possible carry (none, or any of the six): the
    specification runs on these 42 windows only, and a long call's expectation is a lookup."""

    def __init__(self, hrit):
        rng = np.random.default_rng(41)
        self.hrit = hrit
        plain = np.stack([rng.integers(-128, 128, FR), rng.integers(-128, 128, FR), rng.integers(-2, 3, FR), np.zeros(FR, np.int64)])
        assert (plain[:2] == -128).any()
        self.sent, cadus = make_stream(3, rng, counter0=0x7000)
        clean = ccsds.coded_symbols(cadus, hrit=hrit).reshape(3, FR)[1:].astype(np.int64)
        noisy = np.clip(clean + rng.normal(0, 60, clean.shape).round(), -128, 127)
        self.frames = np.concatenate([plain, noisy]).astype(np.int8)
        carries = np.concatenate([np.zeros((1, ccsds.CARRY), np.int8), self.frames[:, -ccsds.CARRY:]])
        windows = [np.concatenate([carries[p], self.frames[c]]) for p in range(7) for c in range(6)]
        bits, self.verr = viterbi_cached(windows)
        self.cadu = ccsds.cadu_from_bits(bits, hrit)
        self.block, self.rs_errors, self.ok = ccsds.rs_decode_blocks(ccsds.derandomize(self.cadu[:, 4:]))
        self.scid, self.vcid, self.counter = ccsds.header_fields(self.block)
        for p in range(7):                                      # the coded frames decode to the sent VCDUs behind any carry
            assert np.array_equal(self.block[6 * p + 4:6 * p + 6, :892], self.sent[1:, :892]), p
        assert self.verr.reshape(7, 6)[:, 4:].min() > 0 and (self.rs_errors.reshape(7, 6, 4)[:, :3] == -1).all()
        assert len(set(self.verr.reshape(7, 6)[[1, 2, 3, 5, 6], 0].tolist())) > 1          # the carry shows in the count

    def expect(self, members, valid, last=-1):
        """(cadu, block, info fields as a dict, the last valid member) of a call on frames[members] with these valid
        flags on a handle whose carry is pool member `last` (-1: the start)."""
        members, valid = np.asarray(members, np.int64), np.asarray(valid, bool)
        prev = np.empty(len(members), np.int64)
        for f in range(len(members)):
            prev[f] = last
            if valid[f]:
                last = int(members[f])
        key = np.where(valid, 6 * (prev + 1) + members, 0)
        pick = lambda a, fill=0: np.where(valid.reshape((-1,) + (1,) * (a.ndim - 1)), a[key], fill)
        info = dict(valid=valid.astype(np.int64), ok=pick(self.ok), viterbi_errors=pick(self.verr), rs_errors=pick(self.rs_errors, -1),
                    scid=pick(self.scid), vcid=pick(self.vcid), counter=pick(self.counter))
        return pick(self.cadu), pick(self.block), info, last


_POOLS = {}


def pool_of(mode):
    if mode not in _POOLS:
        _POOLS[mode] = Pool(mode == "hrit")
    return _POOLS[mode]


def pair_cycle():
    """36 pool members in an order in which, read round and round, every ordered pair (a, b) follows on itself once: an
    Eulerian circuit of the complete directed graph with loops (Hierholzer)."""
    nxt = {a: list(range(6)) for a in range(6)}
    stack, out = [0], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            out.append(stack.pop())
    out = out[::-1][:-1]
    assert len(out) == 36 and len({(out[i], out[(i + 1) % 36]) for i in range(36)}) == 36
    return np.array(out, np.int64)


def members_for(valid, start=0):
    """Pool members of a call: the valid frames walk the pair cycle from position start; a valid = 0 frame holds another
    member than the valid one before it, so that a carry taken from it shows.  Returns (members, next start)."""
    cyc = pair_cycle()
    valid = np.asarray(valid, bool)
    order = start + np.cumsum(valid) - 1
    members = np.where(valid, cyc[order % 36], (cyc[np.maximum(order, 0) % 36] + 1 + np.arange(len(valid)) % 5) % 6)
    return members, start + int(valid.sum())


def check_call(got, want, what):
    cadu, block, info = got
    w_cadu, w_block, w_info, _ = want
    assert np.array_equal(cadu, w_cadu), (what, np.nonzero((cadu != w_cadu).any(axis=1))[0][:8])
    for name, col in w_info.items():
        bad = np.nonzero((info[name].astype(np.int64) != col).reshape(len(col), -1).any(axis=1))[0]
        assert not len(bad), (what, name, bad[:8], info[name][bad[:8]], col[bad[:8]])
    assert np.array_equal(block, w_block), (what, np.nonzero((block != w_block).any(axis=1))[0][:8])


def same_outputs(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()


def small_valid(nf, w, rng):
    """About a third of the frames out, frames 0 and nf - 1 among them (from three frames on), and in the longest call a
    run of w + 1 of them."""
    v = (rng.random(nf) > 0.2).astype(np.uint8)
    if nf >= 3:
        v[[0, nf - 1]] = 0
        v[1] = 1
    if nf >= 5 * w + 3:
        v[2 * w:3 * w + 1] = 0
        v[3 * w + 1] = 1
    return v


@pytest.mark.parametrize("mode", ["lrit", "hrit"])
def test_more_frames_than_windows_small_shapes(xa, mode):
    pool = pool_of(mode)
    rng = np.random.default_rng(43)
    dec, plain = xa.FrameDecoder(mode), xa.FrameDecoder(mode)
    last, at, holes, total = -1, 0, 0, 0
    for w in (7, 1, 3, 2):                                      # one handle: the setting grows and shrinks between calls
        dec.set_windows(w)
        for nf in (w, w + 1, 2 * w, 2 * w + 1, 5 * w + 3):
            valid = small_valid(nf, w, rng)
            members, at = members_for(valid, at)
            frames = pool.frames[members]
            want = pool.expect(members, valid, last)
            got = dec.decode(frames, valid)
            check_call(got, want, (w, nf))
            assert same_outputs(got, plain.decode(frames, valid)), (w, nf)
            last = want[3]
            holes, total = holes + int((valid == 0).sum()), total + nf
    assert 0.25 < holes / total < 0.45
    # 0 and anything above the default are the default: the same outputs again
    for w in (0xFFFFFFFF, 0):
        dec.set_windows(w)
        valid = small_valid(9, 2, rng)
        members, at = members_for(valid, at)
        want = pool.expect(members, valid, last)
        got = dec.decode(pool.frames[members], valid)
        check_call(got, want, w)
        assert same_outputs(got, plain.decode(pool.frames[members], valid)), w
        last = want[3]


def default_slots():
    torch = pytest.importorskip("torch")
    return torch.cuda.get_device_properties(0).multi_processor_count * 8


@pytest.fixture(scope="module")
def big_call(xa):
    """2 x slots + 37 frames in one LRIT call on a handle left at its default: every wave decodes a second frame, some a
    third.  Holes straddle the boundaries of the scan's 1024 thread segments (per frames each), one run is longer than
    three segments, and frames slots - 1 .. slots + 1 are valid, so that a frame's carry is another wave's frame."""
    slots = default_slots()
    nf = 2 * slots + 37
    per = -(-nf // 1024)
    rng = np.random.default_rng(47)
    valid = (rng.random(nf) > 0.25).astype(np.uint8)
    for t in (1, 2, 9, 200, 511, 512, 1000):
        b = min(per * t, nf - 3)
        valid[max(b - 2, 0):b + 2] = 0                           # a hole on both sides of a segment boundary
    run = per * 300 + 1
    valid[run:run + 3 * per + 2] = 0
    valid[slots - 1:slots + 2] = 1
    valid[2 * slots - 1:2 * slots + 2] = 1
    valid[[0, nf - 1]] = 0
    members, _ = members_for(valid)
    ordered = members[valid == 1]
    assert len(set(zip(ordered[:-1].tolist(), ordered[1:].tolist()))) == 36
    frames = pool_of("lrit").frames[members]
    got = xa.FrameDecoder("lrit").decode(frames, valid)
    return dict(slots=slots, nf=nf, per=per, valid=valid, members=members, frames=frames, got=got)


def test_more_frames_than_windows_default_geometry(big_call):
    b = big_call
    assert b["nf"] > 2 * b["slots"] and b["per"] >= 1
    check_call(b["got"], pool_of("lrit").expect(b["members"], b["valid"]), "default geometry")


def test_scratch_growth_and_carry_across_call_sizes(xa):
    pool = pool_of("lrit")
    slots = default_slots()
    sizes = (5, slots + 9, 3, 1500, 4)
    rng = np.random.default_rng(53)
    valid = (rng.random(sum(sizes)) > 0.3).astype(np.uint8)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    valid[cuts[3]:cuts[4]] = 0                                   # a call with no valid frame: the carry stays
    valid[[cuts[1] - 1, cuts[2] - 1, cuts[4]]] = (1, 0, 1)       # carries from a call's last frame, and from before a hole
    members, _ = members_for(valid)
    frames = pool.frames[members]
    dec = xa.FrameDecoder("lrit")
    parts = [dec.decode(frames[a:b], valid[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    joined = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))
    check_call(joined, pool.expect(members, valid), "five calls")
    assert same_outputs(joined, xa.FrameDecoder("lrit").decode(frames, valid))


def test_device_path_with_more_frames_than_windows(xa, big_call):
    torch = pytest.importorskip("torch")
    b = big_call
    nf, cut, item = b["nf"], b["slots"] | 1, xa.FRAME_INFO_DTYPE.itemsize
    dev = torch.device("cuda:0")
    d_frames = torch.from_numpy(b["frames"].view(np.uint8)).to(dev)
    d_valid = torch.from_numpy(b["valid"]).to(dev)
    # an odd cut: the second call's block rows would not start 16-byte aligned in one tensor, so each call has its own
    outs = [(torch.zeros((n, 1024), dtype=torch.uint8, device=dev), torch.zeros((n, 1020), dtype=torch.uint8, device=dev),
             torch.zeros(n * item, dtype=torch.uint8, device=dev)) for n in (cut, nf - cut)]
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    dec = xa.FrameDecoder("lrit")
    with torch.cuda.stream(s):
        for a, n, (c, bl, i) in ((0, cut, outs[0]), (cut, nf - cut, outs[1])):
            dec.decode_device(d_frames[a:].data_ptr(), d_valid[a:].data_ptr(), n, c.data_ptr(), bl.data_ptr(), i.data_ptr(),
                              stream=s.cuda_stream)
    s.synchronize()
    got = [np.concatenate([o[q].cpu().numpy() for o in outs]) for q in range(3)]
    assert np.array_equal(got[0], b["got"][0]) and np.array_equal(got[1], b["got"][1])
    assert got[2].view(xa.FRAME_INFO_DTYPE).tobytes() == b["got"][2].tobytes()
