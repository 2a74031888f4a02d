"""GPU tier: the frame decoder (xrit_decoder_*, FrameDecoder) against the NumPy specification of tests/ccsds.py --
Viterbi bit for bit on arbitrary soft frames, clean round trips of CADUs, RS correction up to and past 16 errors,
the carry across calls, and the whole chain from IQ to VCDUs, in the library and in the host program.  Every
assertion is exact."""
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
