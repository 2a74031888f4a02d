"""CPU tier: the NumPy specification of the frame decoder (tests/ccsds.py) -- PN sequence, dual basis, RS(255,223)
encoder and syndromes, the reference RS decoder (Peterson-Gorenstein-Zierler) by construction, the batched Viterbi
against viterbi_decode_k7, the coded sync words -- the decoder's handle failing loudly without a HIP device, and
rs_solve (rs_core.h) in its host program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ccsds
import synth
from test_oracle_kat import viterbi_decode_k7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pn_sequence():
    assert ccsds.PN[:8].tobytes() == bytes([0xFF, 0x48, 0x0E, 0xC0, 0x9A, 0x0D, 0x70, 0xBC])
    assert len(ccsds.PN) == 255
    bits = np.unpackbits(ccsds.PN)
    # period 255 bits of the m-sequence: no shorter period divides it
    for p in (3, 5, 15, 17, 51, 85):
        assert not np.array_equal(bits[:255 - p], bits[p:255])
    assert bits[:255].sum() == 128 and np.array_equal(bits[:1785], bits[255:])     # period 255 bits


def test_dual_basis_tables():
    assert ccsds.T[:8].tobytes() == bytes([0x00, 0x7B, 0xAF, 0xD4, 0x99, 0xE2, 0x36, 0x4D])
    assert ccsds.TINV[:8].tobytes() == bytes([0x00, 0xCC, 0xAC, 0x60, 0x79, 0xB5, 0xD5, 0x19])
    assert np.array_equal(ccsds.TINV[ccsds.T], np.arange(256))
    assert np.array_equal(ccsds.T[ccsds.TINV], np.arange(256))


def test_rs_encoder_gives_codewords():
    rng = np.random.default_rng(5)
    for _ in range(2):
        data = rng.integers(0, 256, 223).astype(np.uint8)
        cw = ccsds.encode_ccsds(data)
        assert np.array_equal(cw[:223], data)
        assert not ccsds.syndromes(cw).any()
        assert not ccsds.syndromes(ccsds.rs_encode(data), dual=False).any()
        for pos in (0, 100, 222, 223, 254):
            bad = cw.copy()
            bad[pos] ^= rng.integers(1, 256)
            assert ccsds.syndromes(bad).any(), pos


def test_batched_syndromes_equal_the_polynomial_evaluated():
    rng = np.random.default_rng(8)
    w = rng.integers(0, 256, (5, 255)).astype(np.uint8)
    w[3] = ccsds.encode_ccsds(w[3, :223])
    S = ccsds.syndromes(w)
    assert S.shape == (5, 32) and not S[3].any() and S[[0, 1, 2, 4]].any(axis=1).all()
    assert np.array_equal(ccsds.syndromes(w[1]), S[1]) and ccsds.syndromes(w[1]).shape == (32,)
    # term by term: sum_j c_j root^(254 - j)
    c = ccsds.TINV[w].astype(np.int64)
    for i in (0, 1, 17, 31):
        root_log = (ccsds.PRIM * (ccsds.FCR + i)) % 255
        terms = ccsds.gf_mul(c, ccsds.EXP[(root_log * (254 - np.arange(255))) % 255])
        assert np.array_equal(np.bitwise_xor.reduce(terms, axis=1), S[:, i]), i
    assert np.array_equal(ccsds.syndromes(c.astype(np.uint8), dual=False), S)


def test_generator_polynomial_has_33_coefficients():
    lone = np.zeros(223, np.uint8)
    lone[222] = 1
    cw = ccsds.rs_encode(lone)
    assert int((cw != 0).sum()) == 33 and np.array_equal(cw[222:], ccsds.GENPOLY)
    assert np.array_equal(ccsds.generator_codeword(0, 1), ccsds.T[cw])
    for shift, scale in ((0, 1), (222, 255), (100, 37)):
        g = ccsds.generator_codeword(shift, scale)
        assert int((g != 0).sum()) == 33 and not ccsds.syndromes(g).any()


@pytest.fixture(scope="module")
def sent_codeword():
    return ccsds.encode_ccsds(np.random.default_rng(21).integers(0, 256, 223).astype(np.uint8))


def test_reference_rs_decoder_corrects_every_count(sent_codeword):
    rng = np.random.default_rng(22)
    words, counts = [], []
    for v in range(17):
        for rep in range(6):
            pos = rng.choice(255, v, replace=False)
            if rep == 1 and v >= 2:
                pos[:2] = (0, 254)
                pos[2:] = rng.choice(np.arange(1, 254), v - 2, replace=False)
            elif rep == 2:
                pos = 223 + rng.choice(32, v, replace=False)
            words.append(sent_codeword ^ ccsds.error_pattern(pos, rng.integers(1, 256, v)))
            counts.append(v)
    out, n = ccsds.rs_decode_many(np.stack(words))
    assert n.tolist() == counts
    assert (out == sent_codeword).all()
    one, k = ccsds.rs_decode(words[-1])
    assert k == 16 and np.array_equal(one, sent_codeword)
    # every single-error position and every non-zero wire byte as the error
    single = np.tile(sent_codeword, (255, 1))
    single[np.arange(255), np.arange(255)] ^= np.arange(1, 256).astype(np.uint8)
    out, n = ccsds.rs_decode_many(single)
    assert (n == 1).all() and (out == sent_codeword).all()


def test_reference_rs_decoder_refuses_beyond_16(sent_codeword):
    """A random word lies within 16 of a codeword with probability of order 1e-13: a count other than -1 here is a
    failure to look at, never a case to skip."""
    rng = np.random.default_rng(23)
    words = []
    for v in range(17, 41):
        for _ in range(4):
            words.append(sent_codeword ^ ccsds.error_pattern(rng.choice(255, v, replace=False), rng.integers(1, 256, v)))
    words = np.stack(words)
    out, n = ccsds.rs_decode_many(words)
    assert (n == -1).all(), n
    assert np.array_equal(out, words)
    one, k = ccsds.rs_decode(words[0])
    assert k == -1 and np.array_equal(one, words[0])


def test_reference_rs_decoder_zero_syndromes_and_other_spheres(sent_codeword):
    rng = np.random.default_rng(24)
    # chosen syndromes zero: still v errors from the sent word
    for v in (2, 3, 8, 16):
        for zero in ((0,), (0, 1), (15,), (31,)):
            if len(zero) >= v:
                continue
            e = ccsds.zero_syndrome_errors(rng.choice(255, v, replace=False), zero, rng)
            assert int((e != 0).sum()) == v and not ccsds.syndromes(sent_codeword ^ e)[list(zero)].any()
            out, n = ccsds.rs_decode(sent_codeword ^ e)
            assert n == v and np.array_equal(out, sent_codeword), (v, zero)
    # 33 - j symbols of another codeword: j from that one for j <= 16, 16 from the sent one for j = 17
    for j in (1, 8, 16, 17):
        for shift, scale in ((0, 1), (222, 200), (57, 3)):
            e, g = ccsds.near_codeword_error(shift, scale, j, rng)
            assert int((e != 0).sum()) == 33 - j
            out, n = ccsds.rs_decode(sent_codeword ^ e)
            if j <= 16:
                assert n == j and np.array_equal(out, sent_codeword ^ g), (j, shift)
            else:
                assert n == 16 and np.array_equal(out, sent_codeword), (j, shift)


def test_reference_rs_stage_on_blocks():
    rng = np.random.default_rng(25)
    sent = np.stack([ccsds.make_block(0x8C, 9, 0x010203 + i, rng) for i in range(3)])
    blocks = sent.copy()
    blocks[0, [0, 1, 2, 3, 4, 1019]] ^= 0x5A                       # header bytes and the last parity byte
    bad = rng.choice(255, 40, replace=False)
    blocks[1, 4 * bad + 2] ^= rng.integers(1, 256, 40).astype(np.uint8)
    blocks[2] ^= rng.integers(1, 256, 1020).astype(np.uint8)
    fixed, n, ok = ccsds.rs_decode_blocks(blocks)
    assert n.tolist() == [[2, 1, 1, 2], [0, 0, -1, 0], [-1] * 4] and ok.tolist() == [1, 1, 0]
    assert np.array_equal(fixed[0], sent[0]) and np.array_equal(fixed[1:], blocks[1:])
    scid, vcid, counter = ccsds.header_fields(fixed)
    assert (scid[:2] == 0x8C).all() and (vcid[:2] == 9).all() and counter[:2].tolist() == [0x010203, 0x010204]


def test_block_layout():
    rng = np.random.default_rng(1)
    block = ccsds.make_block(0x8C, 5, 0x123456, rng)
    assert block[:6].tolist() == [0x40 | (0x8C >> 2), ((0x8C & 3) << 6) | 5, 0x12, 0x34, 0x56, 0]
    for k in range(4):
        assert not ccsds.syndromes(ccsds.deinterleave(block)[k]).any()
    cadu = ccsds.cadu_from_block(block)
    assert cadu[:4].tobytes() == ccsds.ASM and np.array_equal(ccsds.derandomize(cadu[4:]), block)


@pytest.mark.parametrize("kind", ["uniform", "ties", "zeros", "saturated"])
def test_batched_viterbi_equals_the_plain_one(kind):
    rng = np.random.default_rng({"uniform": 1, "ties": 2, "zeros": 3, "saturated": 4}[kind])
    n = 3
    if kind == "uniform":
        w = rng.integers(-128, 128, (n, 600))
    elif kind == "ties":
        w = rng.integers(-2, 3, (n, 600))
    elif kind == "zeros":
        w = np.zeros((n, 600), np.int64)
        w[1, 100:300] = rng.integers(-1, 2, 200)
    else:
        w = rng.choice([-127, 127], (n, 600))
    bits, err = ccsds.viterbi_batch(w)
    for i in range(n):
        assert np.array_equal(bits[i], viterbi_decode_k7(w[i].astype(np.float64))), i
    # viterbi_errors of a clean coded stream is 0, and counts the flipped symbols when the path survives them
    sent = rng.integers(0, 2, 300).astype(np.uint8)
    s = np.where(synth.conv_encode_k7(sent) == 1, -100, 100)
    b, e = ccsds.viterbi_batch(s[None])
    assert np.array_equal(b[0], sent) and e[0] == 0
    s2 = s.copy()
    s2[[40, 200, 401]] *= -1
    s2[77] = 0
    b, e = ccsds.viterbi_batch(s2[None])
    assert np.array_equal(b[0], sent) and e[0] == 3


def test_coded_sync_words():
    """The coded ASM is LRIT_UW2 (newdecoder.cpp:24); NRZ-M coded behind six ones (previous NRZ-M bit 0, register
    history 0b111111) it is HRIT_UW2 (:22)."""
    asm = ccsds.bytes_to_bits(np.frombuffer(ccsds.ASM, np.uint8))
    as_int = lambda bits: int("".join(map(str, bits)), 2)
    assert as_int(synth.conv_encode_k7(asm)) == 0x035d49c24ff2686b
    hist = np.concatenate([np.ones(6, np.uint8), ccsds.nrzm_encode(asm)])
    assert as_int(synth.conv_encode_k7(hist)[12:]) == 0x25010b02f33d2076


def test_carry_rule():
    rng = np.random.default_rng(0)
    fr = rng.integers(-128, 128, (4, ccsds.FRAME_SYMBOLS)).astype(np.int8)
    w, idx, carry = ccsds.windows(fr, [1, 0, 1, 0])
    assert idx.tolist() == [0, 2]
    assert not w[0, :64].any() and np.array_equal(w[1, :64], fr[0, -64:]) and np.array_equal(carry, fr[2, -64:])
    w2, _, carry2 = ccsds.windows(fr[:1], [0], carry)
    assert len(w2) == 0 and np.array_equal(carry2, carry)


def test_frame_decoder_without_a_device_has_no_cpu_path():
    import xritdemod_amd as xa
    if not os.path.exists(xa.lib_path()):
        xa.build()
    if xa.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(xa.XritError) as e:
        xa.FrameDecoder("lrit")
    assert e.value.code == -2 and "no CPU path" in str(e.value)
    with pytest.raises(ValueError):
        xa.FrameDecoder("bpsk")


def test_rs_solve_host_check_under_sanitizers(tmp_path):
    """make rs-host-check: rs_core.h's decoder in a stand-alone g++ program with -fsanitize=address,undefined, 10 000
    random patterns of every weight 0 .. 16, 2 000 of every weight 17 .. 48 and the constructed classes."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "rs-host-check",
                        f"RS_CHECK={tmp_path / 'rs_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rs host check ok: 241000 words decoded, 170000 corrected" in r.stdout, r.stdout
