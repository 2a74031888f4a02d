"""CPU tier: the NumPy specification of the frame decoder (tests/ccsds.py) -- PN sequence, dual basis, RS(255,223)
encoder and syndromes, the batched Viterbi against viterbi_decode_k7, the coded sync words -- and the decoder's
handle failing loudly without a HIP device."""
import os

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
