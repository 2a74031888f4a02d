"""CCSDS TM channel coding of an xRIT CADU, the NumPy specification of the decoder stage (test infrastructure):
GF(2^8) and Berlekamp's dual basis, the CCSDS pseudo-random sequence, a systematic RS(255,223) encoder, a CADU
builder, NRZ-M, the coded symbol streams of LRIT / HRIT, and a Viterbi over many windows at once whose decisions
are exactly those of test_oracle_kat.viterbi_decode_k7 (the contract in DESIGN.md, "Frame decoder").

What it restates is what the reference's decoder does per frame (decoder/src/newdecoder.cpp:272-359) with the
arithmetic of libSatHelper / libcorrect, which are not in the reference tree: the constants below are those of the
published CCSDS recommendation and libfec's tables, recalled rather than checked against an external vector."""
import numpy as np

import synth

FRAME_SYMBOLS = 16384           # CODEDFRAMESIZE (decoder/src/parameters.h)
CARRY = 64                      # LASTFRAMEDATA symbols prepended to every frame (newdecoder.cpp:274)
WINDOW = FRAME_SYMBOLS + CARRY  # 16448 symbols, 8224 bits
WINDOW_BITS = WINDOW // 2
CADU_BYTES = 1024
BLOCK_BYTES = 1020
VCDU_BYTES = 892
ASM = bytes([0x1A, 0xCF, 0xFC, 0x1D])

# ---- GF(2^8), p(x) = x^8 + x^7 + x^2 + x + 1 ---------------------------------------------------------------
GF_POLY = 0x187
EXP = np.zeros(512, np.int64)
LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= GF_POLY
EXP[255:510] = EXP[0:255]


def gf_mul(a, b):
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    r = EXP[(LOG[a] + LOG[b]) % 255]
    return np.where((a == 0) | (b == 0), 0, r)


# ---- Berlekamp's dual basis: T maps conventional to dual, TINV back ----------------------------------------
_TAL = (0x8D, 0xEF, 0xEC, 0x86, 0xFA, 0x99, 0xAF, 0x7B)
T = np.zeros(256, np.uint8)
for _i in range(256):
    _v = 0
    for _k in range(8):
        if (_i >> _k) & 1:
            _v ^= _TAL[7 - _k]
    T[_i] = _v
TINV = np.zeros(256, np.uint8)
TINV[T] = np.arange(256, dtype=np.uint8)


# ---- CCSDS pseudo-random sequence: h(x) = x^8 + x^7 + x^5 + x^3 + 1, all ones, MSB first ----------------------
def _pn():
    a = [1] * 8
    while len(a) < 255 * 8:
        n = len(a)
        a.append(a[n - 1] ^ a[n - 3] ^ a[n - 5] ^ a[n - 8])
    return np.packbits(np.array(a, np.uint8))


PN = _pn()                       # 255 bytes, one period


def derandomize(block):
    """XOR of bytes with the PN sequence from its start (the same operation randomises)."""
    b = np.asarray(block, np.uint8)
    return b ^ np.resize(PN, b.shape[-1])


# ---- RS(255,223): generator roots alpha^(11 (112 + i)), i = 0 .. 31 -------------------------------------------
FCR, PRIM, NROOTS = 112, 11, 32


def _genpoly():
    g = np.array([1], np.int64)                         # highest degree first
    for i in range(NROOTS):
        r = EXP[(PRIM * (FCR + i)) % 255]
        g = np.concatenate([g, [0]]) ^ np.concatenate([[0], gf_mul(g, r)])
    return g


GENPOLY = _genpoly()


def rs_encode(data):
    """Systematic encoder in the conventional basis: 223 data bytes -> 255-byte codeword (data, then parity).
    Byte 0 is the highest-degree coefficient."""
    d = np.asarray(data, np.int64)
    assert d.shape == (223,)
    rem = np.zeros(NROOTS, np.int64)
    for b in d:
        fb = b ^ rem[0]
        rem = np.concatenate([rem[1:], [0]]) ^ gf_mul(GENPOLY[1:], fb)
    return np.concatenate([d, rem]).astype(np.uint8)


def encode_ccsds(data):
    """The dual-basis encoder (libfec's encode_rs_ccsds): data bytes as they are on the wire, parity in dual."""
    d = np.asarray(data, np.uint8)
    cw = rs_encode(TINV[d])
    return np.concatenate([d, T[cw[223:]]]).astype(np.uint8)


def syndromes(codeword, dual=True):
    """The 32 syndromes S_i = c(alpha^(11 (112 + i))) of one 255-byte codeword (zero for a codeword)."""
    c = np.asarray(codeword, np.uint8)
    c = (TINV[c] if dual else c).astype(np.int64)
    s = np.zeros(NROOTS, np.int64)
    for i in range(NROOTS):
        r = EXP[(PRIM * (FCR + i)) % 255]
        acc = 0
        for b in c:
            acc = int(gf_mul(acc, r)) ^ int(b)
        s[i] = acc
    return s


def interleave(codewords):
    """4 codewords of 255 -> 1020-byte block: byte j is symbol j // 4 of codeword j % 4."""
    cw = np.asarray(codewords, np.uint8)
    return cw.T.reshape(-1).copy()


def deinterleave(block):
    return np.asarray(block, np.uint8).reshape(255, 4).T.copy()


def vcdu_header(scid, vcid, counter):
    """Version 01, 8-bit SCID, 6-bit VCID, 24-bit counter, signalling byte 0 (the fields newdecoder.cpp:342-348 reads)."""
    return np.array([0x40 | (scid >> 2), ((scid & 3) << 6) | vcid, (counter >> 16) & 0xFF, (counter >> 8) & 0xFF,
                     counter & 0xFF, 0], np.uint8)


def make_block(scid, vcid, counter, rng):
    """The 1020-byte RS block of one frame (what the decoder's rsCorrectedData holds): 892-byte VCDU = header +
    random payload, then RS parity, four codewords interleaved."""
    vcdu = np.concatenate([vcdu_header(scid, vcid, counter), rng.integers(0, 256, VCDU_BYTES - 6).astype(np.uint8)])
    data = np.concatenate([vcdu, np.zeros(4 * 223 - VCDU_BYTES, np.uint8)])      # 892 = 4 * 223: no fill
    cws = [encode_ccsds(data[k::4]) for k in range(4)]
    return interleave(cws)


def cadu_from_block(block):
    """ASM + randomised block: 1024 bytes."""
    return np.concatenate([np.frombuffer(ASM, np.uint8), derandomize(block)]).astype(np.uint8)


def bytes_to_bits(b):
    return np.unpackbits(np.asarray(b, np.uint8))


def nrzm_encode(bits):
    """NRZ-M: the line changes level on a one, d[i] = d[i-1] ^ b[i], d[-1] = 0."""
    return (np.cumsum(np.asarray(bits, np.int64)) & 1).astype(np.uint8)


def nrzm_decode(bits):
    b = np.asarray(bits, np.uint8)
    return b ^ np.concatenate([[0], b[:-1]]).astype(np.uint8)


def coded_symbols(cadus, hrit=False, amplitude=100):
    """int8 soft symbols of a stream of CADUs, convolutionally coded as one stream from state 0 (coded bit 0 ->
    +amplitude).  HRIT: NRZ-M before the code."""
    bits = bytes_to_bits(np.concatenate([np.asarray(c, np.uint8) for c in cadus]))
    if hrit:
        bits = nrzm_encode(bits)
    coded = synth.conv_encode_k7(bits)
    return np.where(coded == 1, -amplitude, amplitude).astype(np.int8)


# ---- the carry rule and the batched Viterbi ---------------------------------------------------------------
def windows(frames, valid, carry=None):
    """(windows of the valid frames, indices of those frames, carry after the call): each valid frame is prefixed
    with the last 64 symbols of the most recent earlier valid frame (carry: the previous call's, zeros at start)."""
    frames = np.asarray(frames, np.int8).reshape(-1, FRAME_SYMBOLS)
    carry = np.zeros(CARRY, np.int8) if carry is None else np.asarray(carry, np.int8)
    out, idx = [], []
    for f in range(len(frames)):
        if valid[f]:
            out.append(np.concatenate([carry, frames[f]]))
            idx.append(f)
            carry = frames[f][-CARRY:].copy()
    w = np.stack(out) if out else np.zeros((0, WINDOW), np.int8)
    return w, np.array(idx, np.int64), carry


_PAR = np.array([bin(v).count("1") & 1 for v in range(128)], np.int64)


def viterbi_batch(win):
    """Viterbi of every row of win (n, 16448) exactly as viterbi_decode_k7 decides (start metrics 0, tie keeps the
    predecessor ns >> 1, traceback from the first best end state), in int64.  Returns (bits (n, 8224), errors (n,)):
    errors counts the symbols with s * (1 - 2c) < 0, c the re-encoded decision path (register = the chosen
    transition's, so the first six steps use the start state the traceback ends in)."""
    s = np.asarray(win, np.int64)
    n, m = s.shape[0], s.shape[1] // 2
    ns = np.arange(64)
    regs = np.stack([ns, ns | 64])
    ea = 1 - 2 * _PAR[regs & 0x4F]
    ec = 1 - 2 * _PAR[regs & 0x6D]
    prev = regs >> 1
    pm = np.zeros((n, 64), np.int64)
    dec = np.zeros((m, n, 64), bool)
    for t in range(m):
        cand = pm[:, prev] + s[:, 2 * t, None, None] * ea + s[:, 2 * t + 1, None, None] * ec    # (n, 2, 64)
        c = cand[:, 1] > cand[:, 0]
        dec[t] = c
        pm = np.where(c, cand[:, 1], cand[:, 0])
    st = pm.argmax(axis=1)
    rows = np.arange(n)
    bits = np.zeros((n, m), np.uint8)
    regs_t = np.zeros((n, m), np.int64)
    for t in range(m - 1, -1, -1):
        d = dec[t, rows, st].astype(np.int64)
        bits[:, t] = st & 1
        regs_t[:, t] = st | (d << 6)
        st = (st >> 1) | (d << 5)
    c0 = _PAR[regs_t & 0x4F]
    c1 = _PAR[regs_t & 0x6D]
    err = ((s[:, 0::2] * (1 - 2 * c0)) < 0).sum(axis=1) + ((s[:, 1::2] * (1 - 2 * c1)) < 0).sum(axis=1)
    return bits, err


def cadu_from_bits(bits, hrit=False):
    """The decoded window's 8224 bits -> cadu bytes (n, 1024): HRIT NRZ-M decodes the whole window first, then the 32
    prefix bits go."""
    b = np.asarray(bits, np.uint8)
    if hrit:
        b = b ^ np.concatenate([np.zeros((b.shape[0], 1), np.uint8), b[:, :-1]], axis=1)
    return np.packbits(b[:, 32:], axis=1)
