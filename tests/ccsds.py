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


_ROOT_LOG = (PRIM * (FCR + np.arange(NROOTS))) % 255            # log of the i-th generator root


def syndromes(codeword, dual=True):
    """The 32 syndromes S_i = c(alpha^(11 (112 + i))) of a 255-byte codeword (zero for a codeword): (255,) -> (32,),
    or (n, 255) -> (n, 32), by Horner over all the words and roots at once."""
    c = np.asarray(codeword, np.uint8)
    assert c.shape[-1] == 255 and c.ndim in (1, 2)
    c2 = (TINV[c] if dual else c).astype(np.int64).reshape(-1, 255)
    acc = np.zeros((len(c2), NROOTS), np.int64)
    for j in range(255):
        acc = np.where(acc == 0, 0, EXP[LOG[acc] + _ROOT_LOG]) ^ c2[:, j, None]
    return acc.reshape(c.shape[:-1] + (NROOTS,))


# ---- a reference decoder by Peterson-Gorenstein-Zierler, independent of Berlekamp-Massey ------------------------
MUL = gf_mul(np.arange(256)[:, None], np.arange(256)[None, :]).astype(np.int64)       # the 256 x 256 product table
INV = np.zeros(256, np.int64)
INV[1:] = EXP[(255 - LOG[1:]) % 255]
_BETA_LOG = (PRIM * np.arange(255)) % 255                       # log of X = beta^k, the locator of the degree-k symbol


def gf_eliminate(a):
    """Gauss-Jordan over GF(2^8) on a copy of the matrix a (rows x cols, an augmented matrix if the caller wants):
    (reduced matrix, pivot columns).  The rank is the number of pivots."""
    a = np.array(a, np.int64)
    rows, cols = a.shape
    piv, r = [], 0
    for c in range(cols):
        if r == rows:
            break
        nz = np.nonzero(a[r:, c])[0]
        if not len(nz):
            continue
        p = r + nz[0]
        if p != r:
            a[[r, p]] = a[[p, r]]
        a[r] = MUL[INV[a[r, c]], a[r]]
        f = a[:, c].copy()
        f[r] = 0
        a ^= MUL[f[:, None], a[r][None, :]]
        piv.append(c)
        r += 1
    return a, piv


def gf_solve(m, rhs):
    """x with m x = rhs for a square non-singular m over GF(2^8), or None when m is singular."""
    m = np.asarray(m, np.int64)
    n = len(m)
    a, piv = gf_eliminate(np.concatenate([m, np.asarray(rhs, np.int64).reshape(n, 1)], axis=1))
    return a[:, n].copy() if piv == list(range(n)) else None


def _pgz(S):
    """Errors-only decoding from 32 non-zero syndromes: (degrees k, conventional magnitudes Y) of the unique error
    pattern of weight <= 16 with these syndromes, or None.  With Z_l = Y_l X_l^112 the syndromes are the power sums
    S_i = sum Z_l X_l^i, and the monic p(x) = prod (x - X_l) of degree v obeys S_(i+v) = sum_b p_b S_(i+b): v is the
    largest size at which the Hankel matrix [S_(a+b)] is non-singular.  Every leading block larger than the rank of the
    16 x 16 one is singular, so the search starts there."""
    S = np.asarray(S, np.int64)
    hankel = S[np.arange(16)[:, None] + np.arange(16)[None, :]]
    for v in range(len(gf_eliminate(hankel)[1]), 0, -1):
        p = gf_solve(hankel[:v, :v], S[v:2 * v])
        if p is None:
            continue
        # the roots of x^v + p_(v-1) x^(v-1) + ... + p_0 among all 255 locators, by evaluation
        x = EXP[_BETA_LOG]
        val = np.ones(255, np.int64)
        for b in range(v - 1, -1, -1):
            val = MUL[val, x] ^ p[b]
        k = np.nonzero(val == 0)[0]
        if len(k) != v:
            return None
        # magnitudes from the first v syndromes: S_i = sum_l Y_l X_l^(112 + i)
        van = EXP[(_BETA_LOG[k][None, :] * (FCR + np.arange(v))[:, None]) % 255]
        y = gf_solve(van, S[:v])
        if y is None or not y.all():
            return None
        # ... and it is the answer only if it explains all 32
        full = EXP[(_BETA_LOG[k][None, :] * (FCR + np.arange(NROOTS))[:, None]) % 255]
        if not np.array_equal(np.bitwise_xor.reduce(MUL[full, y[None, :]], axis=1), S):
            return None
        return k, y
    return None


def rs_decode_many(codewords_dual):
    """Reference errors-only decoder of RS(255,223) in the dual basis, (n, 255) -> (corrected (n, 255), counts (n,)):
    the unique codeword within 16 symbols and the distance to it, or the word unchanged and -1."""
    w = np.array(codewords_dual, np.uint8).reshape(-1, 255)
    out = w.copy()
    S = syndromes(w)
    counts = np.zeros(len(w), np.int64)
    for i in np.nonzero(S.any(axis=1))[0]:
        found = _pgz(S[i])
        if found is None:
            counts[i] = -1
            continue
        k, y = found
        conv = TINV[w[i]].astype(np.int64)
        conv[254 - k] ^= y                                     # byte 0 is the highest degree
        out[i] = T[conv]
        counts[i] = len(k)
    assert not syndromes(out[counts >= 0]).any()
    return out, counts


def rs_decode(codeword_dual):
    """One codeword: (corrected_dual (255,), n), n = -1 and the input back when it is uncorrectable."""
    out, n = rs_decode_many(np.asarray(codeword_dual, np.uint8).reshape(1, 255))
    return out[0], int(n[0])


def rs_decode_blocks(blocks):
    """The RS stage of the frame decoder on derandomised blocks (n, 1020): (blocks after correction, rs_errors (n, 4),
    ok (n,)); a frame is ok unless all four of its codewords are -1 (newdecoder.cpp:321)."""
    b = np.asarray(blocks, np.uint8).reshape(-1, BLOCK_BYTES)
    cws = b.reshape(-1, 255, 4).transpose(0, 2, 1).reshape(-1, 255)           # frame-major, codeword k = bytes k::4
    out, n = rs_decode_many(cws)
    fixed = out.reshape(-1, 4, 255).transpose(0, 2, 1).reshape(-1, BLOCK_BYTES)
    n = n.reshape(-1, 4)
    return fixed, n, (~(n == -1).all(axis=1)).astype(np.int64)


def header_fields(blocks):
    """(scid, vcid, counter) as newdecoder.cpp:342-348 reads them from bytes 0 .. 4 of every block."""
    b = np.asarray(blocks, np.uint8).reshape(-1, BLOCK_BYTES).astype(np.int64)
    return ((b[:, 0] & 0x3F) << 2) | ((b[:, 1] & 0xC0) >> 6), b[:, 1] & 0x3F, (b[:, 2] << 16) | (b[:, 3] << 8) | b[:, 4]


# ---- constructed error patterns (wire basis, 255 bytes, to be XORed onto a codeword) ----------------------------
def error_pattern(positions, values_conv):
    """Conventional-basis error values at byte positions, as the wire (dual-basis) XOR pattern: T is GF(2)-linear."""
    e = np.zeros(255, np.int64)
    e[np.asarray(positions, np.int64)] = np.asarray(values_conv, np.int64)
    return T[e]


def zero_syndrome_errors(positions, zero, rng):
    """An error pattern on the given byte positions, every value non-zero, whose syndromes S_i, i in zero, vanish: a
    linear system in the values (S_i = sum Y_l X_l^(112 + i)) with len(zero) < len(positions); the other values are
    drawn."""
    pos = np.asarray(positions, np.int64)
    nz, v = len(zero), len(pos)
    assert 0 < nz < v
    lx = _BETA_LOG[254 - pos]
    coef = EXP[(lx[None, :] * (FCR + np.asarray(zero, np.int64))[:, None]) % 255]          # (nz, v)
    for _ in range(100):
        free = rng.integers(1, 256, v - nz)
        rhs = np.bitwise_xor.reduce(MUL[coef[:, nz:], free[None, :]], axis=1)
        head = gf_solve(coef[:, :nz], rhs)
        if head is not None and head.all():
            e = error_pattern(pos, np.concatenate([head, free]))
            assert not syndromes(e)[list(zero)].any()
            return e
    raise AssertionError("no pattern found")


def generator_codeword(shift, scale):
    """The codeword scale * x^shift * g(x), wire basis: 33 non-zero symbols at bytes 222 - shift .. 254 - shift."""
    assert 0 <= shift <= 222 and 1 <= scale <= 255
    c = np.zeros(255, np.int64)
    c[222 - shift:255 - shift] = MUL[scale, GENPOLY]
    return T[c]


def near_codeword_error(shift, scale, j, rng):
    """(error pattern, the codeword it lies next to): 33 - j of the symbols of generator_codeword(shift, scale), so
    that a word sent + pattern is at distance 33 - j from sent and j from sent + that codeword."""
    g = generator_codeword(shift, scale)
    support = np.nonzero(g)[0]
    assert len(support) == 33
    e = g.copy()
    e[rng.choice(support, j, replace=False)] = 0
    return e, g


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
