"""Python specification of the Rice decoder (xrit_rice_*, RiceDecoder), with the matching encoder
and sample generators (test infrastructure).

The reference tree ends at the VCDU, so this layer is specified here, from the CCSDS lossless data compression
recommendation (CCSDS 121.0-B: the adaptive entropy coder with its zero-block, second-extension, split-sample and
no-compression options and the unit-delay predictor with its mapper): `decode` is the serial statement, one block at a
time, and the device must equal it sample for sample and status for status.  tests/test_rice_libaec.py holds decoder
and encoder against libaec 1.0.4 (tests/aec_ref.py); no recorded downlink was at hand, and DESIGN.md lists what stays
open.

One line = one byte string = one reference-sample interval, bits MSB first.  n bits per sample (1 .. 16), J in
{8, 16, 32, 64} samples per block, S samples per line (1 .. 65535), B = ceil(S / J) blocks; the encoder pads the last
block with repeats of the last sample and the decoder drops them.  The option ID has 3 bits for n <= 8, else 4."""
import math
import os

import numpy as np

BLOCK_SIZES = (8, 16, 32, 64)
SEGMENT = 64                      # blocks per segment: what the rest-of-segment zero-block code counts to
ZERO, SE, RAW = "zero", "se", "raw"


def id_bits(n):
    return 3 if n <= 8 else 4


def check_params(n, J, S):
    if not (1 <= n <= 16 and J in BLOCK_SIZES and 1 <= S <= 65535):
        raise ValueError((n, J, S))


# ---- the serial statement: the decoder -------------------------------------------------------------------------------
class _Fault(Exception):
    pass


class _Bits:
    """MSB-first reader over a byte string: fixed fields through Python integers, fundamental-sequence codes through the
    sorted positions of the set bits."""

    def __init__(self, data):
        self.data = bytes(data)
        self.n = 8 * len(self.data)
        self.pos = 0
        self.ones = np.flatnonzero(np.unpackbits(np.frombuffer(self.data, np.uint8))) if self.data else np.zeros(0, np.int64)

    def get(self, m):
        if self.pos + m > self.n:
            raise _Fault
        if m == 0:
            return 0
        a, b = self.pos >> 3, (self.pos + m + 7) >> 3
        v = int.from_bytes(self.data[a:b], "big") >> (8 * b - self.pos - m)
        self.pos += m
        return v & ((1 << m) - 1)

    def fs(self, count):
        """`count` fundamental-sequence codes (m zeros, then a one): their values."""
        i = int(np.searchsorted(self.ones, self.pos))
        if i + count > len(self.ones):
            raise _Fault
        ends = self.ones[i:i + count]
        vals = np.diff(ends, prepend=self.pos - 1) - 1
        self.pos = int(ends[-1]) + 1
        return [int(v) for v in vals]


def decode(data, n, J, S, stats=None):
    """One line.  -> (samples (S,) int64, status): status 1 on a fault, the samples of the blocks decoded in front of it
    kept and the rest 0.  stats, a dict, counts the options met, under encode's keys, and under "long" the zero-block
    codes of five blocks and more that are not the rest-of-segment code."""
    check_params(n, J, S)
    B, L, xmax = -(-S // J), id_bits(n), (1 << n) - 1
    out = np.zeros(B * J, np.int64)
    rd = _Bits(data)
    status, b, prev = 0, 0, 0

    def count(key):
        if stats is not None:
            stats[key] = stats.get(key, 0) + 1

    try:
        while b < B:
            ref = b == 0
            cnt = J - 1 if ref else J
            ident = rd.get(L)
            nb = 1
            if ident == 0:
                second = rd.get(1)
                r = rd.get(n) if ref else None
                if second:
                    count(SE)
                    dl = []
                    for g in rd.fs(J // 2):
                        beta = (math.isqrt(8 * g + 1) - 1) // 2
                        c = g - beta * (beta + 1) // 2
                        dl += [beta - c, c]
                    if ref:
                        if dl[0] != 0:
                            raise _Fault
                        dl = dl[1:]
                else:
                    v = rd.fs(1)[0]
                    count(ZERO)
                    if v == 4:
                        count("rest")
                        nb = min(B, (b // SEGMENT + 1) * SEGMENT) - b
                    else:
                        nb = v + 1 if v < 4 else v
                        if v > 4:
                            count("long")
                    if b + nb > B:
                        raise _Fault
                    dl = [0] * (nb * J - (1 if ref else 0))
            elif ident == (1 << L) - 1:
                count(RAW)
                r = rd.get(n) if ref else None
                dl = [rd.get(n) for _ in range(cnt)]
            else:
                k = ident - 1
                count(k)
                r = rd.get(n) if ref else None
                hi = rd.fs(cnt)
                dl = [(h << k) | rd.get(k) for h in hi]
            if any(v > xmax for v in dl):
                raise _Fault
            vals = []
            if ref:
                prev = r
                vals.append(r)
            for v in dl:
                th = min(prev, xmax - prev)
                if v <= 2 * th:
                    d = v // 2 if v % 2 == 0 else -((v + 1) // 2)
                else:
                    d = v - th if prev <= xmax - prev else -(v - th)
                prev += d
                if not 0 <= prev <= xmax:
                    raise _Fault
                vals.append(prev)
            out[b * J:b * J + len(vals)] = vals
            b += nb
    except _Fault:
        status = 1
    return out[:S], status


def decode_batch(lines, n, J, S):
    """(samples (len(lines), S) uint8 for n <= 8 else uint16, status (len(lines),) uint8): what the device returns."""
    out = np.zeros((len(lines), S), np.uint8 if n <= 8 else np.uint16)
    status = np.zeros(len(lines), np.uint8)
    for i, ln in enumerate(lines):
        y, status[i] = decode(ln, n, J, S)
        out[i] = y
    return out, status


# ---- the encoder ------------------------------------------------------------------------------------------------------
def map_residuals(x, n):
    """The mapped prediction residuals of a line under the unit-delay predictor (entry 0, the reference, is 0)."""
    x = np.asarray(x, np.int64)
    xmax = (1 << n) - 1
    p = x[:-1]
    d = x[1:] - p
    th = np.minimum(p, xmax - p)
    m = np.where((0 <= d) & (d <= th), 2 * d, np.where((-th <= d) & (d < 0), -2 * d - 1, th + np.abs(d)))
    return np.concatenate([[0], m])


class Writer:
    """MSB-first bit writer: fixed fields, fundamental-sequence codes; bytes() pads the last byte with zeros."""

    def __init__(self):
        self.parts = []

    def put(self, v, m):
        if m:
            self.parts.append(format(int(v), "0%db" % m))

    def fs(self, m):
        self.parts.append("0" * int(m) + "1")

    def bytes(self):
        s = "".join(self.parts)
        s += "0" * (-len(s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def encode(x, n, J, force=None, stats=None):
    """A line of samples -> bytes.  Every block takes its cheapest option (ties: the smallest k, then the second
    extension, then raw); `force` -- a k, SE or RAW -- makes every block that is not all zero take that one, or
    force = "nozero" the cheapest other than the zero block.  stats, a dict, counts the options chosen: ZERO, "rest" (the
    rest-of-segment code among them), SE, RAW and the k's."""
    x = [int(v) for v in x]
    S = len(x)
    check_params(n, J, S)
    xmax = (1 << n) - 1
    assert min(x) >= 0 and max(x) <= xmax
    B, L = -(-S // J), id_bits(n)
    x = x + [x[-1]] * (B * J - S)
    d = map_residuals(x, n).reshape(B, J)
    kmax = (1 << L) - 3
    cost = np.stack([(d >> k).sum(1) + (k + 1) * J for k in range(kmax + 1)])
    cost[:, 0] -= np.arange(kmax + 1) + 1                 # block 0 carries J - 1 values (d[0, 0] is 0)
    g = (d[:, 0::2] + d[:, 1::2]) * (d[:, 0::2] + d[:, 1::2] + 1) // 2 + d[:, 1::2]
    cost_se = 1 + (g + 1).sum(1)
    cost_raw = np.full(B, n * J)
    cost_raw[0] -= n
    zero = ~d.any(1)
    w = Writer()

    def count(key):
        if stats is not None:
            stats[key] = stats.get(key, 0) + 1

    b = 0
    while b < B:
        ref = b == 0
        body = d[b, 1:] if ref else d[b]
        if zero[b] and force in (None,):
            seg_end = min(B, (b // SEGMENT + 1) * SEGMENT)
            z = 1
            while b + z < seg_end and zero[b + z]:
                z += 1
            w.put(0, L + 1)
            if ref:
                w.put(x[0], n)
            if b + z == seg_end and z >= 5:
                w.fs(4)
                count("rest")
            else:
                w.fs(z - 1 if z <= 4 else z)
            count(ZERO)
            b += z
            continue
        if force is None or force == "nozero":
            best, c = 0, int(cost[0, b])
            for k in range(1, kmax + 1):
                if cost[k, b] < c:
                    best, c = k, int(cost[k, b])
            if cost_se[b] < c:
                best, c = SE, int(cost_se[b])
            if cost_raw[b] < c:
                best = RAW
        else:
            best = force
        count(best)
        if best == SE:
            w.put(1, L + 1)
            if ref:
                w.put(x[0], n)
            for v in g[b]:
                w.fs(v)
        elif best == RAW:
            w.put((1 << L) - 1, L)
            if ref:
                w.put(x[0], n)
            for v in body:
                w.put(v, n)
        else:
            k = int(best)
            assert 0 <= k <= kmax
            w.put(k + 1, L)
            if ref:
                w.put(x[0], n)
            for v in body:
                w.fs(int(v) >> k)
            for v in body:
                w.put(int(v) & ((1 << k) - 1), k)
        b += 1
    return w.bytes()


# ---- generators -------------------------------------------------------------------------------------------------------
KINDS = ("uniform", "walk3", "constant", "scaled", "sparse")


def samples(rng, kind, n, J, S):
    """One line of S samples of n bits: uniform noise, a +-3 walk, a constant with rare zeros, a walk whose step scale is
    drawn per block from 0 .. 4000, a sparse +-1 walk.  Together they make the encoder choose every option."""
    xmax = (1 << n) - 1
    if kind == "uniform":
        x = rng.integers(0, xmax + 1, S)
    elif kind == "walk3":
        x = np.cumsum(rng.integers(-3, 4, S)) + xmax // 2
    elif kind == "constant":
        x = np.full(S, int(rng.integers(0, xmax + 1)))
        x[rng.random(S) < 0.002] = 0
    elif kind == "scaled":
        sc = np.repeat(rng.choice([0, 0, 1, 2, 4, 8, 16, 40, 100, 250, 600, 1500, 4000], -(-S // J)), J)[:S]
        x = np.cumsum(rng.normal(0, 1, S) * sc).astype(np.int64) + xmax // 2
    elif kind == "sparse":
        x = np.cumsum(rng.integers(-1, 2, S) * (rng.random(S) < 0.3)) + xmax // 2
    else:
        raise ValueError(kind)
    return np.clip(x, 0, xmax).astype(np.int64)


def random_line(rng, n, J, S, kind=None, stats=None):
    """(samples, bytes) of one generated line."""
    kind = KINDS[int(rng.integers(0, len(KINDS)))] if kind is None else kind
    x = samples(rng, kind, n, J, S)
    return x, encode(x, n, J, stats=stats)


def truncate(rng, line):
    """Damage: the line cut at a random byte."""
    return line[:int(rng.integers(0, len(line)))] if line else line


def flip(rng, line, count=1):
    """Damage: `count` bits flipped."""
    a = bytearray(line)
    for _ in range(count if a else 0):
        a[int(rng.integers(0, len(a)))] ^= 1 << int(rng.integers(0, 8))
    return bytes(a)


# ---- lines made by hand: long codes, chunk edges, limits -------------------------------------------------------------
def samples_of(ref, deltas, n):
    """The samples behind the reference `ref` whose mapped residuals are `deltas`, each found by a search through the
    encoder's mapper (the mapper is a bijection on 0 .. 2^n - 1 for every predecessor; the decoder is not consulted)."""
    cand = np.arange(1 << n)
    out, prev = [int(ref)], int(ref)
    for v in deltas:
        pairs = np.empty(2 * len(cand), np.int64)
        pairs[0::2], pairs[1::2] = prev, cand
        hit = np.flatnonzero(map_residuals(pairs, n)[1::2] == int(v))
        assert len(hit) == 1, (prev, v)
        prev = int(hit[0])
        out.append(prev)
    return np.array(out, np.int64)


def split_line(n, J, k, ref, deltas, pad=True):
    """A one-block line (S = J) under the split-sample option k, written by hand from the J - 1 mapped residuals behind
    the reference -> (bytes, bits written).  pad = False: the bits must fill whole bytes."""
    assert len(deltas) == J - 1
    w = Writer()
    w.put(k + 1, id_bits(n))
    w.put(ref, n)
    for v in deltas:
        w.fs(int(v) >> k)
    for v in deltas:
        w.put(int(v) & ((1 << k) - 1), k)
    bits = sum(len(p) for p in w.parts)
    assert pad or bits % 8 == 0
    return w.bytes(), bits


def se_line(n, J, ref, gammas):
    """A one-block line (S = J) under the second extension, from its J / 2 codes -> bytes."""
    assert len(gammas) == J // 2
    w = Writer()
    w.put(1, id_bits(n) + 1)
    w.put(ref, n)
    for g in gammas:
        w.fs(g)
    return w.bytes()


def longest_zero_run(line):
    """The longest run of zero bits in front of a one."""
    ones = np.flatnonzero(np.unpackbits(np.frombuffer(bytes(line), np.uint8)))
    return int((np.diff(ones, prepend=-1) - 1).max()) if len(ones) else 0


# (n, J, S, k, the zero run the case is for): uniform samples under a forced low k.  Codes across the wave form's 64-bit
# windows (> 64); one block's codes across its 4096-bit chunks (more than 4096 bits of codes in a block of zero runs
# > 64); single codes longer than a chunk, with chunks that hold no one in the middle (> 4096; > 2 * 4096)
FORCED_LOW_K = ((8, 64, 192, 0, 64), (12, 16, 48, 0, 64), (16, 8, 16, 3, 4096), (16, 8, 16, 0, 2 * 4096), (16, 64, 128, 2, 2 * 4096))


def forced_low_k_line(case, seed=11):
    """-> (samples, bytes) of one FORCED_LOW_K case."""
    n, J, S, k, _ = case
    x = samples(np.random.default_rng(seed + n * J + k), "uniform", n, J, S)
    return x, encode(x, n, J, force=k)


CHUNK_EDGES = (4095, 4096, 4097, 8191, 8192, 8193)


def chunk_edge_lines():
    """Split-sample blocks (n = 16, J = 8, k = 2) in which a code's terminating one lies on bit 4095, 4096, 4097, 8191,
    8192, 8193 counted from the start of the codes: once the first code's (its value is measured from the bit in front
    of the section), once the second's (from the first's one) -> [(bytes, samples, bit of the one)]."""
    out = []
    for at in CHUNK_EDGES:
        for lead in ((), (3,)):
            hs = list(lead) + [at - sum(h + 1 for h in lead)] + [1, 0, 2, 0, 5, 0][:6 - len(lead)]
            deltas = [(h << 2) | (i + 1 & 3) for i, h in enumerate(hs)]
            ones = np.cumsum([h + 1 for h in hs]) - 1
            assert at in ones and max(deltas) <= 65535
            line, _ = split_line(16, 8, 2, 40000, deltas)
            out.append((line, samples_of(40000, deltas, 16), at))
    return out


def limit_lines():
    """-> [(n, J, bytes, samples, status)]: a line whose last code ends on its last bit (8 bits, J = 8, k = 0, seven codes
    of value 2: 32 bits, no padding); a split-sample value at the limit h == xmax >> k (n = 12, k = 2, h = 1023: valid);
    h one beyond it (a fault, the line all zero)."""
    line, bits = split_line(8, 8, 0, 0x55, [2] * 7, pad=False)
    assert bits == 32 and len(line) == 4 and line[-1] & 1
    out = [(8, 8, line, samples_of(0x55, [2] * 7, 8), 0)]
    for h, status in ((1023, 0), (1024, 1)):
        deltas = [5, (h << 2) | 3, 0, 9, 1, 0, 2]
        line, _ = split_line(12, 8, 2, 100, deltas)
        out.append((12, 8, line, samples_of(100, deltas, 12) if status == 0 else np.zeros(8, np.int64), status))
    return out


SE_BETAS = (1, 2, 63, 64, 1000, 2895, 2896, 4094)


def se_long_lines():
    """Second-extension blocks (n = 16, J = 8) with the codes 0, g, 3, 0 behind the reference, g = T(beta) -- the pair
    (beta, 0) -- and T(beta) + beta -- the pair (0, beta) --, T(beta) = beta (beta + 1) / 2: from beta = 2896 on
    8 g + 1 is beyond 2^24 and a float32 root of it is only a start -> [(bytes, samples, g)].  The longest line,
    beta = 4094, has 1 048 324 bytes."""
    out = []
    for beta in SE_BETAS:
        t = beta * (beta + 1) // 2
        for g, pair in ((t, (beta, 0)), (t + beta, (0, beta))):
            deltas = [0, pair[0], pair[1], 2, 0, 0, 0]                 # (the first code's own first half stands in for the reference)
            out.append((se_line(16, 8, 12345, [0, g, 3, 0]), samples_of(12345, deltas, 16), g))
    return out


MAX_LINE = 1 << 20                # bytes: the device refuses longer lines (status 2, all zero)

LIBAEC_LINES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rice_libaec_lines.npz")


def libaec_groups():
    """The lines of tests/golden/rice_libaec_lines.npz, encoded by libaec 1.0.4 (source 0) and by its libsz under option
    mask 49 (source 1), not by `encode` (tests/golden/make_rice_golden.py) -> [(n, J, S, source, [bytes], samples
    (lines, S) uint16)]."""
    with np.load(LIBAEC_LINES) as z:
        a = {k: z[k] for k in z.files}
    data, off, out, at = a["data"].tobytes(), a["offsets"], [], 0
    for g in range(len(a["n"])):
        n, J, S, lo, hi = int(a["n"][g]), int(a["J"][g]), int(a["S"][g]), int(a["first"][g]), int(a["first"][g + 1])
        lines = [data[int(off[i]):int(off[i + 1])] for i in range(lo, hi)]
        out.append((n, J, S, int(a["source"][g]), lines, a["samples"][at:at + (hi - lo) * S].reshape(hi - lo, S)))
        at += (hi - lo) * S
    assert at == len(a["samples"]) and int(off[-1]) == len(data)
    return out


def pack(lines):
    """(bytes uint8, descriptors (n,) of {offset u64, length u32, pad u32}): a batch as the device takes it."""
    desc = np.zeros(len(lines), np.dtype([("offset", np.uint64), ("length", np.uint32), ("pad", np.uint32)]))
    off = 0
    for i, ln in enumerate(lines):
        desc[i] = (off, len(ln), 0)
        off += len(ln)
    return np.frombuffer(b"".join(lines), np.uint8), desc
