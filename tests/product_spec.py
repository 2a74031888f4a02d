"""The product stage's specification in NumPy (include/xritdemod_amd.h, "Image products"): what
xrit_product_* computes from an image of 1 .. 16 bit samples -- histogram, tone table, toned image, thumbnail, composite.
Integer arithmetic throughout; the device equals every array and every summary field exactly.  An image here is a 2-D
array of samples (uint8 for bits <= 8, uint16 above): pitch and padding are the device interface's business."""
import numpy as np

LINEAR, TABLE, EQUALISE, STRETCH = 0, 1, 2, 3
TONES = {"linear": LINEAR, "table": TABLE, "equalise": EQUALISE, "stretch": STRETCH}
MAX_FACTOR = 64
SUMMARY_FIELDS = ("total", "zeros", "out_of_range", "min_nz", "max_nz", "lo", "hi", "fallback", "tone", "tone_columns", "tone_rows",
                  "small_columns", "small_rows")


def width_of(bits):
    return 1 if bits <= 8 else 2


def clamped(img, bits):
    """The samples as the stage takes them: above 2^bits - 1 is 2^bits - 1."""
    return np.minimum(np.asarray(img).astype(np.int64), (1 << bits) - 1)


def histogram(img, bits):
    """-> (hist uint32 [2^bits], dict total zeros out_of_range min_nz max_nz)."""
    img = np.asarray(img)
    assert img.ndim == 2 and img.size >= 1 and 1 <= bits <= 16
    hist = np.bincount(clamped(img, bits).reshape(-1), minlength=1 << bits).astype(np.uint32)
    nz = np.flatnonzero(hist[1:]) + 1
    return hist, dict(total=int(img.size), zeros=int(hist[0]), out_of_range=int((img.astype(np.int64) > (1 << bits) - 1).sum()),
                      min_nz=int(nz[0]) if len(nz) else 0, max_nz=int(nz[-1]) if len(nz) else 0)


def linear_lut(bits):
    v = np.arange(1 << bits, dtype=np.int64)
    return (v >> (bits - 8) if bits >= 8 else v << (8 - bits)).astype(np.uint8)


def build_lut(hist, bits, tone, p_lo=0, p_hi=10000, table=None):
    """-> (lut uint8 [2^bits], dict lo hi fallback)."""
    hist = np.asarray(hist).astype(np.int64)
    assert len(hist) == 1 << bits
    c = np.cumsum(hist) - hist[0]                   # c[v] = hist[1] + .. + hist[v]; c[0] = 0
    n = int(c[-1])
    v = np.arange(1 << bits, dtype=np.int64)
    info = dict(lo=0, hi=0, fallback=0)
    if tone == LINEAR:
        return linear_lut(bits), info
    if tone == TABLE:
        table = np.asarray(table, np.uint8)
        assert table.shape == (1 << bits,)
        return table.copy(), info
    if tone == EQUALISE:
        nz = np.flatnonzero(hist[1:]) + 1
        cmin = int(c[nz[0]]) if len(nz) else 0
        d = n - cmin
        if d == 0:
            info["fallback"] = 1
            return linear_lut(bits), info
        lut = np.where(v < nz[0], 1, 1 + (254 * (c - cmin) + d // 2) // d)
        lut[0] = 0
        return lut.astype(np.uint8), info
    assert tone == STRETCH and 0 <= p_lo < p_hi <= 10000
    if n == 0:
        info["fallback"] = 1
        return linear_lut(bits), info
    lo = int(np.flatnonzero((v >= 1) & (c > 0) & (10000 * c >= p_lo * n))[0])
    hi = int(np.flatnonzero((v >= 1) & (10000 * c >= p_hi * n))[0])
    if hi <= lo:
        info["fallback"] = 1
        return linear_lut(bits), info
    lut = np.where(v <= lo, 1, np.where(v >= hi, 255, 1 + (254 * (v - lo) + (hi - lo) // 2) // (hi - lo)))
    lut[0] = 0
    info.update(lo=lo, hi=hi)
    return lut.astype(np.uint8), info


def tone(img, bits, lut):
    """-> uint8 (rows, columns): lut[v]."""
    return np.asarray(lut, np.uint8)[clamped(img, bits)]


def small_shape(rows, columns, f):
    return ((rows + f - 1) // f, (columns + f - 1) // f) if f else (0, 0)


def thumbnail(img, bits, lut, f):
    """-> uint8 (ceil(rows / f), ceil(columns / f)): per f x f block, over its part inside the image, the rounded mean of
    lut[v] over the pixels with v != 0; 0 where there is none."""
    img = np.asarray(img)
    assert 1 <= f <= MAX_FACTOR
    rows, columns = img.shape
    sr, sc = small_shape(rows, columns, f)
    t = np.zeros((sr * f, sc * f), np.int64)
    m = np.zeros((sr * f, sc * f), np.int64)
    t[:rows, :columns] = tone(img, bits, lut)
    m[:rows, :columns] = img != 0
    cnt = m.reshape(sr, f, sc, f).sum(axis=(1, 3))
    s = (t * m).reshape(sr, f, sc, f).sum(axis=(1, 3))
    return np.where(cnt == 0, 0, (2 * s + cnt) // np.maximum(2 * cnt, 1)).astype(np.uint8)


def composite(a, b, table):
    """-> uint8 (rows, columns, 3): table[(a * 256 + b) * 3 + k]."""
    a, b, table = np.asarray(a, np.uint8), np.asarray(b, np.uint8), np.asarray(table, np.uint8).reshape(-1)
    assert a.shape == b.shape and a.ndim == 2 and len(table) == 256 * 256 * 3
    return table.reshape(65536, 3)[a.astype(np.int64) * 256 + b]


def process(img, bits, tone_mode, p_lo=0, p_hi=10000, factor=0, table=None):
    """One call -> dict hist lut tone small (None for factor 0) summary (a dict of SUMMARY_FIELDS)."""
    img = np.asarray(img)
    hist, summ = histogram(img, bits)
    lut, info = build_lut(hist, bits, tone_mode, p_lo, p_hi, table)
    summ.update(info)
    sr, sc = small_shape(img.shape[0], img.shape[1], factor)
    summ.update(tone=tone_mode, tone_columns=img.shape[1], tone_rows=img.shape[0], small_columns=sc, small_rows=sr)
    return dict(hist=hist, lut=lut, tone=tone(img, bits, lut), small=thumbnail(img, bits, lut, factor) if factor else None, summary=summ)


# ---- the table the host check replays (tests/golden/product_rule_table.txt) ----------------------------------------------
def scan_of(hist, bits, tone_mode, p_lo, p_hi):
    """What the device's scan hands to the rule: N, min_nz, max_nz, cmin and STRETCH's lo and hi as found (0 without)."""
    hist = np.asarray(hist).astype(np.int64)
    c = np.cumsum(hist) - hist[0]
    n = int(c[-1])
    nz = np.flatnonzero(hist[1:]) + 1
    min_nz, max_nz = (int(nz[0]), int(nz[-1])) if len(nz) else (0, 0)
    lo = hi = 0
    if tone_mode == STRETCH and n:
        v = np.arange(len(hist))
        lo = int(np.flatnonzero((v >= 1) & (c > 0) & (10000 * c >= p_lo * n))[0])
        hi = int(np.flatnonzero((v >= 1) & (10000 * c >= p_hi * n))[0])
    return n, min_nz, max_nz, int(c[min_nz]), lo, hi, c


def rule_rows(rng):
    """Rows of 12 integers.  Kind 0, a decision: 0 tone bits N min_nz max_nz cmin lo hi | the tone in effect, fallback, 0.
    Kind 1, an entry under the last decision: 1 v c[v] table's entry | lut[v], then zeros.  Kind 2, a thumbnail byte:
    2 sum cnt | byte.  Kind 3, a percentile test: 3 c p N | reaches, is_lo.  Kind 4: 4 bits v maxv | linear, clamp."""
    rows = []
    pad = lambda r: r + [0] * (12 - len(r))
    hists = []
    for bits in (1, 5, 8, 10, 13, 16):
        nb = 1 << bits
        h = np.zeros(nb, np.int64)
        k = min(nb, 40)
        h[rng.choice(nb, k, replace=False)] = rng.integers(1, 1 << 20, k)
        hists.append((bits, h))
        one = np.zeros(nb, np.int64)
        one[nb - 1] = 77
        hists.append((bits, one))
        z = np.zeros(nb, np.int64)
        z[0] = 9
        hists.append((bits, z))
        if nb > 2:
            two = np.zeros(nb, np.int64)
            two[1] = 1 if bits == 16 else 3
            two[nb - 2] = (1 << 31) - 1 if bits == 16 else 5
            hists.append((bits, two))
    for bits, h in hists:
        for tone_mode, p_lo, p_hi in ((LINEAR, 0, 0), (TABLE, 0, 0), (EQUALISE, 0, 0), (STRETCH, 0, 10000), (STRETCH, 200, 9800),
                                      (STRETCH, 9999, 10000)):
            table = rng.integers(0, 256, len(h), dtype=np.uint8)
            lut, info = build_lut(h, bits, tone_mode, p_lo, p_hi, table)
            n, min_nz, max_nz, cmin, lo, hi, c = scan_of(h, bits, tone_mode, p_lo, p_hi)
            eff = LINEAR if info["fallback"] else tone_mode
            rows.append(pad([0, tone_mode, bits, n, min_nz, max_nz, cmin, lo, hi, eff, info["fallback"]]))
            picks = {0, 1, len(h) - 1, min_nz, max_nz, lo, hi, max(lo - 1, 0), min(hi + 1, len(h) - 1), (lo + hi) // 2}
            picks |= {int(x) for x in rng.integers(0, len(h), 6)}
            for v in sorted(picks):
                rows.append(pad([1, v, int(c[v]), int(table[v]), int(lut[v])]))
    for s, cnt in [(0, 0), (0, 1), (255, 1), (4096 * 255, 4096), (1, 2), (3, 2), (1, 3), (2, 3)] + \
            [(int(rng.integers(0, 255 * k + 1)), int(k)) for k in rng.integers(1, 4097, 40)]:
        byte = 0 if cnt == 0 else (2 * s + cnt) // (2 * cnt)
        rows.append(pad([2, s, cnt, byte]))
    for _ in range(40):
        n = int(rng.integers(1, (1 << 31) + 1))
        cc = int(rng.integers(0, n + 1))
        p = int(rng.integers(0, 10001))
        rows.append(pad([3, cc, p, n, int(10000 * cc >= p * n), int(cc > 0 and 10000 * cc >= p * n)]))
    rows.append(pad([3, 1 << 31, 10000, 1 << 31, 1, 1]))
    rows.append(pad([3, 0, 0, 5, 1, 0]))
    for bits in range(1, 17):
        maxv = (1 << bits) - 1
        for v in (0, 1, maxv, maxv + 1, 65535):
            vc = min(v, maxv)
            rows.append(pad([4, bits, v, maxv, int(linear_lut(bits)[vc]), vc]))
    return rows


def rule_table_text():
    return "\n".join(" ".join(str(x) for x in r) for r in rule_rows(np.random.default_rng(23))) + "\n"


if __name__ == "__main__":
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "product_rule_table.txt"), "w") as f:
        f.write(rule_table_text())
