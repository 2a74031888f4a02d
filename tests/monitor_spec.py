"""The serial specification of the link monitor (include/xritdemod_amd.h, "Link monitor"): soft
symbols on an integer lattice, summed block by block.  Everything that is summed is an integer, so the order of the sums
does not matter and the device's rows, summary and state are these, word for word, however a stream is cut into calls.
`derive` turns one block record into level, DC, rates and two Es/N0 estimates in float64; the one subtraction that
cancels (3 s2^2 - n s4) and the two sign tests are taken on Python integers."""
import math

import numpy as np

F32, I8 = 0, 1
MIN_BLOCK, MAX_BLOCK, DEFAULT_BLOCK = 64, 32768, 16384
Q_MAX = 4095
NO_SIGNAL, NO_NOISE = 1, 2

# xrit_monitor_block
BLOCK_DTYPE = np.dtype([("first", np.uint64), ("n", np.uint32), ("flips", np.uint32), ("s1", np.uint64), ("s2", np.uint64), ("s4", np.uint64),
                        ("sum", np.int64), ("sat", np.uint32), ("clamped", np.uint32), ("bad", np.uint32), ("neg", np.uint32)])
# xrit_monitor_summary
SUMMARY_DTYPE = np.dtype([("rows", np.uint64), ("open_n", np.uint64), ("symbols_total", np.uint64), ("blocks_total", np.uint64)])
# xrit_monitor_state
STATE_DTYPE = np.dtype([("open", BLOCK_DTYPE), ("symbols_total", np.uint64), ("blocks_total", np.uint64), ("calls", np.uint64),
                        ("last_neg", np.uint32), ("have_last", np.uint32), ("hist", np.uint64, (256,))])
# xrit_monitor_quality
QUALITY_DTYPE = np.dtype([("level", np.float64), ("dc", np.float64), ("flip_rate", np.float64), ("sat_rate", np.float64), ("neg_rate", np.float64),
                          ("esn0_snv_db", np.float64), ("esn0_m2m4_db", np.float64), ("flags", np.uint32), ("reserved", np.uint32)])
assert BLOCK_DTYPE.itemsize == 64 and SUMMARY_DTYPE.itemsize == 32 and STATE_DTYPE.itemsize == 2144 and QUALITY_DTYPE.itemsize == 64
COUNTS = ("n", "flips", "s1", "s2", "s4", "sum", "sat", "clamped", "bad", "neg")


def block_ok(block):
    return MIN_BLOCK <= block <= MAX_BLOCK and block % 64 == 0


def lattice(symbols, symbol_type):
    """-> (q int64, sat, clamped, bad) of every symbol."""
    if symbol_type == I8:
        s = np.ascontiguousarray(symbols, np.int8).astype(np.int64)
        none = np.zeros(len(s), bool)
        return 4 * s, (s == 127) | (s == -128), none, none
    if symbol_type != F32:
        raise ValueError("monitor: symbol type 0 (float32) or 1 (int8)")
    x = np.ascontiguousarray(symbols, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(x * np.float32(512.0))              # the product is exact (or +-inf); ties go to the even integer
    bad = np.isnan(r)
    clamped = np.abs(r) > np.float32(Q_MAX)                  # +-inf included, NaN not
    q = np.clip(np.where(bad, np.float32(0), r), -Q_MAX, Q_MAX).astype(np.int64)
    return q, np.abs(q) > 512, clamped, bad


def rows_for(open_n, n, block):
    """The blocks that a push of n symbols completes when the open block holds open_n."""
    return (open_n + n) // block


def piece_count(open_n, n, block):
    return (open_n + n + block - 1) // block if n else 0


def piece(open_n, n, block, k):
    """(lo, hi): the call indices of piece k of a push of n symbols behind open_n open ones."""
    return (k * block - open_n if k else 0, min(n, (k + 1) * block - open_n))


def pieces_for(open_n, n, block):
    """The call's symbols cut where the stream's blocks end: none for n = 0.  Piece 0 completes the open block (or is a
    whole block, or all of a short call), the last may be a tail that stays open."""
    return [piece(open_n, n, block, k) for k in range(piece_count(open_n, n, block))]


class Monitor:
    def __init__(self, block=DEFAULT_BLOCK, symbol_type=F32):
        if not block_ok(block) or symbol_type not in (F32, I8):
            raise ValueError("monitor: block a multiple of 64 in 64 .. 32768, symbol type 0 or 1")
        self.block, self.symbol_type = block, symbol_type
        self.reset()

    def reset(self):
        self.st = np.zeros(1, STATE_DTYPE)[0]

    def rows(self, n):
        return rows_for(int(self.st["open"]["n"]), n, self.block)

    def push(self, symbols):
        """-> (the rows this call completes, the summary); one symbol at a time, as the contract words it."""
        q, sat, clamped, bad = lattice(symbols, self.symbol_type)
        st = self.st
        rows = []
        op = {k: int(st["open"][k]) for k in COUNTS}
        have, last = int(st["have_last"]), int(st["last_neg"])
        total, blocks = int(st["symbols_total"]), int(st["blocks_total"])
        hist = [int(v) for v in st["hist"]]
        for i in range(len(q)):
            v = int(q[i])
            neg = int(v < 0)
            op["n"] += 1
            op["flips"] += int(have and neg != last)
            op["s1"] += abs(v)
            op["s2"] += v * v
            op["s4"] += v ** 4
            op["sum"] += v
            op["sat"] += int(sat[i])
            op["clamped"] += int(clamped[i])
            op["bad"] += int(bad[i])
            op["neg"] += neg
            hist[(v + 4096) >> 5] += 1
            have, last = 1, neg
            total += 1
            if op["n"] == self.block:
                row = np.zeros(1, BLOCK_DTYPE)[0]
                row["first"] = blocks * self.block
                for k in COUNTS:
                    row[k] = op[k]
                rows.append(row)
                blocks += 1
                op = dict.fromkeys(COUNTS, 0)
        st["open"]["first"] = blocks * self.block
        for k in COUNTS:
            st["open"][k] = op[k]
        st["have_last"], st["last_neg"] = have, last
        st["symbols_total"], st["blocks_total"] = total, blocks
        st["calls"] += 1
        st["hist"] = hist
        summary = np.zeros(1, SUMMARY_DTYPE)[0]
        summary["rows"], summary["open_n"], summary["symbols_total"], summary["blocks_total"] = len(rows), op["n"], total, blocks
        return (np.array(rows, BLOCK_DTYPE) if rows else np.zeros(0, BLOCK_DTYPE)), summary

    def state(self):
        return self.st.copy()


def push_fast(mon, symbols):
    """Monitor.push with the sums taken by NumPy (uint64 holds every one of them: 4095^4 * 32768 < 2^63): the same words,
    for streams too long for the symbol-by-symbol loop.  tests/test_monitor_spec.py holds the two to each other."""
    q, sat, clamped, bad = lattice(symbols, mon.symbol_type)
    st, B, n = mon.st, mon.block, len(q)
    neg = q < 0
    flip = np.zeros(n, bool)
    if n:
        flip[1:] = neg[1:] != neg[:-1]
        flip[0] = bool(st["have_last"]) and int(neg[0]) != int(st["last_neg"])
    a = np.abs(q).astype(np.uint64)
    cols = {"n": np.ones(n, np.uint64), "flips": flip, "s1": a, "s2": a * a, "s4": a * a * a * a, "sum": q, "sat": sat, "clamped": clamped,
            "bad": bad, "neg": neg}
    o, blocks = int(st["open"]["n"]), int(st["blocks_total"])
    rows = np.zeros((o + n) // B, BLOCK_DTYPE)
    op = st["open"].copy()
    for k, (lo, hi) in enumerate(pieces_for(o, n, B)):
        for name in COUNTS:
            op[name] += cols[name][lo:hi].sum(dtype=np.int64 if name == "sum" else np.uint64)
        if int(op["n"]) == B:
            op["first"] = (blocks + k) * B
            rows[k] = op
            op = np.zeros(1, BLOCK_DTYPE)[0]
    st["hist"] += np.bincount((q + 4096) >> 5, minlength=256).astype(np.uint64)
    if n:
        st["have_last"], st["last_neg"] = 1, int(neg[-1])
    st["symbols_total"] += np.uint64(n)
    st["blocks_total"] += np.uint64(len(rows))
    st["calls"] += np.uint64(1)
    op["first"] = int(st["blocks_total"]) * B
    st["open"] = op
    summary = np.zeros(1, SUMMARY_DTYPE)[0]
    summary["rows"], summary["open_n"], summary["symbols_total"], summary["blocks_total"] = len(rows), op["n"], st["symbols_total"], st["blocks_total"]
    return rows, summary


def derive(b, symbol_type):
    """One block record (anything with the fields of BLOCK_DTYPE) -> a QUALITY_DTYPE scalar; None: the record is refused
    (n = 0, n above 32768, or sums that no n lattice values give)."""
    n, s1, s2, s4, total = int(b["n"]), int(b["s1"]), int(b["s2"]), int(b["s4"]), int(b["sum"])
    if symbol_type not in (F32, I8) or n == 0 or n > MAX_BLOCK or s1 > Q_MAX * n or s2 > Q_MAX ** 2 * n or s4 > Q_MAX ** 4 * n or abs(total) > s1:
        return None
    scale = 512.0 if symbol_type == F32 else 508.0
    out = np.zeros(1, QUALITY_DTYPE)[0]
    m2 = s2 / n
    out["level"] = math.sqrt(m2) / scale
    out["dc"] = total / (scale * n)
    out["flip_rate"], out["sat_rate"], out["neg_rate"] = int(b["flips"]) / n, int(b["sat"]) / n, int(b["neg"]) / n
    flags = 0
    # squared signal to noise variance: m1^2 / (2 (m2 - m1^2)) = s1^2 / (2 (n s2 - s1^2)), the difference an integer
    var = n * s2 - s1 * s1
    if s1 == 0:
        flags |= NO_SIGNAL
        out["esn0_snv_db"] = -99.0
    elif var <= 0:
        flags |= NO_NOISE
        out["esn0_snv_db"] = 99.0
    else:
        out["esn0_snv_db"] = 10.0 * math.log10(float(s1 * s1) / (2.0 * float(var)))
    # second and fourth moments: S = sqrt((3 m2^2 - m4) / 2), N = m2 - S; N <= 0 exactly when n s4 <= s2^2
    d = 3 * s2 * s2 - n * s4
    if d <= 0:
        flags |= NO_SIGNAL
        out["esn0_m2m4_db"] = -99.0
    elif n * s4 <= s2 * s2:
        flags |= NO_NOISE
        out["esn0_m2m4_db"] = 99.0
    else:
        S = math.sqrt(float(d) / 2.0) / n
        N = m2 - S
        if N <= 0.0:                                # float64 rounding at the edge of the integer test
            flags |= NO_NOISE
            out["esn0_m2m4_db"] = 99.0
        else:
            out["esn0_m2m4_db"] = 10.0 * math.log10(S / (2.0 * N))
    out["flags"] = flags
    return out
