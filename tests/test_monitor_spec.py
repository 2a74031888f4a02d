"""CPU tier: the specification of the link monitor (tests/monitor_spec.py) against a brute-force loop, a stream against its
pieces, `derive` against values worked out by hand, the estimators' accuracy on AWGN and behind the oracle chain, and the
CPU side of the stage's ABI -- the header declares the functions, the ctypes layer binds them, the record layouts are the
header's field for field, bad arguments are refused before a device is asked for, xrit_monitor_derive and xrit_monitor_rows
never touch a device; the plain host parts (csrc/monitor_host.h) in a stand-alone program under the sanitizers, held against
a table recorded from the specification.

Accuracy, measured (esn0_m2m4_db minus the channel's Es/N0, blocks of 16384 symbols):
  +-1 BPSK in AWGN, 256 seeds per case (the test runs the first 64), worst |deviation| / mean / standard deviation in dB:
      0 dB: 0.4107 / +0.009 / 0.110      2 dB: 0.2439 / -0.005 / 0.090      4 dB: 0.2321 / +0.002 / 0.071
      8 dB: 0.1522 / -0.000 / 0.055     12 dB: 0.1550 / -0.002 / 0.053
    the bounds are 1.5 times the worst: 0.616, 0.366, 0.348, 0.228, 0.233 dB.
    (esn0_snv_db reads high at low Es/N0, by +1.43 / +0.64 / +0.21 dB at 0 / 2 / 4 dB: |q| folds the noise; within 0.01 dB from 8 dB)
  tests/synth.py bursts of 8 blocks through oracle.Demod (LRIT, 1.25 Msps), block 0 .. 7:
      4 dB:   3.402  3.953  4.071  3.888  4.119  4.088  3.946  4.027
      8 dB:   7.229  7.978  8.042  7.948  8.086  8.080  7.954  8.016
     12 dB:  10.844 11.991 12.026 11.971 12.063 12.078 11.956 12.013
     clean:  18.265 33.207 33.127 33.276 33.223 33.256 33.182 33.149
     8 dB at +23 kHz: 1.451 1.680 1.679 1.565 1.581 1.651 1.788 1.663
    blocks 1 .. 6 lie within 0.119 dB of the channel's value; the margin is 1.5 times that, 0.18 dB."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import monitor_spec as sp
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")
TABLE = os.path.join(ROOT, "tests", "golden", "monitor_host_table.txt")

FUNCTIONS = ["xrit_monitor_create", "xrit_monitor_destroy", "xrit_monitor_reset", "xrit_monitor_rows", "xrit_monitor_push_device",
             "xrit_monitor_push", "xrit_monitor_get_state", "xrit_monitor_derive"]
AWGN_BOUND_DB = {0: 0.616, 2: 0.366, 4: 0.348, 8: 0.228, 12: 0.233}       # 1.5 x the worst of 256 seeds (above)
CHAIN_MARGIN_DB = 0.18                                                    # 1.5 x 0.119 (above)


def same(a, b):
    return np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8))


# ---- the specification against a loop that knows nothing of blocks' sums -----------------------------------------------------------
def brute_force(x, symbol_type, block):
    """Every block's record from per-symbol Python integers, the stream taken whole."""
    q = []
    for v in np.asarray(x).tolist():
        if symbol_type == sp.I8:
            q.append((4 * int(v), int(v) in (127, -128), False, False))
            continue
        v = float(np.float32(v))
        if v != v:
            q.append((0, False, False, True))
            continue
        r = v * 512.0                               # exact in float64 as well
        if math.isinf(r):
            r = math.copysign(1e9, r)
        k = math.floor(r)                           # round half to even by hand
        frac = r - k
        k = k + 1 if frac > 0.5 or (frac == 0.5 and k % 2 == 1) else k
        c = max(-4095, min(4095, k))
        q.append((c, abs(c) > 512, abs(k) > 4095, False))
    rows = []
    for b in range(len(q) // block):
        part = q[b * block:(b + 1) * block]
        flips = sum(1 for i in range(b * block, (b + 1) * block) if i and (q[i][0] < 0) != (q[i - 1][0] < 0))
        rows.append((b * block, block, flips, sum(abs(p[0]) for p in part), sum(p[0] ** 2 for p in part), sum(p[0] ** 4 for p in part),
                     sum(p[0] for p in part), sum(p[1] for p in part), sum(p[2] for p in part), sum(p[3] for p in part),
                     sum(p[0] < 0 for p in part)))
    hist = [0] * 256
    for p in q:
        hist[(p[0] + 4096) >> 5] += 1
    return np.array(rows, sp.BLOCK_DTYPE) if rows else np.zeros(0, sp.BLOCK_DTYPE), hist


def constructed():
    tiny = np.array([1], np.uint32).view(np.float32)[0]
    v = [np.nan, np.inf, -np.inf, 0.0, -0.0, 4095 / 512, -4095 / 512, 4095.5 / 512, -4095.5 / 512, 8.0, -8.0, tiny, -tiny, 1.0, -1.0,
         513 / 512, -513 / 512, 3.4e38, -3.4e38, 4094.5 / 512, -4094.5 / 512]
    for k in (0, 1, 2, 3, 510, 511, 512, 4093, 4094):
        v += [(k + 0.5) / 512, -(k + 0.5) / 512]
    return np.array(v, np.float32)


def random_stream(symbol_type, n, seed=3):
    rng = np.random.default_rng(seed)
    x = (np.where(rng.random(n) < 0.5, -0.4, 0.4) + rng.normal(0.0, 0.3, n)).astype(np.float32)
    x[rng.integers(0, n, max(1, n // 50))] *= np.float32(25.0)
    return np.clip(x * 127.0, -128, 127).astype(np.int8) if symbol_type == sp.I8 else x


@pytest.mark.parametrize("symbol_type", (sp.F32, sp.I8))
def test_specification_against_a_per_symbol_loop(symbol_type):
    streams = [random_stream(symbol_type, 1000)]
    if symbol_type == sp.F32:
        c = constructed()
        streams.append(np.concatenate([c, c[::-1], random_stream(sp.F32, 200), c]))
    else:
        streams.append(np.concatenate([np.full(70, -128, np.int8), np.full(70, 127, np.int8), np.arange(-128, 128).astype(np.int8)]))
    for x in streams:
        for block in (64, 128):
            want, hist = brute_force(x, symbol_type, block)
            slow, fast = sp.Monitor(block, symbol_type), sp.Monitor(block, symbol_type)
            rows, summary = slow.push(x)
            rows_fast, summary_fast = sp.push_fast(fast, x)
            assert len(rows) == len(x) // block and same(rows, want) and same(rows_fast, want)
            assert same(summary, summary_fast) and same(slow.state(), fast.state())
            st = slow.state()
            assert st["hist"].tolist() == hist and int(st["open"]["n"]) == len(x) % block == int(summary["open_n"])
            assert int(st["symbols_total"]) == len(x) and int(st["blocks_total"]) == len(rows) == int(summary["rows"]) and int(st["calls"]) == 1
            assert int(st["open"]["first"]) == len(rows) * block


def test_lattice_by_hand():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 4095.5, -4095.5, 4094.5, 513, 512, -513], np.float32) / np.float32(512)
    q, sat, clamped, bad = sp.lattice(x, sp.F32)
    assert q.tolist() == [0, 2, 2, 0, -2, 4095, -4095, 4094, 513, 512, -513]
    assert sat.tolist() == [False] * 5 + [True, True, True, True, False, True]
    assert clamped.tolist() == [False] * 5 + [True, True] + [False] * 4 and not bad.any()
    q, sat, clamped, bad = sp.lattice(np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), sp.F32)
    assert q.tolist() == [0, 4095, -4095, 0] and bad.tolist() == [True, False, False, False] and clamped.tolist() == [False, True, True, False]
    q, sat, clamped, bad = sp.lattice(np.array([127, -128, 126, -127, 0], np.int8), sp.I8)
    assert q.tolist() == [508, -512, 504, -508, 0] and sat.tolist() == [True, True, False, False, False] and not clamped.any() and not bad.any()
    assert 4095 ** 4 * sp.MAX_BLOCK < 2 ** 63


@pytest.mark.parametrize("symbol_type", (sp.F32, sp.I8))
def test_a_stream_is_its_pieces(symbol_type):
    x = random_stream(symbol_type, 3000, seed=5)
    rng = np.random.default_rng(7)
    for block in (64, 192):
        whole = sp.Monitor(block, symbol_type)
        rows_whole, _ = whole.push(x)
        for style in (sp.Monitor.push, sp.push_fast):
            cuts = np.sort(np.concatenate([rng.integers(0, len(x), 17), [0, 0, 64, 64, 65, len(x), len(x)]]))
            cut = sp.Monitor(block, symbol_type)
            got = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                assert cut.rows(hi - lo) == (int(cut.state()["open"]["n"]) + hi - lo) // block
                rows, summary = style(cut, x[lo:hi])
                assert int(summary["rows"]) == len(rows) and int(summary["symbols_total"]) == hi
                got.append(rows)
            assert same(np.concatenate(got), rows_whole)
            a, b = whole.state(), cut.state()
            assert int(b["calls"]) == len(cuts) - 1
            b["calls"] = a["calls"]
            assert same(a, b)
    with pytest.raises(ValueError):
        sp.Monitor(96 + 1)
    with pytest.raises(ValueError):
        sp.Monitor(32768 + 64)
    with pytest.raises(ValueError):
        sp.Monitor(64, 2)


# ---- derive -----------------------------------------------------------------------------------------------------------------------------
def record(**kw):
    r = np.zeros(1, sp.BLOCK_DTYPE)[0]
    for k, v in kw.items():
        r[k] = v
    return r


def test_derive_by_hand():
    # 64 symbols: 48 at |q| = 200 and 16 at |q| = 300, 24 negative ones among the first
    n, s1, s2, s4 = 64, 48 * 200 + 16 * 300, 48 * 200 ** 2 + 16 * 300 ** 2, 48 * 200 ** 4 + 16 * 300 ** 4
    q = sp.derive(record(n=n, s1=s1, s2=s2, s4=s4, sum=s1 - 2 * 24 * 200, flips=20, sat=0, neg=24), sp.F32)
    m1, m2, m4 = 225.0, 3360000 / 64, 206400000000 / 64
    assert s1 == 14400 and s2 == 3360000 and s4 == 206400000000
    assert q["level"] == pytest.approx(math.sqrt(52500.0) / 512, rel=1e-14) and q["dc"] == pytest.approx(4800 / (512 * 64), rel=1e-14)
    assert q["flip_rate"] == 20 / 64 and q["sat_rate"] == 0 and q["neg_rate"] == 24 / 64 and q["flags"] == 0
    assert q["esn0_snv_db"] == pytest.approx(10 * math.log10(m1 ** 2 / (2 * (m2 - m1 ** 2))), rel=1e-12)
    S = math.sqrt((3 * m2 ** 2 - m4) / 2)
    assert q["esn0_m2m4_db"] == pytest.approx(10 * math.log10(S / (2 * (m2 - S))), rel=1e-12)
    assert S == pytest.approx(50218.27, abs=0.01) and q["esn0_m2m4_db"] == pytest.approx(10.416, abs=1e-3)         # S / (2 N) = 50218.27 / (2 * 2281.73)
    # the same sums as int8 symbols: the level scale is 508
    q8 = sp.derive(record(n=n, s1=s1, s2=s2, s4=s4, sum=4800), sp.I8)
    assert q8["level"] == pytest.approx(q["level"] * 512 / 508, rel=1e-14) and q8["dc"] == pytest.approx(4800 / (508 * 64), rel=1e-14)
    assert q8["esn0_m2m4_db"] == q["esn0_m2m4_db"]
    # every |q| the same: no noise, +99 for both; the flag comes from integers (n s4 = s2^2), not from a float difference
    for a in (1, 3, 205, 4095):
        for n in (1, 7, 64, 32768):
            q = sp.derive(record(n=n, s1=a * n, s2=a * a * n, s4=a ** 4 * n, sum=a * n), sp.F32)
            assert q["flags"] == sp.NO_NOISE and q["esn0_m2m4_db"] == 99.0 and q["esn0_snv_db"] == 99.0
    # all zeros: no signal, -99 for both
    q = sp.derive(record(n=64), sp.F32)
    assert q["flags"] == sp.NO_SIGNAL and q["esn0_m2m4_db"] == -99.0 and q["esn0_snv_db"] == -99.0 and q["level"] == 0.0
    # a kurtosis of 3 and more (3 s2^2 <= n s4): no signal in the moments, the other estimator still reads
    q = sp.derive(record(n=4, s1=10, s2=100, s4=10000, sum=10), sp.F32)                   # one symbol at 10, three at 0
    assert q["flags"] == sp.NO_SIGNAL and q["esn0_m2m4_db"] == -99.0 and q["esn0_snv_db"] == pytest.approx(10 * math.log10(100 / (2 * 300)), rel=1e-12)
    # refused
    for bad in (record(n=0), record(n=32769, s1=1, s2=1, s4=1), record(n=1, s1=4096, s2=4096 ** 2, s4=4096 ** 4), record(n=2, s1=2, s2=2, s4=2, sum=3),
                record(n=2, s1=2, s2=2, s4=2, sum=-3), record(n=1, s1=1, s2=4095 ** 2 + 1, s4=1)):
        assert sp.derive(bad, sp.F32) is None
    assert sp.derive(record(n=1, s1=1, s2=1, s4=1), 2) is None


def awgn(db, seed, n=16384):
    rng = np.random.default_rng(1000 * int(db) + seed)
    sigma = math.sqrt(1.0 / (2.0 * 10 ** (db / 10)))
    return (np.where(rng.random(n) < 0.5, -1.0, 1.0) + rng.normal(0, sigma, n)).astype(np.float32)


@pytest.mark.parametrize("db", sorted(AWGN_BOUND_DB))
def test_accuracy_on_awgn(db):
    dev = []
    for seed in range(64):
        rows, _ = sp.push_fast(sp.Monitor(16384), awgn(db, seed))
        q = sp.derive(rows[0], sp.F32)
        assert q["flags"] == 0
        dev.append(float(q["esn0_m2m4_db"]) - db)
    worst = max(abs(v) for v in dev)
    print(f"Es/N0 {db} dB: worst |deviation| {worst:.4f} dB over 64 seeds, mean {np.mean(dev):+.4f}, std {np.std(dev):.4f}; bound {AWGN_BOUND_DB[db]}")
    assert worst <= AWGN_BOUND_DB[db]


# ---- behind the oracle chain -----------------------------------------------------------------------------------------------------------------
_CHAIN = {}


def chain_blocks(oracle_mod, **kw):
    """esn0_m2m4_db of the 8 blocks of a burst through the oracle chain (LRIT, 1.25 Msps), computed once per burst."""
    key = tuple(sorted(kw.items()))
    if key not in _CHAIN:
        x = synth.generate(synth.SynthParams(fs_in=1.25e6, **kw), 570000)
        soft = oracle_mod.Demod(oracle_mod.config("lrit", 1.25e6, 1)).process(x)
        rows, _ = sp.push_fast(sp.Monitor(16384), soft)
        assert len(rows) == 8 and not rows["clamped"].any() and not rows["bad"].any()
        _CHAIN[key] = [float(sp.derive(r, sp.F32)["esn0_m2m4_db"]) for r in rows]
    return _CHAIN[key]


@pytest.mark.parametrize("db", (4.0, 8.0, 12.0))
def test_accuracy_behind_the_oracle_chain(oracle_mod, db):
    v = chain_blocks(oracle_mod, esn0_db=db)
    print(f"Es/N0 {db} dB through the chain:", " ".join(f"{a:.3f}" for a in v), f"(margin {CHAIN_MARGIN_DB})")
    assert all(abs(a - db) <= CHAIN_MARGIN_DB for a in v[1:7])
    assert v[0] < v[1]                              # the loops are still acquiring in block 0


def test_the_chain_s_ceiling_and_an_untuned_carrier(oracle_mod):
    clean = chain_blocks(oracle_mod, esn0_db=None)
    print("noiseless:", " ".join(f"{a:.3f}" for a in clean))
    assert all(a > 25.0 for a in clean[1:])
    off = chain_blocks(oracle_mod, esn0_db=8.0, carrier_hz=23000.0)
    tuned = chain_blocks(oracle_mod, esn0_db=8.0)
    print("8 dB at +23 kHz:", " ".join(f"{a:.3f}" for a in off), "| tuned:", " ".join(f"{a:.3f}" for a in tuned))
    assert all(a < 3.0 for a in off) and min(tuned[1:7]) > 7.0


# ---- the ABI on the CPU ------------------------------------------------------------------------------------------------------------------------
CTYPES = {"uint64_t": np.uint64, "int64_t": np.int64, "uint32_t": np.uint32, "double": np.float64}


def header_struct(text, name, known):
    """The fields of a struct of the header as a dtype, and the size its comment states."""
    m = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + r";\s*/\* (\d+) bytes", text, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        dt = CTYPES.get(ctype) or known[ctype]
        for nm in names.split(","):
            arr = re.match(r"\s*(\w+)\[(\d+)\]", nm)
            fields.append((arr.group(1), dt, (int(arr.group(2)),)) if arr else (nm.strip(), dt))
    return np.dtype(fields), int(m.group(2))


def test_symbols_and_layouts():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(xrit_[a-z0-9_]+)\s*\(", src))
    import xritdemod_amd as xa
    from xritdemod_amd import _capi
    L = xa.lib()
    for name in FUNCTIONS:
        assert name in declared and name in _capi._SIGNATURES and hasattr(L, name), name
    known = {}
    for struct, dtype, spec, size in (("xrit_monitor_block", xa.MONITOR_BLOCK_DTYPE, sp.BLOCK_DTYPE, 64),
                                      ("xrit_monitor_summary", xa.MONITOR_SUMMARY_DTYPE, sp.SUMMARY_DTYPE, 32),
                                      ("xrit_monitor_state", xa.MONITOR_STATE_DTYPE, sp.STATE_DTYPE, 2144),
                                      ("xrit_monitor_quality", xa.MONITOR_QUALITY_DTYPE, sp.QUALITY_DTYPE, 64)):
        want, stated = header_struct(text, struct, known)
        known[struct] = want
        assert stated == size == dtype.itemsize == want.itemsize and dtype == want == spec, struct
    for name, value in (("XRIT_SYMBOL_F32", sp.F32), ("XRIT_SYMBOL_I8", sp.I8), ("XRIT_MONITOR_NO_SIGNAL", sp.NO_SIGNAL), ("XRIT_MONITOR_NO_NOISE", sp.NO_NOISE)):
        assert re.search(r"#define " + name + r"\s+" + str(value) + r"\b", text), name
    assert (xa.SYMBOL_F32, xa.SYMBOL_I8, xa.MONITOR_NO_SIGNAL, xa.MONITOR_NO_NOISE) == (sp.F32, sp.I8, sp.NO_SIGNAL, sp.NO_NOISE)
    assert "NO LOCK FLAG" in text and "1.5 .. 2.5 dB" in text and "clamp(rintf(x * 512.0f), -4095, 4095)" in text


def test_derive_and_rows_through_the_abi_need_no_device():
    import xritdemod_amd as xa
    L = xa.lib()
    rng = np.random.default_rng(11)
    records = [record(n=64, s1=14400, s2=3360000, s4=206400000000, sum=4800, flips=20, neg=24), record(n=64), record(n=7, s1=21, s2=63, s4=567, sum=-21),
               record(n=4, s1=10, s2=100, s4=10000, sum=10)]
    for db in (0, 4, 12):
        for symbol_type in (sp.F32, sp.I8):
            x = awgn(db, 1) * np.float32(0.4)
            records.append(sp.push_fast(sp.Monitor(16384, symbol_type), x if symbol_type == sp.F32 else np.clip(x * 127, -128, 127).astype(np.int8))[0][0])
    records.append(sp.push_fast(sp.Monitor(64), rng.normal(0, 0.3, 64).astype(np.float32))[0][0])
    for symbol_type in (sp.F32, sp.I8):
        for r in records:
            want, got = sp.derive(r, symbol_type), xa.LinkMonitor.derive(r, symbol_type)
            assert got["flags"] == want["flags"] and got["reserved"] == 0
            for name in ("level", "dc", "flip_rate", "sat_rate", "neg_rate", "esn0_snv_db", "esn0_m2m4_db"):
                assert got[name] == pytest.approx(want[name], rel=1e-12, abs=0), name
    out = np.zeros(1, xa.MONITOR_QUALITY_DTYPE)
    p = out.ctypes.data_as(C.c_void_p)
    for bad in (record(n=0), record(n=32769, s1=1, s2=1, s4=1), record(n=1, s1=4096, s2=4096 ** 2, s4=4096 ** 4)):
        b = np.array([bad], xa.MONITOR_BLOCK_DTYPE)
        assert L.xrit_monitor_derive(b.ctypes.data_as(C.c_void_p), 0, p) == -1
    good = np.array([records[0]], xa.MONITOR_BLOCK_DTYPE)
    assert L.xrit_monitor_derive(good.ctypes.data_as(C.c_void_p), 2, p) == -1 and L.xrit_monitor_derive(None, 0, p) == -1
    assert L.xrit_monitor_derive(good.ctypes.data_as(C.c_void_p), 0, None) == -1
    with pytest.raises(xa.XritError):
        xa.LinkMonitor.derive(record(n=0))
    assert L.xrit_monitor_rows(None, 0) == 0 and L.xrit_monitor_rows(None, 1 << 20) == 0


def test_bad_arguments_are_refused_before_a_device_is_asked_for():
    import xritdemod_amd as xa
    L = xa.lib()
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert L.xrit_monitor_create(None, 0, 0, 0) == -1
    for block, symbol_type in ((63, 0), (96, 0), (32, 0), (32768 + 64, 0), (1 << 20, 0), (16384, 2), (16384, -1)):
        assert L.xrit_monitor_create(C.byref(h), block, symbol_type, 0) == -1 and not h.value, (block, symbol_type)
    n = C.c_size_t(5)
    assert L.xrit_monitor_reset(None) == -1 and L.xrit_monitor_get_state(None, p) == -1
    assert L.xrit_monitor_push(None, p, 0, p, 0, C.byref(n)) == -1 and n.value == 0
    assert L.xrit_monitor_push_device(None, p, 0, p, 0, None, None) == -1
    assert L.xrit_monitor_destroy(None) == 0


def test_no_cpu_path():
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:                   # on a GPU box the same call makes a working object (-m gpu tests it)
        xa.LinkMonitor().close()
        return
    with pytest.raises(xa.XritError) as ei:
        xa.LinkMonitor()
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


def test_host_program_refuses_what_the_stage_cannot_take():
    host_bin = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
    for extra in (["--monitor", "m.csv", "--gpus", "2"], ["--monitor", "m.csv", "--monitor-block", "100"], ["--monitor", "m.csv", "--monitor-block", "32832"],
                  ["--monitor", "m.csv", "--monitor-block", "0"], ["--monitor"]):
        r = subprocess.run([host_bin, "--input", "x.cf32", "--sink", "null"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "usage:" in r.stderr, extra


# ---- the plain host parts ----------------------------------------------------------------------------------------------------------------------
def recorded_table():
    """What the host check replays, as the specification decides it."""
    rows = []
    for block in (0, 1, 63, 64, 65, 96, 128, 16384, 16385, 32704, 32768, 32769, 32832, 65536):
        rows.append(["B", block, int(sp.block_ok(block))])
    for t, b in ((0, 4), (1, 1), (2, 0), (-1, 0)):
        rows.append(["T", t, b])
    # scripted pushes: the open block's fill carries from one to the next, as the handle keeps it
    for block in (64, 16384, 32768):
        open_n = 0
        for n in (0, 1, 63, 64, 65, block - 1, block, block + 1, 3 * block + 17, 100003, 0, 1 << 24, (1 << 30) - 5, 1 << 30, 7):
            count = sp.piece_count(open_n, n, block)
            first, last = (sp.piece(open_n, n, block, 0), sp.piece(open_n, n, block, count - 1)) if count else ((0, 0), (0, 0))
            rows.append(["G", block, open_n, n, count, sp.rows_for(open_n, n, block), (open_n + n) % block, *first, *last])
            open_n = (open_n + n) % block
    records = [record(n=64, s1=14400, s2=3360000, s4=206400000000, sum=4800, flips=20, neg=24), record(n=64), record(n=7, s1=21, s2=63, s4=567, sum=-21),
               record(n=4, s1=10, s2=100, s4=10000, sum=10), record(n=32768, s1=4095 * 32768, s2=4095 ** 2 * 32768, s4=4095 ** 4 * 32768, sum=-4095 * 32768, sat=32768, neg=32768),
               record(n=1, s1=1, s2=1, s4=1, sum=1), record(n=0), record(n=32769, s1=1, s2=1, s4=1), record(n=1, s1=4096, s2=4096 ** 2, s4=4096 ** 4),
               record(n=2, s1=2, s2=2, s4=2, sum=3), record(n=2, s1=1, s2=4095 ** 2 * 2 + 1, s4=1)]
    for db in (0, 2, 4, 8, 12, 30):
        records.append(sp.push_fast(sp.Monitor(16384), awgn(db, 2) * np.float32(0.4))[0][0])
        records.append(sp.push_fast(sp.Monitor(16384, sp.I8), np.clip(awgn(db, 3) * 0.4 * 127, -128, 127).astype(np.int8))[0][0])
    records.append(sp.push_fast(sp.Monitor(64), np.random.default_rng(5).normal(0, 0.3, 64).astype(np.float32))[0][0])
    for symbol_type in (sp.F32, sp.I8, 2):
        for r in records:
            q = sp.derive(r, symbol_type)
            head = ["D", symbol_type] + [int(r[k]) for k in ("n", "flips", "s1", "s2", "s4", "sum", "sat", "neg")]
            if q is None:
                rows.append(head + [0] + [float(0).hex()] * 7 + [0])
            else:
                rows.append(head + [1] + [float(q[k]).hex() for k in ("level", "dc", "flip_rate", "sat_rate", "neg_rate", "esn0_snv_db", "esn0_m2m4_db")]
                            + [int(q["flags"])])
    return rows


def test_recorded_table_is_the_specification_s():
    want = "\n".join(" ".join(str(x) for x in row) for row in recorded_table()) + "\n"
    assert open(TABLE).read() == want
    kinds = [ln.split()[0] for ln in want.splitlines()]
    assert {k: kinds.count(k) for k in "BTGD"} == {"B": 14, "T": 4, "G": 45, "D": 72}


def test_monitor_host_check_under_sanitizers(tmp_path):
    """make monitor-host-check: the functions of csrc/monitor_host.h that monitor.cpp and the kernels' launch code call, over
    the recorded table in a stand-alone g++ program with -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "monitor-host-check",
                        f"MONITOR_CHECK={tmp_path / 'monitor_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    n = len(open(TABLE).read().splitlines())
    assert f"monitor_host_check: {n} rows, the blocks, the symbol types, the plans and the derived records of each: ok" in r.stdout, r.stdout
