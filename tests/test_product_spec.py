"""CPU tier: the product stage's specification (tests/product_spec.py) against brute-force loops on tiny images and against
tone tables worked out by hand; the fallback flag; the CPU side of the ABI (the header declares the functions, the ctypes
layer binds them, the library exports them, the record layouts are the header's, bad arguments are refused before a
device is asked for, there is no CPU path); the rule (csrc/product_rule.h) in a stand-alone program under the sanitizers,
replaying a table recorded from the specification; the host program's checks of the --products flags."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import product_spec as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")
TABLE = os.path.join(ROOT, "tests", "golden", "product_rule_table.txt")
HOST_BIN = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")

FUNCTIONS = ["xrit_product_create", "xrit_product_destroy", "xrit_product_reset", "xrit_product_process_device", "xrit_product_process",
             "xrit_product_process_resident", "xrit_product_composite_device", "xrit_product_composite", "xrit_canvas_pixels_device"]


# ---- brute force ----------------------------------------------------------------------------------------------------------
def brute(img, bits, tone_mode, p_lo, p_hi, f, table):
    """The issue's sentences as Python loops over plain integers."""
    rows, columns = len(img), len(img[0])
    maxv = (1 << bits) - 1
    hist = [0] * (maxv + 1)
    over = 0
    for row in img:
        for v in row:
            over += v > maxv
            hist[min(v, maxv)] += 1
    c = [0] * (maxv + 1)
    for v in range(1, maxv + 1):
        c[v] = c[v - 1] + hist[v]
    n = c[maxv]
    with_count = [v for v in range(1, maxv + 1) if hist[v]]
    min_nz, max_nz = (with_count[0], with_count[-1]) if with_count else (0, 0)
    linear = [v >> (bits - 8) if bits >= 8 else v << (8 - bits) for v in range(maxv + 1)]
    lo = hi = fallback = 0
    if tone_mode == sp.LINEAR:
        lut = linear
    elif tone_mode == sp.TABLE:
        lut = [int(x) for x in table]
    elif tone_mode == sp.EQUALISE:
        cmin = c[min_nz]
        d = n - cmin
        if d == 0:
            lut, fallback = linear, 1
        else:
            lut = [0] + [1 if v < min_nz else 1 + (254 * (c[v] - cmin) + d // 2) // d for v in range(1, maxv + 1)]
    else:
        if n:
            lo = min(v for v in range(1, maxv + 1) if c[v] > 0 and 10000 * c[v] >= p_lo * n)
            hi = min(v for v in range(1, maxv + 1) if 10000 * c[v] >= p_hi * n)
        if n == 0 or hi <= lo:
            lut, fallback, lo, hi = linear, 1, 0, 0
        else:
            lut = [0] + [1 if v <= lo else 255 if v >= hi else 1 + (254 * (v - lo) + (hi - lo) // 2) // (hi - lo) for v in range(1, maxv + 1)]
    toned = [[lut[min(v, maxv)] for v in row] for row in img]
    small = None
    if f:
        small = []
        for y0 in range(0, rows, f):
            out = []
            for x0 in range(0, columns, f):
                cnt = s = 0
                for y in range(y0, min(y0 + f, rows)):
                    for x in range(x0, min(x0 + f, columns)):
                        if img[y][x] != 0:
                            cnt += 1
                            s += toned[y][x]
                out.append(0 if cnt == 0 else (2 * s + cnt) // (2 * cnt))
            small.append(out)
    summary = dict(total=rows * columns, zeros=hist[0], out_of_range=over, min_nz=min_nz, max_nz=max_nz, lo=lo, hi=hi, fallback=fallback,
                   tone=tone_mode, tone_columns=columns, tone_rows=rows, small_columns=len(small[0]) if f else 0,
                   small_rows=len(small) if f else 0)
    return hist, lut, toned, small, summary


CASES = [(1, 1, 1, 8, 1), (2, 7, 5, 8, 3), (3, 9, 11, 10, 4), (4, 5, 6, 1, 2), (5, 6, 7, 5, 64), (6, 4, 9, 13, 0), (7, 3, 3, 16, 2), (8, 8, 8, 12, 8)]


@pytest.mark.parametrize("seed,rows,columns,bits,f", CASES)
@pytest.mark.parametrize("tone_mode,p_lo,p_hi", [(sp.LINEAR, 0, 0), (sp.TABLE, 0, 0), (sp.EQUALISE, 0, 0), (sp.STRETCH, 0, 10000),
                                                 (sp.STRETCH, 1000, 9000), (sp.STRETCH, 9999, 10000)])
def test_specification_against_brute_force(seed, rows, columns, bits, f, tone_mode, p_lo, p_hi):
    rng = np.random.default_rng(seed)
    dtype = np.uint8 if bits <= 8 else np.uint16
    top = min(1 << bits, 24) if seed % 2 else 1 << bits             # few distinct values, or the whole range
    img = rng.integers(0, top, (rows, columns)).astype(dtype)
    img[rng.random((rows, columns)) < 0.3] = 0                      # no data
    if bits in (5, 13):
        img[0, 0] = (1 << bits) + 3                                 # out of range
    table = rng.integers(0, 256, 1 << bits, dtype=np.uint8)
    got = sp.process(img, bits, tone_mode, p_lo, p_hi, f, table)
    hist, lut, toned, small, summary = brute(img.tolist(), bits, tone_mode, p_lo, p_hi, f, table)
    assert got["hist"].dtype == np.uint32 and got["hist"].tolist() == hist
    assert got["lut"].dtype == np.uint8 and got["lut"].tolist() == lut
    assert got["tone"].dtype == np.uint8 and got["tone"].tolist() == toned
    assert (got["small"] is None) == (f == 0) and (f == 0 or (got["small"].dtype == np.uint8 and got["small"].tolist() == small))
    assert got["summary"] == summary and tuple(sorted(summary)) == tuple(sorted(sp.SUMMARY_FIELDS))


def test_composite_against_brute_force():
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 256, (2, 5, 7), dtype=np.uint8)
    table = rng.integers(0, 256, 256 * 256 * 3, dtype=np.uint8)
    got = sp.composite(a, b, table)
    assert got.shape == (5, 7, 3) and got.dtype == np.uint8
    for y in range(5):
        for x in range(7):
            for k in range(3):
                assert got[y, x, k] == table[(int(a[y, x]) * 256 + int(b[y, x])) * 3 + k]


# ---- tone tables by hand -----------------------------------------------------------------------------------------------------
def hist_of(bits, counts):
    h = np.zeros(1 << bits, np.int64)
    for v, n in counts.items():
        h[v] = n
    return h


@pytest.mark.parametrize("bits", [1, 5, 8, 10, 16])
def test_one_distinct_value_falls_back(bits):
    top = (1 << bits) - 1
    for v in {1, top}:
        h = hist_of(bits, {0: 4, v: 9})
        for mode, args in ((sp.EQUALISE, ()), (sp.STRETCH, (0, 10000)), (sp.STRETCH, (200, 9800))):
            lut, info = sp.build_lut(h, bits, mode, *args)
            assert info == dict(lo=0, hi=0, fallback=1) and np.array_equal(lut, sp.linear_lut(bits))
    assert int(sp.linear_lut(bits)[top]) == (255 if bits >= 8 else top << (8 - bits)) and int(sp.linear_lut(bits)[0]) == 0


def test_all_zero_falls_back_and_linear_and_table_never_do():
    h = hist_of(10, {0: 100})
    for mode, args in ((sp.EQUALISE, ()), (sp.STRETCH, (0, 10000))):
        lut, info = sp.build_lut(h, 10, mode, *args)
        assert info["fallback"] == 1 and np.array_equal(lut, np.arange(1024) >> 2)
    table = np.arange(1024, dtype=np.int64).astype(np.uint8)
    assert sp.build_lut(h, 10, sp.LINEAR)[1]["fallback"] == 0 and sp.build_lut(h, 10, sp.TABLE, table=table)[1]["fallback"] == 0
    assert np.array_equal(sp.build_lut(h, 10, sp.TABLE, table=table)[0], table)
    hist, summ = sp.histogram(np.zeros((3, 4), np.uint16), 10)
    assert summ == dict(total=12, zeros=12, out_of_range=0, min_nz=0, max_nz=0) and int(hist[0]) == 12


def test_two_values_by_hand():
    # 10 bits, 30 pixels of 100 and 10 of 900: c = 30 from 100 on, 40 from 900 on; cmin = 30, D = 10
    h = hist_of(10, {0: 7, 100: 30, 900: 10})
    lut, info = sp.build_lut(h, 10, sp.EQUALISE)
    assert info["fallback"] == 0
    assert int(lut[0]) == 0 and set(lut[1:100]) == {1} and set(lut[100:900]) == {1} and set(lut[900:]) == {255}
    # stretch 0 .. 10000: lo = 100 (the first v with c > 0), hi = 900 (c reaches N); in between the line from 1 to 255
    lut, info = sp.build_lut(h, 10, sp.STRETCH, 0, 10000)
    assert info == dict(lo=100, hi=900, fallback=0)
    assert int(lut[0]) == 0 and set(lut[1:101]) == {1} and set(lut[900:]) == {255}
    assert int(lut[101]) == 1 + (254 * 1 + 400) // 800 == 1 and int(lut[500]) == 1 + (254 * 400 + 400) // 800 == 128 and int(lut[899]) == 1 + (254 * 799 + 400) // 800 == 255
    # 75 % of the data lies at 100: up to p_hi = 7500 both percentiles are 100 and the stretch has no width
    assert sp.build_lut(h, 10, sp.STRETCH, 0, 7500)[1] == dict(lo=0, hi=0, fallback=1)
    assert sp.build_lut(h, 10, sp.STRETCH, 7500, 7501)[1] == dict(lo=100, hi=900, fallback=0)
    assert sp.build_lut(h, 10, sp.STRETCH, 7501, 10000)[1] == dict(lo=0, hi=0, fallback=1)         # lo = hi = 900


def test_three_values_equalised_by_hand():
    # 8 bits: 1 x 10, 2 x 20, 5 x 200: c = 1, 3, 8; cmin = 1, D = 7
    h = hist_of(8, {10: 1, 20: 2, 200: 5})
    lut, info = sp.build_lut(h, 8, sp.EQUALISE)
    assert info["fallback"] == 0 and int(lut[9]) == 1 and int(lut[10]) == 1 and int(lut[19]) == 1
    assert int(lut[20]) == 1 + (254 * 2 + 3) // 7 == 74 and int(lut[199]) == 74 and int(lut[200]) == 255 and int(lut[255]) == 255


def test_every_value_at_the_top():
    for bits in (1, 8, 13, 16):
        top = (1 << bits) - 1
        img = np.full((3, 5), top, np.uint8 if bits <= 8 else np.uint16)
        out = sp.process(img, bits, sp.EQUALISE, factor=2)
        assert out["summary"]["fallback"] == 1 and out["summary"]["min_nz"] == out["summary"]["max_nz"] == top
        assert int(out["hist"][top]) == 15 and (out["tone"] == sp.linear_lut(bits)[top]).all() and out["small"].shape == (2, 3)
        assert (out["small"] == sp.linear_lut(bits)[top]).all()
    # 13 bits in uint16: samples above the top are the top, and counted
    img = np.array([[8191, 8192, 65535, 0, 5]], np.uint16)
    out = sp.process(img, 13, sp.LINEAR)
    assert out["summary"]["out_of_range"] == 2 and int(out["hist"][8191]) == 3 and out["tone"].tolist() == [[255, 255, 255, 0, 0]]


def test_missing_rows_do_not_darken_the_thumbnail():
    img = np.full((8, 8), 200, np.uint8)
    img[2:6] = 0                                                    # a lost segment
    lut = sp.linear_lut(8)
    assert sp.thumbnail(img, 8, lut, 4).tolist() == [[200, 200], [200, 200]]
    assert sp.thumbnail(img, 8, lut, 2).tolist() == [[200] * 4, [0] * 4, [0] * 4, [200] * 4]
    assert sp.thumbnail(np.array([[1, 2], [2, 0]], np.uint8), 8, lut, 2).tolist() == [[2]]        # (2 * 5 + 3) // 6: halves round up


# ---- the ABI's CPU side ------------------------------------------------------------------------------------------------------
def test_symbols_and_layouts():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(xrit_[a-z0-9_]+)\s*\(", src))
    import xritdemod_amd as xa
    from xritdemod_amd import _capi
    L = xa.lib()
    for name in FUNCTIONS:
        assert name in declared and name in _capi._SIGNATURES and hasattr(L, name), name
    ctypes_of = {"uint64_t": np.uint64, "uint32_t": np.uint32}
    for struct, dtype, size in (("xrit_product_params", xa.PRODUCT_PARAMS_DTYPE, 16), ("xrit_product_summary", xa.PRODUCT_SUMMARY_DTYPE, 64)):
        m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + r";\s*/\* (\d+) bytes", text, re.S)
        fields = []
        for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
            if decl.strip():
                ctype, names = decl.strip().split(None, 1)
                fields += [(nm.strip(), ctypes_of[ctype]) for nm in names.split(",")]
        assert int(m.group(2)) == size == dtype.itemsize and dtype == np.dtype(fields), struct
    assert tuple(xa.PRODUCT_SUMMARY_DTYPE.names) == sp.SUMMARY_FIELDS
    assert xa.PRODUCT_IMAGE_DTYPE.itemsize == 24 and xa.PRODUCT_IMAGE_DTYPE.fields["columns"][1] == 8
    for i, name in enumerate(xa.PRODUCT_TONES):
        assert re.search(r"#define XRIT_TONE_" + name.upper() + r"\s+" + str(i) + r"\b", text) and sp.TONES[name] == i
    assert re.search(r"#define XRIT_PRODUCT_MAX_FACTOR\s+64\b", text) and xa.PRODUCT_MAX_FACTOR == sp.MAX_FACTOR == 64


def test_bad_arguments_are_refused_before_a_device_is_asked_for():
    import xritdemod_amd as xa
    L = xa.lib()
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.xrit_product_create(None, 0) == -1 and L.xrit_product_reset(None) == -1 and L.xrit_product_destroy(None) == 0
    assert L.xrit_product_process_device(None, p, p, p, p, p, p, p, p, None) == -1
    assert L.xrit_product_process(None, p, p, p, p, p, p, p, p) == -1 and L.xrit_product_process_resident(None, p, p, p, p, p, p, p, p) == -1
    assert L.xrit_product_composite_device(None, p, 4, p, 4, 4, 4, p, p, None) == -1
    assert L.xrit_product_composite(None, p, 4, p, 4, 4, 4, p, p) == -1
    assert L.xrit_canvas_pixels_device(None, 0, C.byref(C.c_void_p())) == -1


def test_no_cpu_path():
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:                   # on a GPU box the same call makes a working object (-m gpu tests it)
        xa.ImageProduct().close()
        return
    with pytest.raises(xa.XritError) as ei:
        xa.ImageProduct()
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


# ---- the rule under the sanitizers ---------------------------------------------------------------------------------------------
def test_recorded_table_is_the_specification_s():
    want = sp.rule_table_text()
    assert open(TABLE).read() == want
    rows = [[int(x) for x in ln.split()] for ln in want.splitlines()]
    assert all(len(r) == 12 for r in rows) and {r[0] for r in rows} == {0, 1, 2, 3, 4}
    decisions = [r for r in rows if r[0] == 0]
    # every tone with and without the fallback where it has one, every bit depth's width, N at its bound
    assert {(r[1], r[10]) for r in decisions} == {(sp.LINEAR, 0), (sp.TABLE, 0), (sp.EQUALISE, 0), (sp.EQUALISE, 1), (sp.STRETCH, 0), (sp.STRETCH, 1)}
    assert {r[2] for r in decisions} == {1, 5, 8, 10, 13, 16} and max(r[3] for r in decisions) == 1 << 31
    assert {r[4] for r in rows if r[0] == 1} >= {0, 1, 255} and any(r[0] == 2 and r[2] == 4096 for r in rows)


def test_product_rule_host_check_under_sanitizers(tmp_path):
    """make product-host-check: the functions of csrc/product_rule.h that the kernels call, replayed over the recorded
    table in a stand-alone g++ program with -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "product-host-check",
                        f"PRODUCT_CHECK={tmp_path / 'product_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(TABLE).read().splitlines()
    n = sum(ln.startswith("1 ") for ln in lines)
    assert f"product_host_check: {len(lines)} rows, {n} table entries, every one the specification's: ok" in r.stdout, r.stdout


# ---- the host program's flags ------------------------------------------------------------------------------------------------
CANVAS = ["--input", "nowhere.cf32", "--files", "nowhere", "--files-decompress", "--canvas"]


@pytest.mark.parametrize("args,says", [
    (["--input", "nowhere.cf32", "--products"], "--products needs --canvas"),
    (["--input", "nowhere.cf32", "--files", "nowhere", "--files-decompress", "--products"], "--products needs --canvas"),
    (CANVAS + ["--product-factor", "8"], "need --products"),
    (CANVAS + ["--product-tone", "linear"], "need --products"),
    (CANVAS + ["--products", "--product-factor", "0"], "--product-factor 0: 1..64"),
    (CANVAS + ["--products", "--product-factor", "65"], "--product-factor 65: 1..64"),
    (CANVAS + ["--products", "--product-factor", "8x"], "--product-factor 8x: 1..64"),
    (CANVAS + ["--products", "--product-factor"], "--product-factor needs a value"),
    (CANVAS + ["--products", "--product-tone", "table"], "--product-tone table:"),
    (CANVAS + ["--products", "--product-tone", "stretch:500:500"], "--product-tone stretch:500:500:"),
    (CANVAS + ["--products", "--product-tone", "stretch:0:10001"], "--product-tone stretch:0:10001:"),
    (CANVAS + ["--products", "--product-tone", "stretch:-1:50"], "--product-tone stretch:-1:50:"),
    (CANVAS + ["--products", "--product-tone", "stretch:5"], "--product-tone stretch:5:"),
    (CANVAS + ["--products", "--product-tone", "stretch:5:60:7"], "--product-tone stretch:5:60:7:"),
])
def test_host_program_refuses_bad_product_flags(args, says):
    r = subprocess.run([HOST_BIN] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and says in r.stderr.splitlines()[0], r.stderr[:300]


@pytest.mark.parametrize("args", [["--products"], ["--products", "--product-tone", "stretch"], ["--products", "--product-tone", "stretch:0:10000"],
                                  ["--products", "--product-tone", "linear", "--product-factor", "64"],
                                  ["--products", "--product-factor", "1", "--product-tone", "equalise"]])
def test_host_program_accepts_good_product_flags(args, tmp_path):
    """Past the flags, the run ends at the input file that is not there (at the device that is not there, without one)."""
    at = ["--input", str(tmp_path / "nowhere.cf32"), "--files", str(tmp_path / "out"), "--files-decompress", "--canvas"]
    r = subprocess.run([HOST_BIN] + at + args, capture_output=True, text=True, timeout=60)
    assert "usage:" not in r.stderr and r.returncode == 1 and ("nowhere.cf32" in r.stderr or "no CPU path" in r.stderr), r.stderr[:300]
