"""CPU tier: the JPEG stage's specification (tests/jpeg_spec.py) against an outside implementation -- the files Pillow's
libjpeg wrote, recorded in tests/golden/jpeg_pil_files.npz (always), and Pillow itself where it imports (whole files:
grey and RGB, the qualities, restarts and shapes of the issue; the caller's own tables through qtables=); the counters
of what the inputs exercised, every event reached through Pillow-comparable input; the pieces by hand (a flat block, the
Huffman codes' prefix property, the bound); the CPU side of the ABI (symbols, the record's layout, the host-only header,
tables and bound against the specification, bad arguments, no CPU path); the rule (csrc/jpeg_rule.h) in a stand-alone
program under the sanitizers, replaying a table recorded from the specification; the host program's --jpeg flag."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_spec as js

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")
TABLE = os.path.join(ROOT, "tests", "golden", "jpeg_rule_table.txt")
FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_pil_files.npz")
HOST_BIN = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")

FUNCTIONS = ["xrit_jpeg_create", "xrit_jpeg_destroy", "xrit_jpeg_reset", "xrit_jpeg_set_quality", "xrit_jpeg_set_tables", "xrit_jpeg_header",
             "xrit_jpeg_quality_tables", "xrit_jpeg_header_for", "xrit_jpeg_bound", "xrit_jpeg_encode_device", "xrit_jpeg_encode",
             "xrit_jpeg_encode_resident"]
SHAPES = [(1, 1), (8, 8), (7, 9), (9, 7), (17, 33), (8, 600), (64, 72)]
QUALITIES = [1, 10, 50, 75, 90, 95, 100]


def restarts_of(shape):
    return [0, 1, 2, 7, (shape[1] + 7) // 8, 5000]             # the last: larger than any of the images


# ---- the recorded files ------------------------------------------------------------------------------------------------------
def test_specification_equals_the_recorded_pillow_files():
    z = np.load(FIXTURE)
    cases = jc.golden_cases()
    assert [str(n) for n in z["names"]] == [name for name, _, _ in cases]
    assert [str(v) for v in z["versions"]] == ["Pillow 12.2.0", "libjpeg 6.2"]
    off = z["offsets"]
    for i, (name, image, params) in enumerate(cases):
        assert np.array_equal(z["image_%02d" % i], image), name
        assert z["data"][off[i]:off[i + 1]].tobytes() == jc.spec_file(image, params)[0], name


def test_every_event_is_reached_through_pillow_comparable_input():
    """A condition, not a measurement: each event the specification counts happens in at least one of event_cases, all of
    which are in the fixture (and so are Pillow's bytes); RSTm wraps twice."""
    total = dict.fromkeys(js.COUNTERS, 0)
    most_restarts = 0
    for _, image, params in jc.event_cases():
        _, cnt = jc.spec_file(image, params)
        assert tuple(cnt) == js.COUNTERS
        for k, v in cnt.items():
            total[k] += v
        most_restarts = max(most_restarts, cnt["restarts"])
    assert all(total[k] > 0 for k in js.COUNTERS), total
    assert most_restarts >= 16                                  # at least 17 intervals
    fixture = {str(n) for n in np.load(FIXTURE)["names"]}
    assert {name for name, _, _ in jc.event_cases()} <= fixture


# ---- live against Pillow -----------------------------------------------------------------------------------------------------
def image_for(shape, rgb, quality):
    full = shape + (3,) if rgb else shape
    return jc.smooth(full) if quality in (10, 75, 95) else jc.noise(quality + 7 * shape[0] + shape[1], full)


@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_whole_file_equals_pillow(shape, rgb):
    pytest.importorskip("PIL")
    for quality in QUALITIES:
        image = image_for(shape, rgb, quality)
        for restart in restarts_of(shape):
            params = dict(quality=quality, restart=restart)
            assert jc.spec_file(image, params)[0] == jc.pillow_file(image, params), (quality, restart)


def test_own_tables_equal_pillow_qtables():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(5)
    for rgb in (False, True):
        for tables in (jc.ONES, jc.late_tables(63), rng.integers(1, 256, (2, 64)), np.full((2, 64), 255)):
            image = jc.noise(9, (19, 21, 3) if rgb else (19, 21))
            params = dict(tables=tables, restart=2)
            ours, theirs = jc.spec_file(image, params)[0], jc.pillow_file(image, params)
            assert ours == theirs
            # and the scan alone: what follows the SOS segment
            at = ours.index(b"\xff\xda")
            assert ours[at:] == theirs[theirs.index(b"\xff\xda"):]


def test_event_cases_equal_pillow():
    pytest.importorskip("PIL")
    for name, image, params in jc.event_cases():
        assert jc.spec_file(image, params)[0] == jc.pillow_file(image, params), name


def test_pillow_decodes_what_the_specification_writes():
    Image = pytest.importorskip("PIL.Image")
    import io
    image = jc.smooth((40, 56, 3))
    back = np.asarray(Image.open(io.BytesIO(js.encode(image, quality=95, restart=3)[0])).convert("RGB"))
    assert back.shape == image.shape and np.abs(back.astype(int) - image).mean() < 3


# ---- by hand -----------------------------------------------------------------------------------------------------------------
def test_flat_block_by_hand():
    """A block of 200s at quality 50 (the Annex K tables as they stand): DC = 8 * (200 - 128) * 8 / (16 * 8) = 36, category 6
    (code 1110), bits 100100; EOB 1010; 1-bits to the byte: 1110 1001 0010 1011."""
    file, cnt = js.encode(np.full((8, 8), 200, np.uint8), quality=50)
    head = js.header(1, 8, 8, js.quality_tables(50), 0)
    assert np.array_equal(js.quality_tables(50)[0], js.STD_LUMINANCE)
    assert file == head + bytes([0b11101001, 0b00101011]) + b"\xff\xd9"
    assert cnt == dict(dict.fromkeys(js.COUNTERS, 0), one_mcu_intervals=1)         # the whole image is one MCU
    assert js.coefficients(np.full((8, 8), 200, np.uint8), js.quality_tables(50)).reshape(-1).tolist() == [36] + [0] * 63


def test_edges_repeat_the_last_column_and_row():
    image = jc.noise(3, (5, 11))
    padded = np.pad(image, ((0, 3), (0, 5)), mode="edge")
    assert np.array_equal(js.coefficients(image, js.quality_tables(90)), js.coefficients(padded, js.quality_tables(90)))


def test_huffman_tables_are_prefix_codes_of_the_right_size():
    for _, _, bits, vals in js.HUFFMAN:
        codes = js.huffman_codes(bits, vals)
        assert len(codes) == len(vals) == sum(bits)
        words = sorted(format(c, "0%db" % n) for c, n in codes.values())
        assert all(not b.startswith(a) for a, b in zip(words, words[1:]))
    assert js.huffman_codes(js.AC_LUM_BITS, js.AC_LUM_VALS)[0xF0] == (0b11111111001, 11)
    assert js.huffman_codes(js.AC_LUM_BITS, js.AC_LUM_VALS)[0x00] == (0b1010, 4)
    assert js.huffman_codes(js.AC_CHROM_BITS, js.AC_CHROM_VALS)[0x00] == (0b00, 2)
    # the longest block of the bound: the longest DC code and 11 bits, 63 times the longest AC code and 10 bits
    assert max(n for _, _, b, v in js.HUFFMAN[::2] for _, n in js.huffman_codes(b, v).values()) + 11 == 22
    assert js.BLOCK_BITS == 22 + 63 * 26
    assert max(n for _, _, b, v in js.HUFFMAN[1::2] for _, n in js.huffman_codes(b, v).values()) + 10 == 26


def test_bound_holds_and_refuses():
    for _, image, params in jc.golden_cases():
        comps = 1 if image.ndim == 2 else 3
        assert len(jc.spec_file(image, params)[0]) <= js.bound(comps, image.shape[1], image.shape[0], params["restart"])
    assert js.bound(2, 8, 8, 0) == js.bound(1, 0, 8, 0) == js.bound(1, 8, 65536, 0) == js.bound(1, 8, 8, 65536) == 0
    assert js.bound(1, 16384, 16384, 0) > 0 and js.bound(1, 16385, 16384, 0) == 0 and js.bound(3, 16384, 16384, 0) == 0
    assert js.bound(1, 8, 8, 0) == len(js.header(1, 8, 8, jc.ONES, 0)) + 2 * (208 + 1) + 2


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
    m = re.search(r"typedef struct xrit_jpeg_result \{(.*?)\} xrit_jpeg_result;\s*/\* (\d+) bytes", text, re.S)
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        if decl.strip():
            ctype, names = decl.strip().split(None, 1)
            fields += [(nm.strip(), {"uint64_t": np.uint64, "uint32_t": np.uint32}[ctype]) for nm in names.split(",")]
    assert int(m.group(2)) == 16 == xa.JPEG_RESULT_DTYPE.itemsize and xa.JPEG_RESULT_DTYPE == np.dtype(fields) == js.RESULT_DTYPE
    assert re.search(r"#define XRIT_JPEG_MAX_BLOCKS \(1u << 22\)", text) and xa.JPEG_MAX_BLOCKS == js.MAX_BLOCKS == 1 << 22


def test_host_only_header_tables_and_bound_equal_the_specification():
    """xrit_jpeg_quality_tables, xrit_jpeg_header_for (what xrit_jpeg_header returns for a handle's parameters) and
    xrit_jpeg_bound never touch a device."""
    import xritdemod_amd as xa
    xa.lib()
    for quality in range(1, 101):
        assert np.array_equal(xa.jpeg_quality_tables(quality), js.quality_tables(quality)), quality
    rng = np.random.default_rng(8)
    for tables in (js.quality_tables(90), jc.ONES, rng.integers(1, 256, (2, 64))):
        for comps in (1, 3):
            for columns, rows, restart in ((1, 1, 0), (600, 8, 75), (65535, 3, 1), (5424, 5424, 678), (7, 65535, 65535)):
                assert xa.jpeg_header(tables, restart, comps, columns, rows) == js.header(comps, columns, rows, tables, restart)
    for comps in (0, 1, 2, 3, 4):
        for columns, rows in ((0, 5), (5, 0), (1, 1), (600, 8), (5424, 5424), (16384, 16384), (16385, 16384), (65535, 65535), (65536, 1)):
            for restart in (0, 1, 75, 65535, 65536):
                assert xa.jpeg_bound(comps, columns, rows, restart) == js.bound(comps, columns, rows, restart), (comps, columns, rows, restart)
    # the recorded Pillow header, once: what stands in front of the scan of a fixture file
    z = np.load(FIXTURE)
    i = [str(n) for n in z["names"]].index("rgb_smooth")
    theirs = z["data"][z["offsets"][i]:z["offsets"][i + 1]].tobytes()
    ours = xa.jpeg_header(js.quality_tables(60), 3, 3, 40, 24)
    assert theirs[:len(ours)] == ours and theirs[len(ours) - 14:len(ours) - 12] == b"\xff\xda"


def test_bad_arguments_are_refused_before_a_device_is_asked_for():
    import xritdemod_amd as xa
    L = xa.lib()
    buf = np.ones(1024, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    n = C.c_size_t()
    assert L.xrit_jpeg_create(None, 0) == -1 and L.xrit_jpeg_reset(None) == -1 and L.xrit_jpeg_destroy(None) == 0
    assert L.xrit_jpeg_set_quality(None, 90, 0) == -1 and L.xrit_jpeg_set_tables(None, p, 0) == -1
    assert L.xrit_jpeg_header(None, 1, 8, 8, p, 1024, C.byref(n)) == -1
    assert L.xrit_jpeg_encode_device(None, p, 1, p, 16, p, None) == -1
    assert L.xrit_jpeg_encode(None, p, 1, p, 16, p) == -1 and L.xrit_jpeg_encode_resident(None, p, 1, p, 16, p) == -1
    assert L.xrit_jpeg_quality_tables(0, p) == -1 and L.xrit_jpeg_quality_tables(101, p) == -1 and L.xrit_jpeg_quality_tables(50, None) == -1
    for comps, columns, rows, restart in ((2, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 0), (3, 65536, 8, 0), (1, 8, 8, 65536), (3, 16384, 16384, 0)):
        assert L.xrit_jpeg_header_for(p, restart, comps, columns, rows, p, 1024, C.byref(n)) == -1
    zero = buf.copy()
    zero[77] = 0                                                # a table entry of 0
    assert L.xrit_jpeg_header_for(zero.ctypes.data_as(C.c_void_p), 0, 1, 8, 8, p, 1024, C.byref(n)) == -1
    assert L.xrit_jpeg_header_for(p, 0, 1, 8, 8, None, 0, C.byref(n)) == 0 and n.value == len(js.header(1, 8, 8, jc.ONES, 0))
    guard = np.full(64, 0xA5, np.uint8)                         # too little room: the length, nothing written
    assert L.xrit_jpeg_header_for(p, 0, 1, 8, 8, guard.ctypes.data_as(C.c_void_p), 64, C.byref(n)) == 0 and (guard == 0xA5).all()


def test_no_cpu_path():
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:                   # on a GPU box the same call makes a working object (-m gpu tests it)
        xa.JpegEncoder().close()
        return
    with pytest.raises(xa.XritError) as ei:
        xa.JpegEncoder()
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


# ---- the rule under the sanitizers ---------------------------------------------------------------------------------------------
def test_recorded_table_is_the_specification_s():
    want = js.rule_table_text()
    assert open(TABLE).read() == want
    rows = [[int(x) for x in ln.split()] for ln in want.splitlines()]
    assert all(len(r) == 18 for r in rows) and {r[0] for r in rows} == {0, 1, 2, 3, 4, 5}
    assert {r[1] for r in rows if r[0] == 0} == {0, 1}                          # both passes
    assert {r[2] for r in rows if r[0] == 3} >= {0, 1, 10, 11}                  # the categories at both ends
    assert {r[2] for r in rows if r[0] == 4} >= {1, 49, 50, 100} and {r[3] for r in rows if r[0] == 4} >= {1, 255}
    assert sum(r[0] == 5 for r in rows) == 2 * (12 + 162)


def test_jpeg_rule_host_check_under_sanitizers(tmp_path):
    """make jpeg-host-check: the functions of csrc/jpeg_rule.h that the kernels call, replayed over the recorded table in
    a stand-alone g++ program with -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "jpeg-host-check",
                        f"JPEG_CHECK={tmp_path / 'jpeg_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(TABLE).read().splitlines()
    n = sum(ln.startswith("0 ") for ln in lines)
    assert f"jpeg_host_check: {len(lines)} rows, {n} transform passes, 348 Huffman codes, every one the specification's: ok" in r.stdout, r.stdout


# ---- the host program's flag -------------------------------------------------------------------------------------------------
CANVAS = ["--input", "nowhere.cf32", "--files", "nowhere", "--files-decompress", "--canvas"]


@pytest.mark.parametrize("args,says", [
    (["--input", "nowhere.cf32", "--jpeg"], "--jpeg needs --products"),
    (CANVAS + ["--jpeg"], "--jpeg needs --products"),
    (CANVAS + ["--products", "--jpeg", "0"], "--jpeg 0: 1..100"),
    (CANVAS + ["--products", "--jpeg", "101"], "--jpeg 101: 1..100"),
    (CANVAS + ["--products", "--jpeg", "9x"], "--jpeg 9x: 1..100"),
])
def test_host_program_refuses_bad_jpeg_flags(args, says):
    r = subprocess.run([HOST_BIN] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and says in r.stderr.splitlines()[0], r.stderr[:300]


@pytest.mark.parametrize("args", [["--products", "--jpeg"], ["--products", "--jpeg", "75"], ["--jpeg", "100", "--products", "--product-factor", "4"],
                                  ["--products", "--jpeg", "--product-tone", "linear"]])
def test_host_program_accepts_good_jpeg_flags(args, tmp_path):
    """Past the flags, the run ends at the input file that is not there (at the device that is not there, without one)."""
    at = ["--input", str(tmp_path / "nowhere.cf32"), "--files", str(tmp_path / "out"), "--files-decompress", "--canvas"]
    r = subprocess.run([HOST_BIN] + at + args, capture_output=True, text=True, timeout=60)
    assert "usage:" not in r.stderr and r.returncode == 1 and ("nowhere.cf32" in r.stderr or "no CPU path" in r.stderr), r.stderr[:300]
