"""CPU tier of the JPEG decoder stage: the specification (tests/jpegdec_spec.py) against Pillow's
libjpeg -- always against the pixels recorded in tests/golden/jpegdec_pil.npz, live where Pillow imports --, its model of
the parallel form against its serial walk (on an adversarial stream too), the statuses of unsupported and damaged streams,
the stand-alone host function xrit_jpegdec_header against the specification at every cut of every stream, and
csrc/jpegdec_rule.h replayed over the recorded table under the sanitizers (make jpegdec-host-check)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc
import jpegdec_cases as dc
import jpegdec_spec as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")
TABLE = os.path.join(ROOT, "tests", "golden", "jpegdec_rule_table.txt")
FORMS = ((0, ds.DEFAULT_S), (1, 128), (1, ds.DEFAULT_S))


@pytest.fixture(scope="module")
def golden():
    return dc.Golden()


def pillow():
    return pytest.importorskip("PIL")


def test_fixture_is_what_the_cases_describe(golden):
    assert golden.names == [c[0] for c in dc.pillow_cases()] + [c[0] for c in dc.unsupported_cases()] and len(golden.names) <= 64
    for name, image, _, _ in dc.pillow_cases():
        # (the rows of 75 blocks, 8 x 600 and 5 x 597, are longer than 72: the GPU tier's case of more blocks than a wave has lanes)
        assert golden.pixels[name].shape == image.shape and (max(image.shape[:2]) <= 72 or "row75" in name)


def test_specification_gives_the_recorded_pillow_pixels(golden):
    """Every sound stream, in the serial form and in the parallel form at 128 bits and at the default; the counters say that
    the set reaches what it is there for, and that it stays where libjpeg's C table and its SIMD paths agree."""
    cnt = ds.new_counters()
    for name in golden.sound:
        for form, S in FORMS:
            status, pixels, h, found = ds.decode(golden.files[name], form, S, cnt)
            assert status == ds.OK and pixels.dtype == np.uint8 and np.array_equal(pixels, golden.pixels[name]), (name, form, S)
            assert found == h["intervals"]
    for k in ("long_codes", "straddle", "tiles_over_one", "rounds_over_one", "stuffed", "restarts", "zrl", "eob", "no_eob"):
        assert cnt[k] > 0, (k, cnt)
    assert cnt["max_rounds"] > 1
    # libjpeg's range-limit table is indexed with 10 bits: values from -512 to 511 in front of the + 128 have one meaning
    assert -384 <= cnt["min_in_front"] < 0 and 255 < cnt["max_in_front"] <= 639, cnt
    tables = {tuple(map(tuple, ds.parse_header(golden.files[n])["huff"][0])) for n in golden.sound}
    assert len(tables) > 5                              # optimised tables among them
    assert {ds.parse_header(golden.files[n])["restart"] for n in golden.sound} >= {0, 1, 2, 7, 5000}


def test_specification_gives_pillow_s_pixels_live(golden):
    """The same where Pillow imports, on streams written now, and on the files of the encoder's fixture and its event-rich
    inputs coded by the encoder's specification: ZRL chains, blocks without EOB, DC category 11, FF pairs, RSTm wrapping."""
    pillow()
    for name, image, kw, tail in dc.pillow_cases():
        f = dc.pillow_write(image, kw, tail)
        status, pixels, _, _ = ds.decode(f, 1, 128)
        assert status == ds.OK and np.array_equal(pixels, dc.pillow_read(f)), name
    for name, f in dc.encoder_files():
        status, pixels, _, _ = ds.decode(f)
        assert status == ds.OK and np.array_equal(pixels, dc.pillow_read(f)), name
    most = 0
    for name, image, params in jc.event_cases():
        f, cnt = jc.spec_file(image, params)
        most = max(most, cnt["restarts"])
        for form, S in FORMS:
            status, pixels, _, found = ds.decode(f, form, S)
            assert status == ds.OK and found == cnt["restarts"] + 1 and np.array_equal(pixels, dc.pillow_read(f)), (name, form)
    assert most >= 16


def test_unsupported_and_damaged_headers(golden):
    for name in golden.unsupported:
        status, pixels, _, _ = ds.decode(golden.files[name])
        assert status == ds.UNSUPPORTED and pixels is None, name
    for what, want in dc.PATCHES.items():
        f = dc.patched(golden.files["rgb_7x9" if what == "two_components" else "grey_7x9"], what)
        assert ds.decode(f)[0] == want, what
        assert ds.header_info(f)["status"] == want and ds.header_info(f)["columns"] == 0
    big = bytearray(golden.files["grey_8x8"])
    sof = dc.find(big, 0xC0)
    big[sof + 5:sof + 9] = bytes([0x80, 0x01, 0x40, 0x00])      # 32769 x 16384: more than 2^22 blocks
    info = ds.header_info(bytes(big))
    assert info["status"] == ds.TOO_LARGE and (info["columns"], info["rows"], info["blocks"]) == (16384, 32769, 0)


def test_damaged_set(golden):
    """Truncations at every byte, byte flips in the scan, RSTm removed, swapped, replaced, inserted: the specified status,
    zero pixels, never an exception, and the two forms agree."""
    seen = {}
    for name, f in dc.damaged_set(golden.files["grey_7x9"], golden.files["grey_smooth_rows"]):
        a, b = ds.decode(f, 0), ds.decode(f, 1, 128)
        assert a[0] == b[0] and a[3] == b[3], name
        if a[1] is not None:
            assert np.array_equal(a[1], b[1]) and (a[0] == ds.OK or not a[1].any()), name
        seen[name] = a[0]
    assert seen["rst_removed"] == ds.RST_ORDER and seen["rst_swapped"] == ds.RST_ORDER and seen["other_marker"] == ds.MARKER
    assert seen["rst_inserted"] == ds.INTERVALS and seen["cut_in_scan"] == ds.INTERVALS and seen["no_eoi"] == ds.OK
    cuts = [v for k, v in seen.items() if k.startswith("cut_") and k != "cut_in_scan"]
    assert set(cuts) >= {ds.DAMAGED, ds.SHORT, ds.INTERVALS} and cuts[0] == ds.DAMAGED
    assert {ds.OK, ds.SHORT} <= {v for k, v in seen.items() if k.startswith("flip_")}


def test_parallel_form_equals_the_serial_walk_on_the_adversarial_stream():
    """Every guess wrong, and every exit computed from a wrong entry wrong: the settled states advance one lane per round, so a
    full tile takes LANES = 64 rounds -- the bound of the argument in DESIGN.md section 27 -- and ends on the serial states."""
    f, coef = dc.adversarial()
    cnt = ds.new_counters()
    serial, parallel = ds.decode(f, 0), ds.decode(f, 1, 128, cnt)
    assert serial[0] == parallel[0] == ds.OK and np.array_equal(serial[1], parallel[1])
    print("rounds:", cnt["max_rounds"], "tiles:", 200 * 128 // 128 // ds.LANES + 1)
    assert cnt["max_rounds"] == ds.LANES and cnt["tiles_over_one"] == 1 and cnt["straddle"] == 200
    got = np.zeros_like(coef)
    h = ds.parse_header(f)
    iv = ds.Interval(ds.cut_scan(f, h["scan"])[0][0], [ds._full_lut(*h["huff"][0][:2]) + ds._full_lut(*h["huff"][0][2:])])

    def sink(block, z, v):
        got[block, z] = v

    assert ds.parallel_walk(iv, 200, sink, 128, ds.new_counters()) == ds.OK
    got[:, 0] = np.cumsum(got[:, 0])
    assert np.array_equal(got, coef)
    for S in (32, 100, 127, 129, 4096):                 # other cuts: fewer rounds, the same coefficients
        assert np.array_equal(ds.decode(f, 1, S)[1], serial[1])
    try:
        assert np.array_equal(dc.pillow_read(f), serial[1])
    except ImportError:
        pass


def test_batch_offsets_capacity_and_too_large(golden):
    files = [golden.files[n] for n in ("grey_7x9", "progressive", "rgb_9x7", "grey_8x8")]
    buf = b"".join(files)
    items, at = [], 0
    for f in files:
        items.append((at, len(f)))
        at += len(f)
    writes, records, summary = ds.decode_batch(buf, items + [(len(buf) - 4, 5)])
    assert list(records["status"]) == [0, 1, 0, 0, 2] and list(records["offset"]) == [0, 0, 64, 64 + 192, 0] and summary["bytes"] == 64 + 192 + 64
    assert list(records["length"]) == [63, 0, 189, 64, 0] and summary["images"] == 3 and summary["overflow"] == 0 and [w[0] for w in writes] == [0, 64, 256]
    assert writes[0][1][63:] == b"\0" and writes[1][1][189:] == b"\0\0\0"
    writes, records, summary = ds.decode_batch(buf, items, cap=64 + 191 + 64)
    assert summary["overflow"] == 1 and [w[0] for w in writes] == [0, 64] and summary["bytes"] == 320 and records[3]["offset"] == 256
    _, records, summary = ds.decode_batch(buf, items, max_blocks=7)
    assert list(records["status"]) == [0, 1, 3, 3] and list(records["columns"]) == [9, 0, 7, 8] and summary["bytes"] == 64


def test_header_lists_the_statuses():
    text = open(HEADER).read()
    for name in ("OK", "UNSUPPORTED", "DAMAGED", "TOO_LARGE", "BAD_CODE", "INDEX", "SHORT", "INTERVALS", "RST_ORDER", "MARKER"):
        assert int(re.search(r"#define XRIT_JPEGDEC_%s\s+(\d+)" % name, text).group(1)) == getattr(ds, name)
    assert "#define XRIT_JPEGDEC_MAX_BLOCKS  (1u << 22)" in text and ds.MAX_BLOCKS == 1 << 22


def test_host_header_function_equals_the_specification(golden):
    """xrit_jpegdec_header, plain host code: every stream of the fixture and the patched ones, each cut at every byte."""
    import xritdemod_amd as xa
    streams = [golden.files[n] for n in ("grey_7x9", "rgb_9x7", "grey_com_app", "rgb_own_tables", "progressive", "s420", "cmyk")]
    streams += [dc.patched(golden.files["rgb_7x9" if w == "two_components" else "grey_7x9"], w) for w in dc.PATCHES]
    for f in streams:
        h = ds.parse_header(f)
        for cut in list(range(min(len(f), (h["scan"] or 700) + 3))) + [len(f)]:
            assert xa.jpegdec_header(f[:cut]).tobytes() == ds.header_info(f[:cut]).tobytes(), cut
    for name in golden.names:
        assert xa.jpegdec_header(golden.files[name]).tobytes() == ds.header_info(golden.files[name]).tobytes(), name
    assert xa.JPEGDEC_RECORD_DTYPE == ds.RECORD_DTYPE and xa.JPEGDEC_SUMMARY_DTYPE == ds.SUMMARY_DTYPE and xa.JPEGDEC_INFO_DTYPE == ds.INFO_DTYPE


def test_recorded_table_is_the_specification_s(golden):
    want = ds.rule_table_text(*dc.rule_table_inputs(golden))
    assert open(TABLE).read() == want
    rows = [[int(x) for x in ln.split()] for ln in want.splitlines()]
    kinds = [r[0] for r in rows]
    assert set(kinds) == set(range(10)) and kinds.count(4) == kinds.count(5) == 5 and len(rows) < 400
    assert [r[1:3] for r in rows if r[0] == 1][0] == [-640, 1281] and [r[1:3] for r in rows if r[0] == 2] == [[0, 256]]
    # a decode step for every code of Annex K (12 + 162 twice) and of the optimised table, one with a bit too few in the short ones
    optimised = dc.rule_table_inputs(golden)[0]
    assert sum((len(r) - 2) // 4 for r in rows if r[0] == 5) == 2 * 162 + 2 * (2 * 12 + len(optimised[1])) + 5 * 4 and 8 < len(optimised[1]) < 100
    # every stream cut at every byte: the ranges of a stream cover 0 .. its length without a gap
    for i in {r[1] for r in rows if r[0] == 7}:
        spans = [r[2:4] for r in rows if r[0] == 7 and r[1] == i]
        assert spans[0][0] == 0 and all(a[1] + 1 == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] > 300


def test_jpegdec_rule_host_check_under_sanitizers(tmp_path):
    """make jpegdec-host-check: csrc/jpegdec_rule.h -- the header walk, the table build and the decode step, the entropy walk,
    both inverse-DCT passes, range limit and colour -- replayed over the recorded table in a stand-alone g++ program with
    -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "jpegdec-host-check",
                        f"JPEGDEC_CHECK={tmp_path / 'jpegdec_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"jpegdec-host-check: {len(open(TABLE).read().splitlines())} rows, " in r.stdout and "ok" in r.stdout, r.stdout
