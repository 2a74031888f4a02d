"""CPU tier: the CPU side of the canvas stage's ABI -- the header declares the functions, the ctypes layer binds them, the
library exports them, the record layouts are the header's field for field and mirror the specification's dtypes, bad
arguments are refused before a device is asked for, and there is no CPU path; the rule (csrc/canvas_rule.h) in a
stand-alone program under the sanitizers, replaying a table recorded from the specification."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import canvas_cases as cc
import canvas_spec as cs
import file_spec as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")
TABLE = os.path.join(ROOT, "tests", "golden", "canvas_rule_table.txt")

FUNCTIONS = ["xrit_canvas_create", "xrit_canvas_destroy", "xrit_canvas_reset", "xrit_canvas_process_device", "xrit_canvas_process",
             "xrit_canvas_read_device", "xrit_canvas_read", "xrit_canvas_segments", "xrit_canvas_key", "xrit_canvas_stats",
             "xrit_canvas_release"]
CTYPES = {"uint64_t": np.uint64, "uint32_t": np.uint32, "int32_t": np.int32, "uint16_t": np.uint16, "uint8_t": np.uint8}


def header_struct(text, name):
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
        for nm in names.split(","):
            arr = re.match(r"\s*(\w+)\[(\d+)\]", nm)
            fields.append((arr.group(1), CTYPES[ctype], (int(arr.group(2)),)) if arr else (nm.strip(), CTYPES[ctype]))
    return np.dtype(fields), int(m.group(2))


def test_symbols_and_layouts():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(xrit_[a-z0-9_]+)\s*\(", src))
    import xritdemod_amd as xa
    from xritdemod_amd import _capi
    L = xa.lib()
    for name in FUNCTIONS:
        assert name in declared, name
        assert name in _capi._SIGNATURES, name
        assert hasattr(L, name), name
    for struct, dtype, size in (("xrit_canvas_file", xa.CANVAS_FILE_DTYPE, 32), ("xrit_canvas_slot", xa.CANVAS_SLOT_DTYPE, 136),
                                ("xrit_canvas_segment", xa.CANVAS_SEGMENT_DTYPE, 32), ("xrit_canvas_key_state", xa.CANVAS_KEY_DTYPE, 32),
                                ("xrit_canvas_counters", xa.CANVAS_STATS_DTYPE, 120), ("xrit_canvas_summary", xa.CANVAS_SUMMARY_DTYPE, 168)):
        want, stated = header_struct(text, struct)
        assert stated == size == dtype.itemsize == want.itemsize, struct
        assert dtype == want, struct
        for f in want.names:
            assert dtype.fields[f][1] % min(dtype.fields[f][0].base.itemsize, 8) == 0, (struct, f)
    assert xa.CANVAS_FILE_DTYPE == cs.FILE_DTYPE and xa.CANVAS_SLOT_DTYPE == cs.SLOT_DTYPE
    assert xa.CANVAS_SEGMENT_DTYPE == cs.SEGMENT_DTYPE and xa.CANVAS_KEY_DTYPE == cs.KEY_DTYPE
    assert tuple(xa.CANVAS_STATS_DTYPE.names) == cs.COUNTERS
    assert tuple(xa.CANVAS_SUMMARY_DTYPE.names) == cs.CALL_COUNTS + cs.COUNTERS + ("overflow", "reserved")
    for i, name in enumerate(xa.CANVAS_REASONS):
        assert re.search(r"#define XRIT_CANVAS_" + name + r"\s+" + str(i) + r"\b", text), name
        assert getattr(cs, name) == i
    assert re.search(r"#define XRIT_CANVAS_MAX_SLOTS\s+64\b", text) and re.search(r"#define XRIT_CANVAS_MAX_SEGMENTS\s+64\b", text)


def test_bad_arguments_are_refused_before_a_device_is_asked_for():
    import xritdemod_amd as xa
    L = xa.lib()
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert L.xrit_canvas_create(None, 0, 4, 16384) == -1
    for slots, slot_bytes in ((0, 16384), (65, 16384), (4, 0), (4, 16392)):
        assert L.xrit_canvas_create(C.byref(h), 0, slots, slot_bytes) == -1 and not h.value
    assert L.xrit_canvas_reset(None) == -1 and L.xrit_canvas_release(None, 0) == -1
    assert L.xrit_canvas_stats(None, p) == -1 and L.xrit_canvas_key(None, 0, 0, p) == -1 and L.xrit_canvas_segments(None, 0, p) == -1
    assert L.xrit_canvas_read(None, 0, p, 0, p) == -1 and L.xrit_canvas_read_device(None, 0, p, 0, None) == -1
    assert L.xrit_canvas_process(None, p, 0, p, 0, p, 0, p, p, 0, p, 0, p, p, p, p, p) == -1
    assert L.xrit_canvas_process_device(None, p, 0, p, 0, p, 0, p, p, 0, p, 0, p, p, p, p, p, None) == -1
    assert L.xrit_canvas_destroy(None) == 0


def test_no_cpu_path():
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:                   # on a GPU box the same call makes a working object (-m gpu tests it)
        xa.ImageCanvas(2, 4096).close()
        return
    with pytest.raises(xa.XritError) as ei:
        xa.ImageCanvas(2, 4096)
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


def recorded_table():
    """The table the host check replays: the constructed cases in one call and cut into calls, as the specification
    decided them."""
    table = []
    stream, _ = cc.mixed_stream()
    cc.Run([stream], slots=6, table=table)
    cc.Run(list(fs.cut_calls(np.random.default_rng(5), stream, 4)), slots=3, table=table)
    stream, _, _ = cc.reasons_stream()
    cc.Run([stream], slots=8, table=table)
    cc.Run(list(fs.cut_calls(np.random.default_rng(6), stream, 9)), slots=8, table=table)
    cc.Run([cc.no_slot_stream()], slots=2, table=table)
    cc.Run([cc.aborted_stream()[0]], table=table)
    first, second, _ = cc.release_streams()
    cc.Run([first, second], actions={1: [0]}, table=table)
    return table


def test_recorded_table_is_the_specification_s():
    want = "\n".join(" ".join(str(x) for x in row) for row in recorded_table()) + "\n"
    assert open(TABLE).read() == want
    rows = [[int(x) for x in ln.split()] for ln in want.splitlines()]
    assert all(len(r) == 18 for r in rows)
    records = [r for r in rows if r[0] == 2]
    # it holds what the rule has to tell apart: every reason, joins and births, records with and without BEGINS, a
    # BEGINS record that is no image, a release
    assert {r[16] for r in records} == set(range(8)) and any(r[0] == 1 for r in rows) and sum(r[0] == 0 for r in rows) == 7
    assert sum(r[16] == cs.PLACED and not r[1] & fs.BEGINS for r in records) > 20
    assert sum(r[16] == cs.BAD_SEGMENT for r in records) >= 18 and any(r[9] == cs.NO_ID and r[16] == cs.PLACED for r in records)


def test_canvas_rule_host_check_under_sanitizers(tmp_path):
    """make canvas-host-check: the functions of csrc/canvas_rule.h that the kernels call, replayed over the recorded
    table in a stand-alone g++ program with -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "canvas-host-check",
                        f"CANVAS_CHECK={tmp_path / 'canvas_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(TABLE).read().splitlines()
    n = sum(ln.startswith("2 ") for ln in lines)
    assert f"canvas_host_check: {len(lines)} rows, {n} records, the reason and the slot of each: ok" in r.stdout, r.stdout
