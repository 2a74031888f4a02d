"""CPU tier: the CPU side of the image stage's ABI -- the header declares the functions, the ctypes layer binds them, the
library exports them, the record layouts are the header's field for field and mirror the specification's dtypes, bad
arguments are refused before a device is asked for, and there is no CPU path; the rule per record and per key
(csrc/image_rule.h) in a stand-alone program under the sanitizers against a table recorded from the specification."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import file_spec as fs
import image_spec as isp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")
TABLE = os.path.join(ROOT, "tests", "golden", "image_rule_table.txt")

FUNCTIONS = ["xrit_images_create", "xrit_images_destroy", "xrit_images_reset", "xrit_images_process_device", "xrit_images_process",
             "xrit_images_stats", "xrit_images_key"]
CTYPES = {"uint64_t": np.uint64, "uint32_t": np.uint32, "uint16_t": np.uint16, "uint8_t": np.uint8}


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
    for struct, dtype, size in (("xrit_image_line", xa.IMAGE_LINE_DTYPE, 32), ("xrit_image_file", xa.IMAGE_FILE_DTYPE, 48),
                                ("xrit_images_summary", xa.IMAGES_SUMMARY_DTYPE, 80), ("xrit_images_counters", xa.IMAGES_STATS_DTYPE, 48),
                                ("xrit_image_key", xa.IMAGE_KEY_DTYPE, 16)):
        want, stated = header_struct(text, struct)
        assert stated == size == dtype.itemsize == want.itemsize, struct
        # (natural alignment without padding: the packed dtype's offsets are the C compiler's)
        assert dtype == want, struct
        for f in want.names:
            assert dtype.fields[f][1] % min(dtype.fields[f][0].base.itemsize, 8) == 0, (struct, f)
    assert xa.IMAGE_LINE_DTYPE == isp.LINE_DTYPE and xa.IMAGE_FILE_DTYPE == isp.FILE_DTYPE
    assert tuple(xa.IMAGES_STATS_DTYPE.names) == isp.COUNTERS
    # a line begins like a packet descriptor and a piece
    for f in ("offset", "length"):
        assert xa.IMAGE_LINE_DTYPE.fields[f][1] == xa.PACKET_DTYPE.fields[f][1] == xa.FILE_PIECE_DTYPE.fields[f][1]
    for name in ("XRIT_IMAGES_MAX_PIECES", "XRIT_IMAGES_MAX_FILES", "XRIT_IMAGES_MAX_LINES", "XRIT_IMAGES_MAX_BYTES"):
        assert re.search(r"#define\s+" + name + r"\b", text), name
    assert re.search(r"#define XRIT_IMAGES_MAX_BYTES\(p\) \(\(size_t\)131072 \* \(p\)\)", text) and isp.MAX_LINE_BYTES == 131072
    for name in ("ImageDecoder", "IMAGE_LINE_DTYPE", "IMAGE_FILE_DTYPE", "IMAGES_SUMMARY_DTYPE", "IMAGES_STATS_DTYPE"):
        assert hasattr(xa, name)


def test_bound_on_the_image_bytes():
    import xritdemod_amd as xa
    rec = np.zeros(3, xa.FILE_RECORD_DTYPE)
    rec["n_pieces"], rec["columns"], rec["bits_per_pixel"] = [4, 2, 1], [5, 33, 65535], [8, 16, 16]
    assert xa.images_max_bytes(rec) == 4 * 8 + 2 * 68 + 131072
    assert xa.images_max_bytes(rec[:0]) == 0


def test_bad_arguments_are_refused_before_a_device_is_asked_for():
    import xritdemod_amd as xa
    L = xa.lib()
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.xrit_images_create(None, 0) == -1
    assert L.xrit_images_reset(None) == -1
    assert L.xrit_images_stats(None, p) == -1 and L.xrit_images_key(None, 0, 0, p) == -1
    assert L.xrit_images_process(None, p, 0, p, 0, p, 0, p, p, 0, p, 0, p, p) == -1
    assert L.xrit_images_process_device(None, p, 0, p, 0, p, 0, p, p, 0, p, 0, p, p, None) == -1
    assert L.xrit_images_destroy(None) == 0


def test_no_cpu_path():
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:                   # on a GPU box the same call makes a working object (-m gpu tests it)
        xa.ImageDecoder().close()
        return
    with pytest.raises(xa.XritError) as ei:
        xa.ImageDecoder()
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


def recorded_table():
    """The table the host check is held against: every record of a few cut streams, damaged ones among them, as the
    specification decided it."""
    table = []
    for seed, k, hurt in ((11, 2, False), (12, 5, True), (13, 1, True)):
        rng = np.random.default_rng(seed)
        spoil = (lambda r, line: rs_spoil(r, line)) if hurt else None
        stream, _ = isp.random_stream(rng, 6, [(0, 10), (0, 11), (9, 2047)], n_other=4, max_cols=40, max_rows=6, spoil=spoil)
        if hurt:
            stream = fs.damage(rng, stream, 0.06)
        fst, ist = fs.State(), isp.State()
        for part in fs.cut_calls(rng, stream, k):
            data, pieces, files, _ = isp.run_files(fst, part)
            isp.process(ist, data, pieces, files, table=table)
    return table


def rs_spoil(rng, line):
    import rice_spec as rs
    return rs.truncate(rng, line) if rng.random() < 0.3 else line


def test_recorded_table_is_the_specification_s():
    want = "\n".join(" ".join(str(x) for x in row) for row in recorded_table()) + "\n"
    assert open(TABLE).read() == want
    rows = [[int(x) for x in ln.split()] for ln in want.splitlines()]
    rice, cont = [r[16] for r in rows], [r[17] for r in rows]
    # it holds what the rule has to tell apart: images begun and continued, files that are none, a continuation refused,
    # bare ABORTED records, faults carried into the state
    assert sum(rice) > 40 and sum(cont) > 20 and rice.count(0) > 20
    assert any(r[0] == fs.ABORTED and r[1] == 0 and r[16] for r in rows) and any(r[23] and r[24] == 1 for r in rows)
    assert any(not (r[0] & fs.BEGINS) and not r[16] for r in rows)


def test_image_rule_host_check_under_sanitizers(tmp_path):
    """make images-host-check: image_mark and image_next (csrc/image_rule.h, the functions the kernels call) row by row
    against the recorded table, in a stand-alone g++ program with -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "images-host-check",
                        f"IMAGES_CHECK={tmp_path / 'image_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    n = len(open(TABLE).read().splitlines())
    assert f"image_host_check: {n} records, the mark and the key after each: ok" in r.stdout, r.stdout
