"""CPU tier: the CPU side of the file assembler's and the Rice decoder's ABI -- the header declares the functions, the
ctypes layer binds them, the library exports them, the record layouts have their documented sizes and mirror the
specifications' dtypes, bad arguments are refused before a device is asked for, and there is no CPU path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import file_spec as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")

FUNCTIONS = ["xrit_files_create", "xrit_files_destroy", "xrit_files_reset", "xrit_files_process_device", "xrit_files_process",
             "xrit_files_stats", "xrit_files_key", "xrit_rice_decode_device", "xrit_rice_decode", "xrit_rice_form"]


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
    assert xa.FILE_PIECE_DTYPE.itemsize == 32 and xa.FILE_PIECE_DTYPE == fs.PIECE_DTYPE
    assert xa.FILE_RECORD_DTYPE.itemsize == 80 and xa.FILE_RECORD_DTYPE == fs.RECORD_DTYPE
    assert xa.FILES_SUMMARY_DTYPE.itemsize == 104 and xa.FILES_STATS_DTYPE.itemsize == 80 and xa.FILE_KEY_DTYPE.itemsize == 56
    # a piece begins like a packet descriptor: either serves as a Rice line descriptor
    for f in ("offset", "length"):
        assert xa.FILE_PIECE_DTYPE.fields[f][1] == xa.PACKET_DTYPE.fields[f][1]
    assert (xa.FILE_BEGINS, xa.FILE_ENDS, xa.FILE_ABORTED, xa.FILE_LENGTH_MATCH) == (fs.BEGINS, fs.ENDS, fs.ABORTED, fs.LENGTH_MATCH)
    for comment in ("/* 32 bytes", "/* 80 bytes", "/* 104 bytes", "/* 56 bytes"):
        assert comment in text
    for source in ("CCSDS 121.0", "CCSDS 133.0", "CGMS 03", "no reference line"):
        assert source in text.replace("\n * ", " "), source
    for name in ("XRIT_FILES_MAX_PACKETS", "XRIT_FILES_MAX_PIECES", "XRIT_FILES_MAX_BYTES", "XRIT_FILES_MAX_FILES", "XRIT_E_ARG"):
        assert re.search(r"#define\s+" + name + r"\b", text), name
    for name in ("FileAssembler", "RiceDecoder", "decode_file_lines", "is_rice_coded"):
        assert hasattr(xa, name)


def test_link_rule_is_the_specification_s():
    import xritdemod_amd as xa
    rec = np.zeros(1, xa.FILE_RECORD_DTYPE)[0]
    for f, v in (("header_state", 2), ("compression", 1), ("bits_per_pixel", 8), ("columns", 100), ("pixels_per_block", 16),
                 ("header_length", 32)):
        rec[f] = v
    assert xa.is_rice_coded(rec, 32) and fs.is_rice_coded(rec, 32)
    for f, v in (("header_state", 1), ("file_type", 2), ("compression", 0), ("bits_per_pixel", 17), ("columns", 0),
                 ("pixels_per_block", 12), ("header_length", 31)):
        bad = rec.copy()
        bad[f] = v
        assert not xa.is_rice_coded(bad, 32) and not fs.is_rice_coded(bad, 32), f


def test_bad_rice_parameters_are_argument_errors():
    """Refused before any device is asked for: XRIT_E_ARG is the existing argument-error code, -1."""
    import xritdemod_amd as xa
    L = xa.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for n, J, S in ((0, 8, 1), (17, 8, 1), (8, 12, 1), (8, 0, 1), (8, 8, 0), (8, 8, 65536)):
        assert L.xrit_rice_decode(p, 64, p, 16, 1, n, J, S, p, p, 0) == -1, (n, J, S)
    for stride in (0, 8, 12, 20):
        assert L.xrit_rice_decode(p, 64, p, stride, 1, 8, 8, 8, p, p, 0) == -1, stride
    assert L.xrit_rice_decode(p, 64, None, 16, 1, 8, 8, 8, p, p, 0) == -1
    assert b"rice" in L.xrit_last_error()
    assert L.xrit_rice_form(3) == -1 and L.xrit_rice_form(-1) == -1
    for form in (1, 2, 0):
        assert L.xrit_rice_form(form) == 0
    assert L.xrit_files_create(None, 0) == -1
    assert L.xrit_files_stats(None, p) == -1 and L.xrit_files_key(None, 0, 0, p) == -1


def test_no_cpu_path():
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:                   # on a GPU box the same calls make working objects (-m gpu tests them)
        xa.FileAssembler().close()
        xa.RiceDecoder(8, 16, 100)
        return
    for make in (lambda: xa.FileAssembler(), lambda: xa.RiceDecoder(8, 16, 100),
                 lambda: xa.RiceDecoder(8, 16, 100).decode(np.zeros(4, np.uint8), np.zeros(1, xa.PACKET_DTYPE))):
        with pytest.raises(xa.XritError) as ei:
            make()
        assert ei.value.code == -2 and "no CPU path" in str(ei.value)
