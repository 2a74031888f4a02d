"""ctypes binding to libaec and its SZIP-compatible libsz: the outside reference that tests/rice_spec.py is held against
(test infrastructure, CPU only).  `struct aec_stream` and `SZ_com_t` are written from the
installed libaec.h and szlib.h of libaec 1.0.4.

The libraries are looked for with ctypes.util.find_library and in the lib directories of the prefixes this Python and
its environment name (sys.prefix and its kin, CONDA_PREFIX, the prefix of an `aec` program on PATH, the customary roots
of a conda installation), and loaded with a plain dlopen.  Where they are missing, available() is False and the tests
that need the live library skip; the GPU tier reads only the fixture made with them (tests/golden/rice_libaec_lines.npz)."""
import ctypes as C
import ctypes.util
import glob
import os
import shutil
import sys

import numpy as np

AEC_DATA_MSB, AEC_DATA_PREPROCESS = 4, 8
AEC_OK, AEC_CONF_ERROR, AEC_STREAM_ERROR, AEC_DATA_ERROR, AEC_MEM_ERROR = 0, -1, -2, -3, -4
FLAGS = AEC_DATA_MSB | AEC_DATA_PREPROCESS
MAX_RSI = 4096                    # libaec's limit on the blocks of a reference-sample interval
SLACK = 8                         # the fewest zero bytes behind a line handed to the decoder (see decode)

SZ_ALLOW_K13, SZ_CHIP, SZ_EC, SZ_LSB, SZ_MSB, SZ_NN, SZ_RAW = 1, 2, 4, 8, 16, 32, 128
SZ_GOES = SZ_ALLOW_K13 | SZ_MSB | SZ_NN                        # 49: what the rice header of a GOES file carries


class aec_stream(C.Structure):
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_size_t), ("total_in", C.c_size_t),
                ("next_out", C.c_void_p), ("avail_out", C.c_size_t), ("total_out", C.c_size_t),
                ("bits_per_sample", C.c_uint), ("block_size", C.c_uint), ("rsi", C.c_uint), ("flags", C.c_uint),
                ("state", C.c_void_p)]


class SZ_com_t(C.Structure):
    _fields_ = [("options_mask", C.c_int), ("bits_per_pixel", C.c_int), ("pixels_per_block", C.c_int),
                ("pixels_per_scanline", C.c_int)]


def _lib_dirs():
    prefixes = [sys.prefix, sys.base_prefix, sys.exec_prefix, os.environ.get("CONDA_PREFIX")]
    tool = shutil.which("aec")
    if tool:
        prefixes.append(os.path.dirname(os.path.dirname(os.path.realpath(tool))))
    home = os.path.expanduser("~")
    prefixes += [os.path.join(root, name) for root in ("/opt", home) for name in ("conda", "miniconda3", "anaconda3", "miniforge3")]
    seen = []
    for p in prefixes:
        d = os.path.join(p, "lib") if p else None
        if d and d not in seen and os.path.isdir(d):
            seen.append(d)
    return seen


def _load(name):
    found = ctypes.util.find_library(name)
    names = [found] if found else []
    for d in _lib_dirs():
        names += sorted(glob.glob(os.path.join(d, "lib%s.so*" % name)) + glob.glob(os.path.join(d, "lib%s*.dylib" % name)))
    for cand in names:
        try:
            return C.CDLL(cand)
        except OSError:
            pass
    return None


_libs = None


def _get():
    global _libs
    if _libs is None:
        aec, sz = _load("aec"), _load("sz")
        if aec is not None:
            for f in (aec.aec_buffer_encode, aec.aec_buffer_decode):
                f.argtypes, f.restype = [C.POINTER(aec_stream)], C.c_int
        if sz is not None:
            sz.SZ_BufftoBuffCompress.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t, C.POINTER(SZ_com_t)]
            sz.SZ_BufftoBuffCompress.restype = C.c_int
        _libs = (aec, sz)
    return _libs


def available():
    """True when both libaec and libsz load."""
    return all(lib is not None for lib in _get())


def sample_dtype(n):
    """One byte a sample for n <= 8, else two, big-endian (AEC_DATA_MSB)."""
    return np.dtype("u1") if n <= 8 else np.dtype(">u2")


def _rsi(S, J, rsi):
    rsi = -(-S // J) if rsi is None else rsi
    if not 1 <= rsi <= MAX_RSI:
        raise ValueError("rsi %d is outside libaec's 1 .. %d" % (rsi, MAX_RSI))
    return rsi


def encode(x, n, J, rsi=None):
    """A line of samples -> bytes: one reference-sample interval of rsi = ceil(S / J) blocks, MSB | PREPROCESS.  libaec
    pads the last block itself."""
    a = np.ascontiguousarray(np.asarray(x).astype(sample_dtype(n)))
    out = np.zeros(2 * a.nbytes + 4096, np.uint8)
    s = aec_stream(a.ctypes.data, a.nbytes, 0, out.ctypes.data, out.nbytes, 0, n, J, _rsi(len(a), J, rsi), FLAGS, None)
    rc = _get()[0].aec_buffer_encode(C.byref(s))
    if rc != AEC_OK:
        raise RuntimeError("aec_buffer_encode: %d" % rc)
    return out[:s.total_out].tobytes()


def decode(data, n, J, S, rsi=None, slack=None):
    """-> (rc, samples (S,) int64, samples written).

    The line is always followed by zero bytes that are counted in avail_in -- a block of raw samples and 64 more, never
    fewer than 8.  Handed exactly the line's bytes, libaec 1.0.4 returns AEC_OK with a wrong last sample when the line
    ends in a long fundamental-sequence code (seen on rice_spec's FORCED_LOW_K cases (8, 64, 192, 0) and
    (12, 16, 48, 0)), and AEC_DATA_ERROR on the hand-made long-code lines; with 8 bytes behind the line it still
    returns AEC_DATA_ERROR on rice_spec.chunk_edge_lines and on two FORCED_LOW_K cases of 16 bits, with 16 bytes on none
    of them.  tests/test_rice_libaec.py holds all those lines against it.  A line that is in truth cut short shows as
    fewer samples written or as an error."""
    slack = max(SLACK, J * n // 8 + 64 if slack is None else int(slack))
    a = np.frombuffer(bytes(data) + bytes(slack), np.uint8)
    out = np.zeros(S, sample_dtype(n))
    s = aec_stream(a.ctypes.data, a.nbytes, 0, out.ctypes.data, out.nbytes, 0, n, J, _rsi(S, J, rsi), FLAGS, None)
    rc = _get()[0].aec_buffer_decode(C.byref(s))
    return rc, out.astype(np.int64), int(s.total_out) // out.itemsize


def sz_encode(x, n, J, mask):
    """One scanline through SZ_BufftoBuffCompress, pixels_per_scanline = len(x) -> bytes.  The samples go in as the mask
    says: big-endian under SZ_MSB, else little-endian."""
    dt = np.dtype("u1") if n <= 8 else np.dtype(">u2" if mask & SZ_MSB else "<u2")
    a = np.ascontiguousarray(np.asarray(x).astype(dt))
    out = np.zeros(2 * a.nbytes + 4096, np.uint8)
    length = C.c_size_t(out.nbytes)
    p = SZ_com_t(mask, n, J, len(a))
    rc = _get()[1].SZ_BufftoBuffCompress(out.ctypes.data, C.byref(length), a.ctypes.data, a.nbytes, C.byref(p))
    if rc != AEC_OK:
        raise RuntimeError("SZ_BufftoBuffCompress: %d" % rc)
    return out[:length.value].tobytes()
