"""CPU tier: the specification of the carrier acquisition stage (tests/acquire_spec.py) against the synthetic burst, against
the closed form of a pure tone's answer (every 16th bin and the edges within 1e-9 of a bin, the half-way offsets), on input
that is not a signal (silence, NaN, Inf, overflow: a WEAK record, no warning; a NaN where nothing is read: the same bytes), the
oracle chain behind it, and the CPU side of the stage's ABI -- the header declares the functions, the ctypes layer binds
them, the record layouts are the header's field for field, bad arguments are refused before a device is asked for, there is
no CPU path; the plain host parts (csrc/acquire_host.h) in a stand-alone program under the sanitizers, held against a table
recorded from the specification."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import acquire_cases as ac
import acquire_spec as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")
TABLE = os.path.join(ROOT, "tests", "golden", "acquire_host_table.txt")

CTYPES = {"uint64_t": np.uint64, "int64_t": np.int64, "uint32_t": np.uint32, "double": np.float64}


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


FUNCTIONS = ["xrit_acquire_create", "xrit_acquire_destroy", "xrit_acquire_reset", "xrit_acquire_set_frequency",
             "xrit_acquire_estimate_device", "xrit_acquire_mix_device", "xrit_acquire_estimate", "xrit_acquire_mix",
             "xrit_acquire_get_state"]


# ---- the estimate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_estimate_is_within_one_hertz(name):
    c = ac.CASES[name]
    rec = ac.spec_record(name)
    print(f"case {name}: {rec['hz']:.4f} Hz for {c['carrier_hz']} Hz, off by {rec['hz'] - c['carrier_hz']:+.4f}; ratio {rec['ratio']:.1f}, "
          f"{rec['segments']} segments, bin {rec['k0']}")
    assert rec["status"] == sp.OK and rec["segments"] == sp.segments_for(c["n"], c["pre_sum"], ac.segments(name))
    assert abs(rec["hz"] - c["carrier_hz"]) <= 1.0
    assert rec["inc"] == sp.inc_from_nu(rec["nu"]) and rec["applied"] == 0


def test_the_long_cases_are_what_they_are_for():
    """h: int8, the fewest segments; i: int16 behind a pre-sum of 4, with samples to spare; j: int8 behind the largest
    pre-sum, nothing clipped; k: as many segments as a handle takes; l: int8 behind a pre-sum of 4, the samples of a sum
    distinct.  In each the line stands clear of the next bin, so the device has to name the same bin."""
    want = {"h": (sp.S8IQ, 1, 31), "i": (sp.S16IQ, 4, 31), "j": (sp.S8IQ, 64, 31), "k": (sp.FLOATIQ, 1, 4095), "l": (sp.S8IQ, 4, 31)}
    for name, (sample_type, pre_sum, segments) in want.items():
        rec, P = ac.spec_record(name, detail=True)
        assert (ac.sample_type(name), ac.CASES[name]["pre_sum"], int(rec["segments"])) == (sample_type, pre_sum, segments)
        top = np.sort(P)[-2:]
        assert top[1] > 1.5 * top[0], name
    j = ac.samples("j")
    assert int(np.abs(j.astype(np.int64)).max()) == 127 and np.array_equal(j[:128], np.tile(j[:2], 64)) and not np.array_equal(j[:2], j[128:130])
    assert ac.CASES["i"]["n"] % 4 == 3 and ac.CASES["j"]["n"] % 64 == 63
    first = ac.samples("l")[:8:2].astype(np.int64)
    assert len(set(first)) > 1 and np.array_equal(ac.samples("l"), ac.samples("i") >> 8)
    k, a = ac.samples("k"), ac.samples("a")
    assert len(k) == 8 * len(a) and np.array_equal(k[-len(a):], a)


def test_case_d_sits_half_way_between_two_bins():
    c = ac.CASES["d"]
    line = (2 * c["carrier_hz"] / c["fs"] * sp.N) % 1.0
    assert abs(line - 0.5) < 0.01


def test_noise_alone_is_weak():
    for seed in range(4):
        rec = sp.estimate(ac.noise(1 << 17, seed), 1.25e6)
        assert rec["status"] == sp.WEAK and rec["segments"] == 63 and rec["ratio"] < 3.0


def test_too_few_samples_are_too_short():
    x = ac.samples("c")
    assert sp.estimate(x[:65535], 1.25e6)["status"] == sp.TOO_SHORT and sp.estimate(x[:65536], 1.25e6)["status"] == sp.OK
    rec = sp.estimate(x, 1.25e6, pre_sum=2)
    assert rec["status"] == sp.TOO_SHORT and rec["segments"] == 15 and rec["k0"] == 0 and rec["inc"] == 0
    assert sp.estimate(x[:100], 1.25e6)["segments"] == 0
    assert sp.segments_for(65536 * 16 - 1, 16) == 30 and sp.segments_for(65536 * 16, 16) == 31


def test_default_min_ratio_lies_between_noise_and_signal():
    """2.28 over 256 seeds of noise at 31 segments, 34.9 for the weakest signal case at 2 dB."""
    assert 2.28 * 3 < sp.DEFAULT_MIN_RATIO < 34.9 / 3
    assert abs(sp.DEFAULT_MIN_RATIO - (2.28 * 34.9) ** 0.5) < 0.05


# ---- the estimate against a closed form: tones --------------------------------------------------------------------------------
def test_tones_are_what_they_say():
    """The table look-up is np.exp of the same phase to float64's last bits; the pre-summed tone is a tone; the quantised
    forms fill their range without clipping."""
    for k, d16 in ((0, -6), (77, 3), (2048, 0), (4095, 8)):
        want = np.exp(1j * np.pi * (16 * k + d16) * np.arange(65536) / (16 * sp.N))
        assert np.abs(ac.tone(k, d16).astype(np.complex128) - want).max() < 1e-7           # complex64's rounding, and a 2e-11 phase
        x4 = ac.tone(k, d16, 4096, 4).astype(np.complex128)
        assert len(x4) == 4 * 4096
        u = x4.reshape(4096, 4).sum(axis=1)
        z = u * u / (u[0] * u[0])
        assert np.abs(z - np.exp(2j * np.pi * (k + d16 / 16.0) * np.arange(4096) / sp.N)).max() < 1e-5
    x = ac.tone(77, 3)
    s16, s8 = ac.tone_as(x, sp.S16IQ), ac.tone_as(x, sp.S8IQ)
    assert s16.dtype == np.int16 and s8.dtype == np.int8 and len(s16) == len(s8) == 2 * len(x)
    assert 29990 <= int(np.abs(s16.astype(np.int64)).max()) <= 30000 and int(np.abs(s8.astype(np.int64)).max()) == 100
    assert sorted({ac.tone_d16(k) for k in range(sp.N)}) == list(range(-6, 7))
    assert ac.tone_nu(2048, 0) == -0.25 and ac.tone_nu(2047, 8, 4) == (2047.5 / sp.N) / 8 and ac.tone_nu(4095, 8) == -0.5 / sp.N / 2
    assert ac.bins_apart(0.25 - 1e-9, -0.25, circle=True) < 1e-5 and ac.bins_apart(0.25 - 1e-9, -0.25) > 4095


def test_specification_meets_the_closed_form_on_tones():
    """Every 16th bin and the edges, each at its own offset of the schedule: the bin, nu within 1e-9 of a bin of
    wrap((k + d16 / 16) / N) / 2 (measured: 3.0e-11), the ratio within 1e-8 of bin 0's at the same offset (measured: 5.8e-10)."""
    worst_nu = worst_ratio = 0.0
    for k in sorted(set(range(0, sp.N, 16)) | set(ac.TONE_EDGES)):
        d16 = ac.tone_d16(k)
        rec = sp.estimate(ac.tone(k, d16), 1.25e6)
        assert rec["status"] == sp.OK and rec["segments"] == 31 and rec["k0"] == k, (k, d16)
        bins = ac.bins_apart(rec["nu"], ac.tone_nu(k, d16))
        rel = abs(float(rec["ratio"]) / ac.tone_ratio(d16) - 1.0)
        worst_nu, worst_ratio = max(worst_nu, bins), max(worst_ratio, rel)
        assert bins <= 1e-9 and rel <= 1e-8, (k, d16, bins, rel)
        assert rec["inc"] == sp.inc_from_nu(rec["nu"]) and rec["hz"] == rec["nu"] * 1.25e6
    print(f"tones: nu at most {worst_nu:.2e} of a bin from the closed form, ratio at most {worst_ratio:.2e} from bin 0's; "
          f"smallest ratio {min(ac.tone_ratio(d) for d in range(-6, 7)):.0f}")
    # the line on the wrap: either side names it
    rec = sp.estimate(ac.tone(2048, 0), 1.25e6)
    assert rec["status"] == sp.OK and rec["k0"] == 2048 and ac.bins_apart(rec["nu"], ac.tone_nu(2048, 0), circle=True) <= 1e-9


def test_specification_places_a_line_half_way_between_two_bins():
    """The coarse peak only has to be right to a bin: with the line half way the two neighbours' powers agree to 1e-9, either
    may be named, and nu is the closed form's all the same."""
    for k in (0, 77, 2047, 4095):
        for d16 in (-8, 8):
            rec, P = sp.estimate(ac.tone(k, d16), 1.25e6, detail=True)
            top = ac.top_two(P)
            other = (k + (1 if d16 > 0 else -1)) % sp.N
            assert abs(top[1] / top[0] - 1.0) <= 1e-9 and {int(i) for i in np.argsort(P)[-2:]} == {k, other}, (k, d16)
            assert rec["status"] == sp.OK and int(rec["k0"]) in (k, other)
            assert ac.bins_apart(rec["nu"], ac.tone_nu(k, d16), circle=True) <= 1e-9, (k, d16)


# ---- input that is not a signal -------------------------------------------------------------------------------------------------
def same_record(a, b):
    return a.tobytes() == b.tobytes()


def test_silence_and_samples_that_are_not_finite_give_a_weak_record():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # the specification emits none
        rec = sp.estimate(np.zeros(65536, np.complex64), 1.25e6)
        assert rec["status"] == sp.WEAK and rec["segments"] == 31 and rec["k0"] == 0 and rec["nu"] == 0.0 and rec["hz"] == 0.0 and rec["inc"] == 0
        assert np.isnan(rec["ratio"]) and rec["applied"] == 0
        clean = ac.samples("c")
        for bad, at in ((np.nan, 0), (np.nan, 40000), (np.nan, 65535), (np.inf, 12345), (-np.inf, 2048)):
            x = clean.copy()
            x[at] = bad
            rec = sp.estimate(x, 1.25e6)
            assert rec["status"] == sp.WEAK and rec["inc"] == 0 and rec["segments"] == 31, (bad, at)
        big = sp.estimate(clean.astype(np.complex128) * 1e200, 1.25e6)              # squares overflow float64
        assert big["status"] == sp.WEAK and big["inc"] == 0
    a = sp.Acquirer(1.25e6)
    a.set_frequency(1234.5)
    x = clean.copy()
    x[100] = np.nan
    rec = a.estimate(x, apply=True)
    assert rec["applied"] == 0 and a.inc == sp.inc_from_hz(1234.5, 1.25e6) and (a.estimates, a.applied) == (1, 0)


def test_samples_that_are_not_read_do_not_count():
    """The n mod R samples behind the last whole pre-sum, and everything beyond (M + 1) * 2048 * R once `segments` caps M."""
    fs = 5e6
    x = ac.tone(300, 5, 65536, 4)
    want = sp.estimate(x, fs, pre_sum=4)
    tail = np.concatenate([x, np.full(3, np.nan, np.complex64)])
    assert want["status"] == sp.OK and same_record(sp.estimate(tail, fs, pre_sum=4), want)
    tail[4 * 65536 - 1] = np.nan                            # the last sample that is read
    assert sp.estimate(tail, fs, pre_sum=4)["status"] == sp.WEAK
    clean = ac.samples("a")                                 # 2^20 samples, 511 segments
    want = sp.estimate(clean, 1.25e6, max_segments=31)
    x = clean.copy()
    x[32 * 2048:] = np.nan
    assert want["status"] == sp.OK and want["segments"] == 31 and same_record(sp.estimate(x, 1.25e6, max_segments=31), want)
    x[32 * 2048 - 1] = np.nan
    assert sp.estimate(x, 1.25e6, max_segments=31)["status"] == sp.WEAK


# ---- the mix ---------------------------------------------------------------------------------------------------------------
def test_inc_from_hertz_against_integer_arithmetic():
    from fractions import Fraction
    for hz, fs in ((23000.0, 1.25e6), (-181234.5, 1.25e6), (0.0, 1.25e6), (0.49 * 1.25e6, 1.25e6), (-23456.0, 40e6), (1.0, 2.5e6),
                   (-624999.9, 1.25e6)):
        q = np.float64(hz) / np.float64(fs)                        # the one rounding the contract has
        exact = Fraction(float(q)) * (1 << 64)
        want = int(exact) if exact.denominator == 1 else round(exact)      # (round: half to even, as llrint)
        got = sp.inc_from_hz(hz, fs)
        assert got == want and -(1 << 63) <= got < (1 << 63)
        assert abs(Fraction(got, 1 << 64) * Fraction(fs) - Fraction(hz)) < Fraction(1, 10 ** 9)


def test_mix_of_a_stream_is_the_mix_of_its_pieces(oracle_mod):
    x = ac.samples("c")[:20000]
    for hz in (23000.0, 0.49 * 1.25e6):
        inc = sp.inc_from_hz(hz, 1.25e6)
        whole, acc = sp.mix(x, 12345 << 40, inc)
        a = sp.Acquirer(1.25e6)
        a.acc, a.inc = 12345 << 40, inc
        pieces = np.concatenate([a.mix(x[lo:hi]) for lo, hi in ((0, 1), (1, 8), (8, 8), (8, 4104), (4104, 20000))])
        assert np.array_equal(whole.view(np.uint32), pieces.view(np.uint32)) and a.acc == acc == ((12345 << 40) + 20000 * inc) % (1 << 64)


def test_mix_takes_the_carrier_out(oracle_mod):
    n = 4096
    inc = sp.inc_from_hz(23000.0, 1.25e6)
    tone = np.exp(2j * np.pi * 23000.0 / 1.25e6 * np.arange(n)).astype(np.complex64)
    out, _ = sp.mix(tone, 0, inc)
    assert np.abs(out - 1.0).max() < 2e-6                          # float32 through and through; the phase itself is exact
    q = np.clip(np.rint(tone.view(np.float32) * 32767.0), -32768, 32767).astype(np.int16)
    out16, _ = sp.mix(q, 0, inc, sp.S16IQ)
    assert np.abs(out16 - 32767.0 / 32768.0).max() < 1e-4
    with pytest.raises(ValueError):
        sp.mix(np.zeros(4, np.uint8), 0, inc, sp.U8IQ)


# ---- end to end on the oracle ------------------------------------------------------------------------------------------------
def test_oracle_chain_locks_only_behind_the_stage(oracle_mod):
    """LRIT at 1.25 Msps, +23 kHz, 8 dB: unmixed the chain's decisions are noise; estimated on the first 2^18 samples and
    mixed by the specification they are the transmitted symbols."""
    o = oracle_mod
    x = ac.burst()
    raw = o.Demod(o.config("lrit", 1.25e6, 1)).process(x)
    ber_raw = ac.second_half_error_rate(raw)
    a = sp.Acquirer(1.25e6)
    rec = a.estimate(x[:1 << 18], apply=True)
    assert rec["status"] == sp.OK and rec["applied"] == 1 and abs(rec["hz"] - ac.BURST_HZ) < 1.0
    soft = o.Demod(o.config("lrit", 1.25e6, 1)).process(a.mix(x))
    ber = ac.second_half_error_rate(soft)
    print(f"second half decision errors: unmixed {ber_raw:.4f}, behind the stage {ber:.2e} ({len(soft)} symbols; estimate {rec['hz']:.2f} Hz)")
    assert ber_raw > 0.40
    assert ber <= 1e-3


# ---- the ABI on the CPU --------------------------------------------------------------------------------------------------------
def test_symbols_and_layouts():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(xrit_[a-z0-9_]+)\s*\(", src))
    import xritdemod_amd as xa
    from xritdemod_amd import _capi
    L = xa.lib()
    for name in FUNCTIONS:
        assert name in declared and name in _capi._SIGNATURES and hasattr(L, name), name
    for struct, dtype, size in (("xrit_acquire_params", xa.ACQUIRE_PARAMS_DTYPE, 24), ("xrit_acquire_estimate_record", xa.ACQUIRE_RECORD_DTYPE, 64),
                                ("xrit_acquire_state", xa.ACQUIRE_STATE_DTYPE, 40)):
        want, stated = header_struct(text, struct)
        assert stated == size == dtype.itemsize == want.itemsize and dtype == want, struct
    assert xa.ACQUIRE_RECORD_DTYPE == sp.RECORD_DTYPE and xa.ACQUIRE_STATE_DTYPE == sp.STATE_DTYPE
    for i, name in enumerate(("OK", "TOO_SHORT", "WEAK")):
        assert re.search(r"#define XRIT_ACQUIRE_" + name + r"\s+" + str(i) + r"\b", text) and getattr(sp, name) == i == getattr(xa, "ACQUIRE_" + name)
    assert "demodulator.cpp:285-290" in text and ":461" in text and "demodulator.cpp:54-74" in text
    assert "sample_rate / (4 * pre_sum)" in text
    assert f"({sp.DEFAULT_MIN_RATIO})" in text          # the default the header states is the specification's


def test_bad_arguments_are_refused_before_a_device_is_asked_for():
    import xritdemod_amd as xa
    L = xa.lib()
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()

    def params(*v):
        a = np.zeros(1, xa.ACQUIRE_PARAMS_DTYPE)
        a[0] = v
        return a
    good = params(1.25e6, 0, 0, 0.0)
    assert L.xrit_acquire_create(None, good.ctypes.data_as(C.c_void_p), 0) == -1
    assert L.xrit_acquire_create(C.byref(h), None, 0) == -1 and not h.value
    for bad in ((0.0, 1, 511, 0.0), (-1.0, 1, 511, 0.0), (float("nan"), 1, 511, 0.0), (1.25e6, 65, 511, 0.0), (1.25e6, 1, 30, 0.0),
                (1.25e6, 1, 4096, 0.0), (1.25e6, 1, 511, -1.0), (1.25e6, 1, 511, float("inf"))):
        a = params(*bad)
        assert L.xrit_acquire_create(C.byref(h), a.ctypes.data_as(C.c_void_p), 0) == -1 and not h.value, bad
    assert L.xrit_acquire_reset(None) == -1 and L.xrit_acquire_set_frequency(None, 0.0) == -1 and L.xrit_acquire_get_state(None, p) == -1
    assert L.xrit_acquire_estimate(None, p, 0, 0, 0, p) == -1 and L.xrit_acquire_mix(None, p, 0, 0, p) == -1
    assert L.xrit_acquire_estimate_device(None, p, 0, 0, 0, p, None) == -1 and L.xrit_acquire_mix_device(None, p, 0, 0, p, None) == -1
    assert L.xrit_acquire_destroy(None) == 0


def test_no_cpu_path():
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:                   # on a GPU box the same call makes a working object (-m gpu tests it)
        xa.CarrierAcquirer(1.25e6).close()
        return
    with pytest.raises(xa.XritError) as ei:
        xa.CarrierAcquirer(1.25e6)
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


def test_host_program_refuses_what_the_stage_cannot_take():
    host_bin = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
    for extra in (["--acquire", "--gpus", "2"], ["--tune", "100", "--gpus", "2"], ["--acquire", "--format", "u8"],
                  ["--acquire", "--acquire-presum", "65"], ["--tune"]):
        r = subprocess.run([host_bin, "--input", "x.cf32", "--sink", "null"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "usage:" in r.stderr, extra


# ---- the plain host parts ------------------------------------------------------------------------------------------------------
def recorded_table():
    """What the host check replays, as the specification decides it."""
    rows = []
    for fs, r, m, ratio in ((1.25e6, 0, 0, 0.0), (1.25e6, 1, 511, 8.9), (40e6, 16, 31, 3.5), (2.5e6, 64, 4095, 100.0), (1.25e6, 65, 511, 0.0),
                            (1.25e6, 1, 30, 0.0), (1.25e6, 1, 4096, 0.0), (0.0, 1, 511, 0.0), (-2.0, 0, 0, 0.0), (1.25e6, 0, 0, -1.0)):
        got = sp.resolve_params(fs, r, m, ratio)
        rows.append(["P", float(fs).hex(), r, m, float(ratio).hex()] + ([1, got[0], got[1], float(got[2]).hex()] if got else [0, 0, 0, float(0).hex()]))
    for hz, fs in ((23000.0, 1.25e6), (-181234.5, 1.25e6), (0.0, 1.25e6), (0.49 * 1.25e6, 1.25e6), (-23456.0, 40e6), (77777.0, 2.5e6),
                   (-381.8, 1.25e6), (624999.999, 1.25e6), (-624999.999, 1.25e6), (1e-3, 40e6)):
        rows.append(["I", float(hz).hex(), float(fs).hex(), 1, sp.inc_from_hz(hz, fs)])
    for hz, fs in ((625000.0, 1.25e6), (-625000.0, 1.25e6), (1e9, 1.25e6), (float("nan"), 1.25e6)):
        rows.append(["I", float(hz).hex(), float(fs).hex(), 0, 0])
    for n in (0, 1, 4095, 4096, 6143, 6144, 65535, 65536, 65537, 100003, 1 << 17, 1 << 20, (1 << 20) - 1, 1 << 21, 600000, 1 << 23, 1 << 28, 1 << 33):
        for r, m in ((1, 511), (16, 511), (3, 31), (64, 4095), (1, 4095)):
            rows.append(["M", n, r, m, sp.segments_for(n, r, m)])
    for m in (0, 1, 30, 31, 63, 511, 4095):
        rows.append(["S", m, *sp.scratch_bytes(m)])
    for t, b in ((0, 8), (1, 4), (2, 2), (3, 0), (4, 0), (-1, 0)):
        rows.append(["T", t, b])
    return rows


def test_recorded_table_is_the_specification_s():
    want = "\n".join(" ".join(str(x) for x in row) for row in recorded_table()) + "\n"
    assert open(TABLE).read() == want
    kinds = [ln.split()[0] for ln in want.splitlines()]
    assert {k: kinds.count(k) for k in "PIMST"} == {"P": 10, "I": 14, "M": 90, "S": 7, "T": 6}


def test_acquire_host_check_under_sanitizers(tmp_path):
    """make acquire-host-check: the functions of csrc/acquire_host.h that acquire.cpp and the kernels' launch code call, over
    the recorded table in a stand-alone g++ program with -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "acquire-host-check",
                        f"ACQUIRE_CHECK={tmp_path / 'acquire_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    n = len(open(TABLE).read().splitlines())
    assert f"acquire_host_check: {n} rows, the parameters, the phase steps, the segments and the sizes of each: ok" in r.stdout, r.stdout
