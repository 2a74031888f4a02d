"""The cases the carrier acquisition tests share (tests/test_acquire_spec.py on the CPU, tests/test_gpu_acquire.py on the
device): the synthetic bursts of the estimate, pure tones with a closed form for the answer, the burst of the end-to-end
check, and how its decisions are counted.  Every burst and every record of the specification is made once per process."""
import numpy as np

import acquire_spec as sp
import synth

# fs, signal, carrier_hz, Es/N0, n, R
CASES = {
    "a": dict(fs=1.25e6, carrier_hz=23000.0, esn0_db=12.0, n=1 << 20, pre_sum=1),
    "b": dict(fs=1.25e6, carrier_hz=-181234.5, esn0_db=3.0, n=1 << 20, pre_sum=1),
    "c": dict(fs=1.25e6, carrier_hz=23000.0, esn0_db=2.0, n=1 << 16, pre_sum=1),
    "d": dict(fs=1.25e6, carrier_hz=-381.8, esn0_db=3.0, n=1 << 17, pre_sum=1),            # half way between two bins
    "e": dict(fs=2.5e6, carrier_hz=77777.0, esn0_db=4.0, n=1 << 18, pre_sum=1, symbol_rate=927000.0, alpha=0.3),
    "f": dict(fs=40e6, carrier_hz=-23456.0, esn0_db=3.0, n=1 << 21, pre_sum=16),
    "g": dict(fs=1.25e6, carrier_hz=40000.0, esn0_db=5.0, n=1 << 17, pre_sum=1, s16=True),
    # what the tests above leave out of the device's estimate: int8 input, a pre-sum over int8 and int16 loads, 4095 segments
    "h": dict(fs=1.25e6, carrier_hz=-52000.0, esn0_db=6.0, n=1 << 16, pre_sum=1, s8=True),               # 31 segments, the fewest
    "i": dict(fs=5e6, carrier_hz=31000.0, esn0_db=4.0, n=4 * 65536 + 3, pre_sum=4, s16=True),
    "j": dict(fs=80e6, carrier_hz=23000.0, esn0_db=2.0, n=64 * 65536 + 63, pre_sum=64, s8=True, held="c"),   # c, every sample 64 times
    "k": dict(fs=1.25e6, carrier_hz=23000.0, esn0_db=12.0, n=1 << 23, pre_sum=1, segments=4095, tiled="a"),  # a, eight times over
    # j's held samples make every partial pre-sum a multiple of the whole one, which the estimate cannot tell apart: i's int16
    # samples cut to their high bytes are a pre-sum over int8 loads of distinct values
    "l": dict(fs=5e6, carrier_hz=31000.0, esn0_db=4.0, n=4 * 65536 + 3, pre_sum=4, s8=True, high_bytes="i"),
}
_SAMPLES, _RECORDS = {}, {}


def sample_type(name):
    return sp.S16IQ if CASES[name].get("s16") else sp.S8IQ if CASES[name].get("s8") else sp.FLOATIQ


def segments(name):
    """The most segments the case's handle takes."""
    return CASES[name].get("segments", sp.DEFAULT_SEGMENTS)


def samples(name):
    """The case's input as the stage takes it: complex64, or interleaved int16 or int8 for the quantised cases.  The long
    cases are made from the short ones' bursts (every sample held 64 times and scaled to int8's range without clipping; the
    burst repeated: its carrier's phase jumps where the copies meet, the line stays where it is), not generated anew."""
    if name not in _SAMPLES:
        c = CASES[name]
        if "held" in c:
            base = samples(c["held"])
            x = np.repeat(base, c["n"] // len(base))
            x = np.concatenate([x, x[:c["n"] - len(x)]])            # (the samples beyond the last whole pre-sum are not read)
            x = np.rint(x.view(np.float32) * (127.0 / float(np.abs(base.view(np.float32)).max()))).astype(np.int8)
        elif "tiled" in c:
            base = samples(c["tiled"])
            x = np.tile(base, c["n"] // len(base))
        elif "high_bytes" in c:
            x = (samples(c["high_bytes"]) >> 8).astype(np.int8)
        else:
            kw = dict(fs_in=c["fs"], carrier_hz=c["carrier_hz"], esn0_db=c["esn0_db"])
            if "symbol_rate" in c:
                kw.update(symbol_rate=c["symbol_rate"], alpha=c["alpha"])
            x = synth.generate(synth.SynthParams(**kw), c["n"])
        if c.get("s16"):
            x = np.clip(np.rint(x.view(np.float32) * 32768.0), -32768, 32767).astype(np.int16)
        elif c.get("s8") and "held" not in c and "high_bytes" not in c:
            x = np.clip(np.rint(x.view(np.float32) * 128.0), -128, 127).astype(np.int8)
        assert len(x) == c["n"] * (1 if sample_type(name) == sp.FLOATIQ else 2)
        x.setflags(write=False)
        _SAMPLES[name] = x
    return _SAMPLES[name]


def spec_record(name, detail=False):
    """The specification's record of the case at its parameters, the default min_ratio (and its power row)."""
    if name not in _RECORDS:
        c = CASES[name]
        _RECORDS[name] = sp.estimate(sp.to_complex(samples(name), sample_type(name), np.complex128), c["fs"], c["pre_sum"],
                                     segments(name), detail=True)
    return _RECORDS[name] if detail else _RECORDS[name][0]


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.1).astype(np.complex64)


def longer(name, n):
    """The case's burst carried on to n samples, in the case's sample type (the generator is counter based: the first
    samples are the case's own).  For the plain cases only."""
    c = CASES[name]
    assert not {"held", "tiled", "high_bytes", "symbol_rate"} & set(c)
    x = synth.generate(synth.SynthParams(fs_in=c["fs"], carrier_hz=c["carrier_hz"], esn0_db=c["esn0_db"]), n)
    if c.get("s16"):
        x = np.clip(np.rint(x.view(np.float32) * 32768.0), -32768, 32767).astype(np.int16)
    elif c.get("s8"):
        x = np.clip(np.rint(x.view(np.float32) * 128.0), -128, 127).astype(np.int8)
    return x


# ---- tones: a pure line at a chosen place, with a closed form for the answer ---------------------------------------------------
_TABLE, _TONE_RATIO = [], {}
TONE_EDGES = (0, 1, 2047, 2048, 2049, 4095)


def tone(k, d16, n=65536, pre_sum=1):
    """n * pre_sum complex64 samples whose pre-summed square is a pure line at bin k + d16 / 16 of the N-point spectrum:
    x[j] = exp(i pi (16 k + d16) j / (16 N R)).  For R = 1 the samples are looked up in a float64 table of the 32 N values
    exp(i pi m / (16 N)) at the integer (j (16 k + d16)) mod 32 N, so no phase is ever rounded; for R > 1 sample m R + r is
    the table's value for m times exp(i pi (16 k + d16) r / (16 N R)), one float64 product."""
    if not _TABLE:
        _TABLE.append(np.exp(1j * np.pi * np.arange(32 * sp.N) / (16 * sp.N)))
    f = 16 * int(k) + int(d16)
    x = _TABLE[0][(np.arange(n, dtype=np.int64) * f) % (32 * sp.N)]
    if pre_sum > 1:
        x = (x[:, None] * np.exp(1j * np.pi * f * np.arange(pre_sum) / (16 * sp.N * pre_sum))[None, :]).reshape(-1)
    return x.astype(np.complex64)


def tone_as(x, sample_type):
    """A tone in the given sample type: cf32 as is, int16 scaled to 30000, int8 to 100, rounded (interleaved)."""
    if sample_type == sp.FLOATIQ:
        return x
    scale, dt = (30000.0, np.int16) if sample_type == sp.S16IQ else (100.0, np.int8)
    return np.rint(x.view(np.float32) * np.float32(scale)).astype(dt)


def tone_d16(k):
    """The schedule that gives every bin an offset of its own: -6 .. 6 sixteenths, so the line's bin is k without doubt."""
    return (37 * int(k)) % 13 - 6


def tone_nu(k, d16, pre_sum=1):
    """The closed form of the answer: wrap((k + d16 / 16) / N) / (2 R), wrap to [-1/2, 1/2)."""
    nu2 = (k + d16 / 16.0) / sp.N
    return (nu2 - np.floor(nu2 + 0.5)) / (2 * pre_sum)


def bins_apart(nu_a, nu_b, pre_sum=1, circle=False):
    """|nu_a - nu_b| in bins of 1 / (2 N R); on the circle the distance modulo N bins (a line on the wrap at bin 2048 may be
    named from either side)."""
    d = (float(nu_a) - float(nu_b)) * 2 * sp.N * pre_sum
    if circle:
        d -= sp.N * np.rint(d / sp.N)
    return abs(d)


def tone_ratio(d16):
    """The specification's ratio for a tone of 65 536 samples d16 sixteenths off a bin: that of bin 0, since the spectrum
    of a shifted tone is the same spectrum shifted (tests/test_acquire_spec.py holds that to 1e-8)."""
    if d16 not in _TONE_RATIO:
        _TONE_RATIO[d16] = float(sp.estimate(tone(0, d16), 1.25e6)["ratio"])
    return _TONE_RATIO[d16]


def top_two(P):
    """The two largest powers of a row, the smaller first."""
    return np.sort(P)[-2:]


# ---- end to end: LRIT at 1.25 Msps, +23 kHz, 8 dB, 600 000 samples -----------------------------------------------------------
BURST_HZ = 23000.0
BURST_N = 600000
BURST_PARAMS = synth.SynthParams(fs_in=1.25e6, carrier_hz=BURST_HZ, esn0_db=8.0)
_BURST = []


def burst():
    if not _BURST:
        x = synth.generate(BURST_PARAMS, BURST_N)
        x.setflags(write=False)
        _BURST.append(x)
    return _BURST[0]


def second_half_error_rate(soft, span=128):
    """The share of the second half's hard decisions that differ from the transmitted symbols, the best over the
    alignment (+-span symbols) and the polarity (a Costas loop locks at 0 or 180 degrees)."""
    soft = np.asarray(soft)
    lo = len(soft) // 2
    d = np.where(soft[lo:] >= 0, 1.0, -1.0)
    tx = synth.transmitted_symbols(BURST_PARAMS, lo - span, len(d) + 2 * span)
    best = 1.0
    for lag in range(2 * span + 1):
        e = float(np.mean(d != tx[lag:lag + len(d)]))
        best = min(best, e, 1.0 - e)
    return best
