"""The cases the carrier acquisition tests share (tests/test_acquire_spec.py on the CPU, tests/test_gpu_acquire.py on the
device): the synthetic bursts of the estimate, the burst of the end-to-end check, and how its decisions are counted.  Every
burst and every record of the specification is made once per process."""
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
