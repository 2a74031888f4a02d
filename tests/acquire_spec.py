"""The NumPy specification of the carrier acquisition stage (include/xritdemod_amd.h, "Carrier acquisition"; DESIGN.md
section 21): the estimate in float64, the mix in float32 exactly as the contract states it.

estimate   the carrier offset of a block of input samples from the spectral line of the squared signal: BPSK squared has
           a line at twice the carrier.  Welch segments of N = 4096 points at a hop of N/2 find the line's bin; the phase
           step of that bin from one segment to the next (half a segment apart, so unambiguous over +-1 bin) places the
           line inside the bin.
mix        derotation by an oscillator whose phase is a 64-bit integer: the output does not depend on how a stream is
           cut into calls.
"""
import numpy as np

import oracle

N = 4096
HOP = N // 2
MIN_SEGMENTS = 31
DEFAULT_SEGMENTS = 511
# the geometric mean of the largest ratio of noise alone (2.28, 256 seeds at M = 31) and the
# smallest of the signal cases at Es/N0 = 2 dB (34.9, case f); csrc/acquire_host.h states the same number
DEFAULT_MIN_RATIO = 8.9
OK, TOO_SHORT, WEAK = 0, 1, 2
FLOATIQ, S16IQ, S8IQ, U8IQ = 0, 1, 2, 3

RECORD_DTYPE = np.dtype([("status", np.uint32), ("k0", np.uint32), ("segments", np.uint32), ("reserved0", np.uint32),
                         ("ratio", np.float64), ("nu", np.float64), ("hz", np.float64), ("inc", np.int64),
                         ("applied", np.uint32), ("reserved", np.uint32, (3,))])
assert RECORD_DTYPE.itemsize == 64
STATE_DTYPE = np.dtype([("acc", np.uint64), ("inc", np.int64), ("samples_mixed", np.uint64), ("estimates", np.uint64),
                        ("applied", np.uint64)])
assert STATE_DTYPE.itemsize == 40

K = np.float32(np.pi * 2.0 ** -31)
MASK64 = (1 << 64) - 1


def to_complex(samples, sample_type=FLOATIQ, dtype=np.complex64):
    """The conversion of onSamplesAvailable (demodulator.cpp:54-74): cf32 as is, int16 * 2^-15, int8 * 2^-7."""
    if sample_type == FLOATIQ:
        return np.ascontiguousarray(samples, np.complex64).astype(dtype)
    if sample_type == S16IQ:
        v = np.ascontiguousarray(samples, np.int16).astype(np.float32) * np.float32(2.0 ** -15)
    elif sample_type == S8IQ:
        v = np.ascontiguousarray(samples, np.int8).astype(np.float32) * np.float32(2.0 ** -7)
    else:
        raise ValueError("the acquisition stage refuses XRIT_SAMPLE_U8IQ: its DC tracker belongs to the chain's ingest")
    return v.view(np.complex64).astype(dtype)


def segments_for(n, pre_sum=1, max_segments=DEFAULT_SEGMENTS):
    """M = min(M_max, floor(floor(n / R) / 2048) - 1), not below 0."""
    return max(0, min(max_segments, (n // pre_sum) // HOP - 1))


def resolve_params(sample_rate, pre_sum=0, segments=0, min_ratio=0.0):
    """The create-time parameters with 0 replaced by the defaults, or None where the stage refuses them."""
    pre_sum = pre_sum or 1
    segments = segments or DEFAULT_SEGMENTS
    min_ratio = min_ratio or DEFAULT_MIN_RATIO
    ok = (np.isfinite(sample_rate) and sample_rate > 0 and pre_sum <= 64 and MIN_SEGMENTS <= segments <= 4095
          and np.isfinite(min_ratio) and min_ratio > 0)
    return (pre_sum, segments, min_ratio) if ok else None


def scratch_bytes(segments):
    """(the spectra of an estimate of M segments, the power row): float pairs and doubles."""
    return max(segments, 1) * N * 8, N * 8


def inc_from_nu(nu):
    """rint(ldexp(nu, 64)) as a Python integer (nu a float64, |nu| < 1/2)."""
    return int(np.rint(np.ldexp(np.float64(nu), 64)))


def inc_from_hz(hz, sample_rate):
    """llrint(ldexp(hz / sample_rate, 64))"""
    return inc_from_nu(np.float64(hz) / np.float64(sample_rate))


def estimate(x, sample_rate, pre_sum=1, max_segments=DEFAULT_SEGMENTS, min_ratio=DEFAULT_MIN_RATIO, detail=False):
    """x: complex samples (any complex dtype; taken to float64).  -> a RECORD_DTYPE scalar record (applied 0); with
    detail also P, the summed power rows.  Only the first (M + 1) * 2048 * R samples are read.  Silence and a sample that is
    not finite among them give a record like any other input: the ratio is NaN, so the status is WEAK, and a nu that is
    not finite gives inc 0."""
    x = np.asarray(x, np.complex128)
    R = int(pre_sum)
    rec = np.zeros(1, RECORD_DTYPE)[0]
    M = segments_for(len(x), R, max_segments)
    rec["segments"] = M
    if M < MIN_SEGMENTS:
        rec["status"] = TOO_SHORT
        return (rec, None) if detail else rec
    nz = (M + 1) * HOP
    with np.errstate(all="ignore"):         # silence (0 / 0) and samples that are not finite give a record, not a warning
        u = x[:nz * R].reshape(nz, R).sum(axis=1)
        z = u * u
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
        P = np.zeros(N)
        X = np.empty((M, N), np.complex128)
        for s in range(M):
            X[s] = np.fft.fft(z[s * HOP:s * HOP + N] * w)
            P += np.abs(X[s]) ** 2
        k0 = int(np.argmax(P))
        col = X[:, k0]
        C = np.sum(col[1:] * np.conj(col[:-1]))
        if k0 & 1:
            C = -C
        d = np.arctan2(C.imag, C.real)
        nu2 = k0 / N + d / (np.pi * N)
        nu2 -= np.floor(nu2 + 0.5)
        nu = nu2 / (2 * R)
        rec["k0"] = k0
        rec["ratio"] = P[k0] / np.mean(P)
        rec["nu"] = nu
        rec["hz"] = nu * sample_rate
    rec["inc"] = inc_from_nu(nu) if np.isfinite(nu) else 0          # the device's nu == nu ? ... : 0
    rec["status"] = OK if rec["ratio"] >= min_ratio else WEAK       # (a ratio that is NaN is WEAK)
    return (rec, P) if detail else rec


def mix(samples, acc, inc, sample_type=FLOATIQ):
    """-> (cf32 output, acc after the call).  acc: Python integer mod 2^64; inc: Python integer (int64)."""
    x = to_complex(samples, sample_type)
    n = len(x)
    a = (np.uint64(acc & MASK64) + np.arange(n, dtype=np.uint64) * np.uint64(inc & MASK64))       # wraps mod 2^64
    h = (a >> np.uint64(32)).astype(np.uint32).view(np.int32)
    theta = h.astype(np.float32) * K
    s, c = oracle.sincosf(theta)
    xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
    out = np.empty(n, np.complex64)
    out.real = xr * c + xi * s
    out.imag = xi * c - xr * s
    return out, (acc + n * inc) & MASK64


class Acquirer:
    """The stage's carried state in the specification's terms."""

    def __init__(self, sample_rate, pre_sum=1, segments=DEFAULT_SEGMENTS, min_ratio=DEFAULT_MIN_RATIO):
        self.sample_rate, self.pre_sum, self.segments, self.min_ratio = float(sample_rate), pre_sum, segments, min_ratio
        self.acc, self.inc = 0, 0
        self.estimates, self.applied = 0, 0

    def set_frequency(self, hz):
        self.inc = inc_from_hz(hz, self.sample_rate)

    def estimate(self, samples, sample_type=FLOATIQ, apply=False):
        return self.take(estimate(to_complex(samples, sample_type, np.complex128), self.sample_rate, self.pre_sum, self.segments,
                                  self.min_ratio), apply)

    def take(self, rec, apply=False):
        """What an estimate does to the state once its record (made with this object's parameters, applied 0) is known."""
        rec = rec.copy()
        self.estimates += 1
        if apply and rec["status"] == OK:
            self.inc = int(rec["inc"])
            self.applied += 1
            rec["applied"] = 1
        return rec

    def mix(self, samples, sample_type=FLOATIQ):
        out, self.acc = mix(samples, self.acc, self.inc, sample_type)
        return out
