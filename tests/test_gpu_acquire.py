"""GPU tier: the carrier acquisition stage (xrit_acquire_*, CarrierAcquirer) against the specification of
tests/acquire_spec.py -- the mix bit for bit (every sample type, the sizes around the 16-byte groups, in place, a stream cut
into calls, a retune between calls, source offsets that take the one-by-one kernel, a call longer than the wide kernel's
grid covers in one trip), the estimate on the cases of tests/acquire_cases.py (cf32, int16 and int8, pre-sums of 1, 4, 16
and 64, 31 to 4095 segments), what `apply` does, the stage in front of the chain on one stream, the host forms, and
xrit_demod_host --acquire from IQ to a locked decoder.  Where the cases do not reach, tones (acquire_cases.tone, with a
closed form for nu that tests/test_acquire_spec.py ties to the specification within 1e-9 of a bin): a line in every one of
the 4096 bins, offsets of -8 .. 8 sixteenths at the spectrum's ends and at the wrap, every sample type with pre-sums of 1,
4 and 64 and samples to spare behind the last whole pre-sum; 31 .. 130 segments, around the finish kernel's second and
third trip; silence, NaN, Inf, squares that overflow, a NaN where nothing is read, int8's corner as a DC line; seven
estimates queued on one handle with no wait between them.

The bounds: nu within 1e-6 of a bin of 1 / (2 N R), ratio within 1e-4 relative, k0 equal whenever the specification's two
largest powers differ by more than 1 %, inc and hz the contract's functions of the device's own nu.

The estimate's distance from the specification, |nu_dev - nu_spec| in bins, measured on an MI355X: on the cases at most
4.3e-10 (a 2.0e-11, b 3.2e-11, c 2.6e-10, d 2.3e-10, e 5.3e-11, f 7.9e-11, g 1.1e-10, h 3.8e-10, i 4.3e-10, j 2.9e-10,
k 6.9e-12, l 6.6e-11).  The largest each of the other tests measured, nu in bins / ratio relative: a line in every bin
1.1e-9 / 6.7e-8 (against the closed form and bin 0's ratio); offsets across a bin 1.1e-9 / 6.5e-8; tones of every sample
type and pre-sum 1.5e-9 / 7.8e-8 (both int16 at a pre-sum of 1; cf32 1.1e-9, int8 1.4e-9); segment counts around the wave
3.8e-10 / 2.1e-8; the int8 DC line 0 / 2.2e-15."""
import os
import subprocess

import numpy as np
import pytest

import acquire_cases as ac
import acquire_spec as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 1.25e6
FREQUENCIES = {"23k": 23000.0, "-181k": -181234.5, "zero": 0.0, "0.49fs": 0.49 * FS}      # at 0.49 fs acc wraps every other sample
SIZES = (0, 1, 63, 64, 65, 4097, 100003)


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def hand_memory_back(torch):
    """The tests after these run on the same device: every test here returns what it cached."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def up(torch, a, lead=0):
    """The array's bytes in device memory behind `lead` bytes of padding: (the tensor, the pointer to the bytes)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), raw])).to("cuda:0")
    return t, t.data_ptr() + lead


def down(torch, t, dtype, count, lead=0):
    torch.cuda.synchronize()
    return t.cpu().numpy()[lead:lead + count * np.dtype(dtype).itemsize].view(dtype).copy()


def typed_input(x, sample_type):
    """A cf32 burst as the given sample type (scaled into range, quantised)."""
    if sample_type == sp.FLOATIQ:
        return np.ascontiguousarray(x, np.complex64)
    scale, dt = ((32768.0, np.int16) if sample_type == sp.S16IQ else (128.0, np.int8))
    v = np.rint(np.ascontiguousarray(x, np.complex64).view(np.float32) * 4.0 * scale)
    return np.clip(v, -scale, scale - 1).astype(dt)


def n_samples(a, sample_type):
    return len(a) if sample_type == sp.FLOATIQ else len(a) // 2


def cut(a, sample_type, lo, hi):
    return a[lo:hi] if sample_type == sp.FLOATIQ else a[2 * lo:2 * hi]


def device_mix(xa, torch, aq, a, sample_type, lead_in=0, lead_out=0, in_place=False):
    n = n_samples(a, sample_type)
    t_in, p_in = up(torch, a, lead_in)
    if in_place:
        t_out, p_out = t_in, p_in
    else:
        t_out = torch.full((lead_out + 8 * n + 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
        p_out = t_out.data_ptr() + lead_out
    aq.mix_device(p_in, n, sample_type, p_out)
    out = down(torch, t_out, np.complex64, n, lead_in if in_place else lead_out)
    if not in_place:            # nothing beyond the n samples is written
        assert (down(torch, t_out, np.uint8, 16, lead_out + 8 * n) == 0x5A).all()
    return out


def same_words(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the mix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("freq", sorted(FREQUENCIES))
def test_mix_equals_the_specification(xa, torch, oracle_mod, freq):
    """Types 0, 1 and 2, calls of 0 .. 100 003 samples one behind the other on one handle: the phase carries on."""
    hz = FREQUENCIES[freq]
    x = ac.burst()[:sum(SIZES)]
    for sample_type in (sp.FLOATIQ, sp.S16IQ, sp.S8IQ):
        a = typed_input(x, sample_type)
        aq, ref = xa.CarrierAcquirer(FS), sp.Acquirer(FS)
        aq.set_frequency(hz)
        ref.set_frequency(hz)
        lo = 0
        for n in SIZES:
            piece = cut(a, sample_type, lo, lo + n)
            got = device_mix(xa, torch, aq, piece, sample_type)
            assert same_words(got, ref.mix(piece, sample_type)), (sample_type, n)
            lo += n
        st = aq.state()
        assert int(st["acc"]) == ref.acc and int(st["inc"]) == ref.inc == sp.inc_from_hz(hz, FS) and int(st["samples_mixed"]) == sum(SIZES)
        aq.close()


def test_mix_in_place_cut_into_calls_and_retuned(xa, torch, oracle_mod):
    x = np.ascontiguousarray(ac.burst()[:100003])
    aq, ref = xa.CarrierAcquirer(FS), sp.Acquirer(FS)
    aq.set_frequency(23000.0)
    ref.set_frequency(23000.0)
    whole = device_mix(xa, torch, aq, x, sp.FLOATIQ, in_place=True)
    assert same_words(whole, ref.mix(x))
    # the same stream as 1 + 7 + 4096 + the rest, from the same start
    aq.reset()
    aq.set_frequency(23000.0)
    pieces = np.concatenate([device_mix(xa, torch, aq, x[lo:hi], sp.FLOATIQ) for lo, hi in ((0, 1), (1, 8), (8, 4104), (4104, 100003))])
    assert same_words(pieces, whole) and int(aq.state()["acc"]) == ref.acc
    # a retune between two calls: a frequency step, the phase goes on
    acc = ref.acc
    aq.set_frequency(-181234.5)
    ref.set_frequency(-181234.5)
    assert int(aq.state()["acc"]) == acc and int(aq.state()["inc"]) == sp.inc_from_hz(-181234.5, FS)
    assert same_words(device_mix(xa, torch, aq, x[:5000], sp.FLOATIQ), ref.mix(x[:5000]))
    assert int(aq.state()["acc"]) == ref.acc != acc
    aq.close()


def test_mix_from_unaligned_sources(xa, torch, oracle_mod):
    """An s8 source an odd number of samples into a buffer, a cf32 source and an output 8 bytes off a 16-byte boundary."""
    x = ac.burst()[:4099]
    for sample_type, lead_in, lead_out in ((sp.S8IQ, 2, 0), (sp.S8IQ, 6, 8), (sp.S16IQ, 4, 0), (sp.FLOATIQ, 8, 0), (sp.FLOATIQ, 0, 8), (sp.FLOATIQ, 8, 8)):
        a = typed_input(x, sample_type)
        aq, ref = xa.CarrierAcquirer(FS), sp.Acquirer(FS)
        aq.set_frequency(0.49 * FS)
        ref.set_frequency(0.49 * FS)
        assert same_words(device_mix(xa, torch, aq, a, sample_type, lead_in, lead_out), ref.mix(a, sample_type)), (sample_type, lead_in, lead_out)
        aq.close()


def test_mix_past_the_wide_kernel_s_grid(xa, torch, oracle_mod):
    """The wide kernel's grid stops at 16384 workgroups of 256 threads, each thread a 16-byte load: 8 388 608 cf32 samples a
    trip.  n = 2 * 4 194 304 + 2 * 256 * 5 + 1 gives five workgroups a second trip and leaves one sample to the one-by-one
    kernel.  The specification takes 8 s over the whole array, so it is held on windows, each from its own phase
    (lo * inc mod 2^64): the first and the last 4096 samples, 4096 either side of the second trip's first, where the second
    trip ends, and 64 windows of 256 at seeded places; then the state and the bytes behind the output."""
    per_trip = 16384 * 256 * 2
    n = per_trip + 2 * 256 * 5 + 1
    x = np.resize(ac.burst(), n)
    hz = FREQUENCIES["0.49fs"]
    inc = sp.inc_from_hz(hz, FS)
    aq = xa.CarrierAcquirer(FS)
    aq.set_frequency(hz)
    got = device_mix(xa, torch, aq, x, sp.FLOATIQ)              # (checks the 16 bytes behind the n samples)
    rng = np.random.default_rng(31)
    assert per_trip + 4096 > n                                  # the second trip is short: the window around its first runs to the end
    windows = [(0, 4096), (per_trip - 4096, n), (n - 4096, n)]
    windows += [(lo, lo + 256) for lo in (int(v) for v in rng.integers(0, n - 256, 64))]
    for lo, hi in windows:
        want, _ = sp.mix(x[lo:hi], (lo * inc) & sp.MASK64, inc)
        assert same_words(got[lo:hi], want), (lo, hi)
    st = aq.state()
    assert int(st["acc"]) == (n * inc) & sp.MASK64 and int(st["samples_mixed"]) == n and int(st["inc"]) == inc
    aq.close()


def test_u8_and_misaligned_pointers_are_refused(xa, torch):
    aq = xa.CarrierAcquirer(FS)
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    for call in (lambda: aq.mix_device(t.data_ptr(), 16, xa.SAMPLE_U8IQ, t.data_ptr()),
                 lambda: aq.estimate_device(t.data_ptr(), 16, xa.SAMPLE_U8IQ, False, t.data_ptr()),
                 lambda: aq.mix_device(t.data_ptr() + 4, 16, xa.SAMPLE_FLOATIQ, t.data_ptr()),
                 lambda: aq.mix_device(t.data_ptr(), 16, xa.SAMPLE_FLOATIQ, t.data_ptr() + 4),
                 lambda: aq.mix(np.zeros(32, np.uint8), xa.SAMPLE_U8IQ),
                 lambda: aq.set_frequency(FS / 2)):
        with pytest.raises(xa.XritError) as ei:
            call()
        assert ei.value.code == -1
    assert int(aq.state()["samples_mixed"]) == 0
    aq.close()


# ---- the estimate -----------------------------------------------------------------------------------------------------------------
def device_estimate(xa, torch, aq, a, sample_type, apply=False):
    t_in, p_in = up(torch, a)
    t_rec = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    aq.estimate_device(p_in, n_samples(a, sample_type), sample_type, apply, t_rec.data_ptr())
    return down(torch, t_rec, xa.ACQUIRE_RECORD_DTYPE, 1)[0]


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_estimate_follows_the_specification(xa, torch, name):
    c = ac.CASES[name]
    want, P = ac.spec_record(name, detail=True)
    aq = xa.CarrierAcquirer(c["fs"], pre_sum=c["pre_sum"], segments=c.get("segments", 0))
    got = device_estimate(xa, torch, aq, ac.samples(name), ac.sample_type(name), apply=True)
    again = device_estimate(xa, torch, aq, ac.samples(name), ac.sample_type(name), apply=True)
    bins = abs(float(got["nu"]) - float(want["nu"])) * 2 * sp.N * c["pre_sum"]
    print(f"case {name}: device {got['hz']:.4f} Hz, specification {want['hz']:.4f} Hz, {bins:.2e} of a bin apart; ratio {got['ratio']:.2f} "
          f"for {want['ratio']:.2f}; bin {got['k0']}")
    assert got["segments"] == want["segments"] and got["status"] == want["status"] == sp.OK
    top = np.sort(P)[-2:]
    if top[1] > 1.01 * top[0]:
        assert got["k0"] == want["k0"]
    assert bins <= 1e-6
    assert abs(float(got["hz"]) - c["carrier_hz"]) <= 1.0 and abs(float(got["ratio"]) / float(want["ratio"]) - 1.0) < 1e-4
    assert int(got["inc"]) == sp.inc_from_nu(got["nu"]) and float(got["hz"]) == float(got["nu"]) * c["fs"]
    assert got.tobytes() == again.tobytes()                     # the same bits from run to run
    st = aq.state()
    assert got["applied"] == 1 and int(st["inc"]) == int(got["inc"]) and int(st["estimates"]) == 2 and int(st["applied"]) == 2 and int(st["acc"]) == 0
    aq.close()


def test_apply_leaves_the_frequency_alone_unless_the_estimate_is_ok(xa, torch):
    aq = xa.CarrierAcquirer(FS)
    aq.set_frequency(1234.5)
    inc = sp.inc_from_hz(1234.5, FS)
    x = ac.samples("c")
    rec = device_estimate(xa, torch, aq, x, sp.FLOATIQ, apply=False)
    assert rec["status"] == sp.OK and rec["applied"] == 0 and int(rec["inc"]) != inc and int(aq.state()["inc"]) == inc
    rec = device_estimate(xa, torch, aq, ac.noise(1 << 17, 1), sp.FLOATIQ, apply=True)
    assert rec["status"] == sp.WEAK and rec["segments"] == 63 and rec["applied"] == 0 and int(aq.state()["inc"]) == inc
    rec = device_estimate(xa, torch, aq, x[:65535], sp.FLOATIQ, apply=True)
    assert rec["status"] == sp.TOO_SHORT and rec["segments"] == 30 and rec["applied"] == 0 and rec["k0"] == 0 and int(aq.state()["inc"]) == inc
    rec = device_estimate(xa, torch, aq, x[:100], sp.FLOATIQ, apply=True)
    assert rec["status"] == sp.TOO_SHORT and rec["segments"] == 0 and int(aq.state()["inc"]) == inc
    rec = device_estimate(xa, torch, aq, x, sp.FLOATIQ, apply=True)
    st = aq.state()
    assert rec["status"] == sp.OK and rec["applied"] == 1 and int(st["inc"]) == int(rec["inc"]) != inc
    assert int(st["estimates"]) == 5 and int(st["applied"]) == 1
    # a min_ratio above the line's makes the same input WEAK; fewer segments than the input holds are taken when asked
    strict = xa.CarrierAcquirer(FS, segments=31, min_ratio=1e4)
    rec = device_estimate(xa, torch, strict, ac.samples("d"), sp.FLOATIQ, apply=True)
    assert rec["status"] == sp.WEAK and rec["segments"] == 31 and int(strict.state()["inc"]) == 0
    strict.close()
    aq.close()


# ---- the estimate where the cases do not reach: every bin, the wave's edges, input that is not a signal ----------------------------
WORST = {}


def note(test, **figures):
    """The largest distances a test measured, printed (the head of this file lists them)."""
    WORST[test] = figures
    print(f"{test}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))


class Slots:
    """Records in 64-byte slots of one device tensor, estimates queued on the null stream with no wait.  An input's memory
    goes back to the caching allocator as soon as its estimate is queued: uploads and estimates share the stream, so whatever
    takes the memory next is ordered behind the estimate that reads it."""

    def __init__(self, torch, count):
        self.torch, self.count = torch, count
        self.t = torch.full((64 * count,), 0xA5, dtype=torch.uint8, device="cuda:0")

    def queue(self, aq, a, sample_type, slot, apply=False):
        t_in, p_in = up(self.torch, a)
        aq.estimate_device(p_in, n_samples(a, sample_type), sample_type, apply, self.t.data_ptr() + 64 * slot)

    def records(self, xa):
        """The one wait and the one download."""
        return down(self.torch, self.t, xa.ACQUIRE_RECORD_DTYPE, self.count)


def consistent(rec, fs):
    """inc and hz are the contract's functions of the device's own nu."""
    return int(rec["inc"]) == sp.inc_from_nu(rec["nu"]) and float(rec["hz"]) == float(rec["nu"]) * fs


def held_to(got, want, P, pre_sum, tag):
    """The file's rules for a record against the specification's: -> (nu's distance in bins, on the circle; ratio's, relative)."""
    assert got["status"] == want["status"] and got["segments"] == want["segments"] and got["applied"] == 0, (tag, got, want)
    top = ac.top_two(P)
    if top[1] > 1.01 * top[0]:
        assert got["k0"] == want["k0"], (tag, got, want)
    bins = ac.bins_apart(got["nu"], want["nu"], pre_sum, circle=True)
    rel = abs(float(got["ratio"]) / float(want["ratio"]) - 1.0)
    assert bins <= 1e-6 and rel <= 1e-4, (tag, bins, rel, got, want)
    return bins, rel


def test_a_line_in_every_bin(xa, torch):
    """4096 tones of 65 536 samples, bin k at (37 k mod 13 - 6) sixteenths of a bin, one handle, no wait in between: every
    output bin of the transform is the peak once, with its twiddles and its place in the digit-reversed write-out."""
    aq = xa.CarrierAcquirer(FS)
    slots = Slots(torch, sp.N)
    for k in range(sp.N):
        slots.queue(aq, ac.tone(k, ac.tone_d16(k)), sp.FLOATIQ, k)
    recs = slots.records(xa)
    worst_nu = worst_ratio = 0.0
    for k in range(sp.N):
        got, d16 = recs[k], ac.tone_d16(k)
        assert got["k0"] == k and got["status"] == sp.OK and got["segments"] == 31 and got["applied"] == 0, (k, got)
        bins = ac.bins_apart(got["nu"], ac.tone_nu(k, d16), circle=(k == 2048))
        rel = abs(float(got["ratio"]) / ac.tone_ratio(d16) - 1.0)
        worst_nu, worst_ratio = max(worst_nu, bins), max(worst_ratio, rel)
        assert bins <= 1e-6 and rel <= 1e-4, (k, d16, bins, rel, got)
        assert consistent(got, FS), (k, got)
    note("a line in every bin", nu=worst_nu, ratio=worst_ratio)
    st = aq.state()
    assert int(st["estimates"]) == sp.N and int(st["applied"]) == 0 and int(st["inc"]) == 0
    aq.close()


def test_offsets_across_a_bin(xa, torch):
    """Bins 0, 77, 2047, 2048 and 4095 with the line -8 .. 8 sixteenths off: through the half-way points, where either
    neighbour may be named, over the wrap at 2048 and round the ends of the spectrum."""
    aq = xa.CarrierAcquirer(FS)
    places = [(k, d16) for k in (0, 77, 2047, 2048, 4095) for d16 in range(-8, 9)]
    slots = Slots(torch, len(places))
    for i, (k, d16) in enumerate(places):
        slots.queue(aq, ac.tone(k, d16), sp.FLOATIQ, i)
    recs = slots.records(xa)
    worst_nu = worst_ratio = 0.0
    for got, (k, d16) in zip(recs, places):
        want, P = sp.estimate(ac.tone(k, d16), FS, detail=True)
        assert want["status"] == sp.OK
        bins, rel = held_to(got, want, P, 1, (k, d16))
        assert int(got["k0"]) in (k, (k + (1 if d16 > 0 else -1)) % sp.N) and consistent(got, FS), (k, d16, got)
        worst_nu, worst_ratio = max(worst_nu, bins), max(worst_ratio, rel)
    note("offsets across a bin", nu=worst_nu, ratio=worst_ratio)
    aq.close()


def seeded_bins():
    rng = np.random.default_rng(2048)
    rest = np.setdiff1d(np.arange(sp.N), (0, 1, 2047, 2048, 4095))
    return sorted({0, 1, 2047, 2048, 4095} | {int(k) for k in rng.choice(rest, 59, replace=False)})


@pytest.mark.parametrize("pre_sum", (1, 4, 64))
@pytest.mark.parametrize("sample_type", (sp.FLOATIQ, sp.S16IQ, sp.S8IQ))
def test_tones_of_every_sample_type_and_pre_sum(xa, torch, sample_type, pre_sum):
    """64 seeded bins (0, 1, 2047, 2048 and 4095 among them) against the specification on the samples as quantised; behind
    the last whole pre-sum stand R - 1 samples that are not read: NaN for cf32, full scale for the integers.  (At a pre-sum
    of 64 a tone is 4 194 304 samples: a case takes 2 s, nearly all of it the host's making the tones and their records.)"""
    fs = FS * pre_sum
    aq = xa.CarrierAcquirer(fs, pre_sum=pre_sum)
    bins_taken = seeded_bins()
    assert len(bins_taken) == 64
    slots = Slots(torch, len(bins_taken))
    wants = []
    spare = {sp.FLOATIQ: np.full(pre_sum - 1, np.nan, np.complex64), sp.S16IQ: np.full(2 * (pre_sum - 1), 32767, np.int16),
             sp.S8IQ: np.full(2 * (pre_sum - 1), -128, np.int8)}[sample_type]
    for i, k in enumerate(bins_taken):
        a = ac.tone_as(ac.tone(k, ac.tone_d16(k), 65536, pre_sum), sample_type)
        wants.append(sp.estimate(sp.to_complex(a, sample_type, np.complex128), fs, pre_sum, detail=True))
        slots.queue(aq, np.concatenate([a, spare]), sample_type, i)
    recs = slots.records(xa)
    worst_nu = worst_ratio = 0.0
    for got, (want, P), k in zip(recs, wants, bins_taken):
        assert want["status"] == sp.OK and want["k0"] == k and want["segments"] == 31
        bins, rel = held_to(got, want, P, pre_sum, (sample_type, pre_sum, k))
        assert got["k0"] == k and consistent(got, fs), (k, got)
        worst_nu, worst_ratio = max(worst_nu, bins), max(worst_ratio, rel)
    note(f"tones, type {sample_type}, pre-sum {pre_sum}", nu=worst_nu, ratio=worst_ratio)
    aq.close()


WAVE_SEGMENTS = (31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130)


def test_segment_counts_around_the_wave(xa, torch):
    """The finish kernel's lane l takes the segment pairs s = 1 + l, 65 + l, ...: 64, 65 and 66 segments are where the
    second trip begins, 128 .. 130 the third.  One pair dropped moves nu of case b by 1.9e-5 .. 6.1e-4 of a bin at these
    sizes (the specification, on the CPU), at least 19 times the bound.  Case b whole, the handle capping M; case g's int16
    burst carried on to 131 half segments and cut to what M needs."""
    b = ac.samples("b")
    g = ac.longer("g", (max(WAVE_SEGMENTS) + 1) * sp.HOP)
    assert g.dtype == np.int16 and np.array_equal(g[:2 * 65536], ac.samples("g")[:2 * 65536])
    slots = Slots(torch, 2 * len(WAVE_SEGMENTS))
    handles, inputs = [], []
    for i, m in enumerate(WAVE_SEGMENTS):
        aq = xa.CarrierAcquirer(FS, segments=m)
        handles.append(aq)
        cut_g = g[:2 * (m + 1) * sp.HOP]
        inputs += [(b, sp.FLOATIQ, m), (cut_g, sp.S16IQ, m)]
        slots.queue(aq, b, sp.FLOATIQ, 2 * i)
        slots.queue(aq, cut_g, sp.S16IQ, 2 * i + 1)
    recs = slots.records(xa)
    worst_nu = worst_ratio = 0.0
    for got, (a, sample_type, m) in zip(recs, inputs):
        want, P = sp.estimate(sp.to_complex(a, sample_type, np.complex128), FS, max_segments=m, detail=True)
        assert want["status"] == sp.OK and want["segments"] == m
        top = ac.top_two(P)
        assert top[1] > 1.01 * top[0]                           # the line stands clear: the bin has to be the same
        bins, rel = held_to(got, want, P, 1, (sample_type, m))
        assert got["k0"] == want["k0"] and consistent(got, FS)
        worst_nu, worst_ratio = max(worst_nu, bins), max(worst_ratio, rel)
    note("segment counts around the wave", nu=worst_nu, ratio=worst_ratio)
    for aq in handles:
        assert int(aq.state()["estimates"]) == 2
        aq.close()


def test_input_that_is_not_a_signal(xa, torch):
    """Silence; a NaN, an Inf and squares that overflow float32 within the samples read (WEAK, never applied, the same bytes
    from run to run); a NaN in the samples that are not read (the clean record's bytes); a DC line from int8's corner."""
    # silence: the specification's record field for field, the ratio NaN in both
    want = sp.estimate(np.zeros(65536, np.complex64), FS)
    assert want["status"] == sp.WEAK and np.isnan(want["ratio"])
    for a, sample_type in ((np.zeros(65536, np.complex64), sp.FLOATIQ), (np.zeros(2 * 65536, np.int8), sp.S8IQ)):
        aq = xa.CarrierAcquirer(FS)
        got = device_estimate(xa, torch, aq, a, sample_type, apply=True)
        for name in sp.RECORD_DTYPE.names:
            if name == "ratio":
                assert np.isnan(got[name])
            else:
                assert np.array_equal(got[name], want[name]), (sample_type, name, got)
        assert float(got["nu"]) == 0.0 and int(aq.state()["applied"]) == 0
        aq.close()
    # three inputs that are not finite, or whose squares are not, where the estimate reads
    clean = ac.samples("c")
    with_nan, with_inf = clean.copy(), clean.copy()
    with_nan[40000] = np.nan
    with_inf[12345] = complex(np.inf, 0.25)
    scaled = (clean.astype(np.complex128) * 1e20).astype(np.complex64)
    assert np.isfinite(scaled.view(np.float32)).all() and float(np.abs(scaled.view(np.float32)).max()) ** 2 > float(np.finfo(np.float32).max)
    inc = sp.inc_from_hz(1234.5, FS)
    for tag, x in (("nan", with_nan), ("inf", with_inf), ("1e20", scaled)):
        for apply in (False, True):
            aq = xa.CarrierAcquirer(FS)
            aq.set_frequency(1234.5)
            got = device_estimate(xa, torch, aq, x, sp.FLOATIQ, apply=apply)
            st = aq.state()
            assert got["status"] == sp.WEAK and got["applied"] == 0 and got["segments"] == 31, (tag, apply, got)
            assert int(st["inc"]) == inc and int(st["estimates"]) == 1 and int(st["applied"]) == 0, (tag, apply, st)
            assert int(got["inc"]) == (sp.inc_from_nu(got["nu"]) if np.isfinite(got["nu"]) else 0), (tag, apply, got)
            again = device_estimate(xa, torch, aq, x, sp.FLOATIQ, apply=apply)
            st = aq.state()
            assert got.tobytes() == again.tobytes(), (tag, apply, got, again)
            assert int(st["inc"]) == inc and int(st["estimates"]) == 2 and int(st["applied"]) == 0
            aq.close()
    # a NaN where the estimate does not read: behind the last whole pre-sum, and beyond the segments the handle takes
    fs4 = 4 * FS
    t4 = ac.tone(300, 5, 65536, 4)
    aq = xa.CarrierAcquirer(fs4, pre_sum=4)
    want = device_estimate(xa, torch, aq, t4, sp.FLOATIQ)
    got = device_estimate(xa, torch, aq, np.concatenate([t4, np.full(3, np.nan, np.complex64)]), sp.FLOATIQ)
    assert want["status"] == sp.OK and want["k0"] == 300 and got.tobytes() == want.tobytes()
    aq.close()
    aq = xa.CarrierAcquirer(FS, segments=31)
    want = device_estimate(xa, torch, aq, clean, sp.FLOATIQ)
    got = device_estimate(xa, torch, aq, np.concatenate([clean, np.full(5000, np.nan, np.complex64)]), sp.FLOATIQ)
    assert want["status"] == sp.OK and got["segments"] == 31 and got.tobytes() == want.tobytes()
    aq.close()
    # every int8 sample -128 - 128i: u = -1 - i, z = 2i, a line at 0 Hz
    dc = np.full(2 * 65536, -128, np.int8)
    want, P = sp.estimate(sp.to_complex(dc, sp.S8IQ, np.complex128), FS, detail=True)
    assert want["status"] == sp.OK and want["k0"] == 0 and want["nu"] == 0.0
    aq = xa.CarrierAcquirer(FS)
    got = device_estimate(xa, torch, aq, dc, sp.S8IQ)
    bins, rel = held_to(got, want, P, 1, "dc")
    assert got["k0"] == 0 and got["status"] == sp.OK and consistent(got, FS)
    note("int8 DC line", nu=bins, ratio=rel)
    aq.close()


def test_estimates_back_to_back_without_a_wait(xa, torch):
    """Seven estimates queued on one stream with no wait between them, on one handle whose spectra scratch the first fills
    to 511 segments: the calls behind it are shorter and must not see what it left.  Every record is the one a fresh handle
    gives for that input alone; the state is the specification's after the same sequence."""
    a, g = ac.samples("a"), ac.samples("g")
    tone = ac.tone(1234, 3)
    silence = np.zeros(65536, np.complex64)
    weak = ac.noise(1 << 17, 1)
    queue = [(a, sp.FLOATIQ, True), (tone, sp.FLOATIQ, False), (g, sp.S16IQ, True), (silence, sp.FLOATIQ, True),
             (a[:100], sp.FLOATIQ, True), (weak, sp.FLOATIQ, True), (a, sp.FLOATIQ, False)]
    aq = xa.CarrierAcquirer(FS, segments=511)
    slots = Slots(torch, len(queue))
    s = torch.cuda.Stream(device="cuda:0")
    uploads = [up(torch, x) for x, _, _ in queue]
    torch.cuda.synchronize()                                    # the uploads; from here on nothing waits
    for i, ((x, sample_type, apply), (_, p_in)) in enumerate(zip(queue, uploads)):
        aq.estimate_device(p_in, n_samples(x, sample_type), sample_type, apply, slots.t.data_ptr() + 64 * i, stream=s.cuda_stream)
    s.synchronize()
    recs = slots.records(xa)
    assert [int(r["segments"]) for r in recs] == [511, 31, 63, 31, 0, 63, 511]
    assert [int(r["status"]) for r in recs] == [sp.OK, sp.OK, sp.OK, sp.WEAK, sp.TOO_SHORT, sp.WEAK, sp.OK]
    assert [int(r["applied"]) for r in recs] == [1, 0, 1, 0, 0, 0, 0]
    for i, (x, sample_type, apply) in enumerate(queue):
        fresh = xa.CarrierAcquirer(FS, segments=511)
        alone = device_estimate(xa, torch, fresh, x, sample_type, apply=apply)
        fresh.close()
        assert recs[i].tobytes() == alone.tobytes(), (i, recs[i], alone)
    ref = sp.Acquirer(FS, segments=511)
    for x, sample_type, apply in queue:
        if x is a:
            ref.take(ac.spec_record("a"), apply)                # (made once per process, with these parameters)
        else:
            ref.estimate(x, sample_type, apply)
    st = aq.state()
    # the state's inc is the device's own record's: the specification's inc differs from it by what 1e-6 of a bin allows
    assert int(st["inc"]) == int(recs[2]["inc"]) and abs(int(st["inc"]) - ref.inc) * 2.0 ** -64 * 2 * sp.N <= 1e-6
    assert (int(st["estimates"]), int(st["applied"])) == (ref.estimates, ref.applied) == (7, 2) and int(st["acc"]) == 0
    aq.close()


# ---- in front of the chain ----------------------------------------------------------------------------------------------------------
def chain_run(xa, torch, d_x, n, acquire, sync_each):
    """estimate(apply) -> mix -> the chain on one stream: (soft symbols, the mixed samples, the record)."""
    dev = torch.device("cuda:0")
    cap = 150000
    dem = xa.Demodulator(xa.Demodulator.config("lrit", FS, 1, device=0))
    d_soft = torch.zeros(cap, dtype=torch.float32, device=dev)
    d_mixed = torch.zeros(2 * n, dtype=torch.float32, device=dev)
    d_rec = torch.zeros(64, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    aq = xa.CarrierAcquirer(FS) if acquire else None
    src = d_x
    if aq:
        aq.estimate_device(d_x.data_ptr(), 1 << 18, sp.FLOATIQ, True, d_rec.data_ptr(), stream=s.cuda_stream)
        if sync_each:
            s.synchronize()
        aq.mix_device(d_x.data_ptr(), n, sp.FLOATIQ, d_mixed.data_ptr(), stream=s.cuda_stream)
        if sync_each:
            s.synchronize()
        src = d_mixed
    ns = dem.process_device(src.data_ptr(), n, d_soft.data_ptr(), cap, stream=s.cuda_stream)
    s.synchronize()
    out = (d_soft.cpu().numpy()[:ns].copy(), d_mixed.cpu().numpy().view(np.complex64).copy(), d_rec.cpu().numpy().view(xa.ACQUIRE_RECORD_DTYPE)[0].copy())
    if aq:
        aq.close()
    dem.close()
    return out


def test_chain_locks_behind_the_stage_and_not_without_it(xa, torch, oracle_mod):
    o = oracle_mod
    x = ac.burst()
    n = len(x)
    d_x = torch.from_numpy(x.view(np.float32).copy()).to("cuda:0")
    soft, mixed, rec = chain_run(xa, torch, d_x, n, True, False)
    soft_s, mixed_s, rec_s = chain_run(xa, torch, d_x, n, True, True)
    assert rec["status"] == sp.OK and rec["applied"] == 1 and abs(float(rec["hz"]) - ac.BURST_HZ) < 1.0 and rec.tobytes() == rec_s.tobytes()
    assert same_words(mixed, mixed_s) and same_words(soft, soft_s)
    # the device's mixed samples are the specification's for the device's own estimate; the chain behind them is the oracle's
    ref = sp.Acquirer(FS)
    ref.inc = int(rec["inc"])
    assert same_words(mixed, ref.mix(x))
    want = o.Demod(o.config("lrit", FS, 1)).process(mixed)
    assert same_words(soft, want)
    ber = ac.second_half_error_rate(soft)
    raw, _, _ = chain_run(xa, torch, d_x, n, False, False)
    ber_raw = ac.second_half_error_rate(raw)
    print(f"second half decision errors: unmixed {ber_raw:.4f}, behind the stage {ber:.2e} ({len(soft)} symbols; estimate {rec['hz']:.2f} Hz)")
    assert ber <= 1e-3
    assert ber_raw > 0.40


# ---- host forms, the class, the host program ---------------------------------------------------------------------------------------------
def test_host_forms_equal_the_device_forms(xa, torch, oracle_mod):
    x = ac.samples("g")                                     # int16
    a, b = xa.CarrierAcquirer(FS), xa.CarrierAcquirer(FS)
    rec_host = a.estimate(x, xa.SAMPLE_S16IQ, apply=True)
    rec_dev = device_estimate(xa, torch, b, x, sp.S16IQ, apply=True)
    assert rec_host.tobytes() == rec_dev.tobytes() and rec_host["applied"] == 1
    piece = x[:2 * 70001]
    got = a.mix(piece, xa.SAMPLE_S16IQ)
    assert got.dtype == np.complex64 and same_words(got, device_mix(xa, torch, b, piece, sp.S16IQ))
    assert same_words(a.mix(piece[:0], xa.SAMPLE_S16IQ), np.zeros(0, np.complex64))
    assert a.state().tobytes() == b.state().tobytes() and int(a.state()["samples_mixed"]) == 70001
    a.reset()
    st = a.state()
    assert all(int(st[k]) == 0 for k in st.dtype.names)
    a.close()
    b.close()


def host_symbols(tmp_path, capture, *extra):
    host_bin = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
    out = tmp_path / ("symbols" + "".join(extra).replace("-", "_") + ".s8")
    r = subprocess.run([host_bin, "--input", str(capture), "--format", "cf32", "--mode", "lrit", "--sample-rate", "1250000", "--block", "524288",
                        "--sink", f"file:{out}", *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(out, np.int8), r.stderr


def test_host_program_acquires_and_locks_in_the_decoder(xa, tmp_path):
    """A capture of coded frames 23 kHz off: with --acquire (and with --tune 23000) the decoder's correlator finds the marker
    in every frame at one position; without either it does not."""
    from test_oracle_kat import _framed_burst, check_frame_lock
    x, _ = _framed_burst(16, carrier_hz=23000.0)
    f = tmp_path / "frames.cf32"
    x.tofile(f)
    s8, err = host_symbols(tmp_path, f, "--acquire")
    assert "acquire: carrier offset 2300" in err or "acquire: carrier offset 2299" in err, err
    check_frame_lock(xa.sync_correlate(s8))
    tuned, _ = host_symbols(tmp_path, f, "--tune", "23000")
    check_frame_lock(xa.sync_correlate(tuned))
    plain, err = host_symbols(tmp_path, f)
    assert "acquire" not in err
    with pytest.raises(AssertionError):
        check_frame_lock(xa.sync_correlate(plain))
