"""GPU tier: the carrier acquisition stage (xrit_acquire_*, CarrierAcquirer) against the specification of
tests/acquire_spec.py -- the mix bit for bit (every sample type, the sizes around the 16-byte groups, in place, a stream cut
into calls, a retune between calls, source offsets that take the one-by-one kernel, a call longer than the wide kernel's
grid covers in one trip), the estimate on the cases of tests/acquire_cases.py (cf32, int16 and int8, pre-sums of 1, 4, 16
and 64, 31 to 4095 segments), what `apply` does, the stage in front of the chain on one stream, the host forms, and
xrit_demod_host --acquire from IQ to a locked decoder.

The estimate's distance from the specification, |nu_dev - nu_spec| in bins of 1 / (2 N R), measured on an MI355X: at most
4.3e-10 (a 2.0e-11, b 3.2e-11, c 2.6e-10, d 2.3e-10, e 5.3e-11, f 7.9e-11, g 1.1e-10, h 3.8e-10, i 4.3e-10, j 2.9e-10,
k 6.9e-12, l 6.6e-11); the bound is 1e-6."""
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
