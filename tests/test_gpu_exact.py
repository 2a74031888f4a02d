"""GPU tier (-m gpu): cfg.front_exact = 2 -- the front end BIT FOR BIT the CPU chain's through the Costas loop.

Every comparison here is np.array_equal on the 32-bit words (or on the complex64 words), not a tolerance: the exact-order
FIR (csrc/fir.hip: fir_exact_kernel), the literally walked AGC (csrc/agc.hip: run_exact), the exactly walked Costas loop
(csrc/costas_exact.hip with csrc/exact_sincos.h) against oracle/xrit_oracle.c on the same inputs, stage by stage through the
C ABI's stage objects and end to end through the chain.  With the clock recovery relayed to closure (cfg.clock_exact = 1: the
serial float32 recurrence) the SOFT SYMBOLS are the oracle's word for word; with the default clock recovery what is left is its
distance from the serial trajectory, asserted PLAINLY against BASELINE.json's 1e-4 for every configuration.
"""
import numpy as np
import pytest

from conftest import synth_signal, rms

pytestmark = pytest.mark.gpu

NORTH_STAR_RMS = 1e-4


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def same_words(a, b):
    return a.shape == b.shape and np.array_equal(words(a), words(b))


def first_diff(a, b):
    d = np.nonzero(words(a) != words(b))[0]
    return (int(d[0]), len(d)) if len(d) else (-1, 0)


# ------------------------------------------------------------------------------------------------ the loop's sincosf
def test_loop_sincosf_is_the_cpu_chains(xa, oracle_mod):
    """csrc/exact_sincos.h on the device against oracle xo_sincosf (= glibc's sincosf, checked exhaustively on the CPU):
    2^22 arguments over the loop's range and the whole branch |x| < 120, plus the branch boundaries, every bit."""
    rng = np.random.default_rng(11)
    x = np.concatenate([
        rng.uniform(-2 * np.pi - 1.5, 2 * np.pi + 1.5, 1 << 21),
        rng.uniform(-120, 120, 1 << 20),
        rng.normal(0, 1e-3, 1 << 18),
        np.array([0.0, -0.0, 2.0 ** -12, np.pi / 4, 0.78539819, 0.7853981, np.pi / 2, np.pi, 2 * np.pi, 6.2831855, -6.2831855,
                  119.99999, 1e-30, 1e-40, -1e-40]),
    ]).astype(np.float32)
    s, c = xa.loop_sincosf(x)
    # the oracle's, through a small C loop (ctypes per element is slow): the Costas loop with zero gains is a sincos table
    import ctypes as C
    L = oracle_mod.lib()
    rs, rc = np.empty_like(x), np.empty_like(x)
    sv, cv = C.c_float(), C.c_float()
    step = 37          # every 37th argument through ctypes (~90 k calls), all of them through the loop below
    for i in range(0, len(x), step):
        L.xo_sincosf(float(x[i]), C.byref(sv), C.byref(cv))
        rs[i], rc[i] = sv.value, cv.value
    assert np.array_equal(words(s[::step]), words(rs[::step]))
    assert np.array_equal(words(c[::step]), words(rc[::step]))
    # all of them: a Costas loop object whose phase is set per call would be slow too; use the loop's own de-rotation with the
    # gains off -- out = in * exp(-j phase): in = 1 gives (cos(-p), sin(-p)) = (cos p, -sin p)
    k = oracle_mod.CostasLoop(0.0)
    k.s.alpha = 0.0
    k.s.beta = 0.0
    k.s.freq = 0.0
    one = np.ones(1, np.complex64)
    idx = rng.integers(0, len(x), 20000)
    for i in idx.tolist():
        k.s.phase = float(x[i])
        y = k.Work(one)
        # (cos(-p), sin(-p)) of the oracle's xo_sincosf(-p): compare with the device's sincosf(-p)
        rs[i], rc[i] = y[0].imag, y[0].real
    ns, nc = xa.loop_sincosf(-x[idx])
    assert np.array_equal(words(ns), words(rs[idx]))
    assert np.array_equal(words(nc), words(rc[idx]))


# ------------------------------------------------------------------------------------------------ stages
@pytest.mark.parametrize("D,kind", [(1, "rrc"), (5, "lp5"), (32, "lp32"), (2, "rrc"), (3, "lp5"), (4, "short"), (16, "lp16"),
                                    (6, "lp5"), (1, "short"), (7, "one"), (17, "lp16"), (25, "lp32"), (19, "short"), (33, "one")])
def test_fir_exact_order_is_the_oracle_bit_for_bit(xa, oracle_mod, D, kind):
    """(odd decimations from 17 up: one output per lane, nothing for a window walk to share -- fir_exact_kernel unskewed)"""
    o = oracle_mod
    taps = {"rrc": o.rrc_taps(1, 1.25e6, 293883, 0.5, 63), "lp5": o.lowpass_taps(1, 6.25e6, 625e3, 100e3),
            "lp32": o.lowpass_taps(1, 40e6, 625e3, 100e3), "short": np.array([0.5, -0.25, 0.125], np.float32),
            "lp16": o.lowpass_taps(1, 20e6, 625e3, 100e3), "one": np.array([0.75], np.float32)}[kind]
    rng = np.random.default_rng(100 + D)
    n_out = [30000, 1, 777, 0, 12345, 3]
    x = (rng.standard_normal(sum(n_out) * D) + 1j * rng.standard_normal(sum(n_out) * D)).astype(np.complex64)
    fo, fg = o.FirFilter(D, taps), xa.FirFilter(D, taps, exact=True)
    pos = 0
    for n in n_out:       # several calls: the history carries over, also through empty and 1-sample calls
        seg = x[pos:pos + n * D]
        pos += n * D
        want, got = fo.Work(seg, n), fg.Work(seg, n)
        assert same_words(got, want), (D, kind, n, first_diff(got, want))


def test_agc_walked_literally_is_the_oracle_bit_for_bit(xa, oracle_mod):
    o = oracle_mod
    rng = np.random.default_rng(3)
    n = 3_000_000
    x = (0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    x[1_000_000:1_400_000] *= 4.0           # a level jump and back
    x[2_000_000:2_000_500] = 0              # silence: the gain ramps
    ao, ag = o.AGC(0.01, 0.5, 1.0, 4000.0), xa.AGC(0.01, 0.5, 1.0, 4000.0, exact=True)
    pos = 0
    for m in (1_500_000, 1, 0, 4095, 4097, 700_000, n - 1_500_000 - 1 - 4095 - 4097 - 700_000):
        seg = x[pos:pos + m]
        pos += m
        want, got = ao.Work(seg), ag.Work(seg)
        assert same_words(got, want), (m, first_diff(got, want))
        assert np.float32(ag.gain).view(np.uint32) == np.float32(ao.s.gain).view(np.uint32)
        if m > 100000:
            st = ag.exact_stats()
            print("exact AGC:", m, st, "rounds per block %.2f, segments per scan %.2f" % (st["picard_rounds"] / max(st["blocks"], 1), st["lattice_segments"] / max(st["picard_rounds"], 1)))
            assert st["joints_open"] == 0 and st["at_round_limit"] == 0
    # the clamp: a silent stretch long enough to reach max_gain
    z = np.zeros(900_000, np.complex64)
    z[:10] = 0.1
    ao, ag = o.AGC(0.01, 0.5, 1.0, 4000.0), xa.AGC(0.01, 0.5, 1.0, 4000.0, exact=True)
    assert same_words(ag.Work(z), ao.Work(z))
    assert ag.gain == 4000.0


@pytest.mark.parametrize("mode,fs,n", [("lrit", 1.25e6, 3_000_000), ("hrit", 2.5e6, 3_000_000)])
def test_costas_walked_exactly_is_the_oracle_bit_for_bit(xa, oracle_mod, mode, fs, n):
    """The stage object on the oracle's own matched-filter output: cold start (acquisition, wraps, a loop far from lock), then
    tracking calls of every size; the carried state after every call is the oracle's too."""
    o = oracle_mod
    kw = {} if mode == "lrit" else {"symbol_rate": 927000.0, "alpha": 0.3}
    x = synth_signal(n, fs_in=fs, **kw)
    cfg = o.config(mode, fs, 1)
    d = o.Demod(cfg)
    d.process(x)
    rrc = d.stage("rrc").copy()
    co, cg = o.CostasLoop(cfg.pll_alpha), xa.CostasLoop(cfg.pll_alpha, exact=True)
    pos = 0
    for m in (1_000_000, 1, 0, 63, 64, 65, 8191, 300_000, 70_000, n):
        seg = rrc[pos:pos + m]
        pos += len(seg)
        want, got = co.Work(seg), cg.Work(seg)
        assert same_words(got, want), (mode, m, first_diff(got, want))
        ph, fr = cg.state()
        assert np.float32(ph).view(np.uint32) == np.float32(co.s.phase).view(np.uint32), (m, ph, co.s.phase)
        assert np.float32(fr).view(np.uint32) == np.float32(co.s.freq).view(np.uint32), (m, fr, co.s.freq)
        if pos >= len(rrc):
            break
    st = cg.exact_stats()
    print("exact Costas:", st, "rounds per block %.2f" % (st["picard_rounds"] / max(st["blocks"], 1)))


def test_costas_exact_without_carrier_offset_and_with_a_negative_one(xa, oracle_mod):
    """Phases that hover (no wraps for the whole call) and phases that run downwards (wraps at -2 pi)."""
    o = oracle_mod
    for hz in (0.0, -700.0, 35.0):
        x = synth_signal(1_200_000, fs_in=1.25e6, carrier_hz=hz, phase0=0.01)
        cfg = o.config("lrit", 1.25e6, 1)
        d = o.Demod(cfg)
        d.process(x)
        rrc = d.stage("rrc").copy()
        co, cg = o.CostasLoop(cfg.pll_alpha), xa.CostasLoop(cfg.pll_alpha, exact=True)
        for seg in (rrc[:500_000], rrc[500_000:]):
            want, got = co.Work(seg), cg.Work(seg)
            assert same_words(got, want), (hz, first_diff(got, want))


def test_costas_exact_short_history_still_exact(xa, oracle_mod):
    """A history far too short for the walkers to merge: the joints do not fit, the fix rounds close them (from the host, many)
    -- slow, but the output is the oracle's whatever the plan."""
    o = oracle_mod
    x = synth_signal(600_000, fs_in=1.25e6)
    cfg = o.config("lrit", 1.25e6, 1)
    d = o.Demod(cfg)
    d.process(x)
    rrc = d.stage("rrc").copy()
    co, cg = o.CostasLoop(cfg.pll_alpha), xa.CostasLoop(cfg.pll_alpha, exact=True, history=1024)
    want, got = co.Work(rrc), cg.Work(rrc)
    assert same_words(got, want), first_diff(got, want)
    st = cg.exact_stats()
    assert st["joints_open_after_batch"] > 0 and st["host_rounds"] > 0, st


# ------------------------------------------------------------------------------------------------ the chain
CASES = {"C1": ("lrit", 1.25e6, 1, {}), "C2": ("lrit", 6.25e6, 5, {}),
         "C3": ("hrit", 2.5e6, 1, {"symbol_rate": 927000.0, "alpha": 0.3}), "C5": ("lrit", 40e6, 32, {})}


@pytest.mark.parametrize("case", ["C1", "C2", "C3", "C5"])
def test_chain_front_exact_2_every_stage_is_the_oracle(xa, oracle_mod, case):
    """keep_stages: decimator, AGC, matched filter and Costas outputs word for word; with the clock recovery relayed to
    closure (cfg.clock_exact = 1) the soft symbols too -- over several calls of a stream (state carried in every stage)."""
    chain_stages_are_the_oracle(xa, oracle_mod, case, CASES[case], 400_000, front_exact=2, soft=True)


def chain_stages_are_the_oracle(xa, oracle_mod, case, what, n_dec, front_exact, soft):
    mode, fs, D, kw = what
    n = n_dec * D
    x = synth_signal(n, fs_in=fs, **kw)
    dem = xa.Demodulator(xa.Demodulator.config(mode, fs, D, front_exact=front_exact, clock_exact=1))
    dem.keep_stages(True)
    od = oracle_mod.Demod(oracle_mod.config(mode, fs, D))
    cuts = [0, n_dec * 3 // 8 * D, (n_dec * 3 // 8 + 1) * D + (3 if D > 1 else 0), n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if front_exact == 0:
            assert dem.front_exact_for(b - a), (case, "a call of this size should take the exact twin", b - a)
        got, want = dem.process(x[a:b]), od.process(x[a:b])
        names = ["decimator", "agc", "rrc", "costas"] if D > 1 else ["agc", "rrc", "costas"]
        for nm in names:
            g, w = dem.stage(nm), od.stage(nm)
            assert same_words(g, w), (case, nm, a, b, first_diff(g, w), rms(g - w) if g.shape == w.shape else None)
        if soft:
            assert same_words(got, want), (case, "soft symbols", a, b, first_diff(got, want))


@pytest.mark.parametrize("front_exact", [0, 2])
def test_chain_at_decimation_17_every_stage_is_the_oracle(xa, oracle_mod, front_exact):
    """LRIT at 21.25 Msps, decimation 17, a burst of 40 000 symbols (171 000 samples behind the decimator): an odd decimation
    from 17 up, where the exact order takes fir_exact_kernel unskewed.  Asked for (cfg.front_exact = 2) and as a chain finds it
    by default (cfg.front_exact = 0: calls below a million symbols go through the exact twin) the decimator, AGC, matched
    filter and Costas outputs are the oracle's word for word."""
    chain_stages_are_the_oracle(xa, oracle_mod, "LRIT/17", ("lrit", 21.25e6, 17, {}), 171_000, front_exact=front_exact, soft=False)


@pytest.mark.parametrize("case", ["C1", "C2", "C3", "C5"])
def test_north_star_1e_4_with_front_exact_2_on_the_test_bursts(xa, oracle_mod, case):
    """BASELINE.json's tolerance, plainly, default clock recovery, cold-started test bursts (0.1-0.2 M symbols)."""
    mode, fs, D, kw = CASES[case]
    n = 600_000 * D
    x = synth_signal(n, fs_in=fs, **kw)
    dem = xa.Demodulator(xa.Demodulator.config(mode, fs, D, front_exact=2))
    got = dem.process(x)
    want = oracle_mod.Demod(oracle_mod.config(mode, fs, D)).process(x)
    assert len(got) == len(want)
    big = np.abs(want) > 1e-3
    assert (np.sign(got)[big] == np.sign(want)[big]).all()
    r = rms(got - want)
    print(f"{case}: soft symbols {r:.3e} rms from the oracle (front_exact = 2, {len(want)} symbols)")
    assert r <= NORTH_STAR_RMS, (case, r)


# (case, samples per burst, bursts): bursts of the BASELINE size where the oracle finishes in seconds per burst -- the bursts
# tests/test_gpu_parity.py::test_north_star_1e_4_in_steady_state holds the default configuration to (expected failures there)
STEADY = {
    "C1": ("lrit", 1.25e6, 1, dict(fs_in=1.25e6), 1 << 26, 3),
    "C2": ("lrit", 6.25e6, 5, dict(fs_in=6.25e6), 1 << 28, 3),
    "C3": ("hrit", 2.5e6, 1, dict(fs_in=2.5e6, symbol_rate=927000.0, alpha=0.3), 1 << 26, 3),
    "C5": ("lrit", 40e6, 32, dict(fs_in=40e6), 1 << 28, 3),
}


@pytest.mark.parametrize("case", ["C1", "C2", "C3", "C5"])
def test_north_star_1e_4_in_steady_state_with_front_exact_2(xa, oracle_mod, case):
    """BASELINE.json's tolerance, plainly, on consecutive bursts of one stream at the BASELINE burst size (the cold-started first
    one is checked for count and hard decisions and left out of the rms, as in test_gpu_parity.py): NO expected failure, HRIT
    included.  What is left is the default clock recovery's distance from the serial trajectory."""
    import torch
    from xritdemod_amd import _capi
    mode, fs, D, kw, n, bursts = STEADY[case]
    dev = torch.device("cuda", 0)
    buf = torch.empty((n, 2), dtype=torch.float32, device=dev)
    sp = _capi.synth_params(**kw)
    dem = xa.Demodulator(xa.Demodulator.config(mode, fs, D, front_exact=2))
    ref = oracle_mod.Demod(oracle_mod.config(mode, fs, D))
    se, cnt = 0.0, 0
    for b in range(bursts):
        _capi.synth_generate_device(sp, b * n, n, buf.data_ptr(), device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        x = buf.cpu().numpy().view(np.complex64).reshape(-1)
        got, want = dem.process(x), ref.process(x)
        assert len(got) == len(want), (case, b)
        big = np.abs(want) > 1e-3
        assert np.array_equal(np.sign(got[big]), np.sign(want[big])), (case, b)
        r_b = rms(got - want)
        print(f"{case} burst {b}: {r_b:.3e} rms from the oracle ({len(want)} symbols)")
        assert r_b <= NORTH_STAR_RMS, (case, b, r_b)
        if b == 0:
            continue
        se += float(np.sum((got - want).astype(np.float64) ** 2))
        cnt += len(want)
    r = (se / cnt) ** 0.5
    print(f"{case}: steady state {r:.3e} rms from the oracle (front_exact = 2, {bursts - 1} bursts of {n} samples)")
    assert r <= NORTH_STAR_RMS, (case, r)


def test_front_exact_2_streamed_is_plain_word_for_word(xa, oracle_mod):
    """Inputs registered ahead (front end, both Costas stages and the walkers of the next bursts run ahead of their calls): the
    words of plain consecutive calls; and with cfg.clock_exact = 1 they are the oracle's."""
    import torch
    from xritdemod_amd import _capi
    n, fs, nb = 1 << 23, 1.25e6, 4
    dev = torch.device("cuda", 0)
    buf = torch.empty((nb, n, 2), dtype=torch.float32, device=dev)
    sp = _capi.synth_params(fs_in=fs)
    for b in range(nb):
        _capi.synth_generate_device(sp, b * n, n, buf[b].data_ptr(), device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    cap = int(n / 4.2) + 4096

    def run(cfg, plan):
        soft = torch.empty(cap, dtype=torch.float32, device=dev)
        dem = xa.Demodulator(cfg)
        out = []
        for op, b in plan:
            if op == "pf":
                dem.prefetch_device(buf[b].data_ptr(), n)
            else:
                k = dem.process_device(buf[b].data_ptr(), n, soft.data_ptr(), cap)
                out.append(soft[:k].cpu().numpy())
        return out

    cfg = lambda **k: xa.Demodulator.config("lrit", fs, 1, front_exact=2, **k)      # noqa: E731
    plain = run(cfg(), [("go", b) for b in range(nb)])
    ahead = run(cfg(), [("pf", 0), ("pf", 1), ("pf", 2), ("go", 0), ("pf", 3), ("go", 1), ("go", 2), ("go", 3)])
    mixed = run(cfg(), [("go", 0), ("pf", 1), ("go", 1), ("pf", 2), ("pf", 3), ("go", 2), ("go", 3)])
    exact = run(cfg(clock_exact=1), [("go", 0), ("pf", 1), ("go", 1), ("go", 2), ("go", 3)])
    ref = oracle_mod.Demod(oracle_mod.config("lrit", fs, 1))
    for b in range(nb):
        want = ref.process(buf[b].cpu().numpy().view(np.complex64).reshape(-1))
        assert same_words(plain[b], ahead[b]), b
        assert same_words(plain[b], mixed[b]), b
        assert same_words(exact[b], want), (b, first_diff(exact[b], want))
        assert len(plain[b]) == len(want)
        r = rms(plain[b] - want)
        assert r <= NORTH_STAR_RMS, (b, r)


@pytest.mark.parametrize("scan_mode", [0, 1, 2, 3])
def test_costas_exact_scan_variants_all_give_the_oracle(xa, oracle_mod, monkeypatch, scan_mode):
    """XRIT_CX_MODE (read when the stage is created): 0 = the general systolic scan only, 1 = the three-instruction systolic
    round where neither wrap nor limiter acts, 2 = the lattice scan with the general one behind it, 3 (default) = lattice, fast
    systolic, general.  Whatever the route, the words are the oracle's (the scans are certified or literal)."""
    o = oracle_mod
    x = synth_signal(700_000, fs_in=1.25e6)
    cfg = o.config("lrit", 1.25e6, 1)
    d = o.Demod(cfg)
    d.process(x)
    rrc = d.stage("rrc").copy()
    monkeypatch.setenv("XRIT_CX_MODE", str(scan_mode))
    co, cg = o.CostasLoop(cfg.pll_alpha), xa.CostasLoop(cfg.pll_alpha, exact=True)
    for seg in (rrc[:400_000], rrc[400_000:]):
        want, got = co.Work(seg), cg.Work(seg)
        assert same_words(got, want), (scan_mode, first_diff(got, want))
    st = cg.exact_stats()
    print(f"scan mode {scan_mode}:", st)
    if scan_mode & 2:
        assert st["lattice_segments"] > 0
    else:
        assert st["lattice_segments"] == 0


@pytest.mark.parametrize("case,seed", [("C2", 1), ("C3", 2), ("C1", 3), ("C5", 4)])
def test_front_exact_2_randomly_cut_streams_are_the_oracle(xa, oracle_mod, case, seed):
    """A stream cut at random into calls of 1 .. 2 M samples (empty ones too), every stage's state carried from call to call:
    with cfg.clock_exact = 1 the soft symbols are the oracle's word for word whatever the cuts; s16 input on the decimating
    configurations (the ingest conversion fused into the exact-order filter's window fill)."""
    mode, fs, D, kw = CASES[case]
    rng = np.random.default_rng(seed)
    n = 3_000_000 * (D if D < 32 else 8)
    x = synth_signal(n, fs_in=fs, **kw)
    st = xa.SAMPLE_FLOATIQ
    if D > 1:
        q = np.empty(2 * n, np.int16)
        q[0::2] = np.clip(np.rint(x.real * 32768.0 * 4), -32768, 32767)
        q[1::2] = np.clip(np.rint(x.imag * 32768.0 * 4), -32768, 32767)
        st = xa.SAMPLE_S16IQ
    dem = xa.Demodulator(xa.Demodulator.config(mode, fs, D, front_exact=2, clock_exact=1))
    od = oracle_mod.Demod(oracle_mod.config(mode, fs, D))
    pos = 0
    while pos < n:
        m = int(rng.choice([0, 1, int(rng.integers(2, 5000)), int(rng.integers(5000, 300_000)), int(rng.integers(300_000, 2_000_000))]))
        m = min(m, n - pos)
        if st == xa.SAMPLE_FLOATIQ:
            got, want = dem.process(x[pos:pos + m]), od.process(x[pos:pos + m])
        else:
            seg = q[2 * pos:2 * (pos + m)]
            got, want = dem.process(seg, xa.SAMPLE_S16IQ), od.process(seg, oracle_mod.SAMPLE_S16IQ)
        assert same_words(got, want), (case, pos, m, first_diff(got, want))
        pos += m


def test_front_exact_2_at_low_snr(xa, oracle_mod):
    """Es/N0 = 4 dB: the Costas loop slips now and then, the approximate solve iterates; the exact stage does not care where its
    start states come from -- the front end is the oracle's bit for bit, and with it (cfg.clock_exact = 1) the soft symbols."""
    x = synth_signal(2_500_000, fs_in=1.25e6, esn0_db=4.0, seed=99)
    dem = xa.Demodulator(xa.Demodulator.config("lrit", 1.25e6, 1, front_exact=2, clock_exact=1))
    dem.keep_stages(True)
    od = oracle_mod.Demod(oracle_mod.config("lrit", 1.25e6, 1))
    for a, b in ((0, 1_200_000), (1_200_000, 2_500_000)):
        got, want = dem.process(x[a:b]), od.process(x[a:b])
        for nm in ("agc", "rrc", "costas"):
            g, w = dem.stage(nm), od.stage(nm)
            assert same_words(g, w), (nm, a, first_diff(g, w))
        assert same_words(got, want), (a, first_diff(got, want))


def test_front_exact_2_host_rounds_inside_the_streaming_pipeline(xa, oracle_mod, monkeypatch):
    """Joints left open by the rounds enqueued with a call are closed from the host when the Costas loop is finished -- which, in
    the streaming pipeline, happens after the burst's clock-recovery walkers have been launched speculatively: they start over on
    the rewritten output.  A warm-up of 1024 samples and few walkers (XRIT_CX_HIST / XRIT_CX_WALKERS, read at create) force that
    path on every burst: the words are those of plain calls, and within 1e-4 of the oracle's."""
    import torch
    from xritdemod_amd import _capi
    monkeypatch.setenv("XRIT_CX_HIST", "1024")
    monkeypatch.setenv("XRIT_CX_WALKERS", "4096")
    n, fs, nb = 1 << 23, 1.25e6, 4
    dev = torch.device("cuda", 0)
    buf = torch.empty((nb, n, 2), dtype=torch.float32, device=dev)
    sp = _capi.synth_params(fs_in=fs)
    for b in range(nb):
        _capi.synth_generate_device(sp, b * n, n, buf[b].data_ptr(), device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    cap = int(n / 4.2) + 4096

    def run(plan):
        soft = torch.empty(cap, dtype=torch.float32, device=dev)
        dem = xa.Demodulator(xa.Demodulator.config("lrit", fs, 1, front_exact=2))
        out = []
        for op, b in plan:
            if op == "pf":
                dem.prefetch_device(buf[b].data_ptr(), n)
            else:
                k = dem.process_device(buf[b].data_ptr(), n, soft.data_ptr(), cap)
                out.append(soft[:k].cpu().numpy())
        return out

    plain = run([("go", b) for b in range(nb)])
    ahead = run([("pf", 0), ("pf", 1), ("pf", 2), ("go", 0), ("pf", 3), ("go", 1), ("go", 2), ("go", 3)])
    ref = oracle_mod.Demod(oracle_mod.config("lrit", fs, 1))
    for b in range(nb):
        want = ref.process(buf[b].cpu().numpy().view(np.complex64).reshape(-1))
        assert same_words(plain[b], ahead[b]), b
        assert len(plain[b]) == len(want)
        assert rms(plain[b] - want) <= NORTH_STAR_RMS, (b, rms(plain[b] - want))
    # (that the host did add rounds: the stage object with the same switches)
    cfg = oracle_mod.config("lrit", fs, 1)
    d = oracle_mod.Demod(cfg)
    d.process(buf[0].cpu().numpy().view(np.complex64).reshape(-1))
    cg = xa.CostasLoop(cfg.pll_alpha, exact=True)
    cg.Work(d.stage("rrc"))
    st = cg.exact_stats()
    assert st["host_rounds"] > 0, st


def test_clock_state_handed_from_one_handle_to_another(xa, oracle_mod):
    """The reference's clock recovery is ONE object that carries its state across every chunk (demodulator.cpp:446-450, :156).
    Across handles -- the GPUs of xrit_group_* -- that state is a device record (xrit_demod_export_clock_carry): handle B, warmed up
    from a cold start over the samples in front of a chunk, walks the chunk's clock recovery again from the record handle A left
    where the chunk begins (xrit_demod_redo_clock_from) and emits A's symbols, which are the CPU chain's, word for word -- whether
    or not its own warm-up had met A's trajectory.  A record that is not one is refused and changes nothing."""
    import torch
    fs, D = 6.25e6, 5
    n1, n2, halo = 1500000, 1000000, 1100000
    x = synth_signal(n1 + n2, fs_in=fs)
    want = oracle_mod.Demod(oracle_mod.config("lrit", fs, D)).process(x)
    A = xa.Demodulator(xa.Demodulator.config("lrit", fs, D, front_exact=2))
    a1 = A.process(x[:n1])
    nbytes = xa.lib().xrit_demod_clock_carry_bytes()
    assert nbytes == 64 + 8192
    rec = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    junk = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    A.export_clock_carry(rec.data_ptr(), 0)
    torch.cuda.synchronize()
    head = rec[:8].cpu().numpy().view(np.uint32)
    assert head[0] == 1 and head[1] <= 1024
    a2 = A.process(x[n1:])
    assert np.array_equal(np.concatenate([a1, a2]).view(np.uint32), want.view(np.uint32))
    cap = n2 // D + 1024
    soft = torch.empty(cap, dtype=torch.float32, device="cuda:0")
    for other_lock in (False, True):
        B = xa.Demodulator(xa.Demodulator.config("lrit", fs, D, front_exact=2))
        if other_lock:
            B.flip_costas_phase()
        B.process(x[n1 - halo:n1])
        b2 = B.process(x[n1:])
        if np.dot(b2[:20000], a2[:20000]) > 0:
            break
    else:
        pytest.fail("neither start phase of the Costas loop fell into the stream's lock")
    assert B.last_clock_exact() and len(b2) == len(a2)
    with pytest.raises(xa.XritError):
        B.redo_clock_from(junk.data_ptr(), soft.data_ptr(), cap)
    k = B.redo_clock_from(rec.data_ptr(), soft.data_ptr(), cap)
    torch.cuda.synchronize()
    b3 = soft[:k].cpu().numpy()
    assert k == len(a2) and np.array_equal(b3.view(np.uint32), a2.view(np.uint32)), (k, len(a2), rms(b3 - a2), rms(b2 - a2))
    # the record of where the last call STARTED is what was handed in
    mine = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    B.export_clock_carry(mine.data_ptr(), 1)
    torch.cuda.synchronize()
    assert torch.equal(mine, rec)


@pytest.mark.parametrize("front_exact", [0, 2])
@pytest.mark.parametrize("mode, fs, kw", [("lrit", 1.25e6, dict(fs_in=1.25e6)),
                                          ("hrit", 2.5e6, dict(fs_in=2.5e6, symbol_rate=927000.0, alpha=0.3))])
def test_parity_mode_at_the_references_largest_chunk_is_the_cpu_chains_words(xa, oracle_mod, mode, fs, kw, front_exact):
    """The reference hands its blocks between 32 Ki and 512 Ki complex samples per call (demodulator.cpp:108-119, the FIFO's
    threshold and capacity): 123 k symbols at LRIT, 194 k at HRIT at most.  In the default configuration (cfg.front_exact = 0: the
    bit-exact front end on calls below a million symbols) and in parity mode (cfg.front_exact = 2) a call of up to
    200 k symbols is ONE exact walk of the clock recovery behind the bit-exact front end: three consecutive chunks of the largest
    size come out as the CPU chain's words -- no relay, no floor -- and so does a stream of the file frontend's 65 535-sample blocks
    (CFileFrontend.cpp:48); a call beyond 200 k symbols is relayed again (close to the serial trajectory, not it)."""
    n = 512 * 1024
    x = synth_signal(3 * n + 700000, **kw)
    ref = oracle_mod.Demod(oracle_mod.config(mode, fs, 1))
    dem = xa.Demodulator(xa.Demodulator.config(mode, fs, 1, front_exact=front_exact))
    for c in range(3):
        want = ref.process(x[c * n:(c + 1) * n])
        got = dem.process(x[c * n:(c + 1) * n])
        st = dem.stats()
        assert st.clock_relay_segments == 1, (c, st.clock_relay_segments)
        assert len(want) > (110000 if mode == "lrit" else 180000)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c, rms(got - want))
    want = ref.process(x[3 * n:])
    got = dem.process(x[3 * n:])
    if len(want) > 200000:
        assert dem.stats().clock_relay_segments > 1 and rms(got - want) < 1e-4, (dem.stats().clock_relay_segments, rms(got - want))
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the file frontend's blocks
    ref = oracle_mod.Demod(oracle_mod.config(mode, fs, 1))
    dem = xa.Demodulator(xa.Demodulator.config(mode, fs, 1, front_exact=front_exact))
    for c in range(6):
        blk = x[c * 65535:(c + 1) * 65535]
        assert np.array_equal(dem.process(blk).view(np.uint32), ref.process(blk).view(np.uint32)), c
