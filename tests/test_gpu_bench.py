"""GPU tier: bench.py's contract on the box -- the one-line JSON of a 1-rank run, plain (the headline and what it needs, nothing
else) and with --full (everything else the benchmark measures, in runs of their own), and the N > 1 launch
(`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`) with two ranks that share the box's one device
(XRIT_BENCH_SHARE_DEVICE=1: gloo for the barrier and the reductions, RCCL refuses two ranks on one device; every rank
still demodulates its own capture segment on the GPU, the timing is the max over ranks, the value the sum)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "3", "--warmup", "2", "--burst-log2", "24", "--no-cpu", "--no-exact", "--no-serial-floor"]
# what only a --full run measures: never in the line of a plain one
FULL_ONLY = {"cpu_baseline", "parity_vs_oracle", "other_configs", "contiguous", "parity_mode", "warm_mode", "exact_mode", "fast_mode",
             "quick_mode"}


def _last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def _check_line(d, n):
    assert d["n_gpus"] == n and d["steps"] == 3 and d["warmup"] == 2
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = the samples all ranks processed / the slowest rank's time
    assert abs(d["value"] - n * (1 << 24) * 3 / (d["ms_per_step"] * 3e-3) / 1e6) <= 0.01 * d["value"]
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1
    assert d["loop_passes"]["costas_unconverged"] == 0


@pytest.mark.gpu
def test_bench_line_of_one_rank():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    _check_line(_last_json(r.stdout), 1)


def test_full_is_an_option_and_its_parts_need_it():
    """No GPU: --full is there, and the options that only add to a --full run say so when given without it (the arguments are
    checked before anything touches a device)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout, r.stdout + r.stderr
    for opt in ("--contiguous-leg", "--legs-in-process"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), opt], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--full" in r.stderr, (opt, r.returncode, r.stderr[-500:])


@pytest.mark.gpu
def test_plain_run_is_lean():
    """The command every change is measured with, at the headline's own size (C2, 256 Mi samples per step), with none of the
    --no-* options: its line carries the headline, the chain's roofline fraction and the decimating FIR as the timed region's
    events saw it -- nothing that takes a run of its own -- and the whole process, start to exit, spends at most 30 s outside
    its warm-up and timed steps."""
    import time
    K, W = 10, 4
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W)],
                       capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert d["steps"] == K and d["warmup"] == W and d["value"] > 0 and d["ms_per_step"] > 0
    assert not FULL_ONLY & set(d), sorted(FULL_ONLY & set(d))
    assert d["read_bw_measured_gbs"] is None
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1
    assert "dominant_kernel" not in d["roofline"] and "by_total_time" not in d["roofline"]
    assert set(d["kernels"]) == {"fir_decim"} and d["kernels"]["fir_decim"]["measured"].startswith("timed region"), d["kernels"]
    assert d["kernels"]["fir_decim"]["launches"] == K and d["roofline"]["input_kernel"]["kernel"] == "fir_decim"
    outside = wall - (K + W) * d["ms_per_step"] * 1e-3
    print("plain run: %.1f s from start to exit, %.1f s of them outside its %d steps" % (wall, outside, K + W))
    assert outside <= 30.0, (wall, d["ms_per_step"])


CONTIG_KEYS = {"value", "unit", "steps", "ms_per_step", "halo_samples", "halo_bytes_per_boundary", "rccl_ranks", "polarity_flips",
               "symbols_per_s", "samples_per_step_per_gpu"}


@pytest.mark.gpu
def test_bench_line_carries_the_contiguous_leg_over_rccl():
    """With N > 1 a --full run times a second region through xrit_group_process_slice_device (ONE stream cut in N
    slices, RCCL edge-sample exchange: BASELINE config 4) and reports it as `contiguous` in the same JSON line; `value` stays the
    independent-segments figure.  One GPU allows an RCCL communicator of ONE rank: --contiguous-leg runs that leg at N = 1, so the
    schema, ncclCommCount and the group path are covered here (two ranks on one device: the in-process fabric tests of
    test_gpu_parity.py)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--contiguous-leg"] + SMALL, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    _check_line(d, 1)
    c = d["contiguous"]
    assert CONTIG_KEYS <= set(c), sorted(c)
    assert c["rccl_ranks"] == 1 and c["halo_samples"] == 0 and c["polarity_flips"] == 0
    assert c["value"] > 0 and c["samples_per_step_per_gpu"] == (1 << 24) - (1 << 24) % 5      # whole decimation periods
    rf = d["roofline"]
    # the kernel a step spends most of its time in is named as such; the kernel that moves the algorithmic bytes beside it
    assert rf["dominant_kernel"]["kernel"] == rf["by_total_time"]["kernel"] and rf["input_kernel"]["kernel"] == "fir_decim"


@pytest.mark.gpu
def test_bench_two_ranks_launched_like_the_driver_does():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, XRIT_BENCH_SHARE_DEVICE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full"] + SMALL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines            # rank 0 prints, nobody else
    d = json.loads(lines[0])
    _check_line(d, 2)
    # (two ranks on ONE device meet over gloo: the RCCL leg says why it did not run; on the driver's multi-GPU node it does)
    assert "skipped" in d["contiguous"]


@pytest.mark.gpu
def test_circuit_rate_burst_walks_overlapping_blocks():
    """C1 at burst size (2^28 samples, no decimator: 63 M symbols): the clock recovery walks overlapping blocks (round 5,
    csrc/clock_overlap.h) -- one launch, no hand-off and no relay passes, 2.5 walkers per CU at most (640 ranges of 98 k symbols
    behind 49 k symbols of history on a 256-CU part) -- and every step closes its Costas loop in one pass over the samples."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--decimation", "1", "--steps", "3", "--warmup", "2",
                        "--no-cpu", "--no-exact", "--no-serial-floor"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    lp = d["loop_passes"]
    assert lp["clock"] == 0 and lp["clock_relay"] == 1 and lp["clock_relay_closed"] == 0 and lp["costas"] == 1 and lp["costas_unconverged"] == 0, lp
    assert 2 * 256 <= lp["clock_relay_segments"] <= 3 * 256, lp           # (2.5 walkers per CU at most: 640 on a 256-CU part)
    assert d["value"] > 0 and d["config"]["decimation"] == 1


def test_dump_outputs_writes_whole_arrays_or_a_fixed_sample_within_the_budget(tmp_path):
    """bench.dump_outputs (--dump-outputs), no GPU: an array that fits is written whole, float32 staying float32 and the rest
    float64; a larger one as the same seeded sample in every run, its positions sorted and in range beside it, and the
    directory within the budget."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(1)
    small = rng.standard_normal(1000).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "a"), {"soft_symbols": small, "n_symbols": [small.size]}, 64000)
    got, n = np.load(tmp_path / "a" / "soft_symbols.npy"), np.load(tmp_path / "a" / "n_symbols.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    assert n.dtype == np.float64 and n.tolist() == [1000.0]
    assert not (tmp_path / "a" / "soft_symbols_index.npy").exists()
    big = rng.standard_normal(100000).astype(np.float32)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"soft_symbols": big, "n_symbols": [big.size]}, 64000)
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= 64000
    pos, vals = np.load(tmp_path / "b" / "soft_symbols_index.npy"), np.load(tmp_path / "b" / "soft_symbols.npy")
    assert pos.dtype == np.float64 and vals.dtype == np.float32 and pos.size == vals.size > 64000 // 16
    ip = pos.astype(np.int64)
    assert np.array_equal(ip, pos) and ip[0] >= 0 and ip[-1] < big.size and (np.diff(ip) > 0).all()
    assert np.array_equal(vals, big[ip])
    for f in ("soft_symbols.npy", "soft_symbols_index.npy", "n_symbols.npy"):
        assert (tmp_path / "b" / f).read_bytes() == (tmp_path / "c" / f).read_bytes(), f


@pytest.mark.gpu
def test_bench_dumps_what_its_last_timed_step_returned(tmp_path):
    """--dump-outputs DIR: the soft symbols the last timed step returned and their count, the same words from two runs with the
    same arguments, and the words plain consecutive calls of a fresh handle give on the same stream's burst (warm-up 2 + 3 timed
    steps: burst 4)."""
    import numpy as np
    dumps = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(tmp_path / run)] + SMALL,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        _check_line(_last_json(r.stdout), 1)
        assert sum(f.stat().st_size for f in (tmp_path / run).iterdir()) <= 64_000_000
        soft, n = np.load(tmp_path / run / "soft_symbols.npy"), np.load(tmp_path / run / "n_symbols.npy")
        assert soft.dtype == np.float32 and n.dtype == np.float64 and soft.size == int(n[0])
        assert abs(soft.size - (1 << 24) / 5 / (1.25e6 / 293883)) < 2000 and np.isfinite(soft).all()
        dumps.append(soft)
    assert np.array_equal(dumps[0].view(np.uint32), dumps[1].view(np.uint32))
    import torch
    import xritdemod_amd as xa
    from xritdemod_amd import _capi
    n, D, fs = 1 << 24, 5, 6.25e6
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    sp = _capi.synth_params(fs_in=fs, symbol_rate=293883.0, alpha=0.5, seed=0x58524954)
    buf = torch.empty((5, n, 2), dtype=torch.float32, device=dev)
    for b in range(5):
        _capi.synth_generate_device(sp, b * n, n, buf[b].data_ptr(), device=0, stream=st)
    torch.cuda.synchronize(dev)
    cap = int(n / (D * 4.2)) + 4096
    soft = torch.empty(cap, dtype=torch.float32, device=dev)
    dem = xa.Demodulator(xa.Demodulator.config("lrit", fs, D, device=0, costas_chain_len=0, clock_chain_syms=0, front_exact=0))
    for b in range(5):
        k = dem.process_device(buf[b].data_ptr(), n, soft.data_ptr(), cap, stream=st)
    torch.cuda.synchronize(dev)
    dem.close()
    assert np.array_equal(soft[:k].cpu().numpy().view(np.uint32), dumps[0].view(np.uint32))


@pytest.mark.gpu
def test_bench_alternative_legs_run_in_processes_of_their_own():
    """Round 6, --full: parity_mode (cfg.front_exact = 2), exact_mode, fast_mode, quick_mode are each a fresh process of bench.py (--leg):
    what a handle's bursts take depends on the hardware queues HIP deals its streams onto, which depends on what the process
    created before.  The parent collects their results and their soft symbols for the parity comparison."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--burst-log2", "24",
                        "--cpu-sample-log2", "22", "--cpu-threads", "1", "--full"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    _check_line(d, 1)
    for key in ("parity_mode", "warm_mode", "exact_mode", "fast_mode", "quick_mode"):
        assert "error" not in d[key], d[key]
        assert d[key]["ms_per_step"] > 0 and "process of its own" in d[key]["process"], d[key]
    pv = d["parity_vs_oracle"]
    assert pv["parity_mode"]["sign_mismatches"] == 0 and pv["parity_mode"]["rms"] <= 1e-4, pv["parity_mode"]
    assert pv["exact_mode"]["words_differing_from_serial_gpu"] == 0
    assert "other_configs" not in d          # (only beside the headline workload: C2 at the full burst size)
    # ... and the rest of what --full adds: the oracle on the host, the read-only sweep, the per-kernel pass
    assert d["cpu_baseline"]["value"] > 0 and d["read_bw_measured_gbs"] > 0
    assert "dominant_kernel" in d["roofline"] and len(d["kernels"]) > 1


@pytest.mark.gpu
def test_handles_created_one_after_the_other_run_alike():
    """Round 6 (task 2): a handle's streams come from a pool per process, so a handle created after others have
    been destroyed runs on the very hardware queues of the first one -- round 5 measured 2.5 ms per C2 burst for such a handle
    against 1.8.  Five handles of the default configuration, one after the other, the same streamed bursts each (best of three
    timings): none takes more than 1.25 x what the first took."""
    import time
    import torch
    import xritdemod_amd as xa
    from xritdemod_amd import _capi
    n, D, fs, nb, steps = 1 << 28, 5, 6.25e6, 4, 12
    dev = torch.device("cuda", 0)
    buf = torch.empty((nb, n, 2), dtype=torch.float32, device=dev)
    sp = _capi.synth_params(fs_in=fs)
    st = torch.cuda.current_stream(dev).cuda_stream
    for b in range(nb):
        _capi.synth_generate_device(sp, b * n, n, buf[b].data_ptr(), device=0, stream=st)
    torch.cuda.synchronize(dev)
    cap = int(n / (D * 4.2)) + 4096
    soft = torch.empty(cap, dtype=torch.float32, device=dev)
    times = []
    for h in range(5):
        dem = xa.Demodulator(xa.Demodulator.config("lrit", fs, D))
        for b in range(3):                                   # warm-up: buffers grow, the loops lock
            dem.process_device(buf[b % nb].data_ptr(), n, soft.data_ptr(), cap, stream=st)
        torch.cuda.synchronize(dev)
        best = None
        for rep in range(3):                                 # (the best of three: a timing, on a box that does other things too)
            t0 = time.perf_counter()
            dem.prefetch_device(buf[3 % nb].data_ptr(), n, stream=st)
            dem.prefetch_device(buf[4 % nb].data_ptr(), n, stream=st)
            for b in range(3, 3 + steps):
                if b + 2 < 3 + steps:
                    dem.prefetch_device(buf[(b + 2) % nb].data_ptr(), n, stream=st)
                dem.process_device(buf[b % nb].data_ptr(), n, soft.data_ptr(), cap, stream=st)
            torch.cuda.synchronize(dev)
            t = (time.perf_counter() - t0) / steps * 1e3
            best = t if best is None else min(best, t)
        times.append(best)
        dem.close()
        del dem
    print("ms per burst, handle by handle:", [round(t, 3) for t in times])
    # (what the pool is for: 2.5 against 1.8 ms, a factor 1.39; one handle in five read 1.22 x the first once, in a single timing)
    assert max(times[1:]) <= 1.25 * times[0], times
