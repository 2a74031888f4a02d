"""The link monitor on device-resident symbols, timed with torch events: medians of --reps calls after --warmup, one JSON
line per case.  (Equality with the specification is tests/test_gpu_monitor.py.)

push      xrit_monitor_push_device on --symbols symbols (default 2^24), float32 and int8, blocks of 64, 16384 and 32768, next
          to xrit_device_read_bandwidth over the same bytes timed in the same run (the stage reads every symbol once and
          writes 64 bytes per block): push_over_read is the ratio of the two times.
chain     xrit_demod_process_device on a generated burst of 2^--burst-log2 samples (LRIT, 6.25 Msps, decimation 5: about
          12 M symbols at 28), alone and with the monitor queued behind it on the same stream.

    python scripts/bench_monitor.py [--symbols N] [--burst-log2 L] [--reps R] [--warmup W]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import xritdemod_amd as xa
from xritdemod_amd import _capi

ap = argparse.ArgumentParser()
ap.add_argument("--symbols", type=int, default=1 << 24)
ap.add_argument("--burst-log2", type=int, default=28)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream(dev)
st = stream.cuda_stream
n = args.symbols


def emit(**row):
    print(json.dumps(row), flush=True)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), min(times)


for name, symbol_type, make in (("f32", xa.SYMBOL_F32, lambda: (torch.randn(n, dtype=torch.float32, device=dev) * 0.25 + 0.4) *
                                  (torch.randint(0, 2, (n,), device=dev) * 2 - 1)),
                                ("i8", xa.SYMBOL_I8, lambda: torch.randint(-128, 128, (n,), dtype=torch.int8, device=dev))):
    src = make().contiguous()
    nbytes = src.numel() * src.element_size()
    read_gbs = _capi.device_read_bandwidth(src.data_ptr(), nbytes, reps=args.reps, stream=st)
    read_ms = nbytes / read_gbs / 1e6
    for block in (64, 16384, 32768):
        mon = xa.LinkMonitor(block, symbol_type)
        cap = n // block + 1
        rows = torch.zeros(64 * cap, dtype=torch.uint8, device=dev)
        summary = torch.zeros(32, dtype=torch.uint8, device=dev)
        ms, mn = timed(lambda: mon.push_device(src.data_ptr(), n, rows.data_ptr(), cap, summary.data_ptr(), stream=st))
        s = summary.cpu().numpy().view(xa.MONITOR_SUMMARY_DTYPE)[0]
        emit(case="push", type=name, block=block, symbols=n, bytes_read=nbytes, bytes_written=int(s["rows"]) * 64, ms_median=round(ms, 4),
             ms_min=round(mn, 4), GB_per_s=round(nbytes / ms / 1e6, 1), Gsymbols_per_s=round(n / ms / 1e6, 2), read_ms=round(read_ms, 4),
             device_read_GB_per_s=round(read_gbs, 1), push_over_read=round(ms / read_ms, 2))
        mon.close()
        del rows, summary
    del src

fs_in, D = 6.25e6, 5
n_burst = 1 << args.burst_log2
burst = torch.empty(2 * n_burst, dtype=torch.float32, device=dev)
_capi.synth_generate_device(_capi.synth_params(fs_in=fs_in), 0, n_burst, burst.data_ptr(), device=0, stream=st)
torch.cuda.synchronize()
cap = int(n_burst / (D * (fs_in / D / 293883.0) * 0.99)) + 64
soft = torch.empty(cap, dtype=torch.float32, device=dev)
dem = xa.Demodulator(xa.Demodulator.config("lrit", fs_in, D, device=0))
mon = xa.LinkMonitor(16384, xa.SYMBOL_F32)
rows = torch.zeros(64 * (cap // 16384 + 1), dtype=torch.uint8, device=dev)
symbols = [0]


def chain_alone():
    symbols[0] = dem.process_device(burst.data_ptr(), n_burst, soft.data_ptr(), cap, stream=st)


def chain_and_monitor():
    ns = dem.process_device(burst.data_ptr(), n_burst, soft.data_ptr(), cap, stream=st)
    mon.push_device(soft.data_ptr(), ns, rows.data_ptr(), cap // 16384 + 1, stream=st)
    symbols[0] = ns


ms_a, mn_a = timed(chain_alone)
ms_b, mn_b = timed(chain_and_monitor)
ms_m, mn_m = timed(lambda: mon.push_device(soft.data_ptr(), symbols[0], rows.data_ptr(), cap // 16384 + 1, stream=st))
emit(case="chain", samples=n_burst, symbols=symbols[0], block=16384, demod_ms_median=round(ms_a, 4), demod_ms_min=round(mn_a, 4),
     demod_and_monitor_ms_median=round(ms_b, 4), demod_and_monitor_ms_min=round(mn_b, 4), monitor_alone_ms_median=round(ms_m, 4),
     monitor_alone_ms_min=round(mn_m, 4), added_ms_median=round(ms_b - ms_a, 4))
