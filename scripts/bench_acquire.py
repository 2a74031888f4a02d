"""The carrier acquisition stage on device-resident data, timed with torch events: medians of --reps calls after --warmup,
one JSON line per case.  (Equality with the specification is tests/test_gpu_acquire.py.)

mix       xrit_acquire_mix_device on --samples complex samples (default 2^28), cf32 and s8, next to a device-to-device
          hipMemcpyAsync of the same bytes (what the mix reads plus what it writes, halved: a copy of b bytes moves 2 b) timed
          in the same run, and next to xrit_device_read_bandwidth.
estimate  xrit_acquire_estimate_device at the defaults (pre_sum 1, 511 segments: 2^20 samples), cf32.

    python scripts/bench_acquire.py [--samples N] [--reps R] [--warmup W]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import xritdemod_amd as xa

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=1 << 28)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev).cuda_stream
n = args.samples


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


out = torch.empty(2 * n, dtype=torch.float32, device=dev)
probe = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
hbm = xa._capi.device_read_bandwidth(probe.data_ptr(), probe.numel(), reps=10, stream=st)
del probe
aq = xa.CarrierAcquirer(1.25e6)
aq.set_frequency(23000.0)
for name, sample_type, make in (("cf32", xa.SAMPLE_FLOATIQ, lambda: torch.randn(2 * n, dtype=torch.float32, device=dev) * 0.1),
                                ("s8", xa.SAMPLE_S8IQ, lambda: torch.randint(-128, 128, (2 * n,), dtype=torch.int8, device=dev))):
    src = make()
    moved = src.numel() * src.element_size() + 8 * n
    ms, mn = timed(lambda: aq.mix_device(src.data_ptr(), n, sample_type, out.data_ptr(), stream=st))
    half = moved // 2                       # a copy of `half` bytes reads and writes as many bytes as the mix moves
    a, b = out.view(torch.uint8)[:half], torch.empty(half, dtype=torch.uint8, device=dev)
    cms, cmn = timed(lambda: b.copy_(a))
    emit(case="mix", type=name, samples=n, bytes_moved=moved, ms_median=round(ms, 4), ms_min=round(mn, 4), GB_per_s=round(moved / ms / 1e6, 1),
         Gsamples_per_s=round(n / ms / 1e6, 2), copy_ms_median=round(cms, 4), copy_ms_min=round(cmn, 4), copy_GB_per_s=round(moved / cms / 1e6, 1),
         mix_over_copy=round(ms / cms, 3), device_read_GB_per_s=round(hbm, 1))
    del src, a, b
ne = 1 << 20
x = torch.randn(2 * ne, dtype=torch.float32, device=dev) * 0.1
rec = torch.zeros(64, dtype=torch.uint8, device=dev)
ms, mn = timed(lambda: aq.estimate_device(x.data_ptr(), ne, xa.SAMPLE_FLOATIQ, False, rec.data_ptr(), stream=st))
r = rec.cpu().numpy().view(xa.ACQUIRE_RECORD_DTYPE)[0]
emit(case="estimate", type="cf32", samples=ne, segments=int(r["segments"]), ms_median=round(ms, 4), ms_min=round(mn, 4),
     Msamples_per_s=round(ne / ms / 1e3, 1), status=int(r["status"]))
