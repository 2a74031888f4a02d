"""The JPEG stage (xrit_jpeg_*) on a device-resident image, timed with torch events after a
warm-up; one JSON line per case, medians.  The device's bytes are checked equal to the specification's on this run.

stage      xrit_jpeg_encode_device on one 5424 x 5424 toned image synthesised on the device (a smooth field plus noise, 339
           rows of a lost segment zero), quality 90, restart = blocks per row, as one component; and the same size as
           interleaved RGB (the field in three phases).  ms per call, GB/s of pixels in, bytes out.
download   the file's bytes from the device, and the raw pixels from the device, wall clock.
host       the yardstick, in the same run: libjpeg-turbo through Pillow on one host core on the same pixels with the same
           parameters, wall clock ("missing" without Pillow); its bytes are compared with the device's too.
claim      device encode + download of the file against download of the raw pixels + the host's encode.
split      per kernel: this script under `rocprofv3 --kernel-trace --stats` with --once (profiles/jpeg_kernel_stats.csv).

    python scripts/bench_jpeg.py [--size N] [--reps R] [--warmup W] [--quality Q] [--once] [--no-spec]"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import xritdemod_amd as xa
import jpeg_spec as js

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=5424)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--quality", type=int, default=90)
ap.add_argument("--once", action="store_true", help="three encodes per case and nothing else: for a kernel trace")
ap.add_argument("--no-spec", action="store_true", help="skip the comparison with the specification (it takes a minute at full size)")
args = ap.parse_args()

dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev).cuda_stream


def emit(**row):
    print(json.dumps(row), flush=True)


def timed(fn, reps, warmup):
    times = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), min(times)


def wall(fn, runs=3):
    out, times = None, []
    for _ in range(runs):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), out


def synthesised(n, phase):
    """n x n toned bytes on the device: a smooth field, noise, and a lost segment's rows of zeros."""
    g = torch.Generator(device=dev)
    g.manual_seed(13 + phase)
    y = torch.arange(n, device=dev, dtype=torch.float32).view(-1, 1)
    x = torch.arange(n, device=dev, dtype=torch.float32).view(1, -1)
    field = (0.45 + 0.35 * torch.sin(x / 700.0 + phase) * torch.cos(y / 900.0 - phase)) * 255
    img = (field + torch.randn(n, n, device=dev, generator=g) * (0.03 * 255)).clamp(1, 255)
    img[n * 3 // 8:n * 3 // 8 + n // 16] = 0
    return img.to(torch.uint8)


n = args.size
restart = (n + 7) // 8
enc = xa.JpegEncoder(quality=args.quality, restart=restart)
grey = synthesised(n, 0).contiguous()
rgb = torch.stack([grey, synthesised(n, 1), synthesised(n, 2)], -1).contiguous()
for name, d_img, comps in (("grey", grey, 1), ("rgb", rgb, 3)):
    cap = enc.bound(comps, n, n)
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(16, dtype=torch.uint8, device=dev)

    def stage():
        enc.encode_device(d_img.data_ptr(), n, n, n * comps, comps, d_out.data_ptr(), cap, d_res.data_ptr(), stream=st)

    if args.once:
        timed(stage, 3, 0)
        continue
    ms, mn = timed(stage, args.reps, args.warmup)
    res = d_res.cpu().numpy().view(xa.JPEG_RESULT_DTYPE)[0]
    size = int(res["size"])
    pixels = n * n * comps
    emit(case="stage", image=name, columns=n, rows=n, components=comps, quality=args.quality, restart=restart, ms_median=round(ms, 4),
         ms_min=round(mn, 4), pixel_bytes_in=pixels, GB_per_s_of_pixels=round(pixels / ms / 1e6, 2), bytes_out=size, status=int(res["status"]),
         restarts=int(res["restarts"]), scratch_bound_bytes=cap, per_kernel_split="profiles/jpeg_kernel_stats.csv (this script with --once under a kernel trace)")
    file_ms, file = wall(lambda: d_out[:size].cpu().numpy().tobytes())
    raw_ms, raw = wall(lambda: d_img.cpu().numpy())
    emit(case="download", image=name, file_ms=round(file_ms, 3), file_bytes=size, raw_pixels_ms=round(raw_ms, 3), raw_bytes=pixels)
    host_ms = None
    try:
        from PIL import Image

        def host():
            buf = io.BytesIO()
            Image.fromarray(raw).save(buf, "JPEG", quality=args.quality, optimize=False, subsampling=0, restart_marker_blocks=restart)
            return buf.getvalue()

        torch.set_num_threads(1)
        host_ms, theirs = wall(host)
        emit(case="host: libjpeg-turbo through Pillow, one core, wall clock", image=name, ms_median=round(host_ms, 2), bytes_out=len(theirs),
             device_equals_pillow=bool(theirs == file))
    except ImportError:
        emit(case="host: libjpeg-turbo through Pillow, one core, wall clock", image=name, ms_median="missing")
    if host_ms is not None:
        ours, theirs_total = ms + file_ms, raw_ms + host_ms
        emit(case="claim: device encode + file download against raw download + host encode", image=name, device_ms=round(ours, 3),
             host_ms=round(theirs_total, 3), device_over_host=round(ours / theirs_total, 4), holds=bool(ours < theirs_total))
    if not args.no_spec:
        t = time.perf_counter()
        want, cnt = js.encode(raw, quality=args.quality, restart=restart)
        emit(case="check", image=name, device_equals_specification=bool(want == file), specification_s=round(time.perf_counter() - t, 1),
             stuffed=cnt["stuffed"], zrl=cnt["zrl"], restarts=cnt["restarts"])
        del want
    del d_out
enc.close()
