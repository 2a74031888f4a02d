"""The projection stage (xrit_geo_*) on a device-resident full disc, timed with torch events on the
stream after a warm-up; one JSON line per case, medians.  (Equality with the specification is tests/test_gpu_geo.py; the
lines "check" here compare the device's output with the host's of the same run.)

source     one 5424 x 5424 image at 8 bits and one at 10 bits, synthesised on the device (a smooth field plus noise, 339
           rows of a lost segment zero), navigated as a full disc: cfac = lfac = 20466275, coff = loff = 2713.
grids      3600 x 1800 (the whole globe at 0.1 degrees) and 5424 x 5424 (the disc's bounding box, 81.3 degrees either way
           of the sub-satellite point), both equirectangular; bilinear unless --mode says otherwise.
calls      fused (xrit_geo_project_device); map + resample (xrit_geo_map_device, xrit_geo_resample_device, queued back to
           back); resample alone on the stored map; map alone.
host       what the stage replaces, in the same run: the image downloaded and the NumPy specification run on it (the
           3600 x 1800 grid only, --host-runs times).  The two sides are not timed alike: the download is inside the host's
           timed region, the host's is wall-clock time of one core, the stage's is event time on the stream and leaves
           its output on the device.
rate       xrit_device_read_bandwidth from the same run, and beside it each call's algorithmic bytes over its time as a
           fraction of it.  Algorithmic bytes: fused -- the source once, the four tables, the output; map -- the tables and
           8 bytes per output pixel; resample -- the map, the source once, the output.  The source is counted whole
           although pixels off the disc or outside the grid are never read: an upper bound.

    python scripts/bench_geo.py [--size N] [--reps R] [--warmup W] [--mode bilinear|nearest] [--host-runs H]"""
import argparse
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
import geo_spec as gs

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=5424)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--mode", default="bilinear")
ap.add_argument("--host-runs", type=int, default=1)
args = ap.parse_args()

dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev).cuda_stream
SUB_LON = -75.2


def emit(**row):
    print(json.dumps(row), flush=True)


def timed(fn, reps=args.reps, warmup=args.warmup):
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


def u8(n):
    return torch.empty(n, dtype=torch.uint8, device=dev)


def synthesised(n, bits):
    """n x n samples of `bits` bits on the device: a smooth field, noise, and a lost segment's rows of zeros -> bytes."""
    g = torch.Generator(device=dev)
    g.manual_seed(5 + bits)
    top = (1 << bits) - 1
    y = torch.arange(n, device=dev, dtype=torch.float32).view(-1, 1)
    x = torch.arange(n, device=dev, dtype=torch.float32).view(1, -1)
    field = (0.45 + 0.35 * torch.sin(x / 700.0) * torch.cos(y / 900.0)) * top
    img = (field + torch.randn(n, n, device=dev, generator=g) * (0.03 * top)).clamp(1, top)
    img[n * 3 // 8:n * 3 // 8 + n // 16] = 0
    if bits <= 8:
        return img.to(torch.uint8).contiguous().view(-1)
    return img.to(torch.int16).contiguous().view(torch.uint8).view(-1)


probe = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
hbm = xa._capi.device_read_bandwidth(probe.data_ptr(), probe.numel(), reps=10, stream=st)
del probe
emit(case="device read rate", GB_per_s=round(hbm, 1))

n = args.size
scale = n / 5424.0
nav = gs.nav_of(int(20466275 * scale), int(20466275 * scale), n // 2 + 1, n // 2 + 1, 1, SUB_LON)
GRIDS = (("globe at 0.1 degrees", (gs.EQUIRECT, 3600, 1800, -180.0, 89.95, 0.1, 0.1), True),
         ("the disc's bounding box", (gs.EQUIRECT, 5424, 5424, SUB_LON - 81.3, 81.3, 162.6 / 5423, 162.6 / 5423), False))
gp = xa.ImageProjector()
mode = gs.MODES[args.mode]

for bits in (8, 10):
    width = 1 if bits <= 8 else 2
    d_img = synthesised(n, bits)
    source = (d_img.data_ptr(), n, n, n * width, bits)
    for name, grid, with_host in GRIDS:
        columns, rows = grid[1], grid[2]
        gp.set_grid(*grid, SUB_LON)
        pixels = columns * rows
        d_map, d_out, d_out2, d_sum, d_sum2 = u8(pixels * 8), u8(pixels * width), u8(pixels * width), u8(56), u8(56)
        fused = lambda: gp.project_device(nav, *source, mode, d_out.data_ptr(), columns * width, d_sum.data_ptr(), stream=st)
        the_map = lambda: gp.map_device(nav, d_map.data_ptr(), stream=st)
        resample = lambda: gp.resample_device(*source, d_map.data_ptr(), mode, d_out2.data_ptr(), columns * width, d_sum2.data_ptr(), stream=st)
        tables = 16 * (columns + rows)
        moved = {"fused": n * n * width + tables + pixels * width, "map": tables + pixels * 8, "resample alone": pixels * 8 + n * n * width + pixels * width}
        moved["map + resample"] = moved["map"] + moved["resample alone"]
        res = {}
        for case, fn in (("fused", fused), ("map + resample", lambda: (the_map(), resample())), ("resample alone", resample), ("map", the_map)):
            ms, mn = timed(fn)
            res[case] = ms
            emit(case=case, grid=name, bits=bits, mode=args.mode, columns=columns, rows=rows, source=n, ms_median=round(ms, 4), ms_min=round(mn, 4),
                 Mpixel_per_s=round(pixels / ms / 1e3, 1), algorithmic_bytes=moved[case], GB_per_s=round(moved[case] / ms / 1e6, 1),
                 fraction_of_read_rate=round(moved[case] / ms / 1e6 / hbm, 4))
        s = d_sum.cpu().numpy().view(xa.GEO_SUMMARY_DTYPE)[0]
        emit(case="check", grid=name, bits=bits, fused_equals_map_plus_resample=bool(torch.equal(d_out, d_out2) and torch.equal(d_sum, d_sum2)),
             fused_over_map_plus_resample=round(res["fused"] / res["map + resample"], 4), fused_no_slower=bool(res["fused"] <= res["map + resample"]),
             **{k: int(s[k]) for k in ("total", "off_disc", "outside", "no_data", "written")})
        if not with_host or args.host_runs < 1:
            emit(case="host: download the image, the NumPy specification (download inside, one core, wall clock)", grid=name, bits=bits,
                 ms_median="missing")
            continue
        tabs = gp.tables()

        def on_the_host():
            t = time.perf_counter()
            img = d_img.cpu().numpy().view(np.uint8 if bits <= 8 else np.uint16).reshape(n, n)
            t_down = time.perf_counter()
            out, _ = gs.project(img, tabs, nav, mode)
            done = time.perf_counter()
            return (done - t) * 1e3, (t_down - t) * 1e3, out

        runs = [on_the_host() for _ in range(args.host_runs)]
        host_ms, down_ms = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
        equal = np.array_equal(d_out.cpu().numpy().view(np.uint8 if bits <= 8 else np.uint16).reshape(rows, columns), runs[-1][2])
        emit(case="host: download the image, the NumPy specification (download inside, one core, wall clock)", grid=name, bits=bits,
             ms_median=round(host_ms, 1), of_which_download_ms=round(down_ms, 2), runs=len(runs), fused_over_host=round(res["fused"] / host_ms, 6),
             device_equals_host=bool(equal))
gp.close()
