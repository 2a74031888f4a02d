"""The map overlay stage (xrit_overlay_*) at one real size, timed with torch events on the stream
after a warm-up; one JSON line per case, medians.  (Equality with the specification is tests/test_gpu_overlay.py; the lines
"check" here compare the two forms of the draw, and the device's blend with the host's of the same run.)

image      5424 x 5424 at 8 bits, synthesised on the device.
vertices   a 1 degree graticule densified to 0.05 degrees (2.6 million vertices of one to three pixels a segment, on the
           grid of the disc's bounding box, which wraps: max_jump half the grid's width) and a random walk of 200 000
           vertices with a segment of thousands of pixels every thousandth: the mixed workload.
calls      map (the graticule's quads through the scan geometry); draw in form 0 and form 1, with clear; blend 1 -> 1 in
           place and 1 -> 3; the product stage's call (histogram, table, toned image) on the same image as the yardstick
           of a kernel that reads and writes an image once.
host       what the blend replaces, in the same run: the image and the mask downloaded, the NumPy specification's blend,
           the result uploaded (--host-runs times, wall clock of one core; the stage's is event time on the stream).
rate       xrit_device_read_bandwidth from the same run, and beside it each call's algorithmic bytes over its time as a
           fraction of it.  Algorithmic bytes: blend -- the image, the mask and the output once; map -- 32 bytes in and 8
           out per vertex; draw -- 8 bytes per vertex (form 1: twice, and 8 bytes of prefix written and read) and the
           mask's clear; the atomics are not counted.

    python scripts/bench_overlay.py [--size N] [--reps R] [--warmup W] [--host-runs H] [--out FILE]   (FILE: where the lines are
    kept as well, profiles/overlay_bench.txt unless given; - for nowhere)"""
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
import overlay_spec as ovs

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=5424)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--host-runs", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_bench.txt"))
args = ap.parse_args()

dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev).cuda_stream
SUB_LON = -75.2
STYLES = [(255, 255, 0, 255), (0, 255, 255, 128)] + [(255, 255, 255, 255)] * 6
out_file = open(args.out, "w") if args.out and args.out != "-" else None


def emit(**row):
    text = json.dumps(row)
    print(text, flush=True)
    if out_file:
        out_file.write(text + "\n")
        out_file.flush()


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


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)


probe = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
hbm = xa._capi.device_read_bandwidth(probe.data_ptr(), probe.numel(), reps=10, stream=st)
del probe
emit(case="device read rate", GB_per_s=round(hbm, 1))

n = args.size
g = torch.Generator(device=dev)
g.manual_seed(28)
y = torch.arange(n, device=dev, dtype=torch.float32).view(-1, 1)
x = torch.arange(n, device=dev, dtype=torch.float32).view(1, -1)
d_img = ((0.45 + 0.35 * torch.sin(x / 700.0) * torch.cos(y / 900.0)) * 255 + torch.randn(n, n, device=dev, generator=g) * 8).clamp(1, 255)
d_img = d_img.to(torch.uint8).contiguous().view(-1)

lon, lat = xa.overlay_densify(*xa.overlay_graticule(1.0, 1.0), 0.05)
step = 162.6 / (n - 1)
grat = xa.overlay_grid_points("equirect", n, n, SUB_LON - 81.3, 81.3, step, step, lon, lat)
rng = np.random.default_rng(50)
walk_step = rng.integers(-600, 601, (200000, 2))
walk_step[::1000] = rng.integers(-(1 << 20), 1 << 20, (200, 2))
walk = (np.cumsum(walk_step, axis=0) + n * 128) % (n * 256 + 100000) - 50000
points = np.concatenate([np.stack([grat["qx"], grat["qy"]], axis=1), [[ovs.BREAK, ovs.BREAK]], walk]).astype(np.int32)
nv = len(points)
d_points = up(points)
pitch = (n + 3) // 4 * 4
ov = xa.MapOverlay()

# ---- map ----
scale = n / 5424.0
nav = gs.nav_of(int(20466275 * scale), int(20466275 * scale), n // 2 + 1, n // 2 + 1, 1, SUB_LON)
quads = xa.overlay_quads(lon, lat, SUB_LON)
d_quads, d_mapped = up(quads), u8(len(quads) * 8)
ms, mn = timed(lambda: ov.map_device(nav, d_quads.data_ptr(), len(quads), d_mapped.data_ptr(), stream=st))
moved = len(quads) * 40
emit(case="map", vertices=len(quads), ms_median=round(ms, 4), ms_min=round(mn, 4), algorithmic_bytes=moved, GB_per_s=round(moved / ms / 1e6, 1),
     fraction_of_read_rate=round(moved / ms / 1e6 / hbm, 4), breaks=int((d_mapped.cpu().numpy().view(np.int32)[::2] == ovs.BREAK).sum()))

# ---- draw, both forms ----
res, masks, sums = {}, {}, {}
for form in (0, 1):
    ov.set_form(form)
    d_mask, d_sum = u8(n * pitch), u8(64)
    ms, mn = timed(lambda: ov.draw_device(d_points.data_ptr(), nv, 0, 1, n * 128, d_mask.data_ptr(), n, n, pitch, True, d_sum.data_ptr(), stream=st))
    s = d_sum.cpu().numpy().view(xa.OVERLAY_DRAW_SUMMARY_DTYPE)[0]
    res[form], masks[form], sums[form] = ms, d_mask, s
    moved = nv * 8 * (1 if form == 0 else 4) + n * pitch
    emit(case="draw, form %d" % form, vertices=nv, ms_median=round(ms, 4), ms_min=round(mn, 4), steps=int(s["steps"]), drawn=int(s["drawn"]),
         jumps=int(s["jumps"]), outside=int(s["outside"]), Msteps_per_s=round(int(s["steps"]) / ms / 1e3, 1), algorithmic_bytes=moved,
         GB_per_s=round(moved / ms / 1e6, 1))
same = bool(torch.equal(masks[0], masks[1]) and sums[0].tobytes() == sums[1].tobytes())
ms_clear, _ = timed(lambda: masks[1].zero_())
emit(case="check", form_1_equals_form_0=same,
     form_1_over_form_0=round(res[1] / res[0], 4), form_1_no_slower=bool(res[1] <= res[0]), the_mask_s_clear_alone_ms=round(ms_clear, 4))
ov.set_form(1)
d_last = u8(64)
ov.draw_device(d_points.data_ptr(), nv, 0, 1, n * 128, masks[1].data_ptr(), n, n, pitch, True, d_last.data_ptr(), stream=st)
torch.cuda.synchronize()
d_mask = masks[1]

# ---- blend, and the product stage's call as the yardstick ----
d_work, d_rgb, d_bsum = d_img.clone(), u8(n * n * 3), u8(96)
blends = {}
for case, fn, moved in (
        ("blend 1 -> 1, in place", lambda: ov.blend_device(d_work.data_ptr(), n, n, n, 1, d_mask.data_ptr(), pitch, STYLES, d_work.data_ptr(), n, 1,
                                                           d_bsum.data_ptr(), stream=st), 3 * n * n),
        ("blend 1 -> 3", lambda: ov.blend_device(d_img.data_ptr(), n, n, n, 1, d_mask.data_ptr(), pitch, STYLES, d_rgb.data_ptr(), 3 * n, 3,
                                                 d_bsum.data_ptr(), stream=st), 5 * n * n)):
    ms, mn = timed(fn)
    blends[case] = ms
    emit(case=case, ms_median=round(ms, 4), ms_min=round(mn, 4), algorithmic_bytes=moved, GB_per_s=round(moved / ms / 1e6, 1),
         fraction_of_read_rate=round(moved / ms / 1e6 / hbm, 4))
pr = xa.ImageProduct()
d_tone, d_psum = u8(n * n), u8(64)
ms, mn = timed(lambda: pr.process_device(d_img.data_ptr(), n, n, n, 8, d_psum.data_ptr(), tone="equalise", d_tone_ptr=d_tone.data_ptr(), stream=st))
moved = 3 * n * n
emit(case="yardstick: the product stage's call (histogram, table, toned image)", ms_median=round(ms, 4), ms_min=round(mn, 4), algorithmic_bytes=moved,
     GB_per_s=round(moved / ms / 1e6, 1), fraction_of_read_rate=round(moved / ms / 1e6 / hbm, 4))

# ---- what the blend replaces ----
if args.host_runs < 1:
    emit(case="host: download the image and the mask, the NumPy specification's blend 1 -> 3, upload", ms_median="missing")
else:
    def on_the_host():
        t = time.perf_counter()
        img = d_img.cpu().numpy().reshape(n, n)
        mask = d_mask.cpu().numpy().reshape(n, pitch)[:, :n]
        t_down = time.perf_counter()
        out, _ = ovs.blend(img, mask, STYLES, 3)
        t_done = time.perf_counter()
        d = torch.from_numpy(out).to(dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, (t_down - t) * 1e3, (t_done - t_down) * 1e3, d

    runs = [on_the_host() for _ in range(args.host_runs)]
    ov.blend_device(d_img.data_ptr(), n, n, n, 1, d_mask.data_ptr(), pitch, STYLES, d_rgb.data_ptr(), 3 * n, 3, d_bsum.data_ptr(), stream=st)
    torch.cuda.synchronize()
    host_ms = float(np.median([r[0] for r in runs]))
    emit(case="host: download the image and the mask, the NumPy specification's blend 1 -> 3, upload", ms_median=round(host_ms, 1),
         of_which_download_ms=round(float(np.median([r[1] for r in runs])), 2), of_which_numpy_ms=round(float(np.median([r[2] for r in runs])), 1),
         runs=len(runs), blend_over_host=round(blends["blend 1 -> 3"] / host_ms, 6), device_equals_host=bool(torch.equal(d_rgb, runs[-1][3].view(-1))))
emit(case="host: the draw", ms_median="missing", why="the specification walks vertex by vertex in Python: no fair yardstick for 2.8 million vertices")
pr.close()
ov.close()
