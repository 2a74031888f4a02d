"""The JPEG decoder stage (xrit_jpegdec_*) on device-resident streams, timed with torch events on the
stream after a warm-up; one JSON line per case, medians.  The inputs are made by the device encoder (section 25) from the
synthetic image of scripts/bench_jpeg.py:
  a  grey, quality 90, no restart markers        b  the same with a marker per block row
  c  RGB, no markers                             d  a batch of 256 segments of 464 x 464, grey, no markers
Per input: form 0 and form 1 in ms, the rounds form 1 needed, Pillow's decode of the same bytes on one host core (wall
clock), upload of the file plus device decode against host decode plus upload of the raw pixels.  The device's pixels are
compared with Pillow's on this run (which the CPU tier holds equal to the specification's), and with the specification's
own with --spec (minutes at full size).  Per kernel: this script with --once under `rocprofv3 --kernel-trace --stats`.

    python scripts/bench_jpegdec.py [--size N] [--reps R] [--warmup W] [--inputs abcd] [--once] [--spec]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=5424)
ap.add_argument("--segment", type=int, default=464)
ap.add_argument("--segments", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--inputs", default="abcd")
ap.add_argument("--once", action="store_true", help="three decodes per input and form and nothing else: for a kernel trace")
ap.add_argument("--spec", action="store_true", help="compare with the specification's own decode too")
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
    """scripts/bench_jpeg.py's: a smooth field, noise, and a lost segment's rows of zeros."""
    g = torch.Generator(device=dev)
    g.manual_seed(13 + phase)
    y = torch.arange(n, device=dev, dtype=torch.float32).view(-1, 1)
    x = torch.arange(n, device=dev, dtype=torch.float32).view(1, -1)
    field = (0.45 + 0.35 * torch.sin(x / 700.0 + phase) * torch.cos(y / 900.0 - phase)) * 255
    img = (field + torch.randn(n, n, device=dev, generator=g) * (0.03 * 255)).clamp(1, 255)
    img[n * 3 // 8:n * 3 // 8 + n // 16] = 0
    return img.to(torch.uint8)


def encoded(images, comps, restart):
    """The device encoder's files for the images, back to back at multiples of 16 -> (bytes on the device, items)."""
    enc = xa.JpegEncoder(quality=90, restart=restart)
    files = []
    for d_img in images:
        rows, columns = d_img.shape[:2]
        cap = enc.bound(comps, columns, rows)
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(16, dtype=torch.uint8, device=dev)
        enc.encode_device(d_img.data_ptr(), columns, rows, columns * comps, comps, d_out.data_ptr(), cap, d_res.data_ptr(), stream=st)
        torch.cuda.synchronize()
        files.append(d_out[:int(d_res.cpu().numpy().view(xa.JPEG_RESULT_DTYPE)[0]["size"])].clone())
    enc.close()
    items, at = np.zeros(len(files), xa.JPEGDEC_ITEM_DTYPE), 0
    for i, f in enumerate(files):
        items[i] = (at, len(f), 0)
        at += (len(f) + 15) & ~15
    d_bytes = torch.zeros(at, dtype=torch.uint8, device=dev)
    for it, f in zip(items, files):
        d_bytes[int(it["offset"]):int(it["offset"]) + len(f)] = f
    return d_bytes, items


n = args.size
grey = synthesised(n, 0).contiguous()
inputs = {}
if "a" in args.inputs:
    inputs["a: grey, no restart markers"] = ([grey], 1, 0)
if "b" in args.inputs:
    inputs["b: grey, a marker per block row"] = ([grey], 1, (n + 7) // 8)
if "c" in args.inputs:
    inputs["c: RGB, no restart markers"] = ([torch.stack([grey, synthesised(n, 1), synthesised(n, 2)], -1).contiguous()], 3, 0)
if "d" in args.inputs:
    s, per = args.segment, max(1, n // args.segment)
    segs = [grey[(i // per % per) * s:(i // per % per) * s + s, (i % per) * s:(i % per) * s + s].contiguous() for i in range(args.segments)]
    inputs["d: %d segments of %d x %d, grey, no restart markers" % (args.segments, s, s)] = (segs, 1, 0)

dec = xa.JpegDecoder()
for name, (images, comps, restart) in inputs.items():
    d_bytes, items = encoded(images, comps, restart)
    blocks = sum(((im.shape[0] + 7) // 8) * ((im.shape[1] + 7) // 8) * comps for im in images)
    out_bytes = sum((im.shape[0] * im.shape[1] * comps + 3) & ~3 for im in images)
    d_items = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    d_pixels = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    d_records = torch.zeros(64 * len(items), dtype=torch.uint8, device=dev)
    d_summary = torch.zeros(64, dtype=torch.uint8, device=dev)

    def stage():
        dec.decode_device(d_bytes.data_ptr(), len(d_bytes), d_items.data_ptr(), 16, len(items), d_pixels.data_ptr(), out_bytes, d_records.data_ptr(),
                          d_summary.data_ptr(), max_blocks=blocks, stream=st)

    host = d_bytes.cpu().numpy()
    files = [host[int(it["offset"]):int(it["offset"]) + int(it["length"])].tobytes() for it in items]
    results = {}
    for form in (0, 1):
        dec.set_form(form, 0)
        if args.once:
            timed(stage, 3, 0)
            continue
        first, _ = timed(stage, 1, 1)
        ms, mn = timed(stage, args.reps if first < 200 else 3, 0 if first >= 200 else args.warmup - 1)   # (a slow form: fewer, stated in `reps`)
        got = d_pixels.cpu().numpy().copy()
        summary = d_summary.cpu().numpy().view(xa.JPEGDEC_SUMMARY_DTYPE)[0]
        results[form] = (ms, got)
        emit(case="stage", input=name, form=form, ms_median=round(ms, 4), ms_min=round(mn, 4), file_bytes=int(items["length"].sum()), blocks=blocks,
             pixel_bytes_out=out_bytes, GB_per_s_of_pixels=round(out_bytes / ms / 1e6, 2), images=int(summary["images"]), overflow=int(summary["overflow"]),
             rounds=dec.rounds(), reps=args.reps if first < 200 else 3)
    if args.once:
        continue
    emit(case="forms agree", input=name, holds=bool(np.array_equal(results[0][1], results[1][1])),
         claim_form_1_beats_form_0=bool(results[1][0] < results[0][0]), form_1_over_form_0=round(results[1][0] / results[0][0], 4))
    records = d_records.cpu().numpy().view(xa.JPEGDEC_RECORD_DTYPE)
    try:
        from PIL import Image
        Image.MAX_IMAGE_PIXELS = None
        torch.set_num_threads(1)
        host_ms, theirs = wall(lambda: [np.asarray(Image.open(io.BytesIO(f))) for f in files], 3 if len(files) == 1 else 1)
        equal = all(np.array_equal(results[1][1][int(r["offset"]):int(r["offset"] + r["length"])], t.reshape(-1)) for r, t in zip(records, theirs))
        emit(case="host: libjpeg-turbo through Pillow, one core, wall clock", input=name, ms_median=round(host_ms, 2), device_equals_pillow=bool(equal))
        up_file, _ = wall(lambda: (torch.from_numpy(host).to(dev), torch.cuda.synchronize()))
        raw = np.concatenate([t.reshape(-1) for t in theirs])
        up_raw, _ = wall(lambda: (torch.from_numpy(raw).to(dev), torch.cuda.synchronize()))
        ours, other = up_file + min(results[0][0], results[1][0]), host_ms + up_raw
        emit(case="claim: upload of the file + device decode against host decode + upload of the raw pixels", input=name, file_upload_ms=round(up_file, 3),
             raw_upload_ms=round(up_raw, 3), device_ms=round(ours, 3), host_ms=round(other, 3), holds=bool(ours < other))
    except ImportError:
        emit(case="host: libjpeg-turbo through Pillow, one core, wall clock", input=name, ms_median="missing")
    if args.spec:
        import jpegdec_spec as ds
        ok = True
        for r, f in zip(records, files):
            status, pixels, _, _ = ds.decode(f)
            ok = ok and status == 0 and np.array_equal(results[1][1][int(r["offset"]):int(r["offset"] + r["length"])], pixels.reshape(-1))
        emit(case="specification", input=name, device_equals_specification=bool(ok))
    del d_bytes, d_pixels
dec.close()
