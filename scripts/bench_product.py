"""The product stage (xrit_product_*) on device-resident images, timed with torch events after a
warm-up; one JSON line per case, medians.  (Equality with the specification is tests/test_gpu_product.py; the lines
"check" here compare the device's outputs with the host's of the same run.)

stage      xrit_product_process_device on one 5424 x 5424 image at 8 bits and one at 10 bits, synthesised on the device (a
           smooth field plus noise, 339 rows of a lost segment zero), tone equalise, factor 8, every output written.
host       what the stage replaces, in the same run: the image downloaded and the same products made with NumPy (bincount,
           the specification's tone table from it, take, block sums).  The two sides are not timed alike: the download is
           inside the host's timed region (the host cannot work on what it has not got), the host's is wall-clock time
           of one core, the stage's is event time on the stream and leaves its products on the device.
rate       xrit_device_read_bandwidth from the same run, and beside it the stage's algorithmic bytes -- the source read twice,
           the histogram, the table, the toned image and the thumbnail written once -- over its time, as a fraction of it.
composite  xrit_product_composite_device on two toned images of that size and a random table.
chain      one packets + files + images + canvas call of `bench_backend.py canvas`'s shape (--canvases images of three
           segments at 2784 and 5424 columns, every call from a reset canvas handle, the reset outside the timed region)
           with and without a product call per canvas queued behind it on the same stream, the slots read in place.

    python scripts/bench_product.py [--size N] [--reps R] [--warmup W] [--canvases K] [--no-chain]"""
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
import product_spec as sp

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=5424)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--canvases", type=int, default=6)
ap.add_argument("--no-chain", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev).cuda_stream
F = 8


def emit(**row):
    print(json.dumps(row), flush=True)


def timed(fn, reps=args.reps, warmup=args.warmup, before=None):
    times = []
    for i in range(warmup + reps):
        if before:
            before()
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

pr = xa.ImageProduct()
n = args.size
toned = {}
for bits in (8, 10):
    width = 1 if bits <= 8 else 2
    d_img = synthesised(n, bits)
    sr, sc = sp.small_shape(n, n, F)
    d_hist, d_lut, d_tone, d_small, d_sum = u8(4 << bits), u8(1 << bits), u8(n * n), u8(sr * sc), u8(64)

    def stage():
        pr.process_device(d_img.data_ptr(), n, n, n * width, bits, d_sum.data_ptr(), tone="equalise", factor=F, d_hist_ptr=d_hist.data_ptr(),
                          d_lut_ptr=d_lut.data_ptr(), d_tone_ptr=d_tone.data_ptr(), d_small_ptr=d_small.data_ptr(), stream=st)

    ms, mn = timed(stage)
    moved = 2 * n * n * width + (4 << bits) + (1 << bits) + n * n + sr * sc
    emit(case="stage", bits=bits, columns=n, rows=n, tone="equalise", factor=F, ms_median=round(ms, 4), ms_min=round(mn, 4),
         algorithmic_bytes=moved, GB_per_s=round(moved / ms / 1e6, 1), fraction_of_read_rate=round(moved / ms / 1e6 / hbm, 4),
         per_kernel_split="missing")

    def on_the_host():
        t = time.perf_counter()
        img = d_img.cpu().numpy().view(np.uint8 if bits <= 8 else np.uint16).reshape(n, n)
        t_down = time.perf_counter()
        hist = np.bincount(img.reshape(-1), minlength=1 << bits)
        lut = sp.build_lut(hist, bits, sp.EQUALISE)[0]
        tone = lut.take(img)
        has = img != 0
        rows, cols = sr * F, sc * F
        cnt = np.zeros((rows, cols), np.int32)
        val = np.zeros((rows, cols), np.int32)
        cnt[:n, :n] = has
        val[:n, :n] = tone * has
        cnt, val = (a.reshape(sr, F, sc, F).sum(axis=(1, 3)) for a in (cnt, val))
        small = np.where(cnt == 0, 0, (2 * val + cnt) // np.maximum(2 * cnt, 1)).astype(np.uint8)
        done = time.perf_counter()
        return (done - t) * 1e3, (t_down - t) * 1e3, (hist, lut, tone, small)

    runs = [on_the_host() for _ in range(3)]
    host_ms, down_ms = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
    hist, lut, tone, small = runs[-1][2]
    s = d_sum.cpu().numpy().view(xa.PRODUCT_SUMMARY_DTYPE)[0]
    equal = (np.array_equal(d_hist.cpu().numpy().view(np.uint32), hist) and np.array_equal(d_lut.cpu().numpy(), lut) and
             np.array_equal(d_tone.cpu().numpy().reshape(n, n), tone) and np.array_equal(d_small.cpu().numpy().reshape(sr, sc), small))
    emit(case="host: download the image, NumPy bincount + take + block sums (download inside, one core, wall clock)", bits=bits,
         ms_median=round(host_ms, 2), of_which_download_ms=round(down_ms, 2), runs=len(runs), stage_over_host=round(ms / host_ms, 6))
    emit(case="check", bits=bits, device_equals_host=bool(equal), zeros=int(s["zeros"]), min_nz=int(s["min_nz"]), max_nz=int(s["max_nz"]),
         fallback=int(s["fallback"]), out_of_range=int(s["out_of_range"]))
    toned[bits] = d_tone

table = torch.randint(0, 256, (256 * 256 * 3,), dtype=torch.uint8, device=dev)
d_rgb = u8(n * n * 3)
ms, mn = timed(lambda: pr.composite_device(toned[8].data_ptr(), n, toned[10].data_ptr(), n, n, n, table.data_ptr(), d_rgb.data_ptr(), stream=st))
moved = 2 * n * n + 3 * n * n
want = sp.composite(toned[8].cpu().numpy().reshape(n, n)[:64], toned[10].cpu().numpy().reshape(n, n)[:64], table.cpu().numpy())
emit(case="composite", columns=n, rows=n, ms_median=round(ms, 4), ms_min=round(mn, 4), bytes_in_plus_out=moved,
     GB_per_s=round(moved / ms / 1e6, 1), fraction_of_read_rate=round(moved / ms / 1e6 / hbm, 4),
     first_64_rows_equal_specification=bool(np.array_equal(d_rgb.cpu().numpy()[:64 * n * 3].reshape(64, n, 3), want)))
del toned, d_rgb


def bench_chain():
    """`bench_backend.py canvas`'s stream and buffers; behind the canvas call one product call per canvas."""
    import canvas_spec as cs
    import image_spec as isp
    import packet_spec as ps
    rng = np.random.default_rng(4)
    keys = [(0, 10), (0, 11), (5, 700), (31, 2046)]
    items, shapes = [], {}
    for i in range(args.canvases):
        bits, J, cols, rows = (8, 16, 2784, 36) if i % 2 else (10, 32, 5424, 36)
        img = cs.samples(rng, bits, J, cols, rows, kinds=("walk3", "scaled"))
        key = keys[i % len(keys)]
        shapes[(key[0], 100 + i)] = (img, bits)
        items += cs.split_image(rng, img, bits, J, 100 + i, [key], [12, 24], name=b"bench image %d" % i)
    stream = isp.stream_of(rng, items)
    vcdu, offsets = ps.group({v: s.rows for v, s in ps.build_streams([(v, p) for v, p, _ in stream], rng, fill=0.0, idle=0.0).items()})
    rows = len(vcdu)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_vcdu, d_off = up(vcdu), up(offsets)
    mb, mp = xa.packets_max_bytes(rows), len(stream) + 64 * 3
    p_bytes, p_desc, p_off, p_sum = u8(mb), u8(mp * 32), u8(65 * 4), u8(xa.PACKETS_SUMMARY_DTYPE.itemsize)
    f_bytes, f_pieces, f_recs, f_sum = u8(mb), u8(mp * 32), u8(2 * mp * 80), u8(xa.FILES_SUMMARY_DTYPE.itemsize)
    slots, slot_bytes = max(8, args.canvases), 1 << 19
    pa, fa, im, cv = xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder(), xa.ImageCanvas(slots, slot_bytes)

    def packets():
        pa.process_device(d_vcdu.data_ptr(), d_off.data_ptr(), rows, p_bytes.data_ptr(), mb, p_desc.data_ptr(), mp, p_off.data_ptr(),
                          p_sum.data_ptr(), stream=st)

    def files():
        fa.process_device(p_bytes.data_ptr(), mb, p_desc.data_ptr(), p_off.data_ptr(), mp, f_bytes.data_ptr(), mb, f_pieces.data_ptr(), mp,
                          f_recs.data_ptr(), 2 * mp, f_sum.data_ptr(), stream=st)

    packets()
    files()
    torch.cuda.synchronize()
    fsum = f_sum.cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)[0]
    assert int(fsum["overflow"]) == 0
    recs = f_recs.cpu().numpy().view(xa.FILE_RECORD_DTYPE)[:int(fsum["files"])]
    max_out = xa.images_max_bytes(recs)
    o_bytes, o_lines, o_files, o_sum = u8(max_out + 8), u8(mp * 32), u8(2 * mp * 48), u8(xa.IMAGES_SUMMARY_DTYPE.itemsize)
    c_files, c_slots, c_sum = u8(2 * mp * 32), u8(slots * xa.CANVAS_SLOT_DTYPE.itemsize), u8(xa.CANVAS_SUMMARY_DTYPE.itemsize)

    def images():
        im.process_device(f_bytes.data_ptr(), mb, f_pieces.data_ptr(), mp, f_recs.data_ptr(), 2 * mp, f_sum.data_ptr(), o_bytes.data_ptr(),
                          max_out, o_lines.data_ptr(), mp, o_files.data_ptr(), o_sum.data_ptr(), stream=st)

    def canvas():
        cv.process_device(f_bytes.data_ptr(), mb, f_pieces.data_ptr(), mp, f_recs.data_ptr(), 2 * mp, f_sum.data_ptr(), o_bytes.data_ptr(),
                          max_out, o_lines.data_ptr(), mp, o_files.data_ptr(), o_sum.data_ptr(), c_files.data_ptr(), c_slots.data_ptr(),
                          c_sum.data_ptr(), stream=st)

    # the geometry of the canvases, which the product calls need on the host, from one run beforehand
    images()
    canvas()
    torch.cuda.synchronize()
    table = c_slots.cpu().numpy().view(xa.CANVAS_SLOT_DTYPE).copy()
    done = [i for i in range(slots) if table[i]["complete"]]
    outs = {}
    for i in done:
        r, c, bits = int(table[i]["max_row"]), int(table[i]["max_column"]), int(table[i]["bits"])
        sr, sc = sp.small_shape(r, c, F)
        outs[i] = (u8(r * c), u8(sr * sc), u8(64))

    def products():
        for i in done:
            t = table[i]
            d_tone, d_small, d_s = outs[i]
            pr.process_device(cv.pixels_device(i), int(t["max_column"]), int(t["max_row"]), int(t["pitch"]), int(t["bits"]), d_s.data_ptr(),
                              tone="equalise", factor=F, d_tone_ptr=d_tone.data_ptr(), d_small_ptr=d_small.data_ptr(), stream=st)

    res = {"packets+files+images+canvas": timed(lambda: (packets(), files(), images(), canvas()), before=cv.reset),
           "packets+files+images+canvas+products": timed(lambda: (packets(), files(), images(), canvas(), products()), before=cv.reset),
           "products alone, on the canvases of the call before": timed(products)}
    for name, (ms, mn) in res.items():
        emit(case=name, rows=rows, canvases=len(done), ms_median=round(ms, 4), ms_min=round(mn, 4))
    equal = True
    for i in done:
        img, bits = shapes[(int(table[i]["vcid"]), int(table[i]["image_id"]))]
        want = sp.process(img, bits, sp.EQUALISE, factor=F)
        equal = equal and np.array_equal(outs[i][0].cpu().numpy().reshape(img.shape), want["tone"]) and \
            np.array_equal(outs[i][1].cpu().numpy().reshape(want["small"].shape), want["small"])
    emit(case="chain check", canvases=len(done), product_calls=len(done), products_equal_specification=bool(equal),
         chain_difference_ms=round(res["packets+files+images+canvas+products"][0] - res["packets+files+images+canvas"][0], 4))
    for h in (pa, fa, im, cv):
        h.close()


if not args.no_chain:
    bench_chain()
pr.close()
