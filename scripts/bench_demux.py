"""Channel demultiplexer (xrit_demux_process_device) on the frame decoder's device-resident outputs: 65536 frames per
call with a skewed VCID mix (about 90 % on one channel, the rest on 20 others, fill included) and about 3 % corrupted
frames, timed with torch events after a warm-up -- the demux alone, and decode + demux queued on one stream.  Prints
one JSON line per case.  (Equality with the specification is tests/test_gpu_demux.py.)

    python scripts/bench_demux.py [--frames N] [--reps R] [--warmup W]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import xritdemod_amd as xa
import ccsds

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1 << 16)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

FR = ccsds.FRAME_SYMBOLS
nf = args.frames
dev = torch.device("cuda:0")

# 256 distinct CADUs with the skewed VCID mix, coded as one stream and tiled to nf frames
rng = np.random.default_rng(1)
base_n = min(256, nf)
others = [0, 1, 2, 3, 4, 6, 7, 9, 13, 20, 21, 30, 31, 32, 40, 41, 50, 60, 62, 63]
vcids = [5 if rng.random() < 0.9 else others[rng.integers(0, len(others))] for _ in range(base_n)]
blocks = np.stack([ccsds.make_block(0x8C, v, i, rng) for i, v in enumerate(vcids)])
cadus = np.stack([ccsds.cadu_from_block(b) for b in blocks])
base = torch.from_numpy(ccsds.coded_symbols(cadus, amplitude=40).reshape(base_n, FR).astype(np.int8)).to(dev)
frames = base.repeat((nf + base_n - 1) // base_n, 1)[:nf].contiguous()
bad = torch.from_numpy(np.nonzero(rng.random(nf) < 0.03)[0]).to(dev)
g = torch.Generator(device=dev)
g.manual_seed(7)
frames[bad] = torch.randint(-128, 128, (len(bad), FR), dtype=torch.int8, device=dev, generator=g)
valid = torch.ones(nf, dtype=torch.uint8, device=dev)
hits = torch.zeros((nf, 4), dtype=torch.int32, device=dev)
hits[:, 0] = torch.randint(0, 2, (nf,), dtype=torch.int32, device=dev, generator=g)
hits[:, 2] = 60
cadu = torch.empty((nf, 1024), dtype=torch.uint8, device=dev)
block = torch.empty((nf, 1020), dtype=torch.uint8, device=dev)
info = torch.empty(nf * xa.FRAME_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
vcdu = torch.empty((nf, 892), dtype=torch.uint8, device=dev)
offsets = torch.empty(65, dtype=torch.int32, device=dev)
records = torch.empty(nf * xa.FRAME_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
st = torch.cuda.current_stream(dev).cuda_stream
dec, dm = xa.FrameDecoder("lrit"), xa.ChannelDemux()


def decode():
    dec.decode_device(frames.data_ptr(), valid.data_ptr(), nf, cadu.data_ptr(), block.data_ptr(), info.data_ptr(), stream=st)


def demux():
    dm.process_device(hits.data_ptr(), cadu.data_ptr(), block.data_ptr(), info.data_ptr(), nf, vcdu.data_ptr(),
                      offsets.data_ptr(), records.data_ptr(), stream=st)


def both():
    decode()
    demux()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), min(times)


decode()
torch.cuda.synchronize()
inf = info.cpu().numpy().view(xa.FRAME_INFO_DTYPE)
good = int(inf["ok"].sum())
moved = nf * (16 + 4 + 40 + 88) + good * (892 + 892)          # bytes read + written, the VCDUs twice
for name, fn, reps, warm in (("demux", demux, args.reps, args.warmup), ("decode+demux", both, max(3, args.reps // 5), 2)):
    ms, mn = timed(fn, reps, warm)
    row = {"case": name, "frames": nf, "good": good, "channels": int((np.bincount(inf["vcid"][inf["ok"] == 1], minlength=64) > 0).sum()),
           "ms_median": round(ms, 4), "ms_min": round(mn, 4)}
    if name == "demux":
        row.update({"bound_ms": 0.5, "within_bound": ms <= 0.5, "GB_per_s": round(moved / ms / 1e6, 1)})
    print(json.dumps(row), flush=True)
off = offsets.cpu().numpy()
print(json.dumps({"case": "check", "vcdu_rows": int(off[64]), "good": good, "dropped": int(nf - good)}), flush=True)
