"""Frame decoder (xrit_decoder_decode_device: Viterbi27 + derandomiser + 4 x RS(255,223)) on device-resident frames:
65536 valid frames per call, clean coded CADUs and the same at Es/N0 4 dB, timed with torch events after a warm-up.
Prints one JSON line per case, and one for the test side's NumPy Viterbi (tests/ccsds.py) on a few frames on one host
core -- the specification, not the reference decoder.  (Equality with the specification is tests/test_gpu_decode.py.)

    python scripts/bench_decode.py [--frames N] [--reps R] [--no-cpu]"""
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
import ccsds

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1 << 16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-cpu", action="store_true")
args = ap.parse_args()

FR = ccsds.FRAME_SYMBOLS
nf = args.frames
dev = torch.device("cuda:0")

# 256 distinct CADUs coded as one stream, tiled to nf frames (one seam every 256 frames)
rng = np.random.default_rng(1)
base_n = min(256, nf)
blocks = np.stack([ccsds.make_block(0x8C, i % 64, i, rng) for i in range(base_n)])
cadus = np.stack([ccsds.cadu_from_block(b) for b in blocks])
amp = 40
base = torch.from_numpy(ccsds.coded_symbols(cadus, amplitude=amp).reshape(base_n, FR).astype(np.int16)).to(dev)
clean16 = base.repeat((nf + base_n - 1) // base_n, 1)[:nf]
g = torch.Generator(device=dev)
g.manual_seed(7)
sigma = amp / np.sqrt(2.0 * 10 ** (4.0 / 10))              # BPSK, Es/N0 = 4 dB
noisy = (clean16.float() + sigma * torch.randn(clean16.shape, device=dev, generator=g)).round().clamp(-128, 127).to(torch.int8)
clean = clean16.to(torch.int8)
del clean16

valid = torch.ones(nf, dtype=torch.uint8, device=dev)
cadu = torch.empty((nf, 1024), dtype=torch.uint8, device=dev)
block = torch.empty((nf, 1020), dtype=torch.uint8, device=dev)
info = torch.empty(nf * xa.FRAME_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
st = torch.cuda.current_stream(dev).cuda_stream

for name, frames in (("clean", clean), ("esn0_4dB", noisy)):
    dec = xa.FrameDecoder("lrit")

    def run():
        dec.decode_device(frames.data_ptr(), valid.data_ptr(), nf, cadu.data_ptr(), block.data_ptr(), info.data_ptr(), stream=st)

    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    inf = info.cpu().numpy().view(xa.FRAME_INFO_DTYPE)
    ms = float(np.median(times))
    print(json.dumps({"case": name, "frames": nf, "ms_median": round(ms, 3), "ms_min": round(min(times), 3),
                      "frames_per_ms": round(nf / ms, 1), "decoded_Mbit_per_s": round(nf * 8192 / ms / 1e3, 1),
                      "ok_frac": round(float(inf["ok"].mean()), 5),
                      "mean_viterbi_errors": round(float(inf["viterbi_errors"].mean()), 2),
                      "rs_corrections": int(np.where(inf["rs_errors"] > 0, inf["rs_errors"], 0).sum())}), flush=True)
    dec.close()

if not args.no_cpu:
    k = 4
    fr = noisy[:k].cpu().numpy()
    w, _, _ = ccsds.windows(fr, np.ones(k, np.uint8))
    t = time.perf_counter()
    ccsds.viterbi_batch(w)
    s = time.perf_counter() - t
    print(json.dumps({"case": "numpy_viterbi_spec_one_core", "frames": k, "s": round(s, 3), "frames_per_ms": round(k / s / 1e3, 5)}))
