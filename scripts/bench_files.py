"""File assembler (xrit_files_process_device) and Rice decoder (xrit_rice_decode_device), device resident.

Files: the 65536-frame case of scripts/bench_packets.py (skewed VCID mix, about 3 % corrupted frames, LRIT-like packets
of random bytes: every packet is unsegmented, so nearly every one is a one-piece file with a garbage header, over some
2000 APIDs per channel), timed with torch events after a warm-up -- the file stage alone, and decode + demux + packets
with and without the file stage queued behind it on the same stream, in the same run.

Rice: a batch of 8-bit lines (--lines x --samples, J = 16, on both kernel forms and then on the default; 512 distinct lines tiled, a fifth of each of the
specification's five generators, so every option occurs), as Msamples/s out and as a fraction of the device read rate
measured in the same run on bytes in plus bytes out.  Prints one JSON line per case; medians after the warm-up.
(Equality with the specifications is tests/test_gpu_files.py and tests/test_gpu_rice.py.)

    python scripts/bench_files.py [--frames N] [--reps R] [--warmup W] [--lines L] [--samples S]"""
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
import packet_spec as ps
import rice_spec as rs

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1 << 16)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--lines", type=int, default=8192)
ap.add_argument("--samples", type=int, default=2048)
args = ap.parse_args()

FR = ccsds.FRAME_SYMBOLS
nf = args.frames
dev = torch.device("cuda:0")

# 512 distinct CADUs with the skewed VCID mix; every channel's rows are one generator stream
rng = np.random.default_rng(1)
base_n = min(512, nf)
others = [0, 1, 2, 3, 4, 6, 7, 9, 13, 20, 21, 30, 31, 32, 40, 41, 50, 60, 62, 63]
vcids = [5 if rng.random() < 0.9 else others[rng.integers(0, len(others))] for _ in range(base_n)]


def lrit_like(n_rows):
    out, have = [], 0
    while have < (n_rows + 2) * ps.ZONE:
        u = rng.random()
        total = int(rng.integers(100, 8199)) if u < 0.85 else int(rng.integers(7, 100)) if u < 0.95 else int(rng.integers(8199, 30000))
        out.append(ps.make_packet(int(rng.integers(0, 2047)), len(out) & 0x3FFF, total, rng))
        have += total
    return out


rows = {}
for v in sorted(set(vcids)):
    n = vcids.count(v)
    if v == 63:
        z = rng.integers(0, 256, (n, 892), dtype=np.uint8)
        z[:, :6] = [ccsds.vcdu_header(0x8C, 63, i) for i in range(n)]
        rows[v] = [bytes(r) for r in z]
    else:
        rows[v] = [bytes(r) for r in ps.build_stream(v, lrit_like(n), rng, start_counter=1000 * v).rows][:n]
nxt = {v: 0 for v in rows}
sent = []
for v in vcids:
    sent.append(rows[v][nxt[v]])
    nxt[v] += 1
cadus = np.stack([ccsds.cadu_from_block(ps.block_of(r)) for r in sent])
base = torch.from_numpy(ccsds.coded_symbols(cadus, amplitude=40).reshape(base_n, FR).astype(np.int8)).to(dev)
frames = base.repeat((nf + base_n - 1) // base_n, 1)[:nf].contiguous()
bad = torch.from_numpy(np.nonzero(rng.random(nf) < 0.03)[0]).to(dev)
g = torch.Generator(device=dev)
g.manual_seed(7)
frames[bad] = torch.randint(-128, 128, (len(bad), FR), dtype=torch.int8, device=dev, generator=g)
valid = torch.ones(nf, dtype=torch.uint8, device=dev)
hits = torch.zeros((nf, 4), dtype=torch.int32, device=dev)
hits[:, 2] = 60
cadu = torch.empty((nf, 1024), dtype=torch.uint8, device=dev)
block = torch.empty((nf, 1020), dtype=torch.uint8, device=dev)
info = torch.empty(nf * xa.FRAME_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
vcdu = torch.empty((nf, 892), dtype=torch.uint8, device=dev)
offsets = torch.empty(65, dtype=torch.int32, device=dev)
records = torch.empty(nf * xa.FRAME_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
max_bytes, max_packets = xa.packets_max_bytes(nf), 16 * nf + 64
out_bytes = torch.empty(max_bytes, dtype=torch.uint8, device=dev)
out_desc = torch.empty(max_packets * xa.PACKET_DTYPE.itemsize, dtype=torch.uint8, device=dev)
pkt_offsets = torch.empty(65, dtype=torch.int32, device=dev)
summary = torch.empty(xa.PACKETS_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
st = torch.cuda.current_stream(dev).cuda_stream
dec, dm, pa = xa.FrameDecoder("lrit"), xa.ChannelDemux(), xa.PacketAssembler()


def decode():
    dec.decode_device(frames.data_ptr(), valid.data_ptr(), nf, cadu.data_ptr(), block.data_ptr(), info.data_ptr(), stream=st)


def demux():
    dm.process_device(hits.data_ptr(), cadu.data_ptr(), block.data_ptr(), info.data_ptr(), nf, vcdu.data_ptr(),
                      offsets.data_ptr(), records.data_ptr(), stream=st)


def packets():
    pa.process_device(vcdu.data_ptr(), offsets.data_ptr(), nf, out_bytes.data_ptr(), max_bytes, out_desc.data_ptr(),
                      max_packets, pkt_offsets.data_ptr(), summary.data_ptr(), stream=st)


def two():
    decode()
    demux()


def three():
    decode()
    demux()
    packets()


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



# the file stage's buffers: no call emits more pieces than packets, more bytes than it was given, more records than 2 x packets
fa = xa.FileAssembler()
f_bytes = torch.empty(max_bytes, dtype=torch.uint8, device=dev)
f_pieces = torch.empty(max_packets * xa.FILE_PIECE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
f_recs = torch.empty(2 * max_packets * xa.FILE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
f_summary = torch.empty(xa.FILES_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)


def files():
    fa.process_device(out_bytes.data_ptr(), max_bytes, out_desc.data_ptr(), pkt_offsets.data_ptr(), max_packets, f_bytes.data_ptr(),
                      max_bytes, f_pieces.data_ptr(), max_packets, f_recs.data_ptr(), 2 * max_packets, f_summary.data_ptr(), stream=st)


def four():
    three()
    files()


three()
torch.cuda.synchronize()
few = max(3, args.reps // 5)
res = {}
for name, fn, reps, warm in (("packets", packets, args.reps, args.warmup), ("files", files, args.reps, args.warmup),
                             ("decode+demux+packets", three, few, 2), ("decode+demux+packets+files", four, few, 2),
                             ("decode+demux+packets again", three, few, 2)):
    ms, mn = timed(fn, reps, warm)
    res[name] = ms
    print(json.dumps({"case": name, "frames": nf, "ms_median": round(ms, 4), "ms_min": round(mn, 4)}), flush=True)
fa.reset()
pa.reset()
packets()
files()
torch.cuda.synchronize()
s = f_summary.cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)[0]
p = summary.cpu().numpy().view(xa.PACKETS_SUMMARY_DTYPE)[0]
moved = int(p["bytes"]) + int(p["packets"]) * 32 + int(s["bytes"]) + int(s["pieces"]) * 32 + int(s["files"]) * 80
print(json.dumps({"case": "files check", "packets_in": int(p["packets"]), "bytes_in": int(p["bytes"]), "pieces": int(s["pieces"]),
                  "bytes": int(s["bytes"]), "records": int(s["files"]), "files_begun": int(s["files_begun"]),
                  "files_completed": int(s["files_completed"]), "bad_packets": int(s["bad_packets"]), "short_first": int(s["short_first"]),
                  "orphans": int(s["orphans"]), "overflow": int(s["overflow"]), "files_GB_per_s": round(moved / res["files"] / 1e6, 1),
                  "chain_difference_ms": round(res["decode+demux+packets+files"] - res["decode+demux+packets"], 4)}), flush=True)

# ---- Rice ----------------------------------------------------------------------------------------------------------
n, J, S, L = 8, 16, args.samples, args.lines
rng = np.random.default_rng(2)
stats = {}
distinct = [rs.random_line(rng, n, J, S, kind=rs.KINDS[i % len(rs.KINDS)], stats=stats)[1] for i in range(min(512, L))]
lines = [distinct[i % len(distinct)] for i in range(L)]
data, desc = rs.pack(lines)
d_data = torch.from_numpy(data.copy()).to(dev)
d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
d_out = torch.empty(L * S, dtype=torch.uint8, device=dev)
d_status = torch.empty(L, dtype=torch.uint8, device=dev)
rd = xa.RiceDecoder(n, J, S)


def rice():
    rd.decode_device(d_data.data_ptr(), len(data), d_desc.data_ptr(), 16, L, d_out.data_ptr(), d_status.data_ptr(), stream=st)


want = rs.decode_batch(distinct[:8], n, J, S)[0]
probe = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
hbm = xa._capi.device_read_bandwidth(probe.data_ptr(), probe.numel(), reps=10, stream=st)
moved = len(data) + L * S + L * 17
for form in ("lane", "wave", "default"):
    xa.rice_form(form)
    d_out.zero_()
    ms, mn = timed(rice, args.reps, args.warmup)
    assert np.array_equal(d_out.cpu().numpy().reshape(L, S)[:8], want) and not d_status.cpu().numpy().any()
    print(json.dumps({"case": "rice", "form": form, "bits": n, "block": J, "samples": S, "lines": L, "bytes_in": len(data),
                      "options": {str(k): v for k, v in sorted(stats.items(), key=str)}, "ms_median": round(ms, 4), "ms_min": round(mn, 4),
                      "Msamples_per_s": round(L * S / ms / 1e3, 1), "GB_per_s_in_plus_out": round(moved / ms / 1e6, 2),
                      "device_read_GB_per_s": round(hbm, 1), "fraction_of_read_rate": round(moved / ms / 1e6 / hbm, 5)}), flush=True)
