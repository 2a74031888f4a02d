"""Packet assembler (xrit_packets_process_device) behind the frame decoder and the channel demultiplexer, everything
device resident: 65536 frames per call with a skewed VCID mix (about 90 % on one channel, the rest on 20 others, fill
included), about 3 % corrupted frames, and packet zones that carry LRIT-like space packets (most between 100 and 8198
bytes), timed with torch events after a warm-up -- the packet stage alone next to the demux alone on the same rows, and
decode + demux + packets next to decode + demux queued on one stream.  Prints one JSON line per case.  The frames are a
tile of 512 distinct CADUs repeated, so every channel's counters break once per tile (one packet dropped there).
(Equality with the specification is tests/test_gpu_packets.py.)

    python scripts/bench_packets.py [--frames N] [--reps R] [--warmup W]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1 << 16)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
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


two()
torch.cuda.synchronize()
few = max(3, args.reps // 5)
res = {}
for name, fn, reps, warm in (("demux", demux, args.reps, args.warmup), ("packets", packets, args.reps, args.warmup),
                             ("decode", decode, few, 2), ("decode+demux", two, few, 2), ("decode+demux+packets", three, few, 2)):
    ms, mn = timed(fn, reps, warm)
    res[name] = ms
    print(json.dumps({"case": name, "frames": nf, "ms_median": round(ms, 4), "ms_min": round(mn, 4)}), flush=True)
pa.reset()
packets()
torch.cuda.synchronize()
s = summary.cpu().numpy().view(xa.PACKETS_SUMMARY_DTYPE)[0]
moved = int(offsets.cpu().numpy()[64]) * 892 + int(s["bytes"]) + int(s["packets"]) * 32
print(json.dumps({"case": "check", "rows": int(s["rows"]), "packets": int(s["packets"]), "bytes": int(s["bytes"]),
                  "crc_failures": int(s["crc_failures"]), "discarded": int(s["discarded"]), "fill_packets": int(s["fill_packets"]),
                  "overflow": int(s["overflow"]), "packets_GB_per_s": round(moved / res["packets"] / 1e6, 1),
                  "packets_share_of_decode_percent": round(100 * res["packets"] / res["decode"], 3),
                  "chain_difference_ms": round(res["decode+demux+packets"] - res["decode+demux"], 4)}), flush=True)
