"""The stages behind the demodulator on device-resident data, timed with torch events after a warm-up; one JSON line per
case, medians.  (Equality with the specifications is tests/test_gpu_{decode,demux,packets,files,rice}.py.)

decode   xrit_decoder_decode_device (Viterbi27 + derandomiser + 4 x RS(255,223)): 65536 valid frames per call, clean
         coded CADUs and the same at Es/N0 4 dB; and the test side's NumPy Viterbi (tests/ccsds.py) on a few frames on
         one host core -- the specification, not the reference decoder (--no-cpu leaves it out).
demux    xrit_demux_process_device on the decoder's outputs: a skewed VCID mix (about 90 % on one channel, the rest on
         20 others, fill included), about 3 % corrupted frames -- the demux alone, and decode + demux on one stream.
packets  xrit_packets_process_device behind the two: the same mix with packet zones that carry LRIT-like space packets
         (most between 100 and 8198 bytes; a tile of 512 distinct CADUs repeated, so every channel's counters break once
         per tile) -- the packet stage next to the demux on the same rows, and the chain with and without it.
files    xrit_files_process_device on that case's packets (random bytes: nearly every one is a one-piece file with a
         garbage header, over some 2000 APIDs per channel) -- the file stage alone, and the chain with and without it.
rice     xrit_rice_decode_device: --lines x --samples 8-bit lines, J = 16, on both kernel forms and then on the default
         (512 distinct lines tiled, a fifth of each of the specification's five generators, so every option occurs), as
         Msamples/s and as a fraction of the device read rate measured in the same run on bytes in plus bytes out.
framer   xrit_framer_push_device (the stream frame synchroniser) on a frame-aligned LRIT stream of --frames frames, the same
         stream with one symbol deleted every 50 frames, and what existed before it on the aligned stream:
         xrit_sync_correlate_device + xrit_sync_fix_frames_device over fixed windows (calls of at most 65535 frames).  Then
         the framer at other segment lengths, with the share of chunks its joints walked again.
lock     xrit_lock_push_device (the frame lock: framer and decoder as the reference's one loop, with its flywheel) on the
         framer leg's two streams, at recheck 4 and at recheck 1, next to xrit_framer_push_device +
         xrit_decoder_decode_device queued on one stream: ms per call, rounds, sensitive chunks, chunks kept and missed in
         the short range.
images   xrit_images_process_device on one files call that holds --images rice-coded images of mixed (bits, block, columns,
         rows) and half as many files that are no images, next to what it replaces in the same process on the same
         device-resident bytes: one xrit_rice_decode_device per rice record (the records read back beforehand, which the
         loop needs and the stage does not; that read-back and its synchronisation are outside the timed region).  Then
         packets + files on one stream with and without the stage behind them.
canvas   xrit_canvas_process_device on one files call of --canvases images of three segments each over four keys at real
         widths (2784 and 5424 columns), every call from a reset handle (the reset is outside the timed region): the stage
         alone, and packets + files + images with and without it on one stream.  Beside it what the stage replaces:
         downloading the image stage's lines and placing them on the host with NumPy (the download is inside that timed
         region: the host cannot place what it has not got; the stage's own read-back of the finished canvases is
         outside its timed region and reported on its own line).  The bytes the place kernel reads plus writes over
         the whole stage's time -- a lower bound on that kernel's rate -- next to the device read rate of the same run.
all      the seven in front of images, in this order (images and canvas are asked for by name).

    python scripts/bench_backend.py {decode,demux,packets,files,rice,framer,lock,images,canvas,all} [--frames N] [--images I] [--reps R] [--warmup W]
                                    [--lines L] [--samples S] [--no-cpu]"""
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
import packet_spec as ps
import rice_spec as rs

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["decode", "demux", "packets", "files", "rice", "framer", "lock", "images", "canvas", "all"])
ap.add_argument("--canvases", type=int, default=6)
ap.add_argument("--images", type=int, default=96)
ap.add_argument("--frames", type=int, default=1 << 16)
ap.add_argument("--reps", type=int, default=None, help="timed calls per case (decode: 5, the others: 20)")
ap.add_argument("--warmup", type=int, default=None, help="calls before them (decode: 2, the others: 3)")
ap.add_argument("--lines", type=int, default=8192)
ap.add_argument("--samples", type=int, default=2048)
ap.add_argument("--no-cpu", action="store_true")
args = ap.parse_args()

FR = ccsds.FRAME_SYMBOLS
nf = args.frames
dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev).cuda_stream
OTHERS = [0, 1, 2, 3, 4, 6, 7, 9, 13, 20, 21, 30, 31, 32, 40, 41, 50, 60, 62, 63]


def emit(**row):
    print(json.dumps(row), flush=True)


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


def u8(n):
    return torch.empty(n, dtype=torch.uint8, device=dev)


def tiled(cadus, dtype):
    """The CADUs coded as one stream, tiled to nf frames (one seam per tile)."""
    base = torch.from_numpy(ccsds.coded_symbols(cadus, amplitude=40).reshape(len(cadus), FR).astype(dtype)).to(dev)
    return base.repeat((nf + len(cadus) - 1) // len(cadus), 1)[:nf].contiguous()


def skewed_vcids(rng, n):
    return [5 if rng.random() < 0.9 else OTHERS[rng.integers(0, len(OTHERS))] for _ in range(n)]


def lrit_like_rows(rng, vcids):
    """One 892-byte row per entry of vcids; every channel's rows are one generator stream of LRIT-like packets."""
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
    return sent


class Chain:
    """The skewed mix with about 3 % corrupted frames, every stage's buffers and handle, and the stages as closures that
    queue on the current stream.  zones: "random" (256 distinct CADUs, random phase words in the hits) or "packets" (512)."""

    def __init__(self, zones):
        rng = np.random.default_rng(1)
        base_n = min(256 if zones == "random" else 512, nf)
        vcids = skewed_vcids(rng, base_n)
        if zones == "random":
            blocks = [ccsds.make_block(0x8C, v, i, rng) for i, v in enumerate(vcids)]
        else:
            blocks = [ps.block_of(r) for r in lrit_like_rows(rng, vcids)]
        self.frames = tiled(np.stack([ccsds.cadu_from_block(b) for b in blocks]), np.int8)
        bad = torch.from_numpy(np.nonzero(rng.random(nf) < 0.03)[0]).to(dev)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        self.frames[bad] = torch.randint(-128, 128, (len(bad), FR), dtype=torch.int8, device=dev, generator=g)
        self.valid = torch.ones(nf, dtype=torch.uint8, device=dev)
        self.hits = torch.zeros((nf, 4), dtype=torch.int32, device=dev)
        if zones == "random":
            self.hits[:, 0] = torch.randint(0, 2, (nf,), dtype=torch.int32, device=dev, generator=g)
        self.hits[:, 2] = 60
        self.cadu, self.block, self.info = u8(nf * 1024), u8(nf * 1020), u8(nf * xa.FRAME_INFO_DTYPE.itemsize)
        self.vcdu, self.records = u8(nf * 892), u8(nf * xa.FRAME_STATS_DTYPE.itemsize)
        self.offsets, self.pkt_offsets = (torch.empty(65, dtype=torch.int32, device=dev) for _ in range(2))
        self.max_bytes, self.max_packets = xa.packets_max_bytes(nf), 16 * nf + 64
        self.handles = []
        if zones == "packets":
            self.out_bytes, self.out_desc = u8(self.max_bytes), u8(self.max_packets * xa.PACKET_DTYPE.itemsize)
            self.summary = u8(xa.PACKETS_SUMMARY_DTYPE.itemsize)
            # the file stage: no call emits more pieces than packets, more bytes than it was given, more records than 2 x packets
            self.f_bytes, self.f_pieces = u8(self.max_bytes), u8(self.max_packets * xa.FILE_PIECE_DTYPE.itemsize)
            self.f_recs, self.f_summary = u8(2 * self.max_packets * xa.FILE_RECORD_DTYPE.itemsize), u8(xa.FILES_SUMMARY_DTYPE.itemsize)

    def fresh_handles(self):
        for h in self.handles:
            h.close()
        self.dec, self.dm, self.pa, self.fa = self.handles = [xa.FrameDecoder("lrit"), xa.ChannelDemux(), xa.PacketAssembler(),
                                                               xa.FileAssembler()]

    def decode(self):
        self.dec.decode_device(self.frames.data_ptr(), self.valid.data_ptr(), nf, self.cadu.data_ptr(), self.block.data_ptr(),
                               self.info.data_ptr(), stream=st)

    def demux(self):
        self.dm.process_device(self.hits.data_ptr(), self.cadu.data_ptr(), self.block.data_ptr(), self.info.data_ptr(), nf,
                               self.vcdu.data_ptr(), self.offsets.data_ptr(), self.records.data_ptr(), stream=st)

    def packets(self):
        self.pa.process_device(self.vcdu.data_ptr(), self.offsets.data_ptr(), nf, self.out_bytes.data_ptr(), self.max_bytes,
                               self.out_desc.data_ptr(), self.max_packets, self.pkt_offsets.data_ptr(), self.summary.data_ptr(), stream=st)

    def files(self):
        self.fa.process_device(self.out_bytes.data_ptr(), self.max_bytes, self.out_desc.data_ptr(), self.pkt_offsets.data_ptr(),
                               self.max_packets, self.f_bytes.data_ptr(), self.max_bytes, self.f_pieces.data_ptr(), self.max_packets,
                               self.f_recs.data_ptr(), 2 * self.max_packets, self.f_summary.data_ptr(), stream=st)

    def chain(self, *stages):
        def run():
            for s in stages:
                s()
        return run

    def run_cases(self, first, cases):
        """On fresh handles first() once, then every (name, fn, many) timed: args.reps calls after args.warmup, or a fifth
        of them after 2."""
        self.fresh_handles()
        first()
        torch.cuda.synchronize()
        reps, warm = args.reps or 20, 3 if args.warmup is None else args.warmup
        res = {}
        for name, fn, many in cases:
            res[name] = timed(fn, reps if many else max(3, reps // 5), warm if many else 2)
        return res


def bench_decode():
    rng = np.random.default_rng(1)
    base_n = min(256, nf)
    blocks = [ccsds.make_block(0x8C, i % 64, i, rng) for i in range(base_n)]
    clean16 = tiled(np.stack([ccsds.cadu_from_block(b) for b in blocks]), np.int16)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    sigma = 40 / np.sqrt(2.0 * 10 ** (4.0 / 10))               # BPSK, Es/N0 = 4 dB
    noisy = (clean16.float() + sigma * torch.randn(clean16.shape, device=dev, generator=g)).round().clamp(-128, 127).to(torch.int8)
    clean = clean16.to(torch.int8)
    del clean16
    valid = torch.ones(nf, dtype=torch.uint8, device=dev)
    cadu, block, info = u8(nf * 1024), u8(nf * 1020), u8(nf * xa.FRAME_INFO_DTYPE.itemsize)
    for name, frames in (("clean", clean), ("esn0_4dB", noisy)):
        dec = xa.FrameDecoder("lrit")
        ms, mn = timed(lambda: dec.decode_device(frames.data_ptr(), valid.data_ptr(), nf, cadu.data_ptr(), block.data_ptr(),
                                                 info.data_ptr(), stream=st), args.reps or 5, 2 if args.warmup is None else args.warmup)
        inf = info.cpu().numpy().view(xa.FRAME_INFO_DTYPE)
        emit(case=name, frames=nf, ms_median=round(ms, 3), ms_min=round(mn, 3), frames_per_ms=round(nf / ms, 1),
             decoded_Mbit_per_s=round(nf * 8192 / ms / 1e3, 1), ok_frac=round(float(inf["ok"].mean()), 5),
             mean_viterbi_errors=round(float(inf["viterbi_errors"].mean()), 2),
             rs_corrections=int(np.where(inf["rs_errors"] > 0, inf["rs_errors"], 0).sum()))
        dec.close()
    if not args.no_cpu:
        k = 4
        w, _, _ = ccsds.windows(noisy[:k].cpu().numpy(), np.ones(k, np.uint8))
        t = time.perf_counter()
        ccsds.viterbi_batch(w)
        s = time.perf_counter() - t
        emit(case="numpy_viterbi_spec_one_core", frames=k, s=round(s, 3), frames_per_ms=round(k / s / 1e3, 5))


def bench_demux():
    c = Chain("random")
    seen = {}

    def first():
        c.decode()
        seen["info"] = c.info.cpu().numpy().view(xa.FRAME_INFO_DTYPE)

    res = c.run_cases(first, (("demux", c.demux, True), ("decode+demux", c.chain(c.decode, c.demux), False)))
    inf = seen["info"]
    good = int(inf["ok"].sum())
    moved = nf * (16 + 4 + 40 + 88) + good * (892 + 892)          # bytes read + written, the VCDUs twice
    for name, (ms, mn) in res.items():
        row = dict(case=name, frames=nf, good=good, channels=int((np.bincount(inf["vcid"][inf["ok"] == 1], minlength=64) > 0).sum()),
                   ms_median=round(ms, 4), ms_min=round(mn, 4))
        if name == "demux":
            row.update(bound_ms=0.5, within_bound=ms <= 0.5, GB_per_s=round(moved / ms / 1e6, 1))
        emit(**row)
    emit(case="check", vcdu_rows=int(c.offsets.cpu().numpy()[64]), good=good, dropped=int(nf - good))


def emit_times(res):
    for name, (ms, mn) in res.items():
        emit(case=name, frames=nf, ms_median=round(ms, 4), ms_min=round(mn, 4))
    return {k: v[0] for k, v in res.items()}


def bench_packets(c):
    two, three = c.chain(c.decode, c.demux), c.chain(c.decode, c.demux, c.packets)
    res = emit_times(c.run_cases(two, (("demux", c.demux, True), ("packets", c.packets, True), ("decode", c.decode, False),
                                       ("decode+demux", two, False), ("decode+demux+packets", three, False))))
    c.pa.reset()
    c.packets()
    torch.cuda.synchronize()
    s = c.summary.cpu().numpy().view(xa.PACKETS_SUMMARY_DTYPE)[0]
    moved = int(c.offsets.cpu().numpy()[64]) * 892 + int(s["bytes"]) + int(s["packets"]) * 32
    emit(case="check", rows=int(s["rows"]), packets=int(s["packets"]), bytes=int(s["bytes"]), crc_failures=int(s["crc_failures"]),
         discarded=int(s["discarded"]), fill_packets=int(s["fill_packets"]), overflow=int(s["overflow"]),
         packets_GB_per_s=round(moved / res["packets"] / 1e6, 1), packets_share_of_decode_percent=round(100 * res["packets"] / res["decode"], 3),
         chain_difference_ms=round(res["decode+demux+packets"] - res["decode+demux"], 4))


def bench_files(c):
    three = c.chain(c.decode, c.demux, c.packets)
    res = emit_times(c.run_cases(three, (("packets", c.packets, True), ("files", c.files, True), ("decode+demux+packets", three, False),
                                         ("decode+demux+packets+files", c.chain(three, c.files), False),
                                         ("decode+demux+packets again", three, False))))
    c.fa.reset()
    c.pa.reset()
    c.packets()
    c.files()
    torch.cuda.synchronize()
    s = c.f_summary.cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)[0]
    p = c.summary.cpu().numpy().view(xa.PACKETS_SUMMARY_DTYPE)[0]
    moved = int(p["bytes"]) + int(p["packets"]) * 32 + int(s["bytes"]) + int(s["pieces"]) * 32 + int(s["files"]) * 80
    emit(case="files check", packets_in=int(p["packets"]), bytes_in=int(p["bytes"]), pieces=int(s["pieces"]), bytes=int(s["bytes"]),
         records=int(s["files"]), files_begun=int(s["files_begun"]), files_completed=int(s["files_completed"]),
         bad_packets=int(s["bad_packets"]), short_first=int(s["short_first"]), orphans=int(s["orphans"]), overflow=int(s["overflow"]),
         files_GB_per_s=round(moved / res["files"] / 1e6, 1),
         chain_difference_ms=round(res["decode+demux+packets+files"] - res["decode+demux+packets"], 4))


def bench_rice():
    n, J, S, L = 8, 16, args.samples, args.lines
    rng = np.random.default_rng(2)
    stats = {}
    distinct = [rs.random_line(rng, n, J, S, kind=rs.KINDS[i % len(rs.KINDS)], stats=stats)[1] for i in range(min(512, L))]
    data, desc = rs.pack([distinct[i % len(distinct)] for i in range(L)])
    d_data = torch.from_numpy(data.copy()).to(dev)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_out = torch.empty(L * S, dtype=torch.uint8, device=dev)
    d_status = torch.empty(L, dtype=torch.uint8, device=dev)
    rd = xa.RiceDecoder(n, J, S)
    want = rs.decode_batch(distinct[:8], n, J, S)[0]
    probe = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
    hbm = xa._capi.device_read_bandwidth(probe.data_ptr(), probe.numel(), reps=10, stream=st)
    moved = len(data) + L * S + L * 17
    for form in ("lane", "wave", "default"):
        xa.rice_form(form)
        d_out.zero_()
        ms, mn = timed(lambda: rd.decode_device(d_data.data_ptr(), len(data), d_desc.data_ptr(), 16, L, d_out.data_ptr(), d_status.data_ptr(),
                                                stream=st), args.reps or 20, 3 if args.warmup is None else args.warmup)
        assert np.array_equal(d_out.cpu().numpy().reshape(L, S)[:8], want) and not d_status.cpu().numpy().any()
        emit(case="rice", form=form, bits=n, block=J, samples=S, lines=L, bytes_in=len(data),
             options={str(k): v for k, v in sorted(stats.items(), key=str)}, ms_median=round(ms, 4), ms_min=round(mn, 4),
             Msamples_per_s=round(L * S / ms / 1e3, 1), GB_per_s_in_plus_out=round(moved / ms / 1e6, 2),
             device_read_GB_per_s=round(hbm, 1), fraction_of_read_rate=round(moved / ms / 1e6 / hbm, 5))


def framer_streams():
    """A frame-aligned LRIT stream of nf frames (256 distinct CADUs tiled), and the same with one symbol deleted every 50
    frames."""
    rng = np.random.default_rng(1)
    base_n = min(256, nf)
    blocks = [ccsds.make_block(0x8C, i % 64, i, rng) for i in range(base_n)]
    aligned = tiled(np.stack([ccsds.cadu_from_block(b) for b in blocks]), np.int8).reshape(-1)
    whole = (nf // 50) * 50                      # one symbol deleted every 50 frames: the last of each run of 50
    deleted = torch.cat([aligned[:whole * FR].view(-1, 50 * FR)[:, :-1].reshape(-1), aligned[whole * FR:]]) if whole else aligned
    return aligned, deleted


def bench_framer():
    aligned, deleted = framer_streams()
    sync = xa.FrameSynchroniser("lrit")
    cap = sync.rows(len(aligned))
    frames, valid, hits = u8(cap * FR), u8(cap), u8(cap * 16)
    start, count = u8(cap * 8), u8(4)
    reps, warm = args.reps or 10, 2 if args.warmup is None else args.warmup

    def push(x):
        return lambda: sync.push_device(x.data_ptr(), len(x), frames.data_ptr(), valid.data_ptr(), hits.data_ptr(), start.data_ptr(),
                                        count.data_ptr(), stream=st)

    def pair():                                  # the fixed-window pair takes at most 65535 frames per call
        for a in range(0, nf, 65535):
            k = min(65535, nf - a)
            xa.sync_correlate_device(aligned[a * FR:].data_ptr(), k * FR, hits[a * 16:].data_ptr(), stream=st)
            xa.sync_fix_frames_device(aligned[a * FR:].data_ptr(), k * FR, hits[a * 16:].data_ptr(), frames[a * FR:].data_ptr(),
                                      valid[a:].data_ptr(), stream=st)

    def framer_case(name, x, segment):
        sync.set_segment(segment)
        times = []
        for i in range(warm + reps):             # every call from a fresh cursor: the reset is outside the events
            sync.reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            push(x)()
            b.record()
            torch.cuda.synchronize()
            if i >= warm:
                times.append(a.elapsed_time(b))
        s = sync.stats()
        rows = int(s["rows"])
        emit(case=name, segment=segment or "default", symbols=len(x), ms_median=round(float(np.median(times)), 4), ms_min=round(min(times), 4),
             frames_per_ms=round(int(s["frames"]) / float(np.median(times)), 1), GB_per_s_in=round(len(x) / float(np.median(times)) / 1e6, 1),
             rows=rows, frames=int(s["frames"]), dropped_chunks=int(s["dropped_chunks"]), resyncs=int(s["resyncs"]),
             rewalked_chunks=int(s["rewalked_chunks"]), rewalked_share=round(int(s["rewalked_chunks"]) / max(rows, 1), 5))
        return float(np.median(times))

    ms_a = framer_case("framer aligned", aligned, 0)
    emit(case="framer aligned check", count=int(count.cpu().numpy().view(np.uint32)[0]), valid=int(valid[:nf].sum()), frames=nf)
    ms_d = framer_case("framer one symbol deleted every 50 frames", deleted, 0)
    ms_p, mn_p = timed(pair, reps, warm)
    emit(case="fixed windows: correlate + fix_frames, aligned", frames=nf, ms_median=round(ms_p, 4), ms_min=round(mn_p, 4),
         frames_per_ms=round(nf / ms_p, 1), GB_per_s_in=round(nf * FR / ms_p / 1e6, 1), valid=int(valid[:nf].sum()))
    emit(case="framer check", aligned_over_pair=round(ms_a / ms_p, 3), deleted_over_pair=round(ms_d / ms_p, 3))
    for segment in (16, 64, 128, 256, 1024):
        framer_case("framer aligned", aligned, segment)
        framer_case("framer one symbol deleted every 50 frames", deleted, segment)
    sync.close()


def bench_lock():
    aligned, deleted = framer_streams()
    sync, dec = xa.FrameSynchroniser("lrit"), xa.FrameDecoder("lrit")
    locks = {4: xa.FrameLock("lrit", flywheel=4), 1: xa.FrameLock("lrit", flywheel=1)}
    cap = sync.rows(len(aligned))
    frames, valid, hits, start, mode, count = u8(cap * FR), u8(cap), u8(cap * 16), u8(cap * 8), u8(cap), u8(4)
    cadu, block, info = u8(cap * 1024), u8(cap * 1020), u8(cap * xa.FRAME_INFO_DTYPE.itemsize)
    reps, warm = args.reps or 5, 2 if args.warmup is None else args.warmup

    def from_reset(reset, fn):                   # every call from the start state: the reset is outside the events
        times = []
        for i in range(warm + reps):
            reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warm:
                times.append(a.elapsed_time(b))
        return float(np.median(times)), min(times)

    for name, x in (("aligned", aligned), ("one symbol deleted every 50 frames", deleted)):
        def pair():
            sync.push_device(x.data_ptr(), len(x), frames.data_ptr(), valid.data_ptr(), hits.data_ptr(), start.data_ptr(),
                             count.data_ptr(), stream=st)
            dec.decode_device(frames.data_ptr(), valid.data_ptr(), cap, cadu.data_ptr(), block.data_ptr(), info.data_ptr(), stream=st)

        ms_p, mn_p = from_reset(lambda: (sync.reset(), dec.reset()), pair)
        inf = info.cpu().numpy().view(xa.FRAME_INFO_DTYPE)
        emit(case="framer + decoder on one stream, " + name, symbols=len(x), ms_median=round(ms_p, 3), ms_min=round(mn_p, 3),
             rows=int(sync.stats()["rows"]), frames_ok=int(inf["ok"].sum()), frames_bad=int((inf["valid"] != 0).sum() - inf["ok"].sum()))
        for recheck, lk in locks.items():
            ms, mn = from_reset(lk.reset, lambda: lk.push_device(
                x.data_ptr(), len(x), frames.data_ptr(), valid.data_ptr(), hits.data_ptr(), start.data_ptr(), mode.data_ptr(),
                cadu.data_ptr(), block.data_ptr(), info.data_ptr(), count.data_ptr(), stream=st))
            s = lk.stats()
            emit(case="lock, " + name, recheck=recheck, symbols=len(x), ms_median=round(ms, 3), ms_min=round(mn, 3),
                 over_pair=round(ms / ms_p, 4), rounds=int(s["rounds"]), sensitive_chunks=int(s["sensitive_chunks"]),
                 short_kept=int(s["short_kept"]), short_missed=int(s["short_missed"]), rechecks=int(s["rechecks"]),
                 rows=int(s["rows"]), frames_ok=int(s["frames_ok"]), frames_bad=int(s["frames_bad"]), resyncs=int(s["resyncs"]),
                 rewalked_chunks=int(s["rewalked_chunks"]))
    for h in (sync, dec, *locks.values()):
        h.close()


def bench_images():
    import file_spec as fs
    import image_spec as isp
    rng = np.random.default_rng(3)
    keys = [(v, a) for v in (0, 5, 31) for a in (10, 11, 700, 2046)]
    items, sources, serial = [], {}, {}
    order = ["image"] * args.images + ["other"] * (args.images // 2)
    rng.shuffle(order)
    for what in order:
        key = keys[int(rng.integers(0, len(keys)))]
        k = serial.get(key, 0)
        serial[key] = k + 1
        if what == "image":
            n, J = int(rng.choice([4, 8, 8, 10, 12, 16])), int(rng.choice(rs.BLOCK_SIZES))
            img, data, cuts = isp.image_file(rng, n, J, int(rng.integers(256, 2049)), int(rng.integers(16, 49)))
            sources[key + (k,)] = img
            items.append((key, data, cuts, 8190))
        else:
            items.append((key, fs.random_file(rng, 20000), None, int(rng.choice([1000, 8190]))))
    stream = isp.stream_of(rng, items)
    by_vc = {}
    for v, pkt, _ in stream:
        by_vc.setdefault(v, []).append(pkt)
    vcdu, offsets = ps.group({v: s.rows for v, s in ps.build_streams([(v, p) for v, p, _ in stream], rng, fill=0.0, idle=0.0).items()})
    rows = len(vcdu)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_vcdu, d_off = up(vcdu), up(offsets)
    mb, mp = xa.packets_max_bytes(rows), len(stream) + 64 * 3
    p_bytes, p_desc, p_off, p_sum = u8(mb), u8(mp * 32), u8(65 * 4), u8(xa.PACKETS_SUMMARY_DTYPE.itemsize)
    f_bytes, f_pieces, f_recs, f_sum = u8(mb), u8(mp * 32), u8(2 * mp * 80), u8(xa.FILES_SUMMARY_DTYPE.itemsize)
    pa, fa, im = xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder()

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
    pieces = f_pieces.cpu().numpy().view(xa.FILE_PIECE_DTYPE)[:int(fsum["pieces"])]
    recs = f_recs.cpu().numpy().view(xa.FILE_RECORD_DTYPE)[:int(fsum["files"])]
    max_out = xa.images_max_bytes(recs)
    o_bytes, o_lines, o_files, o_sum = u8(max_out + 8), u8(mp * 32), u8(2 * mp * 48), u8(xa.IMAGES_SUMMARY_DTYPE.itemsize)

    def images():
        im.process_device(f_bytes.data_ptr(), mb, f_pieces.data_ptr(), mp, f_recs.data_ptr(), 2 * mp, f_sum.data_ptr(), o_bytes.data_ptr(),
                          max_out, o_lines.data_ptr(), mp, o_files.data_ptr(), o_sum.data_ptr(), stream=st)

    # what the stage replaces: the host walks the records it read back and launches one decode per rice record
    loop, at = [], 0
    l_out, l_status = u8(max_out + 8), u8(len(pieces) + 1)
    decoders = {}
    for r in recs:
        first, count = int(r["first_piece"]), int(r["n_pieces"])
        if not (int(r["flags"]) & xa.FILE_BEGINS) or count < 2 or not xa.is_rice_coded(r, pieces[first]["length"]):
            continue
        par = (int(r["bits_per_pixel"]), int(r["pixels_per_block"]), int(r["columns"]))
        rd = decoders.setdefault(par, xa.RiceDecoder(*par))
        loop.append((rd, f_pieces.data_ptr() + 32 * (first + 1), count - 1, l_out.data_ptr() + at, l_status.data_ptr() + first + 1))
        at += (count - 1) * ((par[2] * (1 if par[0] <= 8 else 2) + 3) & ~3)

    def per_record():
        for rd, desc, count, out, status in loop:
            rd.decode_device(f_bytes.data_ptr(), mb, desc, 32, count, out, status, stream=st)

    reps, warm = args.reps or 20, 3 if args.warmup is None else args.warmup
    res = {"images": timed(images, reps, warm), "per-record loop": timed(per_record, reps, warm), "files": timed(files, reps, warm),
           "packets+files": timed(lambda: (packets(), files()), reps, warm),
           "packets+files+images": timed(lambda: (packets(), files(), images()), reps, warm)}
    for name, (ms, mn) in res.items():
        emit(case=name, rows=rows, ms_median=round(ms, 4), ms_min=round(mn, 4))
    # the stage's lines are the generated images
    torch.cuda.synchronize()
    s = o_sum.cpu().numpy().view(xa.IMAGES_SUMMARY_DTYPE)[0]
    lines = o_lines.cpu().numpy().view(xa.IMAGE_LINE_DTYPE)[:int(s["lines"])]
    recs = f_recs.cpu().numpy().view(xa.FILE_RECORD_DTYPE)[:int(f_sum.cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)[0]["files"])]
    got = isp.Rows()
    got.add(o_bytes.cpu().numpy(), lines, recs)
    first_serial = {}
    for r in recs:
        k = (int(r["vcid"]), int(r["apid"]))
        first_serial[k] = min(first_serial.get(k, 1 << 32), int(r["key_serial"]))
    equal = all(np.array_equal(got.image(v, a, first_serial[(v, a)] + k)[0], img) for (v, a, k), img in sources.items())
    moved = int(fsum["bytes"]) + int(s["bytes"]) + int(s["lines"]) * 64
    emit(case="images check", images=int(s["images"]), records=len(recs), launches_replaced=len(loop), lines=int(s["lines"]),
         faults=int(s["total_faults"]) , bytes_in=int(fsum["bytes"]), bytes_out=int(s["bytes"]), overflow=int(s["overflow"]),
         parameter_sets=len(decoders), lines_equal_sources=bool(equal), Msamples_per_s=round(int(lines["samples"].astype(np.int64).sum()) / res["images"][0] / 1e3, 1),
         GB_per_s_in_plus_out=round(moved / res["images"][0] / 1e6, 2), stage_over_loop=round(res["images"][0] / res["per-record loop"][0], 4),
         chain_difference_ms=round(res["packets+files+images"][0] - res["packets+files"][0], 4))
    for h in (pa, fa, im):
        h.close()


def bench_canvas():
    import canvas_spec as cs
    import file_spec as fs
    import image_spec as isp
    rng = np.random.default_rng(4)
    keys = [(0, 10), (0, 11), (5, 700), (31, 2046)]
    items, sources = [], {}
    for i in range(args.canvases):
        bits, J, cols, rows = (8, 16, 2784, 36) if i % 2 else (10, 32, 5424, 36)
        img = cs.samples(rng, bits, J, cols, rows, kinds=("walk3", "scaled"))
        key = keys[i % len(keys)]
        sources[(key[0], 100 + i)] = img
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
    nrec = int(fsum["files"])
    recs = f_recs.cpu().numpy().view(xa.FILE_RECORD_DTYPE)[:nrec]
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

    images()
    torch.cuda.synchronize()
    isum = o_sum.cpu().numpy().view(xa.IMAGES_SUMMARY_DTYPE)[0]
    nl, nb = int(isum["lines"]), int(isum["bytes"])
    reps, warm = args.reps or 20, 3 if args.warmup is None else args.warmup

    def from_reset(fn):                         # every call on a handle without canvases: the reset is outside the events
        times = []
        for i in range(warm + reps):
            cv.reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warm:
                times.append(a.elapsed_time(b))
        return float(np.median(times)), min(times)

    # what the stage replaces: the lines come to the host, which places them by the segment records it parsed itself
    heads = {}
    pieces = f_pieces.cpu().numpy().view(xa.FILE_PIECE_DTYPE)[:int(fsum["pieces"])]
    raw = f_bytes.cpu().numpy()
    for f, r in enumerate(recs):
        if int(r["flags"]) & xa.FILE_BEGINS:
            pc = pieces[int(r["first_piece"])]
            heads[f] = cs.walk_header(raw[int(pc["offset"]):int(pc["offset"]) + int(pc["length"])].tobytes(), r["columns"], r["lines"])[0]

    def on_the_host():
        t = time.perf_counter()
        data, lines = o_bytes[:nb].cpu().numpy(), o_lines[:nl * 32].cpu().numpy().view(xa.IMAGE_LINE_DTYPE)
        out = {}
        for ln in lines:
            h, r = heads[int(ln["file"])], recs[int(ln["file"])]
            w = 1 if int(r["bits_per_pixel"]) <= 8 else 2
            img = out.setdefault((int(r["vcid"]), h["image_id"]), np.zeros((h["max_row"], h["max_column"] * w), np.uint8))
            a = int(ln["offset"])
            img[h["start_line"] + int(ln["row"]), h["start_column"] * w:h["start_column"] * w + int(ln["length"])] = data[a:a + int(ln["length"])]
        return (time.perf_counter() - t) * 1e3, out

    host_ms = [on_the_host()[0] for _ in range(max(3, reps // 4))]
    host_images = on_the_host()[1]
    res = {"canvas": from_reset(canvas), "packets+files+images": from_reset(lambda: (packets(), files(), images())),
           "packets+files+images+canvas": from_reset(lambda: (packets(), files(), images(), canvas()))}
    for name, (ms, mn) in res.items():
        emit(case=name, rows=rows, ms_median=round(ms, 4), ms_min=round(mn, 4))
    emit(case="host: download the lines, place with NumPy (download inside)", lines=nl, ms_median=round(float(np.median(host_ms)), 3),
         ms_min=round(min(host_ms), 3))
    # the stage's canvases are the generated images, and the host's
    cv.reset()
    canvas()
    torch.cuda.synchronize()
    s = c_sum.cpu().numpy().view(xa.CANVAS_SUMMARY_DTYPE)[0]
    table = c_slots.cpu().numpy().view(xa.CANVAS_SLOT_DTYPE)
    t = time.perf_counter()
    got = {(int(info["vcid"]), int(info["image_id"])): img for info, img in (cv.image(i) for i in range(slots) if table[i]["complete"])}
    read_ms = (time.perf_counter() - t) * 1e3
    equal = got.keys() == sources.keys() and all(np.array_equal(got[k], v) for k, v in sources.items())
    host_equal = all(np.array_equal(host_images[k] if host_images[k].shape[1] == v.shape[1] else host_images[k].view("<u2"), v) for k, v in sources.items())
    probe = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
    hbm = xa._capi.device_read_bandwidth(probe.data_ptr(), probe.numel(), reps=10, stream=st)
    lines = o_lines.cpu().numpy().view(xa.IMAGE_LINE_DTYPE)[:nl]
    moved = 2 * int(lines["length"].astype(np.int64).sum()) + 32 * nl
    emit(case="canvas check", canvases=args.canvases, records=nrec, lines=nl, lines_placed=int(s["call_lines_placed"]),
         completed=int(s["completed"]), overflow=int(s["overflow"]), canvases_equal_sources=bool(equal), host_equal_sources=bool(host_equal),
         read_back_of_the_finished_canvases_ms=round(read_ms, 3), stage_over_host=round(res["canvas"][0] / float(np.median(host_ms)), 5),
         chain_difference_ms=round(res["packets+files+images+canvas"][0] - res["packets+files+images"][0], 4),
         place_bytes_read_plus_written=moved, place_GB_per_s_at_least=round(moved / res["canvas"][0] / 1e6, 2),
         device_read_GB_per_s=round(hbm, 1))
    for h in (pa, fa, im, cv):
        h.close()


shared = []                                     # the packets and the files cases run on one stream of frames


def packet_chain():
    if not shared:
        shared.append(Chain("packets"))
    return shared[0]


for what in ["decode", "demux", "packets", "files", "rice", "framer", "lock"] if args.what == "all" else [args.what]:
    {"decode": bench_decode, "demux": bench_demux, "rice": bench_rice, "framer": bench_framer, "lock": bench_lock, "images": bench_images, "canvas": bench_canvas,
     "packets": lambda: bench_packets(packet_chain()),
     "files": lambda: bench_files(packet_chain())}[what]()
