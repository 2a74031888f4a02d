#!/usr/bin/env python3
"""Two builds of xrit_demod_host on the same captures: do they write the same files and say the same on stderr?

    python scripts/host_program_identity.py PARENT_BIN TREE_BIN [--out FILE] [--speed SAMPLES]

Needs a HIP device.  The captures are built with the builders the host-program tests use (tests/test_gpu_canvas.py,
tests/test_oracle_kat.py) and the items of tests/test_gpu_geo.py's end-to-end case.  Every case runs PARENT_BIN, TREE_BIN and
PARENT_BIN a second time (what varies without any change), one process at a time under `timeout -k 10`, each into a
directory of its own.  Compared: the directory trees (names and bytes) and the stderr texts line for line; in the
`samples in ...` line the seconds and the Msamples/s are masked, and in --decoder-stats' records startTime (the second the
demultiplexer's handle was made).  --drop depends on thread timing: the exit status and the
capacity field of the `symbol queue` line only.  The first run that ends by signal or with status 124, 134, 137 or 139
ends the script; nothing is tried again.

--speed N: after the cases, one capture of about N samples through --decode, --files, --files-decompress, --canvas,
--products, three runs of each binary in turn; the Msamples/s of the --stats line.
"""
import argparse
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FATAL = (124, 134, 137, 139)
RATE = re.compile(r"^(samples in \d+, symbols out \d+), [0-9.]+ s \([0-9.]+ Msamples/s")


class Fatal(Exception):
    pass


def image_capture(work, seed=71):
    """The items of tests/test_gpu_geo.py::test_host_program_project: an 8-bit image of two segments with an annotation and a
    navigation record, a 10-bit image, an image that stays partial, one whose record does not parse -> IQ (cf32) path."""
    import canvas_spec as cs
    import geo_spec as gs
    import image_spec as isp
    from test_gpu_canvas import host_capture
    rng = np.random.default_rng(seed)
    a, b, c, d = cs.samples(rng, 8, 16, 64, 12), cs.samples(rng, 10, 32, 33, 8), cs.samples(rng, 8, 8, 16, 4), cs.samples(rng, 8, 8, 16, 4)
    nav_a = gs.nav_of(230000, -44000, 33, 7, 1, -75.2)
    nav_b = gs.nav_of(-120000, 29000, 17, 5, 1, -137.0)
    body = lambda nav, name=None: gs.navigation_record(nav, name)[3:]
    seg = lambda img, bits, J, ident, key, **kw: (key,) + cs.segment_file(rng, img, bits, J, ident=ident, **kw) + (8190,)
    items = [seg(a[:7], 8, 16, (21, 1, 0, 0, 2, 64, 12), (5, 40), name=b"GOES test/full disk.lrit", extra=[(2, body(nav_a))]),
             seg(a[7:], 8, 16, (21, 2, 0, 7, 2, 64, 12), (5, 41), name=b"GOES test/full disk.lrit"),
             seg(b, 10, 32, (22, 1, 0, 0, 1, 33, 8), (5, 42), extra=[(2, body(nav_b))]),
             seg(c, 8, 8, (23, 2, 0, 4, 2, 16, 8), (5, 43)),
             seg(d, 8, 8, (24, 1, 0, 0, 1, 16, 4), (5, 44), extra=[(2, body(nav_a, b"MERCATOR(0)"))])]
    return host_capture(work, {5: [p for _, p, _ in isp.stream_of(rng, items)]}, seed)


def converted(iq, fmt):
    """The cf32 capture as s16, s8 or u8 next to it."""
    x = np.fromfile(iq, np.float32)
    x = x / np.abs(x).max()
    out = str(iq)[:-4] + fmt
    if fmt == "s16":
        np.round(x * 20000).astype(np.int16).tofile(out)
    elif fmt == "s8":
        np.round(x * 100).astype(np.int8).tofile(out)
    else:
        (np.round(x * 100) + 128).astype(np.uint8).tofile(out)
    return out


def run(binary, args, out_dir, seconds=120):
    """One process; `@` in an argument stands for the run's output directory -> (status, stderr, {name: bytes})."""
    os.makedirs(out_dir)
    argv = ["timeout", "-k", "10", str(seconds), binary] + [a.replace("@", out_dir) for a in args]
    r = subprocess.run(argv, capture_output=True, text=True, errors="replace")
    if r.returncode < 0 or r.returncode in FATAL:
        raise Fatal("status %d from %s\n%s" % (r.returncode, " ".join(argv), r.stderr[-2000:]))
    tree = {}
    for base, _, names in os.walk(out_dir):
        for nm in names:
            path = os.path.join(base, nm)
            with open(path, "rb") as f:
                tree[os.path.relpath(path, out_dir)] = f.read()
    return r.returncode, r.stderr.replace(out_dir, "@"), tree


def without_start_time(name, data):
    """--decoder-stats' file with Statistics_st::startTime zeroed in every record."""
    import demux_spec as ds
    if os.path.basename(name) != "stats.bin" or len(data) % ds.WIRE_SIZE:
        return data
    at = struct.calcsize(ds.WIRE_FORMAT.replace("I4sBBB", ""))
    rec = np.frombuffer(data, np.uint8).reshape(-1, ds.WIRE_SIZE).copy()
    rec[:, at:at + 4] = 0
    return rec.tobytes()


def masked(err):
    return [RATE.sub(r"\1, * s (* Msamples/s", ln) for ln in err.splitlines()]


def drop_view(result):
    status, err, _ = result
    cap = [re.match(r"symbol queue: capacity (\d+),", ln).group(1) for ln in err.splitlines() if ln.startswith("symbol queue:")]
    return status, cap


def differences(a, b, drop):
    if drop:
        return [] if drop_view(a) == drop_view(b) else ["status or symbol queue capacity: %r / %r" % (drop_view(a), drop_view(b))]
    out = []
    if a[0] != b[0]:
        out.append("exit status %d / %d" % (a[0], b[0]))
    if sorted(a[2]) != sorted(b[2]):
        out.append("file names differ: %s" % sorted(set(a[2]) ^ set(b[2])))
    out += ["bytes of %s differ" % nm for nm in sorted(set(a[2]) & set(b[2])) if without_start_time(nm, a[2][nm]) != without_start_time(nm, b[2][nm])]
    la, lb = masked(a[1]), masked(b[1])
    if la != lb:
        k = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        out.append("stderr differs from line %d: %r / %r" % (k + 1, la[k:k + 1], lb[k:k + 1]))
    return out


def cases(iq, burst, two_gpus):
    base = ["--input", str(iq), "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null", "--block", "200000"]
    files = ["--files", "@/files", "--files-decompress"]
    canvas = files + ["--canvas", "--canvas-slots", "6", "--canvas-mib", "1"]
    products = canvas + ["--products"]
    project = canvas + ["--project"]
    tuned = ["--input", str(burst), "--mode", "lrit", "--sample-rate", "1250000", "--block", "524288", "--sink", "file:@/symbols.s8"]
    c = [("decode", base + ["--decode", "@/vcdu.bin", "--stats"]),
         ("decode_stream_sync", base + ["--decode", "@/vcdu.bin", "--stream-sync"]),
         ("flywheel", base + ["--decode", "@/vcdu.bin", "--flywheel"]),
         ("flywheel_2", base + ["--flywheel", "2", "--decode", "@/vcdu.bin"]),
         ("channels_decoder_stats", base + ["--channels", "@/channels", "--decoder-stats", "@/stats.bin"]),
         ("packets", base + ["--packets", "@/packets"]),
         ("files", base + ["--files", "@/files"]),
         ("files_decompress", base + files),
         ("all_outputs_flywheel", base + files + ["--decode", "@/vcdu.bin", "--channels", "@/channels", "--decoder-stats", "@/stats.bin", "--packets", "@/packets", "--flywheel"]),
         ("canvas", base + canvas),
         ("canvas_2_slots", base + files + ["--canvas", "--canvas-slots", "2", "--canvas-mib", "1"]),
         ("products", base + products),
         ("products_tone_factor", base + products + ["--product-tone", "stretch:100:9900", "--product-factor", "3"]),
         ("products_linear", base + products + ["--product-tone", "linear"]),
         ("jpeg", base + products + ["--jpeg"]),
         ("jpeg_75", base + products + ["--jpeg", "75"]),
         ("project", base + project),
         ("project_grid", base + project + ["--project-grid", "-170:60:3:50:41"]),
         ("project_nearest", base + project + ["--project-grid", "-170:60:3:50:41", "--project-mode", "nearest"]),
         ("products_project", base + products + ["--project", "--project-grid", "-170:60:3:50:41", "--jpeg", "60", "--stream-sync"]),
         ("monitor", base + ["--monitor", "@/monitor.csv", "--monitor-block", "4096"]),
         ("tune", tuned + ["--tune", "23000"]),
         ("acquire", tuned + ["--acquire"]),
         ("acquire_fifo", tuned + ["--acquire", "--fifo", "--stats"]),
         ("fifo_lag_3", base + ["--fifo", "--fifo-lag", "3", "--stats", "--decode", "@/vcdu.bin"]),
         ("fifo_overflow", base + ["--fifo", "--fifo-lag", "9", "--stats"]),
         ("sink_file", base[:6] + ["--sink", "file:@/symbols.s8", "--block", "200000"]),
         ("sink_refused", base[:6] + ["--sink", "pipe:x"]),
         ("decode_output_refused", base + ["--decode", "@/nowhere/vcdu.bin", "--channels", "@/channels"]),
         ("mode_hrit", ["--input", str(iq), "--mode", "hrit", "--sample-rate", "3000000", "--sink", "null", "--block", "200000", "--decode", "@/vcdu.bin"]),
         ("drop", base[:6] + ["--sink", "tcp://127.0.0.1:9", "--drop", "--queue-symbols", "65536", "--stats", "--block", "200000"])]
    for fmt in ("s16", "s8", "u8"):
        c.append(("format_" + fmt, ["--input", converted(iq, fmt), "--format", fmt] + base[2:] + ["--decode", "@/vcdu.bin"]))
    if two_gpus:
        c.append(("gpus_2", base[:6] + ["--sink", "file:@/symbols.s8", "--gpus", "2", "--block", "1000000", "--stats"]))
    return c


def speed(parent, tree, work, samples, say):
    """One long capture (the image capture's frames repeated), three runs of each binary in turn."""
    iq = np.fromfile(os.path.join(work, "iq.cf32"), np.complex64)
    big = os.path.join(work, "big.cf32")
    np.tile(iq, max(1, samples // len(iq))).tofile(big)
    args = ["--input", big, "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null", "--decode", "@/vcdu.bin", "--files", "@/files",
            "--files-decompress", "--canvas", "--products", "--stats"]
    rates = {"parent": [], "tree": []}
    for k in range(3):
        for name, binary in (("parent", parent), ("tree", tree)):
            status, err, _ = run(binary, args, os.path.join(work, "speed_%s_%d" % (name, k)), 300)
            m = re.search(r"\(([0-9.]+) Msamples/s", err)
            if status != 0 or not m:
                raise Fatal("speed run of %s: status %d\n%s" % (name, status, err[-1000:]))
            rates[name].append(float(m.group(1)))
            shutil.rmtree(os.path.join(work, "speed_%s_%d" % (name, k)))
    p, t = sorted(rates["parent"]), sorted(rates["tree"])
    say("speed: %d samples through --decode --files --files-decompress --canvas --products --stats, --sink null, Msamples/s incl. file and PCIe, three runs each in turn"
        % (len(iq) * max(1, samples // len(iq))))
    say("speed parent: %s median %.2f spread (max - min) %.2f" % (" ".join("%.2f" % v for v in rates["parent"]), p[1], p[2] - p[0]))
    say("speed tree:   %s median %.2f; below the parent's median by %.2f (allowed: the parent's spread) -> %s"
        % (" ".join("%.2f" % v for v in rates["tree"]), t[1], p[1] - t[1], "ok" if p[1] - t[1] <= p[2] - p[0] else "SLOWER"))
    return p[1] - t[1] <= p[2] - p[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--speed", type=int, default=0)
    ap.add_argument("--only", default=None, help="a regular expression on the case names")
    o = ap.parse_args()
    import xritdemod_amd
    devices = xritdemod_amd.device_count()
    if devices < 1:
        sys.exit("needs a HIP device")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    from test_oracle_kat import _framed_burst
    import pathlib
    work = tempfile.mkdtemp(prefix="host_identity_")
    ok = True
    try:
        iq = image_capture(pathlib.Path(work))
        burst = os.path.join(work, "burst.cf32")
        _framed_burst(16, carrier_hz=23000.0)[0].tofile(burst)
        say("# xrit_demod_host: parent (%s) against tree (%s), one MI355X, one process at a time" % (o.parent, o.tree))
        say("# captures: the segment files of tests/test_gpu_geo.py's end-to-end case (%d samples, LRIT 1.25 Msps, 12 dB) and a burst of 16 frames 23 kHz off"
            % (os.path.getsize(iq) // 8))
        say("# compared per case: names and bytes of every file written, stderr line for line (seconds and Msamples/s masked; startTime in stats.bin masked); drop: exit status and queue capacity only")
        if devices < 2:
            say("# gpus_2: not run, %d device" % devices)
        different = varying = n = 0
        for name, args in cases(iq, burst, devices >= 2):
            if o.only and not re.search(o.only, name):
                continue
            results = [run(binary, args, os.path.join(work, "%s_%d" % (name, k))) for k, binary in enumerate((o.parent, o.tree, o.parent))]
            diff = differences(results[0], results[1], name == "drop")
            again = differences(results[0], results[2], name == "drop")
            status, err, tree = results[1]
            say("%s: exit %d, %d files, %d bytes, %d stderr lines; %s%s" % (name, status, len(tree), sum(len(v) for v in tree.values()), len(err.splitlines()),
                                                                          "IDENTICAL" if not diff else "DIFFERENT: " + "; ".join(diff),
                                                                          "" if not again else " (parent against itself: " + "; ".join(again) + ")"))
            n += 1
            different += bool(diff)
            varying += bool(again)
            for k in range(3):
                shutil.rmtree(os.path.join(work, "%s_%d" % (name, k)))
        say("cases: %d different: %d" % (n, different))
        say("parent run 1 against parent run 2 (what varies without any change): cases: %d different: %d" % (n, varying))
        ok = different == 0
        if o.speed:
            ok = speed(o.parent, o.tree, work, o.speed, say) and ok
    except Fatal as e:
        say("STOPPED: %s" % e)
        ok = False
    finally:
        shutil.rmtree(work, ignore_errors=True)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
