"""GPU tier: the JPEG decoder stage (xrit_jpegdec_*, JpegDecoder) against the specification of tests/jpegdec_spec.py --
pixels, records and summary compared with np.array_equal -- and directly against the pixels Pillow's libjpeg recorded in
tests/golden/jpegdec_pil.npz.  Both forms of the entropy decoder on every case, form 1 at subsequences of 128 bits and at
the default.  The shapes are the smallest at which the kernels can still go wrong: one pixel; one block; partial blocks on
both edges; one row of 75 blocks (more than a wave of subsequences, more than the 32 MCUs of a pixels workgroup); a
64 x 72 quality-100 image without restart markers (more than 64 subsequences of 128 bits in one interval: several tiles);
the adversarial stream whose guesses stay wrong for 64 rounds; restart intervals 0, 1, 2, 7, a block row and beyond the
image; item counts and block counts one below, at and above the scan tile (scan.h's SCAN_TILE = 1024 elements; the item scan
has one element more than it has items); a mixed batch with unsupported and damaged streams between sound ones at odd
offsets with garbage between and a stride larger than the record; the damaged set (every truncation, byte flips, RSTm
removed, swapped, inserted); a scratch too small for the batch; an output too small, with a guard behind it; calls back to
back; the encoder's output decoded on the same stream; the host-buffer form; bad arguments; more than 2^20 scan bytes
in a call (the byte scan's second level); xrit_demod_host --files-jpeg on a capture."""
import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_spec as js
import jpegdec_cases as dc
import jpegdec_spec as ds

pytestmark = pytest.mark.gpu

GUARD = 64
SCAN_TILE = 1024
FORMS = [(0, 0), (1, 128), (1, 0)]
FORM_IDS = ["lanes", "waves_s128", "waves_default"]
CACHE = {}                                              # the specification's decode of a stream, shared by every test


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def golden():
    return dc.Golden()


@pytest.fixture(scope="module")
def dec(xa):
    h = xa.JpegDecoder()
    yield h
    h.close()


def laid_out(files, seed=0, gaps=False):
    """The streams in one buffer -> (bytes, [(offset, length)]); gaps: odd base offsets and non-zero garbage between and behind."""
    rng = np.random.default_rng(seed)
    parts, items, at = [], [], 0
    for f in files:
        if gaps:
            g = rng.integers(1, 256, int(rng.integers(1, 8)) * 2 - 1, dtype=np.uint8).tobytes()
            parts.append(g)
            at += len(g)
        items.append((at, len(f)))
        parts.append(f)
        at += len(f)
    if gaps:
        parts.append(rng.integers(1, 256, 37, dtype=np.uint8).tobytes())
    return b"".join(parts), items


def item_records(items, stride, seed=0):
    """{uint64 offset; uint32 length} every `stride` bytes, non-zero garbage in the rest of a record."""
    raw = np.random.default_rng(seed).integers(1, 256, max(len(items), 1) * stride, dtype=np.uint8)
    for i, (offset, length) in enumerate(items):
        raw[i * stride:i * stride + 8] = np.frombuffer(np.uint64(offset).tobytes(), np.uint8)
        raw[i * stride + 8:i * stride + 12] = np.frombuffer(np.uint32(length).tobytes(), np.uint8)
    return raw


def expected(buf, items, cap, max_blocks=ds.MAX_BLOCKS):
    writes, records, summary = ds.decode_batch(buf, items, cap=cap, max_blocks=max_blocks, cache=CACHE)
    pixels = np.full(cap + GUARD, 0xA5, np.uint8)
    for at, data in writes:
        pixels[at:at + len(data)] = np.frombuffer(data, np.uint8)
    return pixels, records, summary


def prepare(torch, buf, items, cap, stride=16, seed=0):
    dev = torch.device("cuda:0")
    d_bytes = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).to(dev) if len(buf) else torch.zeros(16, dtype=torch.uint8, device=dev)
    d_items = torch.from_numpy(item_records(items, stride, seed)).to(dev)
    d_pixels = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_records = torch.full((64 * len(items) + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_summary = torch.full((64 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    args = (d_bytes.data_ptr(), len(buf), d_items.data_ptr(), stride, len(items), d_pixels.data_ptr(), cap, d_records.data_ptr(), d_summary.data_ptr())
    return args, (d_bytes, d_items, d_pixels, d_records, d_summary)


def same(keep, want, n_items):
    """Pixels (with the guard and everything the call must not write), records and summary equal the specification's."""
    _, _, d_pixels, d_records, d_summary = keep
    pixels, records, summary = want
    got_r, got_s = d_records.cpu().numpy(), d_summary.cpu().numpy()
    assert (got_r[64 * n_items:] == 0xA5).all() and (got_s[64:] == 0xA5).all()
    assert got_s[:64].tobytes() == summary.tobytes(), (got_s[:64].view(ds.SUMMARY_DTYPE)[0], summary)
    got = got_r[:64 * n_items].view(ds.RECORD_DTYPE)
    for name in ds.RECORD_DTYPE.names:
        assert np.array_equal(got[name], records[name]), (name, got[name][:8], records[name][:8])
    assert np.array_equal(d_pixels.cpu().numpy(), pixels)


def check(torch, dec, files, form=(0, 0), cap=None, max_blocks=0, gaps=False, stride=16, seed=0):
    buf, items = laid_out(files, seed, gaps)
    if cap is None:
        cap = int(ds.decode_batch(buf, items, cache=CACHE, max_blocks=max_blocks or ds.DEFAULT_BLOCKS)[2]["bytes"]) + 5
    want = expected(buf, items, cap, max_blocks or ds.DEFAULT_BLOCKS)
    dec.set_form(*form)
    args, keep = prepare(torch, buf, items, cap, stride, seed)
    dec.decode_device(*args, max_blocks=max_blocks)
    torch.cuda.synchronize()
    same(keep, want, len(items))
    return want


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_recorded_pillow_streams(xa, torch, dec, golden, form):
    """Every sound stream of the fixture, one call each and all in one call: the specification's pixels, and Pillow's own."""
    for name in ("grey_1x1", "rgb_1x1", "grey_8x8", "rgb_8x8", "grey_7x9", "rgb_7x9", "grey_9x7", "rgb_9x7", "grey_row75", "rgb_row75", "grey_row75_noise",
                 "rgb_row75_noise"):
        pixels, records, _ = check(torch, dec, [golden.files[name]], form)
        n = int(records[0]["length"])
        assert records[0]["status"] == 0 and np.array_equal(pixels[:n], golden.pixels[name].reshape(-1)), name
    pixels, records, summary = check(torch, dec, [golden.files[n] for n in golden.sound], form)
    assert summary["images"] == len(golden.sound)
    for r, name in zip(records, golden.sound):
        assert np.array_equal(pixels[int(r["offset"]):int(r["offset"] + r["length"])], golden.pixels[name].reshape(-1)), name
        assert r["offset"] % 4 == 0 and (r["columns"], r["rows"]) == golden.pixels[name].shape[1::-1]


def test_more_than_64_subsequences_in_one_interval(xa, torch, dec, golden):
    """64 x 72 of noise at quality 100 without restart markers: at 128 bits more than 64 subsequences, so several tiles with
    the exit state carried; the rounds the device took are the model's."""
    for name in ("grey_q100_noise", "rgb_q100_noise"):
        f = golden.files[name]
        cnt = ds.new_counters()
        status, pixels, h, _ = ds.decode(f, 1, 128, cnt)
        assert status == 0 and h["restart"] == 0 and (len(f) - h["scan"]) * 8 // 128 > 64 and cnt["tiles_over_one"] == 1 and cnt["max_rounds"] > 1
        assert np.array_equal(pixels, golden.pixels[name])
        check(torch, dec, [f], (1, 128))
        assert dec.rounds() == cnt["max_rounds"]
        check(torch, dec, [f], (0, 0))
        assert dec.rounds() == 0


def test_adversarial_stream_takes_64_rounds(xa, torch, dec):
    """Every guess wrong and every exit computed from a wrong entry wrong: the right states advance one lane per round."""
    f, coef = dc.adversarial()
    cnt = ds.new_counters()
    status, pixels, _, _ = ds.decode(f, 1, 128, cnt)
    assert status == 0 and cnt["max_rounds"] == ds.LANES and cnt["tiles_over_one"] == 1
    for form in FORMS:
        want = check(torch, dec, [f], form)
        assert want[1][0]["status"] == 0 and np.array_equal(want[0][:pixels.size], pixels.reshape(-1))
        if form == (1, 128):
            assert dec.rounds() == ds.LANES


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_restart_intervals(xa, torch, dec, rgb, form):
    """The encoder specification's files: 5 x 13 MCUs (grey), 3 x 5 (RGB); intervals of one MCU, a short last interval, a block
    row, one interval more than the image has MCUs; 65 intervals: RSTm wraps eight times."""
    image = jc.noise(60, (24, 40, 3)) if rgb else jc.smooth((40, 104))
    mcus, per_row = (15, 5) if rgb else (65, 13)
    files = [js.encode(image, quality=85, restart=r)[0] for r in (0, 1, 2, 7, per_row, mcus - 1, mcus, mcus + 1, 65535)]
    _, records, _ = check(torch, dec, files, form)
    assert (records["status"] == 0).all() and list(records["intervals"][:4]) == [1, mcus, (mcus + 1) // 2, (mcus + 6) // 7]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_mixed_batch(xa, torch, dec, golden, form):
    """About 40 streams of mixed shape, component count, tables and restart settings, unsupported and damaged ones between
    sound ones, at odd offsets with garbage between and behind them, records 40 bytes apart: the neighbours are untouched."""
    base, rgb = golden.files["grey_7x9"], golden.files["rgb_7x9"]
    odd = [golden.files[n] for n in golden.unsupported] + [dc.patched(rgb if w == "two_components" else base, w) for w in dc.PATCHES]
    damaged = dc.damaged_set(base, golden.files["grey_smooth_rows"])
    odd += [f for n, f in damaged if n in ("rst_removed", "rst_swapped", "other_marker", "rst_inserted", "no_eoi", "cut_in_scan")]
    odd += [f for n, f in damaged if n.startswith("flip_")][:4] + [base[:40], b"", b"\xff"]
    sound = [golden.files[n] for n in golden.sound if "row75" not in n]
    files = []
    for i, f in enumerate(sound):
        files.append(f)
        if i < len(odd):
            files.append(odd[i])
    assert len(files) >= 40
    pixels, records, summary = check(torch, dec, files, form, gaps=True, stride=40, seed=3)
    assert summary["images"] >= len(sound) and summary["by_status"][1] >= 5 and summary["by_status"][2] >= 5 and summary["by_status"][7:].sum() >= 5
    pillow = {golden.files[n]: golden.pixels[n] for n in golden.sound}
    for r, f in zip(records[::2], sound):
        assert r["status"] == 0 and np.array_equal(pixels[int(r["offset"]):int(r["offset"] + r["length"])], pillow[f].reshape(-1))


def test_item_and_block_counts_around_the_scan_tile(xa, torch, dec, golden):
    """Items n: the item scan has n + 1 elements.  Blocks b: the DC scan has b."""
    tiny = [golden.files["grey_1x1"], golden.files["rgb_1x1"], golden.files["grey_8x8"], b"\xff\xd8\xff"]
    for n in (SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        check(torch, dec, [tiny[i % 4] for i in range(n)], (1, 128))
    for blocks in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        f = js.encode(jc.smooth((8, 8 * blocks)), quality=50, restart=0)[0]
        check(torch, dec, [f], (1, 0))
        check(torch, dec, [f, golden.files["rgb_8x8"]], (0, 0))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_damaged_set(xa, torch, dec, golden, form):
    """Every truncation of a small stream, byte flips in its scan, RSTm removed, swapped, replaced, inserted, the EOI gone: the
    device equals the specification item for item, and the sound stream at both ends of the batch keeps its pixels."""
    base = golden.files["grey_7x9"]
    files = [base] + [f for _, f in dc.damaged_set(base, golden.files["grey_smooth_rows"])] + [base]
    pixels, records, summary = check(torch, dec, files, form)
    assert records[0]["status"] == 0 and records[-1]["status"] == 0 and len(set(records["status"])) >= 6
    for r in (records[0], records[-1]):
        assert np.array_equal(pixels[int(r["offset"]):int(r["offset"] + r["length"])], golden.pixels["grey_7x9"].reshape(-1))
    bad = records["status"] >= 4
    assert bad.any() and all(not pixels[int(r["offset"]):int(r["offset"] + r["length"])].any() for r in records[bad])


def test_scratch_too_small_for_the_batch(xa, torch, dec, golden):
    """max_blocks below the batch's blocks: the item that passes it and every sound one behind it are TOO_LARGE, with no pixels."""
    files = [golden.files[n] for n in ("grey_7x9", "rgb_7x9", "grey_q100_noise", "progressive", "grey_8x8", "rgb_8x8")]
    for max_blocks in (1, 2, 7, 8, 79, 80, 81, 83, 84):      # the running totals: 2, 8, 80, 81, 84 blocks
        _, records, summary = check(torch, dec, files, (1, 128), max_blocks=max_blocks)
        assert summary["by_status"][3] == sum(b > max_blocks for b in (2, 8, 80, 81, 84))


def test_output_that_does_not_fit(xa, torch, dec, golden):
    """cap at, one below and far below the batch's bytes, and 0: overflow 1, the images that fit written, nothing behind cap."""
    files = [golden.files[n] for n in ("grey_7x9", "rgb_9x7", "grey_smooth_rows", "rgb_1x1", "grey_8x8")]
    buf, items = laid_out(files)
    total = int(ds.decode_batch(buf, items, cache=CACHE)[2]["bytes"])
    for cap in (total, total - 1, total - 64, 64 + 192 + 3, 64, 63, 4, 0):
        want = check(torch, dec, files, (0, 0), cap=cap)
        assert want[2]["overflow"] == (cap < total) and want[2]["bytes"] == total


def test_calls_back_to_back_without_a_wait(xa, torch, dec, golden):
    """Five calls on one handle and one stream, forms and batches changing between them, one wait at the end."""
    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    jobs = [(["grey_q100_noise", "rgb_7x9"], (1, 128)), (["rgb_q100_noise_opt"], (0, 0)), (["grey_1x1", "progressive", "rgb_row75"], (1, 0)),
            (["grey_smooth_rows", "grey_own_tables", "rgb_ones"], (1, 128)), (["grey_q100_noise", "rgb_7x9"], (0, 0))]
    calls = []
    for i, (names, form) in enumerate(jobs):
        buf, items = laid_out([golden.files[n] for n in names], i, gaps=True)
        cap = int(ds.decode_batch(buf, items, cache=CACHE)[2]["bytes"])
        args, keep = prepare(torch, buf, items, cap, seed=i)
        calls.append((args, keep, expected(buf, items, cap), form, len(items)))
    for args, _, _, _, _ in calls:                     # once each, so that the scratch is as large as any of them needs
        dec.decode_device(*args, max_blocks=4096)
    torch.cuda.synchronize()
    for _, keep, _, _, _ in calls:
        for t in keep[2:]:
            t.fill_(0xA5)
    torch.cuda.synchronize()
    for args, _, _, form, _ in calls:
        dec.set_form(*form)
        dec.decode_device(*args, max_blocks=4096, stream=s.cuda_stream)
    s.synchronize()                                     # the only one behind the five calls
    for _, keep, want, _, n in calls:
        same(keep, want, n)


def test_behind_the_encoder_on_one_stream(xa, torch, dec):
    """xrit_jpeg_encode_device -> xrit_jpegdec_decode_device on one stream with no wait in between: the item record is made
    on the device from the encoder's result record.  The pixels are the specification's decode of the specification's file."""
    dev = torch.device("cuda:0")
    enc = xa.JpegEncoder()
    s = torch.cuda.Stream(device=dev)
    for image, restart in ((jc.smooth((40, 104)), 13), (jc.noise(5, (24, 40, 3)), 0)):
        comps = 1 if image.ndim == 2 else 3
        file, _ = js.encode(image, quality=85, restart=restart)
        status, pixels, _, _ = ds.decode(file)
        assert status == 0
        enc.set_quality(85, restart)
        cap = enc.bound(comps, image.shape[1], image.shape[0])
        d_img = torch.from_numpy(image.reshape(-1).copy()).to(dev)
        d_file = torch.zeros(cap, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(16, dtype=torch.uint8, device=dev)
        d_item = torch.zeros(16, dtype=torch.uint8, device=dev)
        d_pixels = torch.full((pixels.size + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        d_records = torch.zeros(64, dtype=torch.uint8, device=dev)
        d_summary = torch.zeros(64, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        dec.set_form(1, 128)
        with torch.cuda.stream(s):
            enc.encode_device(d_img.data_ptr(), image.shape[1], image.shape[0], image.shape[1] * comps, comps, d_file.data_ptr(), cap, d_res.data_ptr(),
                              stream=s.cuda_stream)
            d_item[8:12] = d_res[0:4]                   # {offset 0, length = the file's size}, on the same stream
            dec.decode_device(d_file.data_ptr(), cap, d_item.data_ptr(), 16, 1, d_pixels.data_ptr(), pixels.size, d_records.data_ptr(),
                              d_summary.data_ptr(), max_blocks=1024, stream=s.cuda_stream)
        s.synchronize()
        assert d_file.cpu().numpy()[:len(file)].tobytes() == file
        rec = d_records.cpu().numpy().view(ds.RECORD_DTYPE)[0]
        assert rec["status"] == 0 and rec["length"] == pixels.size
        out = d_pixels.cpu().numpy()
        assert np.array_equal(out[:pixels.size], pixels.reshape(-1)) and (out[(pixels.size + 3) & ~3:] == 0xA5).all()
    enc.close()


def test_host_buffer_form_and_header_function(xa, torch, dec, golden):
    files = [golden.files[n] for n in ("grey_com_app", "rgb_trailing", "s420", "rgb_q1", "grey_ones")]
    buf, items = laid_out(files, 1, gaps=True)
    writes, records, summary = ds.decode_batch(buf, items, cache=CACHE)
    for form in FORMS:
        dec.set_form(*form)
        pixels, got_r, got_s = dec.decode(buf, items)
        assert got_s.tobytes() == summary.tobytes() and got_r.tobytes() == records.tobytes() and len(pixels) == summary["bytes"]
        for at, data in writes:
            assert pixels[at:at + len(data)].tobytes() == data
    with pytest.raises(xa.XritError) as ei:
        dec.decode(buf, items, cap=int(summary["bytes"]) - 4)
    assert ei.value.code == -5 and ei.value.summary["overflow"] == 1 and ei.value.records.tobytes() == records.tobytes()
    first = writes[0]
    assert ei.value.pixels[first[0]:first[0] + len(first[1])].tobytes() == first[1]
    for f in files + [files[0][:100], b""]:
        assert xa.jpegdec_header(f).tobytes() == ds.header_info(f).tobytes()
    dec.reset()


def test_bad_arguments_leave_the_outputs_untouched(xa, torch, dec, golden):
    buf, items = laid_out([golden.files["grey_7x9"]])
    args, keep = prepare(torch, buf, items, 256)
    good = dict(zip(("bytes", "n_bytes", "items", "stride", "n_items", "pixels", "cap", "records", "summary"), args))
    bad = [dict(bytes=None), dict(items=None), dict(pixels=None), dict(records=None), dict(summary=None), dict(stride=8), dict(stride=18), dict(stride=0),
           dict(n_bytes=(1 << 28) + 1), dict(n_items=(1 << 20) + 1), dict(records=good["records"] + 4), dict(summary=good["summary"] + 2), dict(max_blocks=(1 << 22) + 1)]
    for change in bad:
        a = dict(dict(good, max_blocks=0), **change)
        with pytest.raises(xa.XritError) as ei:
            dec.decode_device(a["bytes"], a["n_bytes"], a["items"], a["stride"], a["n_items"], a["pixels"], a["cap"], a["records"], a["summary"],
                              max_blocks=a["max_blocks"])
        assert ei.value.code == -1, change
    for call in (lambda: dec.set_form(2), lambda: dec.set_form(1, 31), lambda: dec.set_form(1, (1 << 20) + 1)):
        with pytest.raises(xa.XritError) as ei:
            call()
        assert ei.value.code == -1
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 0xA5).all() for t in keep[2:])
    dec.set_form(0, 0)
    dec.decode_device(*args)
    torch.cuda.synchronize()
    same(keep, expected(buf, items, 256), 1)


def test_second_level_of_the_byte_scan(xa, torch, dec, golden):
    """More than 2^20 scan bytes in a call: a stream with a megabyte behind its EOI (ignored, but scan bytes of the item), so
    that the two streams behind it take their place in the unstuffed stream from the byte scan's second level."""
    tail = np.random.default_rng(8).integers(0, 256, (1 << 20) + 5000, dtype=np.uint8).tobytes()
    files = [golden.files["grey_7x9"] + tail, golden.files["rgb_9x7"], golden.files["grey_smooth_rows"]]
    for form in ((0, 0), (1, 128)):
        _, records, _ = check(torch, dec, files, form, max_blocks=64)
        assert (records["status"] == 0).all()


def test_host_program_files_jpeg(xa, golden, tmp_path):
    """End to end from IQ: image files whose structure record says compression 2 with Pillow's streams as data fields (grey,
    RGB, one that takes several packets), a progressive and a cut one, and a file that is no image.  With --files-jpeg every
    sound one has its .pgm / .ppm, Pillow's pixels; the others write nothing and get a line on stderr; without the flag the
    directory and stderr are what they are with it, less those."""
    import os
    import subprocess

    import file_spec as fs
    import image_spec as isp
    from test_gpu_canvas import host_capture
    rng = np.random.default_rng(71)
    sound = ["grey_smooth_rows", "rgb_7x9", "grey_q100_noise", "rgb_com_app"]
    streams = [golden.files[n] for n in sound] + [golden.files["progressive"], golden.files["grey_7x9"][:200]]
    items = [((5, 40 + i % 2), fs.lrit_file(s, image=(8, 8, 8, 2)), None, 900) for i, s in enumerate(streams)]
    items.append(((5, 42), fs.lrit_file(b"no image " * 300), None, 900))
    iq = host_capture(tmp_path, {5: [p for _, p, _ in isp.stream_of(rng, items)]}, 71)
    host_bin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xritdemod_amd", "bin", "xrit_demod_host")
    base = [host_bin, "--input", str(iq), "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null", "--block", "200000"]
    runs = {}
    for name, extra in (("without", []), ("with", ["--files-jpeg"])):
        r = subprocess.run(base + ["--files", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        runs[name] = ({nm: (tmp_path / name / nm).read_bytes() for nm in os.listdir(tmp_path / name)}, r.stderr)
    plain, err = runs["without"]
    got, err2 = runs["with"]
    # (the capture's filler packets on apid 99 become files too)
    assert len([nm for nm in plain if nm.endswith(".lrit") and "apid99" not in nm]) == 7 and not [nm for nm in plain if nm.endswith((".pgm", ".ppm"))] and "files-jpeg" not in err
    images = {nm for nm in got if nm.endswith((".pgm", ".ppm"))}
    assert {nm: v for nm, v in got.items() if nm not in images} == plain and len(images) == 4
    mine = [ln for ln in err2.splitlines() if ln.startswith("files-jpeg:")]
    assert [ln for ln in err2.splitlines() if not ln.startswith("files-jpeg:")] == err.splitlines()
    assert mine[-1] == "files-jpeg: 4 images written, 2 streams refused" and len(mine) == 3
    pillow = {golden.files[n]: golden.pixels[n] for n in sound}
    seen = 0
    for nm, body in plain.items():
        if not nm.endswith(".lrit"):
            continue
        data = body[int.from_bytes(body[4:8], "big"):]
        stem = nm[:-len(".lrit")]
        if data in pillow:
            want = pillow[data]
            kind, suffix = (b"P5", ".pgm") if want.ndim == 2 else (b"P6", ".ppm")
            assert got[stem + suffix] == kind + b"\n%d %d\n255\n" % (want.shape[1], want.shape[0]) + want.tobytes(), nm
            seen += 1
        else:
            assert stem + ".pgm" not in got and stem + ".ppm" not in got
            assert (data in streams) == any(stem + ".lrit: status" in ln for ln in mine), nm
    assert seen == 4
