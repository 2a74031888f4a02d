"""GPU tier: the JPEG stage (xrit_jpeg_*, JpegEncoder) against the specification of tests/jpeg_spec.py -- the whole file
and the result record, compared with np.array_equal.  The shapes are the smallest at which the kernels can still go wrong:
one pixel; exactly one block; partial blocks on both edges; one block row of 75 blocks (more than a wave of blocks, more
than the 32 MCUs of a transform workgroup); block, interval and stream-group counts one below, at and one above the scan
tile (scan.h's SCAN_TILE = 1024 elements; every scan here has one element more than it has blocks, intervals or groups of
16 stream bytes); more than 2^20 blocks and intervals, where the scans of the tiles' sums take their second level; grey and
RGB.  Restart 0, 1, 2, 7, 64, 65, blocks per row and larger than the image, with a short last interval; 24 intervals; the
event-rich inputs of the CPU tier, their events asserted through the counters; the recorded Pillow files reproduced by the
device.  A pitch with garbage in the padding and bases that are no multiple of 16, 4 or 2; guard bytes behind the output;
cap one byte short, cutting into the header, and 0; encodes back to back without a wait; the stage queued behind product
and composite on one stream; the host-buffer and resident forms; every bad argument; xrit_demod_host --jpeg.

Not reached at a test's size: 0xFF counts that differ across a second-level tile of the stuffing scan (that takes more
than 16 MiB of entropy-coded data); the second level itself runs in test_more_than_2_20_blocks."""
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_spec as js

pytestmark = pytest.mark.gpu

GUARD = 64                                              # bytes behind the output and the record that must stay as they were
SCAN_TILE = 1024                                        # csrc/scan.h: elements per workgroup of a scan


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
def enc(xa):
    h = xa.JpegEncoder()
    yield h
    h.close()


def laid_out(rng, image, pitch, offset):
    """The image's bytes at `offset` of a buffer, `pitch` bytes from row to row, non-zero garbage everywhere else; the
    buffer ends with the last row's last byte."""
    rows = image.shape[0]
    raw = np.ascontiguousarray(image).reshape(rows, -1)
    buf = rng.integers(1, 256, offset + pitch * (rows - 1) + raw.shape[1], dtype=np.uint8)
    for r in range(rows):
        buf[offset + r * pitch:offset + r * pitch + raw.shape[1]] = raw[r]
    return buf


def setup(enc, params):
    if "quality" in params:
        enc.set_quality(params["quality"], params["restart"])
    else:
        enc.set_tables(params["tables"], params["restart"])


def prepare(torch, image, cap, pitch=None, offset=0, out_offset=0, seed=0):
    """The image laid out in device memory, the output and the record filled with 0xA5 -> what encode_device takes."""
    dev = torch.device("cuda:0")
    rows, columns = image.shape[:2]
    comps = 1 if image.ndim == 2 else 3
    pitch = columns * comps if pitch is None else pitch
    d_img = torch.from_numpy(laid_out(np.random.default_rng(seed), image, pitch, offset)).to(dev)
    d_out = torch.full((out_offset + cap + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((16 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert d_img.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()                            # the fills are done before anything is queued on another stream
    args = (d_img.data_ptr() + offset, columns, rows, pitch, comps, d_out.data_ptr() + out_offset, cap, d_res.data_ptr())
    return args, (d_img, d_out, d_res, out_offset, cap)


def same(keep, want, restarts):
    """The file and the record equal the specification's; the bytes in front of, behind the output and behind the record
    are untouched.  A file that did not fit: status 1, the right size, nothing at or behind cap."""
    _, d_out, d_res, out_offset, cap = keep
    out, res = d_out.cpu().numpy(), d_res.cpu().numpy()
    assert (out[:out_offset] == 0xA5).all() and (out[out_offset + cap:] == 0xA5).all() and (res[16:] == 0xA5).all()
    fits = len(want) <= cap
    assert np.array_equal(res[:16].view(js.RESULT_DTYPE), np.array([(len(want), 0 if fits else 1, restarts)], js.RESULT_DTYPE))
    if fits:
        assert np.array_equal(out[out_offset:out_offset + len(want)], np.frombuffer(want, np.uint8))
        assert (out[out_offset + len(want):] == 0xA5).all()


def check(xa, torch, enc, image, params, slack=7, **layout):
    want, cnt = jc.spec_file(image, params)
    setup(enc, params)
    args, keep = prepare(torch, image, len(want) + slack, **layout)
    enc.encode_device(*args)
    torch.cuda.synchronize()
    same(keep, want, cnt["restarts"])
    return cnt


def test_one_pixel(xa, torch, enc):
    for image in (np.array([[0]], np.uint8), np.array([[255]], np.uint8), np.array([[77]], np.uint8), np.array([[[250, 3, 99]]], np.uint8),
                  np.array([[[0, 255, 0]]], np.uint8)):
        for quality in (1, 90, 100):
            check(xa, torch, enc, image, dict(quality=quality, restart=0))
    check(xa, torch, enc, np.array([[[9, 200, 31]]], np.uint8), dict(quality=75, restart=1))


@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_one_block_and_partial_blocks(xa, torch, enc, rgb):
    for i, shape in enumerate(((8, 8), (7, 9), (9, 7), (17, 33), (1, 64), (64, 1), (23, 5))):
        image = jc.noise(30 + i, shape + (3,) if rgb else shape)
        for params in (dict(quality=90, restart=0), dict(quality=50, restart=2), dict(tables=jc.ONES, restart=1)):
            check(xa, torch, enc, image, params)


@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_one_block_row_of_75_blocks(xa, torch, enc, rgb):
    for image in (jc.noise(40, (8, 600, 3) if rgb else (8, 600)), jc.smooth((8, 600, 3) if rgb else (8, 600)), jc.noise(41, (5, 597, 3) if rgb else (5, 597))):
        for restart in (0, 75, 33):
            check(xa, torch, enc, image, dict(quality=95, restart=restart))


def test_block_and_interval_counts_around_the_scan_tile(xa, torch, enc):
    """Blocks b: the scan over bit offsets has b + 1 elements; with restart 1 the scan over intervals has as many.  1022
    .. 1025 blocks put that at one below the tile, at it, and one and two above it; 2047 .. 2049 at the second tile's end."""
    for blocks in (SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE - 1, 2 * SCAN_TILE, 2 * SCAN_TILE + 1):
        image = jc.noise(blocks, (8, 8 * blocks), 64, 192)
        for restart in (0, 1):
            check(xa, torch, enc, image, dict(quality=50, restart=restart))
    for mcus in (341, 342):                             # 1023 and 1026 blocks in three components
        check(xa, torch, enc, jc.noise(mcus, (8, 8 * mcus, 3)), dict(quality=75, restart=1))


def test_stream_group_counts_around_the_scan_tile(xa, torch, enc):
    """The scan over the 0xFF counts has one element per 16 bytes of entropy-coded data and one more.  A row of noise
    blocks (with 0xFF bytes among theirs) and then flat ones, 6 bits each, as many as bring the data to 1022, 1023 and
    1024 groups: the file's length, which is the last element, then lies one below the tile's end, at it, and in the next."""
    noise_blocks = 500
    noisy = jc.noise(50, (8, 8 * noise_blocks))
    head = len(js.header(1, 8, 8, js.quality_tables(50), 0))

    def stream_bytes(flat):
        image = np.concatenate([noisy, np.full((8, 8 * flat), noisy[0, -1], np.uint8)], 1) if flat else noisy
        file, cnt = js.encode(image, quality=50, restart=0)
        return image, len(file) - head - 2 - cnt["stuffed"] - cnt["pad_ff"], cnt

    _, t0, _ = stream_bytes(0)
    assert t0 < 16 * (SCAN_TILE - 3)
    reached = set()
    for groups in (SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE):
        flat = ((16 * groups - 8 - t0) * 8) // 6       # 6 bits a flat block: the middle of the group
        image, t, cnt = stream_bytes(flat)
        assert (t + 15) // 16 == groups and cnt["stuffed"] > 5
        check(xa, torch, enc, image, dict(quality=50, restart=0))
        reached.add(groups + 1)
    assert reached == {SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1}


def test_more_than_2_20_blocks(xa, torch):
    """1024 x 1025 blocks, each its own restart interval: the bit-offset and the interval scans have more than 2^20
    elements, the stuffing scan's bound more than 2^23, so all three scan their tiles' sums at a second level.  The image
    is a tile of 25 flat blocks repeated, so its coefficients are the tile's repeated and the specification is cheap."""
    levels = np.array([128, 128, 131, 90, 255, 0, 17, 128, 200, 201, 199, 64, 64, 64, 250, 5, 128, 127, 129, 30, 220, 110, 111, 128, 96], np.uint8)
    tile = np.repeat(np.repeat(levels[None, :], 8, 0), 8, 1)
    image = np.tile(tile, (1024, 41))
    assert image.shape == (8192, 8200)
    tables = js.quality_tables(90)
    coef = np.tile(js.coefficients(tile, tables), (1024 * 41, 1, 1))
    assert len(coef) == 1024 * 1025 > (1 << 20)
    body, cnt = js.scan(coef, 1)
    want = js.header(1, 8200, 8192, tables, 1) + body + b"\xff\xd9"
    big = xa.JpegEncoder(quality=90, restart=1)         # a handle of its own: the scratch of this size goes with it
    dev = torch.device("cuda:0")
    d_img = torch.from_numpy(image).to(dev)
    d_out = torch.full((len(want) + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((16 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    big.encode_device(d_img.data_ptr(), 8200, 8192, 8200, 1, d_out.data_ptr(), len(want), d_res.data_ptr())
    torch.cuda.synchronize()
    same((d_img, d_out, d_res, 0, len(want)), want, cnt["restarts"])
    assert cnt["restarts"] == 1024 * 1025 - 1
    del d_img, d_out
    big.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_restart_intervals(xa, torch, enc, rgb):
    """5 x 131 MCUs (grey) and 3 x 25 (RGB): 655 % 64 = 15 and 75 % 7 = 5 leave a short last interval, 655 % 2 = 1 an
    interval of one MCU."""
    image = jc.noise(60, (24, 200, 3)) if rgb else jc.smooth((40, 1048))
    mcus, per_row = ((3 * 25, 25) if rgb else (5 * 131, 131))
    for restart in (0, 1, 2, 7, 64, 65, per_row, mcus - 1, mcus, mcus + 1, 65535):
        cnt = check(xa, torch, enc, image, dict(quality=85, restart=restart))
        assert cnt["restarts"] == ((mcus + restart - 1) // restart - 1 if restart else 0)
        assert cnt["short_last"] == (1 if restart and mcus % restart and restart < mcus else 0)


def test_event_rich_inputs_still_carry_their_events(xa, torch, enc):
    total = dict.fromkeys(js.COUNTERS, 0)
    most = 0
    for _, image, params in jc.event_cases():
        cnt = check(xa, torch, enc, image, params)
        most = max(most, cnt["restarts"])
        for k, v in cnt.items():
            total[k] += v
    assert all(total[k] > 0 for k in js.COUNTERS), total
    assert most >= 16                                   # RSTm wraps twice


def test_device_reproduces_the_recorded_pillow_files(xa, torch, enc):
    """No encoder of ours in between: the images of tests/golden/jpeg_pil_files.npz in, libjpeg's bytes out."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_pil_files.npz"))
    cases = jc.golden_cases()
    assert len(z["names"]) == len(cases)
    for i, (name, _, params) in enumerate(cases):
        image, want = z["image_%02d" % i], z["data"][z["offsets"][i]:z["offsets"][i + 1]].tobytes()
        setup(enc, params)
        assert enc.encode(image) == want, name
        args, keep = prepare(torch, image, len(want))
        enc.encode_device(*args)
        torch.cuda.synchronize()
        same(keep, want, keep[2].cpu().numpy()[:16].view(js.RESULT_DTYPE)[0]["restarts"])


def test_pitch_with_garbage_and_odd_bases(xa, torch, enc):
    """Input bases off every 16-, 4- and 2-byte boundary, rows a prime number of bytes apart, the output off them too."""
    for i, (rgb, offset, extra, out_offset) in enumerate(((False, 1, 3, 1), (False, 2, 1, 3), (False, 5, 0, 2), (False, 16, 61, 6), (True, 1, 1, 5),
                                                          (True, 3, 2, 1), (True, 6, 7, 9), (True, 0, 13, 0))):
        image = jc.noise(70 + i, (21, 37, 3) if rgb else (21, 37))
        pitch = 37 * (3 if rgb else 1) + extra
        check(xa, torch, enc, image, dict(quality=90, restart=3), pitch=pitch, offset=offset, out_offset=out_offset, seed=i)


def test_file_that_does_not_fit(xa, torch, enc):
    """cap one byte short, a cap that cuts into the header, cap = 0: status 1, the size of the whole file, nothing at or
    behind cap, no fault; then the same call with room."""
    for image in (jc.noise(80, (33, 70)), jc.noise(81, (19, 21, 3))):
        params = dict(quality=100, restart=2)
        want, cnt = jc.spec_file(image, params)
        setup(enc, params)
        for cap in (len(want) - 1, len(want) - 2, len(want) // 2, 100, 1, 0, len(want)):
            args, keep = prepare(torch, image, cap)
            enc.encode_device(*args)
            torch.cuda.synchronize()
            same(keep, want, cnt["restarts"])
            if cap < len(want):
                out = keep[1].cpu().numpy()
                assert np.array_equal(out[:min(cap, 100)], np.frombuffer(want, np.uint8)[:min(cap, 100)])        # (what fits of the header is there)


def test_calls_back_to_back_without_a_wait(xa, torch, enc):
    """Five encodes on one handle and one stream, shapes and parameters changing between them, one wait at the end: the
    scratch of one call must not show in the next, and the parameters travel with each call."""
    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    jobs = [(jc.noise(90, (64, 72)), dict(quality=90, restart=0)), (jc.noise(91, (9, 7, 3)), dict(tables=jc.ONES, restart=1)),
            (jc.smooth((40, 104)), dict(quality=30, restart=13)), (jc.noise(92, (64, 72)), dict(quality=100, restart=9)),
            (jc.noise(90, (64, 72)), dict(quality=90, restart=0))]
    enc.set_quality(100, 0)
    enc.encode(jc.noise(93, (128, 128, 3)))             # the scratch is as large as any of them needs: nothing is allocated below
    calls = []
    for i, (image, params) in enumerate(jobs):
        want, cnt = jc.spec_file(image, params)
        args, keep = prepare(torch, image, len(want) + 5, seed=i)
        calls.append((args, keep, want, cnt, params))
    for args, _, _, _, params in calls:
        setup(enc, params)
        enc.encode_device(*args, stream=s.cuda_stream)
    s.synchronize()                                     # the only one behind the five calls
    for _, keep, want, cnt, _ in calls:
        same(keep, want, cnt["restarts"])


def test_queued_behind_product_and_composite_on_one_stream(xa, torch, enc):
    """Two 10-bit images toned by the product stage, their composite, and three encodes -- the two toned images as grey, the
    composite as RGB -- all on one stream with one wait at the end, every stage reading its predecessor's output in place."""
    import product_spec as sp
    rng = np.random.default_rng(95)
    rows, columns = 45, 150
    a, b = (rng.integers(0, 1024, (rows, columns)).astype(np.uint16) for _ in range(2))
    table = rng.integers(0, 256, 256 * 256 * 3, dtype=np.uint8)
    tone_a, tone_b = (sp.process(x, 10, sp.EQUALISE)["tone"] for x in (a, b))
    rgb = sp.composite(tone_a, tone_b, table)
    params = dict(quality=92, restart=(columns + 7) // 8)
    wants = [jc.spec_file(x, params) for x in (tone_a, tone_b, rgb)]
    dev = torch.device("cuda:0")
    pr = xa.ImageProduct()
    d_a, d_b = (torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to(dev) for x in (a, b))
    d_table = torch.from_numpy(table).to(dev)
    d_tone = [torch.zeros(rows * columns, dtype=torch.uint8, device=dev) for _ in range(2)]
    d_sum = [torch.zeros(64, dtype=torch.uint8, device=dev) for _ in range(2)]
    d_rgb = torch.zeros(rows * columns * 3, dtype=torch.uint8, device=dev)
    outs = [(torch.full((len(w) + GUARD,), 0xA5, dtype=torch.uint8, device=dev), torch.full((16 + GUARD,), 0xA5, dtype=torch.uint8, device=dev))
            for w, _ in wants]
    setup(enc, params)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    for d_x, d_t, d_s in zip((d_a, d_b), d_tone, d_sum):
        pr.process_device(d_x.data_ptr(), columns, rows, 2 * columns, 10, d_s.data_ptr(), tone="equalise", d_tone_ptr=d_t.data_ptr(), stream=s.cuda_stream)
    pr.composite_device(d_tone[0].data_ptr(), columns, d_tone[1].data_ptr(), columns, columns, rows, d_table.data_ptr(), d_rgb.data_ptr(),
                        stream=s.cuda_stream)
    for d_x, comps, (d_o, d_r), (w, _) in zip((d_tone[0], d_tone[1], d_rgb), (1, 1, 3), outs, wants):
        enc.encode_device(d_x.data_ptr(), columns, rows, columns * comps, comps, d_o.data_ptr(), len(w), d_r.data_ptr(), stream=s.cuda_stream)
    s.synchronize()                                     # the only one
    for (d_o, d_r), (w, cnt) in zip(outs, wants):
        same((None, d_o, d_r, 0, len(w)), w, cnt["restarts"])
    # the resident form on what the product stage's host-buffer call left on the device
    got = pr.process(a, 10, "equalise", factor=4)
    d_t, d_s = pr.outputs_device()
    enc.set_quality(80, 0)
    assert enc.encode_resident(d_t, columns, rows, columns, 1) == js.encode(got["tone"], quality=80)[0]
    assert enc.encode_resident(d_s, got["small"].shape[1], got["small"].shape[0], got["small"].shape[1], 1) == js.encode(got["small"], quality=80)[0]
    pr.close()


def test_host_buffer_and_resident_forms(xa, torch, enc):
    for i, (shape, params) in enumerate((((33, 70), dict(quality=90, restart=0)), ((19, 21, 3), dict(quality=75, restart=4)),
                                         ((64, 200, 3), dict(tables=jc.late_tables(20, 63), restart=25)))):
        image = jc.noise(100 + i, shape)
        want, _ = jc.spec_file(image, params)
        setup(enc, params)
        assert enc.encode(image) == want
        assert enc.encode(image, cap=len(want)) == want
        padded = np.pad(image, ((0, 0), (0, 5)) + (((0, 0),) if image.ndim == 3 else ()), constant_values=9)[:, :shape[1]]     # a pitch of the host's
        assert padded.strides[0] > image.strides[0] and enc.encode(padded) == want
        with pytest.raises(xa.XritError) as ei:
            enc.encode(image, cap=len(want) - 1)
        assert ei.value.code == -5 and str(len(want)) in str(ei.value)
        d_img = torch.from_numpy(image.reshape(-1).copy()).to("cuda:0")
        comps = 1 if image.ndim == 2 else 3
        assert enc.encode_resident(d_img.data_ptr(), shape[1], shape[0], shape[1] * comps, comps) == want
        with pytest.raises(xa.XritError) as ei:
            enc.encode_resident(d_img.data_ptr(), shape[1], shape[0], shape[1] * comps, comps, cap=50)
        assert ei.value.code == -5
        # the handle's header and bound: host only, the specification's
        tables = js.quality_tables(params["quality"]) if "quality" in params else params["tables"]
        assert enc.header(comps, shape[1], shape[0]) == js.header(comps, shape[1], shape[0], tables, params["restart"]) == want[:len(enc.header(comps, shape[1], shape[0]))]
        assert enc.bound(comps, shape[1], shape[0]) == js.bound(comps, shape[1], shape[0], params["restart"]) >= len(want)
    enc.reset()


def test_bad_arguments_leave_the_outputs_untouched(xa, torch, enc):
    dev = torch.device("cuda:0")
    d_img = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    d_out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((64,), 0xA5, dtype=torch.uint8, device=dev)
    enc.set_quality(90, 0)
    good = dict(img=0, columns=30, rows=20, pitch=90, comps=3, out=0, cap=4000, res=0)
    bad = [dict(comps=0), dict(comps=2), dict(comps=4), dict(columns=0), dict(rows=0), dict(columns=65536), dict(rows=65536), dict(pitch=89),
           dict(comps=1, pitch=29), dict(img=None), dict(out=None), dict(out=None, cap=0), dict(res=None), dict(res=4), dict(columns=16385, rows=16384, comps=1, pitch=16385),
           dict(columns=16384, rows=16384, pitch=3 * 16384)]
    for change in bad:
        a = dict(good, **change)
        ptr = lambda t, k: None if a[k] is None else t.data_ptr() + a[k]
        with pytest.raises(xa.XritError) as ei:
            enc.encode_device(ptr(d_img, "img"), a["columns"], a["rows"], a["pitch"], a["comps"], ptr(d_out, "out"), a["cap"], ptr(d_res, "res"))
        assert ei.value.code == -1, change
    for call in (lambda: enc.set_quality(0), lambda: enc.set_quality(101), lambda: enc.set_quality(90, 65536), lambda: enc.set_tables(np.zeros((2, 64))),
                 lambda: enc.set_tables(np.where(np.arange(128) == 127, 0, 7)), lambda: enc.set_tables(jc.ONES, 65536),
                 lambda: xa.JpegEncoder(quality=0), lambda: enc.header(2, 8, 8), lambda: enc.header(1, 0, 8)):
        with pytest.raises(xa.XritError) as ei:
            call()
        assert ei.value.code == -1
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all() and (d_res.cpu().numpy() == 0xA5).all()
    # a refused setting changes nothing: the call that is good, from the same arguments, at quality 90 and restart 0
    enc.encode_device(d_img.data_ptr(), 30, 20, 90, 3, d_out.data_ptr(), 4000, d_res.data_ptr())
    torch.cuda.synchronize()
    want = js.encode(np.zeros((20, 30, 3), np.uint8), quality=90)[0]
    assert d_out.cpu().numpy()[:len(want)].tobytes() == want and int(d_res.cpu().numpy()[:16].view(js.RESULT_DTYPE)[0]["size"]) == len(want)


def test_host_program_jpeg(xa, tmp_path):
    """The capture of the product stage's host program test: with --jpeg every .view.pgm and .thumb.pgm has its .jpg, the
    specification's of that file's pixels at the quality given with a restart marker per row of blocks, and Pillow opens
    it; everything else the run writes, and every stderr line but the stage's own, is what it writes without the flag."""
    import canvas_spec as cs
    import image_spec as isp
    from test_gpu_canvas import host_capture
    rng = np.random.default_rng(70)
    a, b, c = cs.samples(rng, 8, 16, 64, 12), cs.samples(rng, 10, 32, 33, 5), cs.samples(rng, 8, 8, 16, 4)
    items = cs.split_image(rng, a, 8, 16, 21, [(5, 40), (5, 41)], [7], name=b"GOES test/full disk.lrit")
    items += cs.split_image(rng, b, 10, 32, 22, [(5, 42)], [])
    items += cs.split_image(rng, np.concatenate([c, c]), 8, 8, 23, [(5, 43)], [4])[:1]
    by_vc = {5: [p for _, p, _ in isp.stream_of(rng, items)]}
    iq = host_capture(tmp_path, by_vc, 70)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host_bin = os.path.join(root, "xritdemod_amd", "bin", "xrit_demod_host")
    base = [host_bin, "--input", str(iq), "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null", "--block", "200000",
            "--files-decompress", "--canvas", "--canvas-slots", "4", "--canvas-mib", "1", "--products", "--product-factor", "3"]
    runs = {}
    for name, extra in (("without", []), ("default", ["--jpeg"]), ("q60", ["--jpeg", "60"])):
        r = subprocess.run(base + ["--files", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        runs[name] = ({nm: (tmp_path / name / nm).read_bytes() for nm in os.listdir(tmp_path / name)}, r.stderr)
    plain, err = runs["without"]
    assert not [nm for nm in plain if nm.endswith(".jpg")] and "jpeg:" not in err and len([nm for nm in plain if nm.endswith(".view.pgm")]) == 3
    for name, quality in (("default", 90), ("q60", 60)):
        got, err2 = runs[name]
        jpgs = {nm for nm in got if nm.endswith(".jpg")}
        assert {nm: v for nm, v in got.items() if nm not in jpgs} == plain and len(jpgs) == 6
        assert [ln for ln in err2.splitlines() if not ln.startswith("jpeg:")] == err.splitlines()
        total = 0
        for nm in (x for x in plain if x.endswith(".view.pgm") or x.endswith(".thumb.pgm")):
            magic, dims, maxv, pixels = plain[nm].split(b"\n", 3)
            columns, rows = (int(v) for v in dims.split())
            image = np.frombuffer(pixels, np.uint8).reshape(rows, columns)
            want = js.encode(image, quality=quality, restart=(columns + 7) // 8)[0]
            jpg = got[nm[:-len(".pgm")] + ".jpg"]
            assert jpg == want, nm
            total += len(jpg)
            try:
                from PIL import Image
            except ImportError:
                continue
            back = np.asarray(Image.open(io.BytesIO(jpg)))
            assert back.shape == image.shape and back.dtype == np.uint8
        assert f"jpeg: 6 files of quality {quality}, {total} bytes" in err2
