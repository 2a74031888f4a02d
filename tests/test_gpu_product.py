"""GPU tier: the product stage (xrit_product_*, ImageProduct) against the specification of tests/product_spec.py -- the
histogram, the tone table, the toned image, the thumbnail, the composite and every field of the summary, compared with
np.array_equal.  The shapes are the smallest at which the kernels can still go wrong: one pixel; a pitch with garbage in
the padding; partial blocks on both edges and a block without data; a real width with several waves to a row; the
global-atomic path above 12 bits and the clamp of samples out of range; 1 and 5 bits; bases and pitches that are no
multiple of 16, 4 or 2 bytes; more rows than the grid has waves; images that fall back; every output left out in turn;
two calls back to back without a wait; the product queued behind files, images and canvas on one stream and read in
place; the host-buffer forms; every bad argument; and xrit_demod_host --canvas --products from IQ to .pgm files."""
import os
import subprocess

import numpy as np
import pytest

import canvas_cases as cc
import canvas_spec as cs
import file_spec as fs
import image_spec as isp
import packet_spec as ps
import product_spec as sp

pytestmark = pytest.mark.gpu

OUTPUTS = ("hist", "lut", "tone", "small")
GUARD = 32                                              # bytes behind every output that must stay as they were


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
def pr(xa):
    h = xa.ImageProduct()
    yield h
    h.close()


def image_of(rng, rows, columns, bits, over=False, holes=0.2):
    """Samples of `bits` bits with pixels without data; with `over`, some above 2^bits - 1 (two-byte samples only)."""
    img = rng.integers(0, 1 << bits, (rows, columns)).astype(np.uint8 if bits <= 8 else np.uint16)
    img[rng.random((rows, columns)) < holes] = 0
    if over:
        where = rng.random((rows, columns)) < 0.1
        img[where] = rng.integers(1 << bits, 1 << 16, int(where.sum()))
        img.flat[0] = 1 << bits                         # the first value out of range, and the last
        img.flat[-1] = 65535
    return img


def laid_out(rng, img, pitch, offset):
    """The image's bytes at `offset` of a buffer, `pitch` bytes from row to row, non-zero garbage everywhere else; the
    buffer ends with the last row's last sample."""
    rows, columns = img.shape
    row_bytes = columns * img.itemsize
    buf = rng.integers(1, 256, offset + pitch * (rows - 1) + row_bytes, dtype=np.uint8)
    raw = np.ascontiguousarray(img).view(np.uint8).reshape(rows, row_bytes)
    for r in range(rows):
        buf[offset + r * pitch:offset + r * pitch + row_bytes] = raw[r]
    return buf


def sizes_of(rows, columns, bits, f):
    sr, sc = sp.small_shape(rows, columns, f)
    return dict(hist=4 << bits, lut=1 << bits, tone=rows * columns, small=sr * sc, summary=64)


def prepare(torch, img, bits, tone, p_lo=0, p_hi=10000, f=0, table=None, pitch=None, offset=0, skip=(), seed=0):
    """The image laid out in device memory and the outputs' tensors, filled with 0xA5 -> what launch takes."""
    dev = torch.device("cuda:0")
    rows, columns = img.shape
    pitch = columns * img.itemsize if pitch is None else pitch
    d_img = torch.from_numpy(laid_out(np.random.default_rng(seed), img, pitch, offset)).to(dev)
    assert d_img.data_ptr() % 16 == 0
    d_table = None if table is None else torch.from_numpy(np.ascontiguousarray(table, np.uint8)).to(dev)
    out = {k: torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for k, n in sizes_of(rows, columns, bits, f).items()}
    ptr = lambda k: None if k in skip else out[k].data_ptr()
    out["keep"] = (d_img, d_table)
    torch.cuda.synchronize()                            # the fills are done before anything is queued on another stream
    args = (d_img.data_ptr() + offset, columns, rows, pitch, bits, out["summary"].data_ptr())
    kwargs = dict(tone=tone, p_lo=p_lo, p_hi=p_hi, factor=f, d_table_in_ptr=None if d_table is None else d_table.data_ptr(),
                  d_hist_ptr=ptr("hist"), d_lut_ptr=ptr("lut"), d_tone_ptr=ptr("tone"), d_small_ptr=ptr("small"))
    return args, kwargs, out


def device_call(xa, torch, pr, img, bits, tone, *a, **kw):
    """One process_device on the image laid out in device memory -> the outputs' tensors (0xA5 where nothing was written)."""
    args, kwargs, out = prepare(torch, img, bits, tone, *a, **kw)
    pr.process_device(*args, **kwargs)
    torch.cuda.synchronize()
    return out


def same_summary(xa, got, want):
    for k in sp.SUMMARY_FIELDS:
        assert int(got[k]) == want[k], (k, int(got[k]), want[k])
    assert tuple(got.dtype.names) == sp.SUMMARY_FIELDS


def same(xa, out, want, rows, columns, bits, f, skip=()):
    """Every output equals the specification's; what was left out, and the bytes behind each output, are untouched."""
    n = sizes_of(rows, columns, bits, f)
    got = {k: out[k].cpu().numpy() for k in n}
    for k in n:
        assert (got[k][n[k]:] == 0xA5).all(), k
        if k in skip:
            assert (got[k] == 0xA5).all(), k
    same_summary(xa, got["summary"][:64].view(xa.PRODUCT_SUMMARY_DTYPE)[0], want["summary"])
    if "hist" not in skip:
        assert np.array_equal(got["hist"][:n["hist"]].view(np.uint32), want["hist"])
    if "lut" not in skip:
        assert np.array_equal(got["lut"][:n["lut"]], want["lut"])
    if "tone" not in skip:
        assert np.array_equal(got["tone"][:n["tone"]].reshape(rows, columns), want["tone"])
    if f and "small" not in skip:
        assert np.array_equal(got["small"][:n["small"]].reshape(want["small"].shape), want["small"])


def check(xa, torch, pr, img, bits, tone, p_lo=0, p_hi=10000, f=0, table=None, **layout):
    want = sp.process(img, bits, sp.TONES[tone], p_lo, p_hi, f, table)
    out = device_call(xa, torch, pr, img, bits, tone, p_lo, p_hi, f, table, **layout)
    same(xa, out, want, img.shape[0], img.shape[1], bits, f, layout.get("skip", ()))
    return want


MODES = (("linear", 0, 0), ("equalise", 0, 0), ("stretch", 200, 9800))


def test_one_pixel(xa, torch, pr):
    for bits, v in ((8, 0), (8, 77), (1, 1), (16, 65535), (10, 1023)):
        img = np.array([[v]], np.uint8 if bits <= 8 else np.uint16)
        for tone, lo, hi in MODES:
            want = check(xa, torch, pr, img, bits, tone, lo, hi, f=1)
            assert want["summary"]["fallback"] == (tone != "linear")            # one value or none: nothing to equalise or stretch


def test_padding_is_not_counted(xa, torch, pr):
    """131 x 7 at 8 bits, pitch 136: the five bytes behind every row are garbage, and the rows' heads move through the
    residues of 8 mod 16."""
    img = image_of(np.random.default_rng(1), 7, 131, 8)
    for tone, lo, hi in MODES:
        want = check(xa, torch, pr, img, 8, tone, lo, hi, f=8, pitch=136)
        assert want["summary"]["total"] == 131 * 7 and int(want["hist"].sum()) == 131 * 7 and want["summary"]["fallback"] == 0


@pytest.mark.parametrize("f", [64, 3])
def test_partial_blocks_and_a_block_without_data(xa, torch, pr, f):
    """67 x 65: a block column of 3 and a block row of 1 at f = 64; 23 x 22 blocks with a 1 x 2 corner at f = 3."""
    img = image_of(np.random.default_rng(2), 65, 67, 8, holes=0.05)
    img[:min(f, 65) if f == 3 else 64, :f] = 0              # the first block has no data
    img[9:12] = 0                                           # and rows of a lost segment
    for tone, lo, hi in MODES:
        want = check(xa, torch, pr, img, 8, tone, lo, hi, f=f)
        assert want["small"].shape == ((2, 2) if f == 64 else (22, 23)) and want["small"][0, 0] == 0 and want["small"].any()
    if f == 3:
        assert not want["small"][3].any() and want["small"][2].all() and want["small"][4].all()


def test_a_real_width_with_several_waves_per_row(xa, torch, pr):
    """5424 x 9 at 10 bits, f = 8: rows of 10848 bytes (678 units of 16), three tiles of 2048 columns, a band of one row."""
    img = image_of(np.random.default_rng(3), 9, 5424, 10)
    for tone, lo, hi in MODES:
        want = check(xa, torch, pr, img, 10, tone, lo, hi, f=8)
    assert want["small"].shape == (2, 678) and want["summary"]["lo"] > 0 and want["summary"]["hi"] < 1023


def test_sixteen_bits_takes_the_global_atomic_path(xa, torch, pr):
    img = image_of(np.random.default_rng(4), 5, 4099, 16)
    img[0, :3] = (65535, 1, 65535)
    for tone, lo, hi in MODES:
        want = check(xa, torch, pr, img, 16, tone, lo, hi, f=8)
    assert want["summary"]["max_nz"] == 65535 and want["summary"]["out_of_range"] == 0


def test_thirteen_bits_with_samples_out_of_range(xa, torch, pr):
    img = image_of(np.random.default_rng(5), 5, 4099, 13, over=True)
    table = np.random.default_rng(6).integers(0, 256, 1 << 13, dtype=np.uint8)
    for tone, lo, hi in MODES + (("table", 0, 0),):
        want = check(xa, torch, pr, img, 13, tone, lo, hi, f=8, table=table if tone == "table" else None)
        assert want["summary"]["out_of_range"] > 1500 and int(want["hist"][8191]) >= want["summary"]["out_of_range"]
    # twelve bits: the same clamp in front of the bins and the table in LDS
    img = image_of(np.random.default_rng(7), 3, 1000, 12, over=True)
    want = check(xa, torch, pr, img, 12, "equalise", f=4)
    assert want["summary"]["out_of_range"] > 200 and want["summary"]["max_nz"] == 4095


@pytest.mark.parametrize("bits", [1, 5])
def test_few_bits(xa, torch, pr, bits):
    img = image_of(np.random.default_rng(8 + bits), 6, 300, bits)
    img[0, :2] = (1 << bits) - 1, 255                       # bits < 8 in a byte: out of range there too
    table = np.random.default_rng(9).integers(0, 256, 1 << bits, dtype=np.uint8)
    for tone, lo, hi in MODES + (("table", 0, 0),):
        want = check(xa, torch, pr, img, bits, tone, lo, hi, f=5, table=table if tone == "table" else None)
        assert want["summary"]["out_of_range"] >= 1
    assert want["summary"]["fallback"] == 0 or bits == 1


def test_bases_and_pitches_off_every_boundary(xa, torch, pr):
    """Width 1 from a base one byte off with an odd pitch: every row's head has another length.  Width 2 from a base two
    bytes off with a pitch of 2 mod 16.  Columns below, at and above what one 16-byte unit holds."""
    rng = np.random.default_rng(10)
    for columns in (1, 15, 16, 17, 100):
        img = image_of(rng, 19, columns, 8)
        check(xa, torch, pr, img, 8, "equalise", f=4, pitch=columns + 7 + (columns % 2), offset=1)
        wide = image_of(rng, 19, columns, 10)
        check(xa, torch, pr, wide, 10, "equalise", f=4, pitch=2 * columns + 18 - (2 * columns) % 16, offset=2)
    img = image_of(rng, 5, 333, 8)
    for offset in (3, 8, 13):
        check(xa, torch, pr, img, 8, "stretch", 100, 9900, f=2, pitch=333, offset=offset)


def test_more_rows_than_the_grid_has_waves(xa, torch, pr):
    """3000 x 5; 5000 rows, past the 4096 waves of the histogram's grid; 9000 bands of one row, past the tone kernel's 8192
    workgroups."""
    for rows, bits, f in ((3000, 8, 7), (5000, 10, 7), (9000, 8, 1)):
        img = image_of(np.random.default_rng(11), rows, 5, bits)
        want = check(xa, torch, pr, img, bits, "equalise", f=f)
        assert want["small"].shape == ((rows + f - 1) // f, (5 + f - 1) // f)


def test_fallbacks_on_the_device(xa, torch, pr):
    for bits in (8, 10, 16):
        dtype = np.uint8 if bits <= 8 else np.uint16
        zero, one = np.zeros((9, 40), dtype), np.full((9, 40), 37, dtype)
        one[2] = 0
        for img in (zero, one):
            for tone, lo, hi in MODES:
                want = check(xa, torch, pr, img, bits, tone, lo, hi, f=4)
                assert want["summary"]["fallback"] == (tone != "linear") and want["summary"]["lo"] == want["summary"]["hi"] == 0
        assert not sp.process(zero, bits, sp.EQUALISE, factor=4)["small"].any()


def test_table_with_a_random_table(xa, torch, pr):
    rng = np.random.default_rng(12)
    for bits in (8, 10, 16):
        img = image_of(rng, 7, 131, bits)
        table = rng.integers(0, 256, 1 << bits, dtype=np.uint8)
        want = check(xa, torch, pr, img, bits, "table", f=8, table=table)
        assert np.array_equal(want["lut"], table)


@pytest.mark.parametrize("tone", ["linear", "table", "equalise", "stretch"])
def test_every_output_left_out_in_turn(xa, torch, pr, tone):
    rng = np.random.default_rng(13)
    img = image_of(rng, 11, 70, 10)
    table = rng.integers(0, 256, 1024, dtype=np.uint8) if tone == "table" else None
    for skip in [(k,) for k in OUTPUTS] + [OUTPUTS, ("tone", "small")]:
        check(xa, torch, pr, img, 10, tone, 500, 9000, f=4, table=table, skip=skip)


def test_two_calls_back_to_back_without_a_wait(xa, torch, pr):
    """10 bits then 8 bits on one handle and one stream, the scratch histogram and table in use (none passed): stale bins
    or a stale table of the first call would show in the second's toned image and summary."""
    rng = np.random.default_rng(14)
    first, second = image_of(rng, 40, 500, 10), image_of(rng, 33, 260, 8)
    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    calls = [prepare(torch, img, bits, "equalise", f=4, skip=("hist", "lut"), seed=i) for i, (img, bits) in enumerate(((first, 10), (second, 8), (first, 10)))]
    for args, kwargs, _ in calls:
        pr.process_device(*args, stream=s.cuda_stream, **kwargs)
    s.synchronize()                                     # the only one behind the three calls
    outs = [c[2] for c in calls]
    for out, (img, bits) in zip(outs, ((first, 10), (second, 8), (first, 10))):
        same(xa, out, sp.process(img, bits, sp.EQUALISE, factor=4), img.shape[0], img.shape[1], bits, 4, skip=("hist", "lut"))


def test_composite(xa, torch, pr):
    """131 x 7 with unequal pitches (rows off every 4-byte boundary, the output too), and a width below one group."""
    rng = np.random.default_rng(15)
    dev = torch.device("cuda:0")
    table = rng.integers(0, 256, 256 * 256 * 3, dtype=np.uint8)
    d_table = torch.from_numpy(table).to(dev)
    for columns, rows, pitch_a, pitch_b, off in ((131, 7, 133, 140, 0), (3, 5, 3, 9, 1), (128, 4, 128, 128, 0)):
        a, b = rng.integers(0, 256, (2, rows, columns), dtype=np.uint8)
        d_a, d_b = (torch.from_numpy(laid_out(rng, x, p, off)).to(dev) for x, p in ((a, pitch_a), (b, pitch_b)))
        d_rgb = torch.full((rows * columns * 3 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        pr.composite_device(d_a.data_ptr() + off, pitch_a, d_b.data_ptr() + off, pitch_b, columns, rows, d_table.data_ptr(), d_rgb.data_ptr())
        torch.cuda.synchronize()
        got = d_rgb.cpu().numpy()
        want = sp.composite(a, b, table)
        assert np.array_equal(got[:-GUARD].reshape(rows, columns, 3), want) and (got[-GUARD:] == 0xA5).all()
        assert np.array_equal(pr.composite(a, b, table), want)
        assert np.array_equal(pr.composite(np.pad(a, ((0, 0), (0, 5)))[:, :columns], b, table), want)        # a pitch of the host's


def test_host_buffer_forms(xa, torch, pr):
    rng = np.random.default_rng(16)
    for bits, tone, f in ((8, "equalise", 8), (10, "stretch", 3), (16, "linear", 0), (5, "table", 2)):
        img = image_of(rng, 21, 150, bits)
        table = rng.integers(0, 256, 1 << bits, dtype=np.uint8) if tone == "table" else None
        want = sp.process(img, bits, sp.TONES[tone], 300, 9700, f, table)
        padded = np.pad(img, ((0, 0), (0, 3)), constant_values=9)[:, :150]      # rows 153 samples apart
        for source in (img, padded):
            got = pr.process(source, bits, tone, 300, 9700, f, table)
            same_summary(xa, got["summary"], want["summary"])
            assert all(np.array_equal(got[k], want[k]) for k in ("hist", "lut", "tone")) and ("small" in got) == bool(f)
            assert not f or np.array_equal(got["small"], want["small"])
        got = pr.process(img, bits, tone, 300, 9700, f, table, outputs=("small",))
        assert set(got) == ({"summary", "small"} if f else {"summary"})
        # the image where it lies in device memory, the outputs to the host
        d_img = torch.from_numpy(np.ascontiguousarray(img).view(np.uint8).reshape(-1)).to("cuda:0")
        got = pr.process_resident(d_img.data_ptr(), 150, 21, 150 * img.itemsize, bits, tone, 300, 9700, f, table)
        same_summary(xa, got["summary"], want["summary"])
        assert all(np.array_equal(got[k], want[k]) for k in ("hist", "lut", "tone")) and (not f or np.array_equal(got["small"], want["small"]))
    pr.reset()


def test_bad_arguments_leave_the_outputs_untouched(xa, torch, pr):
    dev = torch.device("cuda:0")
    d_img = torch.zeros(4096, dtype=torch.uint8, device=dev)
    out = {k: torch.full((n,), 0xA5, dtype=torch.uint8, device=dev) for k, n in dict(hist=4 << 16, lut=1 << 16, tone=4096, small=4096, summary=64).items()}
    good = dict(columns=30, rows=20, pitch=64, bits=10, tone="stretch", p_lo=100, p_hi=9000, factor=4, table=True, img=0, hist=0, summary=0)
    bad = [dict(bits=0), dict(bits=17), dict(columns=0), dict(rows=0), dict(columns=1 << 16, rows=(1 << 15) + 1, pitch=1 << 17), dict(pitch=59),
           dict(pitch=63), dict(img=1), dict(bits=8, pitch=29), dict(tone=4), dict(tone="table", table=False), dict(p_lo=9000), dict(p_lo=9001),
           dict(p_hi=10001), dict(factor=65), dict(hist=2), dict(summary=4), dict(img=None), dict(summary=None)]
    for change in [{}] + bad:
        a = dict(good, **change)
        call = lambda: pr.process_device(
            0 if a["img"] is None else d_img.data_ptr() + a["img"], a["columns"], a["rows"], a["pitch"], a["bits"],
            None if a["summary"] is None else out["summary"].data_ptr() + a["summary"], tone=a["tone"], p_lo=a["p_lo"], p_hi=a["p_hi"],
            factor=a["factor"], d_table_in_ptr=out["lut"].data_ptr() if a["table"] else None, d_hist_ptr=out["hist"].data_ptr() + a["hist"],
            d_lut_ptr=out["lut"].data_ptr(), d_tone_ptr=out["tone"].data_ptr(), d_small_ptr=out["small"].data_ptr())
        if not change:
            continue                                    # (the good call is made last)
        with pytest.raises(xa.XritError) as ei:
            call()
        assert ei.value.code == -1, change
    tab = out["lut"].data_ptr()
    for args in ((None, 30, out["tone"].data_ptr(), 30, 30, 20, tab, out["small"].data_ptr()), (d_img.data_ptr(), 29, d_img.data_ptr(), 30, 30, 20, tab, out["small"].data_ptr()),
                 (d_img.data_ptr(), 30, d_img.data_ptr(), 30, 0, 20, tab, out["small"].data_ptr()), (d_img.data_ptr(), 30, d_img.data_ptr(), 30, 30, 20, None, out["small"].data_ptr()),
                 (d_img.data_ptr(), 30, d_img.data_ptr(), 30, 30, 20, tab, None), (d_img.data_ptr(), 1 << 16, d_img.data_ptr(), 1 << 16, 1 << 16, (1 << 15) + 1, tab, out["small"].data_ptr())):
        with pytest.raises(xa.XritError) as ei:
            pr.composite_device(*args)
        assert ei.value.code == -1, args
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 0xA5).all() for t in out.values())
    with pytest.raises(xa.XritError) as ei:
        pr.process(np.zeros((4, 4), np.uint8), 8, "stretch", 5, 5)
    assert ei.value.code == -1
    # the call that is good, from the same arguments
    pr.process_device(d_img.data_ptr(), 30, 20, 64, 10, out["summary"].data_ptr(), tone="stretch", p_lo=100, p_hi=9000, factor=4,
                      d_tone_ptr=out["tone"].data_ptr())
    torch.cuda.synchronize()
    assert int(out["summary"].cpu().numpy().view(xa.PRODUCT_SUMMARY_DTYPE)[0]["zeros"]) == 600 and not out["tone"].cpu().numpy()[:600].any()


def test_queued_behind_files_images_and_canvas_on_one_stream(xa, torch, pr):
    """canvas_cases.mixed_stream through packets, files, images and canvas on one stream, and behind them, with no wait in
    between, a product call per canvas on the slot's pixels where they lie (xrit_canvas_pixels_device).  The geometry the
    calls need on the host is the slot table of the same stream through the host-buffer forms; the products must be the
    specification's of the images the stream was built from, which are what the canvas specification builds."""
    rng = np.random.default_rng(68)
    stream, images = cc.mixed_stream(69)
    by_vc = {}
    for v, p, *_ in stream:
        by_vc.setdefault(v, []).append(p)
    dummies = lambda count: [fs.space_packet(99, i, 3, rng.integers(0, 256, 800, dtype=np.uint8).tobytes()) for i in range(count)]
    rows = {v: ps.rows_of(ps.build_stream(v, dummies(1) + pk + dummies(2), rng, fill=0.0, idle=0.0)) for v, pk in by_vc.items()}
    vcdu, off = ps.group(rows)
    h_pa, h_fa, h_im, h_cv = xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder(), xa.ImageCanvas(6, cc.SLOT_BYTES)
    pdata, pdesc, pko = h_pa.process(vcdu, off)[:3]
    files_out = h_fa.process(pdata, pdesc, pko)
    slots = h_cv.process(files_out, h_im.process(*files_out))[1]
    used = [i for i in range(6) if slots[i]["in_use"]]
    assert len(used) == 5 and all(int(slots[i]["complete"]) == 1 for i in used) and {int(slots[i]["bits"]) for i in used} == {8, 10, 12}
    dev = torch.device("cuda:0")
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    pa, fa, im, cv = xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder(), xa.ImageCanvas(6, cc.SLOT_BYTES)
    n = int(off[64])
    cap = 2 * n
    mb, mp = xa.packets_max_bytes(cap), 16 * cap + 64
    b = {k: z(v) for k, v in dict(pbytes=mb, desc=mp * 32, pko=65 * 4, psum=72, fbytes=mb, pieces=mp * 32, frecs=2 * mp * 80, fsum=104, out=mp * 256,
                                  lines=mp * 32, ifiles=2 * mp * 48, isum=80, cfiles=2 * mp * 32, slots=6 * 136, csum=168).items()}
    b["vcdu"] = torch.cat([torch.from_numpy(vcdu.reshape(-1).copy()).to(dev), z((cap - n) * 892)])
    b["off"] = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
    f = 4
    outs = {}
    for i in used:
        r, c, bits = int(slots[i]["max_row"]), int(slots[i]["max_column"]), int(slots[i]["bits"])
        outs[i] = {k: torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for k, nb in sizes_of(r, c, bits, f).items()}
    q = {k: t.data_ptr() for k, t in b.items()}
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    pa.process_device(q["vcdu"], q["off"], cap, q["pbytes"], mb, q["desc"], mp, q["pko"], q["psum"], stream=s.cuda_stream)
    fa.process_device(q["pbytes"], mb, q["desc"], q["pko"], mp, q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"], stream=s.cuda_stream)
    im.process_device(q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"], q["out"], mp * 256, q["lines"], mp, q["ifiles"], q["isum"],
                      stream=s.cuda_stream)
    cv.process_device(q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"], q["out"], mp * 256, q["lines"], mp, q["ifiles"], q["isum"],
                      q["cfiles"], q["slots"], q["csum"], stream=s.cuda_stream)
    for i in used:
        o = outs[i]
        pr.process_device(cv.pixels_device(i), int(slots[i]["max_column"]), int(slots[i]["max_row"]), int(slots[i]["pitch"]), int(slots[i]["bits"]),
                          o["summary"].data_ptr(), tone="equalise", factor=f, d_hist_ptr=o["hist"].data_ptr(), d_lut_ptr=o["lut"].data_ptr(),
                          d_tone_ptr=o["tone"].data_ptr(), d_small_ptr=o["small"].data_ptr(), stream=s.cuda_stream)
    s.synchronize()                                             # the only one
    assert b["slots"].cpu().numpy().tobytes() == slots.tobytes()
    for i in used:
        _, bits, img = images[int(slots[i]["image_id"])]
        assert np.array_equal(cv.image(i)[1], img)
        same(xa, outs[i], sp.process(img, bits, sp.EQUALISE, factor=f), img.shape[0], img.shape[1], bits, f)
    assert cv.pixels_device(1) - cv.pixels_device(0) == cc.SLOT_BYTES
    with pytest.raises(xa.XritError) as ei:
        cv.pixels_device(6)
    assert ei.value.code == -1
    for x in (pa, fa, im, cv, h_pa, h_fa, h_im, h_cv):
        x.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_host_program_products(xa, tmp_path):
    """The capture of the canvas stage's host program test: with --products every canvas that is written has its .view.pgm
    and .thumb.pgm, the specification's of that canvas; everything else the run writes is what it writes without the flag,
    and that is what the canvas test expects."""
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
            "--files-decompress", "--canvas", "--canvas-slots", "4", "--canvas-mib", "1"]
    runs = {}
    for name, extra in (("plain", []), ("products", ["--products"]), ("stretch", ["--products", "--product-tone", "stretch:100:9900", "--product-factor", "3"])):
        r = subprocess.run(base + ["--files", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        runs[name] = ({nm: (tmp_path / name / nm).read_bytes() for nm in os.listdir(tmp_path / name)}, r.stderr)
    plain, err = runs["plain"]
    assert plain["GOES_test_full_disk.lrit.pgm"] == b"P5\n64 12\n255\n" + a.astype(np.uint8).tobytes() and "products:" not in err
    assert len([nm for nm in plain if nm.endswith(".pgm")]) == 3 and not [nm for nm in plain if ".view." in nm or ".thumb." in nm]
    partial = np.concatenate([c.astype(np.uint8), np.zeros((4, 16), np.uint8)])
    for name, mode, lo, hi, f in (("products", sp.EQUALISE, 0, 10000, 8), ("stretch", sp.STRETCH, 100, 9900, 3)):
        got, err = runs[name]
        extra = {nm for nm in got if nm.endswith(".view.pgm") or nm.endswith(".thumb.pgm")}
        assert {nm: v for nm, v in got.items() if nm not in extra} == plain and len(extra) == 6
        for nm in (x for x in plain if x.endswith(".pgm")):
            img, bits = ((a, 8) if nm.startswith("GOES") else (b, 10) if "_img22_" in nm else (partial, 8))
            want = sp.process(img.astype(np.uint8 if bits <= 8 else np.uint16), bits, mode, lo, hi, f)
            stem = nm[:-len(".pgm")]
            head = lambda m: b"P5\n%d %d\n255\n" % (m.shape[1], m.shape[0])
            assert got[stem + ".view.pgm"] == head(want["tone"]) + want["tone"].tobytes(), nm
            assert got[stem + ".thumb.pgm"] == head(want["small"]) + want["small"].tobytes(), nm
        assert f"products: 3 canvases toned and reduced {f} times" in err
