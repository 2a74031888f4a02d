"""GPU tier: the projection stage (xrit_geo_*, ImageProjector) against the specification of tests/geo_spec.py -- the map,
the output of both sampling modes and every field of the summary, compared with np.array_equal; every test feeds the
specification the tables read back from the handle.  The shapes are the smallest at which the kernels can still go wrong:
the fixed case of the CPU tier at 8 and 10 bits from bases and pitches off every boundary into an output with guard bytes;
one pixel; a row that several waves share with a partial last lane group; a zoom in which many outputs fall on one source
pixel and a coarse grid; holes and missing rows; a grid off the disc; tables that hold NaN, infinities and 1e300; two calls
back to back without a wait; the stage queued behind files, images and canvas on one stream with the product stage behind
it; the host-buffer forms; every bad argument; one real size for the index arithmetic; and xrit_demod_host --canvas
--project from IQ to .geo.pgm files.  Every call is made as map + resample and fused, and the two must agree byte for
byte."""
import os
import subprocess

import numpy as np
import pytest

import canvas_cases as cc
import canvas_spec as cs
import file_spec as fs
import geo_spec as gs
import image_spec as isp
import packet_spec as ps
import product_spec as sp

pytestmark = pytest.mark.gpu

GUARD = 32                                              # bytes behind every output that must stay as they were
FILL = 0xA5


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
def gp(xa):
    h = xa.ImageProjector()
    yield h
    h.close()


@pytest.fixture(scope="module")
def fixed(gp):
    """The fixed case's grid in the handle -> the tables read back, and the map the specification makes of them: computed
    once, shared, never written to."""
    gp.set_grid(*gs.FIXED_GRID, gs.FIXED_NAV["sub_lon"])
    tables = gp.tables()
    for t in tables:
        t.setflags(write=False)
    return tables


def image_of(rng, rows, columns, bits, holes=0.0):
    img = rng.integers(1, 1 << bits, (rows, columns)).astype(np.uint8 if bits <= 8 else np.uint16)
    if holes:
        img[rng.random((rows, columns)) < holes] = 0
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


def same_summary(xa, got, want):
    assert tuple(got.dtype.names) == gs.SUMMARY_FIELDS
    for k in gs.SUMMARY_FIELDS:
        assert int(got[k]) == want[k], (k, int(got[k]), want[k])


class Call:
    """One image laid out in device memory and the outputs of map, resample and fused for the grid in the handle, filled
    with 0xA5 and with GUARD bytes behind each."""

    def __init__(self, torch, gp, img, bits, pitch=None, offset=0, out_pad=0, out_offset=0, seed=0):
        dev = torch.device("cuda:0")
        self.img, self.bits, self.rows, self.columns = img, bits, gp.rows, gp.columns
        self.width = img.itemsize
        self.pitch = img.shape[1] * self.width if pitch is None else pitch
        self.offset, self.out_offset = offset, out_offset
        self.out_pitch = self.columns * self.width + out_pad
        self.d_img = torch.from_numpy(laid_out(np.random.default_rng(seed), img, self.pitch, offset)).to(dev)
        assert self.d_img.data_ptr() % 16 == 0
        self.out_bytes = self.out_pitch * (self.rows - 1) + self.columns * self.width
        full = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device=dev)
        self.d_map = full(self.rows * self.columns * 8 + GUARD)
        self.d_out = {k: full(out_offset + self.out_bytes + GUARD) for k in ("resample", "fused")}
        self.d_summary = {k: full(56 + GUARD) for k in ("resample", "fused")}
        torch.cuda.synchronize()                        # the fills are done before anything is queued on another stream

    def source(self):
        return (self.d_img.data_ptr() + self.offset, self.img.shape[1], self.img.shape[0], self.pitch, self.bits)

    def launch(self, gp, nav, mode, stream=None):
        gp.map_device(nav, self.d_map.data_ptr(), stream=stream)
        gp.resample_device(*self.source(), self.d_map.data_ptr(), mode, self.d_out["resample"].data_ptr() + self.out_offset, self.out_pitch,
                           self.d_summary["resample"].data_ptr(), stream=stream)
        gp.project_device(nav, *self.source(), mode, self.d_out["fused"].data_ptr() + self.out_offset, self.out_pitch,
                          self.d_summary["fused"].data_ptr(), stream=stream)

    def verify(self, xa, tables, nav, mode):
        """-> (out, summary) of the specification, which the device's map, resample and fused call must equal."""
        mode = gs.MODES[mode] if isinstance(mode, str) else mode
        qx, qy = gs.map_points(*tables, nav)
        want, summary = gs.resample(self.img, qx, qy, mode)
        got_map = self.d_map.cpu().numpy()
        assert (got_map[-GUARD:] == FILL).all()
        points = got_map[:-GUARD].view(xa.GEO_POINT_DTYPE).reshape(self.rows, self.columns)
        assert np.array_equal(points["qx"], qx) and np.array_equal(points["qy"], qy)
        row_bytes = self.columns * self.width
        outs = {}
        for k in ("resample", "fused"):
            raw = self.d_out[k].cpu().numpy()
            assert (raw[:self.out_offset] == FILL).all() and (raw[self.out_offset + self.out_bytes:] == FILL).all(), k
            body = np.concatenate([raw[self.out_offset:self.out_offset + self.out_bytes], np.full(self.out_pitch - row_bytes, FILL, np.uint8)])
            body = body.reshape(self.rows, self.out_pitch)
            assert (body[:, row_bytes:] == FILL).all(), k                      # the bytes of a row behind the samples stay
            got = np.ascontiguousarray(body[:, :row_bytes]).view(self.img.dtype)
            assert np.array_equal(got, want), (k, int((got != want).sum()))
            s = self.d_summary[k].cpu().numpy()
            assert (s[56:] == FILL).all()
            same_summary(xa, s[:56].view(xa.GEO_SUMMARY_DTYPE)[0], summary)
            outs[k] = raw
        assert np.array_equal(outs["resample"], outs["fused"])
        return want, summary


def check(xa, torch, gp, tables, img, bits, nav, mode, **layout):
    call = Call(torch, gp, img, bits, **layout)
    call.launch(gp, nav, mode)
    torch.cuda.synchronize()
    return call.verify(xa, tables, nav, mode)


MSG_NAV = dict(gs.FIXED_NAV, cfac=-gs.FIXED_NAV["cfac"], lfac=-gs.FIXED_NAV["lfac"])


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("bits", [8, 10])
def test_fixed_case(xa, torch, gp, fixed, bits, mode):
    """96 x 80 onto 171 x 163 (a row is 171 bytes or 342: the rows' heads move through every residue of 4 and 8): tight
    and aligned; from a base and a pitch that are no multiple of 16, 4 or (one-byte samples) 2 into an output whose rows are
    wider than the grid, from a base off the dword; and with both factors negative."""
    gp.set_tables(*fixed)
    img = image_of(np.random.default_rng(bits), 80, 96, bits)
    want, summary = check(xa, torch, gp, fixed, img, bits, gs.FIXED_NAV, mode)
    assert summary["written"] == 24069 and summary["off_disc"] == 171 * 163 - 24069 and summary["outside"] == summary["no_data"] == 0
    w = img.itemsize
    odd = dict(pitch=96 + 7, offset=1, out_pad=5, out_offset=1) if w == 1 else dict(pitch=2 * 96 + 6, offset=2, out_pad=6, out_offset=2)
    assert check(xa, torch, gp, fixed, img, bits, gs.FIXED_NAV, mode, seed=1, **odd)[1] == summary
    flipped = check(xa, torch, gp, fixed, img, bits, MSG_NAV, mode, out_pad=4 * w)[0]
    assert not np.array_equal(flipped, want) and (flipped != 0).sum() == 24069


def test_one_pixel_and_a_row_shared_by_several_waves(xa, torch, gp):
    nav = gs.FIXED_NAV
    img = image_of(np.random.default_rng(3), 80, 96, 8)
    gp.set_grid(gs.EQUIRECT, 1, 1, nav["sub_lon"], 0.0, 1.0, 1.0, nav["sub_lon"])
    for mode in ("nearest", "bilinear"):
        want, _ = check(xa, torch, gp, gp.tables(), img, 8, nav, mode)
        assert want.tolist() == [[int(img[40, 48])]]                            # (coff - origin, loff - origin)
    # 1100 columns: five waves to a row, the last with 76 columns: 19 lanes; 1101 and 1102: a lane group of one and of two
    for columns in (1100, 1101, 1102):
        gp.set_grid(gs.EQUIRECT, columns, 9, nav["sub_lon"] - 82.0, 10.0, 164.0 / columns, 2.5, nav["sub_lon"])
        tables = gp.tables()
        for bits, mode in ((8, "bilinear"), (10, "nearest"), (10, "bilinear")):
            wide = img if bits == 8 else image_of(np.random.default_rng(4), 80, 96, 10)
            _, summary = check(xa, torch, gp, tables, wide, bits, nav, mode, out_offset=0 if columns % 2 else 2 * wide.itemsize)
            assert summary["total"] == 9 * columns and summary["written"] > 8 * columns and summary["off_disc"] > 0


def test_a_zoom_and_a_coarse_grid(xa, torch, gp):
    nav = gs.FIXED_NAV
    img = image_of(np.random.default_rng(5), 80, 96, 10, holes=0.1)
    # 0.01 degrees: 300 x 200 outputs on about 4 x 3 source pixels, east and south of the middle
    gp.set_grid(gs.EQUIRECT, 300, 200, nav["sub_lon"] + 2.0, -3.0, 0.01, 0.01, nav["sub_lon"])
    tables = gp.tables()
    qx, qy = gs.map_points(*tables, nav)
    assert int(qx.max() - qx.min()) < 6 * 256 and int(qy.max() - qy.min()) < 4 * 256
    for mode in ("nearest", "bilinear"):
        want, _ = check(xa, torch, gp, tables, img, 10, nav, mode)
        assert len(np.unique(want)) > (3 if mode == "nearest" else 50)
    # 2 degrees: neighbouring outputs ten source pixels apart
    gp.set_grid(gs.EQUIRECT, 90, 85, nav["sub_lon"] - 90.0, 85.0, 2.0, 2.0, nav["sub_lon"])
    for mode in ("nearest", "bilinear"):
        check(xa, torch, gp, gp.tables(), img, 10, nav, mode)
    # Mercator rows
    gp.set_grid(gs.MERCATOR, 130, 77, nav["sub_lon"] - 65.0, 1.2, 1.0, 0.03, nav["sub_lon"])
    _, summary = check(xa, torch, gp, gp.tables(), img, 10, nav, "bilinear")
    assert summary["written"] > 8000


def test_holes_missing_rows_and_an_image_smaller_than_the_disc(xa, torch, gp, fixed):
    """20 % holes, a band of zero rows, and the navigation of the fixed case on an image of 70 x 50: the disc goes on
    outside the image to the east and south.  Every class has members, and every field is checked."""
    gp.set_tables(*fixed)
    for bits in (8, 10):
        img = image_of(np.random.default_rng(6), 50, 70, bits, holes=0.2)
        img[20:27] = 0
        for mode in ("nearest", "bilinear"):
            _, summary = check(xa, torch, gp, fixed, img, bits, gs.FIXED_NAV, mode)
            assert min(summary[k] for k in ("off_disc", "outside", "no_data", "written")) > 300, summary
            assert summary["off_disc"] + summary["outside"] + summary["no_data"] + summary["written"] == summary["total"] == 171 * 163
            assert (summary["columns"], summary["rows"], summary["width"], summary["mode"]) == (171, 163, img.itemsize, gs.MODES[mode])


def test_a_grid_off_the_disc_writes_zeros_and_only_counts(xa, torch, gp):
    nav = gs.FIXED_NAV
    gp.set_grid(gs.EQUIRECT, 40, 30, nav["sub_lon"] + 100.0, 60.0, 2.0, 2.0, nav["sub_lon"])
    img = image_of(np.random.default_rng(7), 80, 96, 8)
    want, summary = check(xa, torch, gp, gp.tables(), img, 8, nav, "bilinear", out_pad=3)
    assert not want.any() and summary["off_disc"] == summary["total"] == 1200


def test_tables_that_hold_anything(xa, torch, gp, fixed):
    """The caller's tables with NaN, infinities and 1e300 in rows and columns: zeros there, the neighbours right, and
    nothing read outside the image (the rule clamps every tap into it; csrc/geo_host_check.cpp holds that on the host)."""
    A, B, Cc, S = (t.copy() for t in fixed)
    bad = [np.nan, np.inf, -np.inf, 1e300, -1e300]
    A[[70, 75, 80, 85, 90]] = bad
    B[[72, 77, 82, 87, 92]] = bad
    Cc[[60, 70, 80, 90, 100]] = bad
    S[[62, 72, 82, 92, 102]] = bad
    S[110], Cc[110] = 1e300, 1e-300
    gp.set_tables(A, B, Cc, S)
    tables = gp.tables()
    assert all(np.array_equal(t, w, equal_nan=True) for t, w in zip(tables, (A, B, Cc, S)))
    img = image_of(np.random.default_rng(8), 80, 96, 10)
    for mode in ("nearest", "bilinear"):
        want, _ = check(xa, torch, gp, tables, img, 10, gs.FIXED_NAV, mode)
        assert not want[[70, 75, 80, 85, 90, 72, 77, 82, 87, 92]].any() and not want[:, [60, 70, 80, 90, 100, 62, 72, 82, 92, 102, 110]].any()
        assert want[81, 61] and want[81, 63] and want[71, 85] and want[73, 85]
    gp.set_tables(*fixed)
    clean, _ = check(xa, torch, gp, fixed, img, 10, gs.FIXED_NAV, "bilinear")
    keep_r, keep_c = np.setdiff1d(np.arange(163), [70, 75, 80, 85, 90, 72, 77, 82, 87, 92]), np.setdiff1d(np.arange(171), [60, 70, 80, 90, 100, 62, 72, 82, 92, 102, 110])
    assert np.array_equal(want[np.ix_(keep_r, keep_c)], clean[np.ix_(keep_r, keep_c)])


def test_a_map_that_holds_anything_reads_nothing_outside(xa, torch, gp, fixed):
    """xrit_geo_resample_device on entries of the caller's: the extremes of int32 and random ones."""
    gp.set_tables(*fixed)
    rng = np.random.default_rng(9)
    img = image_of(rng, 80, 96, 8)
    call = Call(torch, gp, img, 8)
    n = 163 * 171
    q = rng.integers(-(1 << 31), 1 << 31, (n, 2)).astype(np.int32)
    q[::3] = rng.integers(-600, 97 * 256, (len(q[::3]), 2))
    q[:8] = [(gs.OFF, 0), (0, gs.OFF), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 0), (0, 2 ** 31 - 1), (-2 ** 31 + 1, 5), (95 * 256 + 255, 79 * 256 + 255), (-1, -1)]
    d_map = torch.from_numpy(q.reshape(-1).view(np.uint8).copy()).to("cuda:0")
    for mode in (gs.NEAREST, gs.BILINEAR):
        gp.resample_device(*call.source(), d_map.data_ptr(), mode, call.d_out["resample"].data_ptr(), call.out_pitch, call.d_summary["resample"].data_ptr())
        torch.cuda.synchronize()
        want, summary = gs.resample(img, q[:, 0].reshape(163, 171), q[:, 1].reshape(163, 171), mode)
        assert np.array_equal(call.d_out["resample"].cpu().numpy()[:n].reshape(163, 171), want)
        same_summary(xa, call.d_summary["resample"].cpu().numpy()[:56].view(xa.GEO_SUMMARY_DTYPE)[0], summary)
        assert summary["off_disc"] >= 2 and summary["outside"] > n // 2 and summary["written"] > n // 5


def test_two_calls_back_to_back_without_a_wait(xa, torch, gp, fixed):
    """10 bits then 8 bits then 10 bits on one handle and one stream: a summary or a map left over from the call in front
    would show."""
    gp.set_tables(*fixed)
    rng = np.random.default_rng(10)
    first, second = image_of(rng, 80, 96, 10, holes=0.1), image_of(rng, 50, 70, 8, holes=0.3)
    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    plan = ((first, 10, gs.FIXED_NAV, "bilinear"), (second, 8, MSG_NAV, "nearest"), (first, 10, MSG_NAV, "bilinear"))
    calls = [Call(torch, gp, img, bits, seed=i) for i, (img, bits, _, _) in enumerate(plan)]
    for call, (_, _, nav, mode) in zip(calls, plan):
        call.launch(gp, nav, mode, stream=s.cuda_stream)
    s.synchronize()                                     # the only one behind the nine calls
    for call, (_, _, nav, mode) in zip(calls, plan):
        call.verify(xa, fixed, nav, mode)


def test_host_buffer_forms(xa, torch, gp, fixed):
    gp.set_tables(*fixed)
    rng = np.random.default_rng(11)
    qx, qy = gs.map_points(*fixed, gs.FIXED_NAV)
    for bits, mode in ((8, "bilinear"), (10, "bilinear"), (10, "nearest"), (16, "bilinear")):
        img = image_of(rng, 80, 96, bits, holes=0.2)
        want, summary = gs.resample(img, qx, qy, gs.MODES[mode])
        padded = np.pad(img, ((0, 0), (0, 3)), constant_values=9)[:, :96]       # rows 99 samples apart
        for source in (img, padded):
            got, s = gp.project(gs.FIXED_NAV, source, bits, mode)
            assert got.dtype == img.dtype and np.array_equal(got, want)
            same_summary(xa, s, summary)
        # the image where it lies in device memory, the output to the host
        d_img = torch.from_numpy(np.ascontiguousarray(img).view(np.uint8).reshape(-1)).to("cuda:0")
        got, s = gp.project_resident(gs.FIXED_NAV, d_img.data_ptr(), 96, 80, 96 * img.itemsize, bits, mode)
        assert np.array_equal(got, want)
        same_summary(xa, s, summary)
    # an output of the host's with rows wider than the grid: the bytes in between stay
    import ctypes as C
    img = image_of(rng, 80, 96, 8)
    out = np.full((163, 180), FILL, np.uint8)
    s = np.zeros(1, xa.GEO_SUMMARY_DTYPE)
    image = np.zeros(1, xa.PRODUCT_IMAGE_DTYPE)
    image[0] = (img.ctypes.data, 96, 80, 96, 8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert xa.lib().xrit_geo_project(gp._h, p(xa.geo_nav(357469, 297890, 49, 41, 1, -75.2)), p(image), 1, p(out), 180, p(s)) == 0
    assert np.array_equal(out[:, :171], gs.resample(img, qx, qy, gs.BILINEAR)[0]) and (out[:, 171:] == FILL).all()
    gp.reset()


def test_bad_arguments_leave_the_outputs_untouched(xa, torch, gp, fixed):
    dev = torch.device("cuda:0")
    d_img = torch.zeros(1 << 15, dtype=torch.uint8, device=dev)
    out = {k: torch.full((n,), FILL, dtype=torch.uint8, device=dev) for k, n in dict(out=171 * 163 * 2 + 64, map=171 * 163 * 8 + 64, summary=64).items()}
    torch.cuda.synchronize()
    nav = gs.FIXED_NAV
    fresh = xa.ImageProjector()
    for h in (fresh, gp):
        if h is gp:
            gp.set_tables(*fixed)
        good = dict(columns=96, rows=80, pitch=200, bits=10, mode=1, out_pitch=342, img=0, out=0, map=0, summary=0)
        bad = [dict(bits=0), dict(bits=17), dict(columns=0), dict(rows=0), dict(columns=1 << 16, rows=(1 << 15) + 1, pitch=1 << 17), dict(pitch=190),
               dict(pitch=201), dict(img=1), dict(bits=8, pitch=95), dict(mode=2), dict(mode=0xFFFFFFFF), dict(out_pitch=341), dict(out_pitch=340),
               dict(out_pitch=343), dict(out=1), dict(bits=8, out_pitch=170), dict(img=None), dict(out=None), dict(summary=None), dict(summary=4),
               dict(map=None), dict(map=4)]
        for change in ([{}] if h is fresh else bad):
            a = dict(good, **change)
            ptr = lambda k: None if a[k] is None else out[k].data_ptr() + a[k]
            source = (None if a["img"] is None else d_img.data_ptr() + a["img"], a["columns"], a["rows"], a["pitch"], a["bits"])
            calls = [lambda: h.resample_device(*source, ptr("map"), a["mode"], ptr("out"), a["out_pitch"], ptr("summary"))]
            if "map" not in change:
                calls.append(lambda: h.project_device(nav, *source, a["mode"], ptr("out"), a["out_pitch"], ptr("summary")))
            if set(change) <= {"map"}:
                calls.append(lambda: h.map_device(nav, ptr("map")))
            for call in calls:
                with pytest.raises(xa.XritError) as ei:         # the fresh handle: no tables set
                    call()
                assert ei.value.code == -1, change
        if h is fresh:
            with pytest.raises(xa.XritError) as ei:
                h.tables()
            assert ei.value.code == -1
            for shape in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
                with pytest.raises(xa.XritError) as ei:
                    h.set_tables(np.zeros(shape[1]), np.zeros(shape[1]), np.zeros(shape[0]), np.zeros(shape[0]))
                assert ei.value.code == -1
            with pytest.raises(xa.XritError) as ei:
                h.set_grid(2, 4, 4, 0.0, 0.0, 1.0, 1.0, 0.0)
            assert ei.value.code == -1
            with pytest.raises(xa.XritError) as ei:             # and a refused grid leaves it without tables
                h.project(nav, np.ones((4, 4), np.uint8), 8)
            assert ei.value.code == -1
    fresh.close()
    with pytest.raises(xa.XritError) as ei:
        gp.project(nav, np.ones((4, 4), np.uint8), 8, 2)
    assert ei.value.code == -1
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in out.values())
    # the call that is good, from the same arguments: all zero is all "no data"
    gp.project_device(nav, d_img.data_ptr(), 96, 80, 200, 10, 1, out["out"].data_ptr(), 342, out["summary"].data_ptr())
    torch.cuda.synchronize()
    s = out["summary"].cpu().numpy()[:56].view(xa.GEO_SUMMARY_DTYPE)[0]
    assert int(s["no_data"]) == 24069 and int(s["written"]) == 0 and not out["out"].cpu().numpy()[:342 * 163].any()


def test_queued_behind_files_images_and_canvas_on_one_stream(xa, torch, gp):
    """canvas_cases.mixed_stream through packets, files, images and canvas on one stream, and behind them, with no wait in
    between, a fused projection per canvas on the slot's pixels where they lie (xrit_canvas_pixels_device) and the product
    stage on the projected image.  The geometry the calls need on the host is the slot table of the same stream through
    the host-buffer forms; each image is navigated so that the disc just fills it."""
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
    assert len(used) == 5 and all(int(slots[i]["complete"]) == 1 for i in used)
    sub_lon = 0.0
    gp.set_grid(gs.EQUIRECT, 61, 51, -90.0, 75.0, 3.0, 3.0, sub_lon)
    tables = gp.tables()
    navs = {}
    for i in used:
        c, r = int(slots[i]["max_column"]), int(slots[i]["max_row"])
        navs[i] = gs.nav_of(int(c / 2 / 8.8 * 65536), -int(r / 2 / 8.8 * 65536), (c + 1) // 2 + 1, (r + 1) // 2 + 1, 1, sub_lon)
    dev = torch.device("cuda:0")
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    pa, fa, im, cv, pr = xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder(), xa.ImageCanvas(6, cc.SLOT_BYTES), xa.ImageProduct()
    n = int(off[64])
    cap = 2 * n
    mb, mp = xa.packets_max_bytes(cap), 16 * cap + 64
    b = {k: z(v) for k, v in dict(pbytes=mb, desc=mp * 32, pko=65 * 4, psum=72, fbytes=mb, pieces=mp * 32, frecs=2 * mp * 80, fsum=104, out=mp * 256,
                                  lines=mp * 32, ifiles=2 * mp * 48, isum=80, cfiles=2 * mp * 32, slots=6 * 136, csum=168).items()}
    b["vcdu"] = torch.cat([torch.from_numpy(vcdu.reshape(-1).copy()).to(dev), z((cap - n) * 892)])
    b["off"] = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
    outs = {}
    for i in used:
        w = 1 if int(slots[i]["bits"]) <= 8 else 2
        outs[i] = {k: torch.full((nb + GUARD,), FILL, dtype=torch.uint8, device=dev)
                   for k, nb in dict(geo=61 * 51 * w, gsum=56, tone=61 * 51, psum=64).items()}
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
        o, bits = outs[i], int(slots[i]["bits"])
        w = 1 if bits <= 8 else 2
        gp.project_device(navs[i], cv.pixels_device(i), int(slots[i]["max_column"]), int(slots[i]["max_row"]), int(slots[i]["pitch"]), bits, "bilinear",
                          o["geo"].data_ptr(), 61 * w, o["gsum"].data_ptr(), stream=s.cuda_stream)
        pr.process_device(o["geo"].data_ptr(), 61, 51, 61 * w, bits, o["psum"].data_ptr(), tone="equalise", d_tone_ptr=o["tone"].data_ptr(),
                          stream=s.cuda_stream)
    s.synchronize()                                             # the only one
    assert b["slots"].cpu().numpy().tobytes() == slots.tobytes()
    written = 0
    for i in used:
        _, bits, img = images[int(slots[i]["image_id"])]
        assert np.array_equal(cv.image(i)[1], img)
        img = img.astype(np.uint8 if bits <= 8 else np.uint16)
        want, summary = gs.project(img, tables, navs[i], gs.BILINEAR)
        got = {k: t.cpu().numpy() for k, t in outs[i].items()}
        assert all((g[-GUARD:] == FILL).all() for g in got.values())
        assert np.array_equal(got["geo"][:-GUARD].view(img.dtype).reshape(51, 61), want)
        same_summary(xa, got["gsum"][:56].view(xa.GEO_SUMMARY_DTYPE)[0], summary)
        assert np.array_equal(got["tone"][:-GUARD].reshape(51, 61), sp.process(want, bits, sp.EQUALISE)["tone"])
        written += summary["written"]
    assert written > 2000
    for x in (pa, fa, im, cv, pr, h_pa, h_fa, h_im, h_cv):
        x.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_one_real_size(xa, torch, gp):
    """A 5424 x 5424 10-bit full disc (the index of its last sample is past 2^25 samples, its byte offset past 58 MB), random
    with 339 zero rows, onto 1800 x 1800 at 0.1 degrees, bilinear."""
    rng = np.random.default_rng(12)
    img = rng.integers(1, 1024, (5424, 5424), dtype=np.uint16)
    img[2034:2034 + 339] = 0
    nav = gs.nav_of(20466275, 20466275, 2713, 2713, 1, -75.2)
    gp.set_grid(gs.EQUIRECT, 1800, 1800, nav["sub_lon"] - 90.0, 89.95, 0.1, 0.1, nav["sub_lon"])
    tables = gp.tables()
    want, summary = gs.project(img, tables, nav, gs.BILINEAR)
    got, s = gp.project(nav, img, 10, "bilinear")
    assert np.array_equal(got, want)
    same_summary(xa, s, summary)
    assert summary["written"] > 1800 * 1800 // 2 and summary["no_data"] > 50000
    d_img = torch.from_numpy(img.view(np.uint8).reshape(-1)).to("cuda:0")
    d_map = torch.empty(1800 * 1800 * 8, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((1800 * 1800 * 2 + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    d_sum = torch.zeros(56, dtype=torch.uint8, device="cuda:0")
    gp.map_device(nav, d_map.data_ptr())
    gp.resample_device(d_img.data_ptr(), 5424, 5424, 10848, 10, d_map.data_ptr(), "bilinear", d_out.data_ptr(), 3600, d_sum.data_ptr())
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert np.array_equal(raw[:-GUARD].view(np.uint16).reshape(1800, 1800), want) and (raw[-GUARD:] == FILL).all()
    same_summary(xa, d_sum.cpu().numpy().view(xa.GEO_SUMMARY_DTYPE)[0], summary)
    del d_img, d_map, d_out
    torch.cuda.empty_cache()


def test_host_program_project(xa, tmp_path):
    """End to end from IQ: an 8-bit image of two segments whose first carries a navigation record, a 10-bit image of one
    segment under another sub-satellite longitude, an image whose first segment never comes and one whose record names
    another projection -> .geo.pgm for the first two, the specification's of that canvas on the library's tables of the grid; a
    line on stderr for each of the others.  Everything else the run writes is what it writes without --project."""
    from test_gpu_canvas import host_capture
    rng = np.random.default_rng(71)
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
    by_vc = {5: [p for _, p, _ in isp.stream_of(rng, items)]}
    iq = host_capture(tmp_path, by_vc, 71)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host_bin = os.path.join(root, "xritdemod_amd", "bin", "xrit_demod_host")
    base = [host_bin, "--input", str(iq), "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null", "--block", "200000",
            "--files-decompress", "--canvas", "--canvas-slots", "6", "--canvas-mib", "1"]
    grid = (gs.EQUIRECT, 50, 41, -170.0, 60.0, 3.0, 3.0)
    flags = ["--project", "--project-grid", "-170:60:3:50:41"]
    runs = {}
    for name, extra in (("plain", []), ("bilinear", flags), ("nearest", flags + ["--project-mode", "nearest", "--products"])):
        r = subprocess.run(base + ["--files", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        runs[name] = ({nm: (tmp_path / name / nm).read_bytes() for nm in os.listdir(tmp_path / name)}, r.stderr)
    plain, err = runs["plain"]
    assert plain["GOES_test_full_disk.lrit.pgm"] == b"P5\n64 12\n255\n" + a.astype(np.uint8).tobytes() and "project:" not in err
    assert len([nm for nm in plain if nm.endswith(".pgm")]) == 4 and not [nm for nm in plain if ".geo." in nm]
    for name, mode in (("bilinear", gs.BILINEAR), ("nearest", gs.NEAREST)):
        got, err = runs[name]
        geo = {nm for nm in got if ".geo." in nm}
        rest = {nm: v for nm, v in got.items() if nm not in geo and ".view." not in nm and ".thumb." not in nm}
        assert rest == plain and {nm for nm in geo if nm.endswith(".geo.pgm")} == {"GOES_test_full_disk.lrit.geo.pgm", [nm for nm in plain if "_img22_" in nm][0][:-4] + ".geo.pgm"}
        for nm in sorted(geo):
            if not nm.endswith(".geo.pgm"):
                continue
            img, bits, nav = (a.astype(np.uint8), 8, nav_a) if nm.startswith("GOES") else (b.astype(np.uint16), 10, nav_b)
            want, summary = gs.project(img, xa.geo_grid_tables(*grid, nav["sub_lon"]), nav, mode)
            assert summary["written"] > 300
            assert got[nm] == b"P5\n50 41\n%d\n" % ((1 << bits) - 1) + (want.tobytes() if bits <= 8 else want.astype(">u2").tobytes()), nm
            if name == "nearest":                       # with --products the projected image is toned too
                assert got[nm[:-4] + ".view.pgm"] == b"P5\n50 41\n255\n" + sp.process(want, bits, sp.EQUALISE)["tone"].tobytes()
        assert len(geo) == (4 if name == "nearest" else 2)
        lines = [ln for ln in err.splitlines() if ln.startswith("project:")]
        assert len(lines) == 3 and sum("no segment file at line 0, column 0" in ln or "does not parse" in ln for ln in lines) == 2
        assert sum("does not parse" in ln for ln in lines) == 1 and f"project: 2 canvases projected onto 50 x 41 ({'bilinear' if mode else 'nearest'}), 2 skipped" in lines[-1]
