"""GPU tier: the map overlay stage (xrit_overlay_*, MapOverlay) against the specification of tests/overlay_spec.py -- the
mask, every field of both summaries and the blended image compared with np.array_equal, in both forms of the draw.  The
shapes are the smallest at which the kernels can still go wrong: images of 70 x 50 and 301 x 203 (columns no multiple of
4, a pitch larger than the columns, sentinel bytes behind every row and behind the buffer); segments in all eight octants,
from either end, points, sub-pixel segments, ones outside, across every edge and corner, longer than a wave's 64 steps and
than the image, at +-(2^29 - 1) and at the break threshold; 1 to 5000 segments (one wave, one workgroup, several workgroups
of the scan); stamps over every edge; eight layers into one mask through the atomic OR; max_jump; the vertex map on quads
that hold anything; the blend 1 -> 1, 1 -> 3, 3 -> 3, aligned and not, in place; calls back to back on one stream, between
the product stage and the JPEG stage; the host-buffer and resident forms; every bad argument; one real size; and xrit_demod_host --products --overlay --graticule
from IQ to .view.map.ppm files."""
import os
import subprocess

import numpy as np
import pytest

import geo_spec as gs
import overlay_spec as ovs

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64
B = (ovs.BREAK, ovs.BREAK)
BIG = ovs.LIMIT - 1


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
def ov(xa):
    h = xa.MapOverlay()
    yield h
    h.close()


def upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def points_bytes(xa, points):
    a = np.asarray(points, np.int64).reshape(-1, 2).astype(np.int32)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Mask:
    """A mask of rows x columns in device memory, `pitch` bytes from row to row, every other byte a sentinel."""

    def __init__(self, torch, columns, rows, pitch=None, start=None):
        self.columns, self.rows = columns, rows
        self.pitch = (columns + 3) // 4 * 4 + 8 if pitch is None else pitch
        host = np.full(self.rows * self.pitch + GUARD, FILL, np.uint8)
        body = host[:self.rows * self.pitch].reshape(self.rows, self.pitch)
        body[:, :columns] = 0 if start is None else start
        self.d = torch.from_numpy(host).to("cuda:0")
        self.d_summary = torch.full((64 + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")

    def draw(self, ov, d_points, n, layer, width, max_jump=0, clear=False, stream=None):
        ov.draw_device(d_points.data_ptr() if d_points is not None else None, n, layer, width, max_jump, self.d.data_ptr(), self.columns, self.rows,
                       self.pitch, clear, self.d_summary.data_ptr(), stream=stream)

    def read(self, cleared=False):
        """-> the mask; the bytes behind the rows' columns and behind the buffer must be the sentinel (zero after a clear)."""
        raw = self.d.cpu().numpy()
        assert (raw[self.rows * self.pitch:] == FILL).all()
        body = raw[:self.rows * self.pitch].reshape(self.rows, self.pitch)
        assert (body[:, self.columns:] == (0 if cleared else FILL)).all()
        return body[:, :self.columns].copy()

    def summary(self, xa):
        s = self.d_summary.cpu().numpy()
        assert (s[64:] == FILL).all()
        return s[:64].view(xa.OVERLAY_DRAW_SUMMARY_DTYPE)[0]


def same_summary(got, want, fields):
    assert tuple(got.dtype.names) == fields
    for k in fields:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k], np.int64)), (k, got[k], want[k])


def check_draw(xa, torch, ov, points, columns, rows, layer=0, width=1, max_jump=0, start=None, clear=False, pitch=None):
    """One list drawn in both forms into fresh masks; both must be the specification's.  -> (mask, summary) of it."""
    zero = np.zeros((rows, columns), np.uint8) if start is None else start
    want, summary = ovs.draw(points, layer, width, max_jump, zero, clear)
    n = len(np.asarray(points, np.int64).reshape(-1, 2))
    d_points = upload(torch, points_bytes(xa, points)) if n else None
    for form in (0, 1):
        ov.set_form(form)
        m = Mask(torch, columns, rows, pitch, start)
        m.draw(ov, d_points, n, layer, width, max_jump, clear)
        torch.cuda.synchronize()
        got = m.read(cleared=clear)
        assert np.array_equal(got, want), (form, int((got != want).sum()))
        same_summary(m.summary(xa), summary, ovs.DRAW_FIELDS)
    ov.set_form(1)
    return want, summary


def direction_segments(columns, rows):
    """Pairs of ends (1/256 pixel) for an image of columns x rows."""
    cx, cy = columns * 256, rows * 256
    mx, my = cx // 2 + 37, cy // 2 - 51
    out = []
    # horizontal, vertical, both diagonals, steep and shallow in all eight octants
    for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1), (3, 1), (1, 3), (-3, 1), (-1, 3), (3, -1), (1, -3), (-3, -1), (-1, -3)):
        out.append(((mx, my), (mx + dx * 1500, my + dy * 1500)))
    out += [((mx, my), (mx, my)), ((mx + 3, my + 5), (mx + 90, my - 60)), ((300, 300), (300 + 255, 300)), ((127, 128), (128, 127))]       # points, sub-pixel
    out += [((-9000, -9000), (-3000, -5000)), ((cx + 400, 100), (cx + 5000, 9000)), ((100, cy + 300), (4000, cy + 2000))]                 # outside
    out += [((-700, my), (900, my + 300)), ((cx - 800, my), (cx + 800, my - 200)), ((mx, -600), (mx + 200, 700)), ((mx, cy - 700), (mx - 150, cy + 900))]
    out += [((-500, -400), (600, 700)), ((cx + 500, -400), (cx - 700, 600)), ((-500, cy + 400), (700, cy - 600)), ((cx + 300, cy + 500), (cx - 600, cy - 500))]
    out += [((10, 20), (10 + 69 * 256, 20 + 30 * 256)), ((-20 * 256, -20 * 256), (cx + 20 * 256, cy + 20 * 256)), ((cx + 5000, 0), (-5000, cy))]  # > 64 steps, > the image
    out += [((-BIG, -BIG), (BIG, BIG)), ((BIG, -BIG), (-BIG, BIG)), ((-BIG, my), (BIG, my + 256)), ((mx, BIG), (mx + 256, -BIG))]
    return out


def as_list(pairs, both_orders=True):
    pts = []
    for a, b in pairs:
        pts += [a, b, B]
        if both_orders:
            pts += [b, a, B]
    return pts


# ---- directions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("columns,rows", [(70, 50), (301, 203)])
def test_directions(xa, torch, ov, columns, rows):
    pairs = direction_segments(columns, rows)
    want, s = check_draw(xa, torch, ov, as_list(pairs), columns, rows)
    assert s["outside"] == 6 and s["drawn"] == 2 * len(pairs) and want.any()
    # each segment alone equals its own pixel set from either end (the specification's property, on the device)
    for a, b in pairs[12:16] + pairs[-4:]:
        one, _ = check_draw(xa, torch, ov, [a, b], columns, rows)
        other, _ = check_draw(xa, torch, ov, [b, a], columns, rows)
        assert np.array_equal(one, other)


def test_the_break_threshold(xa, torch, ov):
    pts = [(0, 0), (ovs.LIMIT, 0), (0, 0), (0, -ovs.LIMIT), (0, 0), (BIG, 0), (2000, 2000), (-ovs.LIMIT, ovs.LIMIT), B, (2**31 - 1, 5), (300, 300)]
    want, s = check_draw(xa, torch, ov, pts, 70, 50)
    assert s["hidden"] == 8 and s["drawn"] == 2 and want[0, :].all()


# ---- counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 64, 65, 300, 5000])
def test_segment_counts(xa, torch, ov, count):
    """A polyline of `count` segments, most of one to three pixels, every 97th of hundreds, a break now and then."""
    rng = np.random.default_rng(count)
    step = rng.integers(-700, 701, (count + 1, 2))
    step[::97] = rng.integers(-40000, 40001, (len(step[::97]), 2))
    pts = (np.cumsum(step, axis=0) + (150 * 256, 100 * 256)) % (330 * 256) - 10 * 256
    if count > 64:
        pts[rng.integers(1, count, count // 50)] = B
    _, s = check_draw(xa, torch, ov, pts, 301, 203, width=2)
    assert s["vertices"] == count + 1 and s["segments"] + s["hidden"] == count


def test_few_vertices_and_breaks_at_the_ends(xa, torch, ov):
    for pts in ([], [(500, 500)], [B], [B, (500, 500), (900, 900)], [(500, 500), (900, 900), B], [B, B, (500, 500), B, B, (600, 700), (900, 100), B, B],
                [B, B], [(500, 500), B, (900, 900)]):
        _, s = check_draw(xa, torch, ov, pts, 70, 50, layer=3)
        assert s["vertices"] == len(pts)


# ---- stamps and layers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 8])
def test_stamps_over_every_edge_and_corner(xa, torch, ov, width):
    columns, rows = 70, 50
    pts = []
    for px in (-5, -4, -3, -1, 0, 1, 35, columns - 2, columns - 1, columns, columns + 3, columns + 4):
        for py in (-5, -4, -1, 0, 25, rows - 1, rows, rows + 3, rows + 4):
            pts += [(px * 256 + 7, py * 256 - 9), (px * 256 + 7, py * 256 - 9), B]
    pts += [(-3 * 256, 3 * 256), (columns * 256 + 900, 3 * 256 + 40), B, (4 * 256, -900), (4 * 256 - 90, rows * 256 + 900)]
    want, _ = check_draw(xa, torch, ov, pts, columns, rows, layer=6, width=width)
    assert want[0, 0] and want[rows - 1, columns - 1]


def test_eight_layers_into_one_mask_and_clear(xa, torch, ov):
    """Every layer draws through one pixel and through the four bytes of one dword; the calls add up in the mask, in either
    order of the layers; clear zeroes the whole pitch first."""
    columns, rows = 70, 50
    rng = np.random.default_rng(8)
    lists = []
    for layer in range(8):
        pts = []
        for _ in range(40):                              # many segments through pixel (33, 21) and its dword's other bytes (32 .. 35)
            a = rng.integers(-10 * 256, 80 * 256, 2)
            c = np.array([(32 + rng.integers(0, 4)) * 256, 21 * 256])
            pts += [tuple(a), tuple(c), tuple(2 * c - a), B]
        lists.append(pts)
    want = np.zeros((rows, columns), np.uint8)
    for layer, pts in enumerate(lists):
        want, _ = ovs.draw(pts, layer, 1 + layer % 3, 0, want)
    assert want[21, 32:36].tolist() == [255] * 4
    for form in (0, 1):
        ov.set_form(form)
        for order in (range(8), reversed(range(8))):
            m = Mask(torch, columns, rows)
            for layer in order:
                m.draw(ov, upload(torch, points_bytes(xa, lists[layer])), len(lists[layer]), layer, 1 + layer % 3)
            torch.cuda.synchronize()
            assert np.array_equal(m.read(), want)
    ov.set_form(1)
    start = rng.integers(0, 256, (rows, columns)).astype(np.uint8)
    check_draw(xa, torch, ov, lists[0], columns, rows, layer=4, start=start)
    check_draw(xa, torch, ov, lists[0], columns, rows, layer=4, start=start, clear=True)


def test_max_jump_on_a_wrapped_polyline(xa, torch, ov):
    """A slanted line round the globe on a grid whose longitudes wrap behind the image's right edge: without max_jump the
    two ends of the wrap are joined by a line across the picture."""
    lon = np.arange(-180.0, 180.5, 0.5)
    pts = xa.overlay_grid_points("equirect", 300, 200, 20.0, 50.0, 0.5, 0.5, lon, 10.0 + lon / 10.0)
    pts = np.stack([pts["qx"], pts["qy"]], axis=1)
    with_line, s0 = check_draw(xa, torch, ov, pts, 300, 200)
    cut, s1 = check_draw(xa, torch, ov, pts, 300, 200, max_jump=150 * 256)
    assert s0["jumps"] == 0 and s1["jumps"] == 1 and s1["drawn"] == s0["drawn"] - 1
    assert (with_line & ~cut).sum() > 100 and not (cut & ~with_line).any()


# ---- the vertex map -----------------------------------------------------------------------------------------------------------
def test_vertex_map_is_the_projection_s_point_rule(xa, torch, ov):
    rng = np.random.default_rng(9)
    lon, lat = rng.uniform(-180, 180, 400), rng.uniform(-90, 90, 400)
    lon[:40] = gs.FIXED_NAV["sub_lon"] + rng.uniform(-82, 82, 40)                 # around the limb
    quads = xa.overlay_quads(lon, lat, gs.FIXED_NAV["sub_lon"])
    odd = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 0.0, 1.0, 6378.0])
    quads = np.concatenate([quads, rng.choice(odd, (200, 4)), np.full((1, 4), np.nan)])
    want = ovs.points_of_quads(quads, gs.FIXED_NAV)
    assert 100 < (want[:, 0] == ovs.BREAK).sum() < len(want) - 100
    n = len(quads)
    d_quads = upload(torch, quads)
    d_points = torch.full((n * 8 + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    ov.map_device(gs.FIXED_NAV, d_quads.data_ptr(), n, d_points.data_ptr())
    torch.cuda.synchronize()
    raw = d_points.cpu().numpy()
    assert (raw[n * 8:] == FILL).all()
    got = raw[:n * 8].view(np.int32).reshape(n, 2)
    assert np.array_equal(got, want)
    host = ov.map(gs.FIXED_NAV, quads)
    assert np.array_equal(host["qx"], want[:, 0]) and np.array_equal(host["qy"], want[:, 1])
    assert len(ov.map(gs.FIXED_NAV, np.zeros((0, 4)))) == 0


# ---- blend ----------------------------------------------------------------------------------------------------------------------
STYLES = [(255, 255, 0, 255), (0, 255, 255, 128), (255, 0, 0, 0), (1, 2, 3, 1), (250, 128, 7, 254), (0, 0, 0, 127), (255, 255, 255, 200), (9, 200, 90, 255)]


def blend_case(rng, columns, rows, cin):
    image = rng.integers(0, 256, (rows, columns) if cin == 1 else (rows, columns, 3)).astype(np.uint8)
    mask = np.where(rng.random((rows, columns)) < 0.3, rng.integers(0, 256, (rows, columns)), 0).astype(np.uint8)
    mask[:, columns // 3:2 * columns // 3] = 0         # whole groups of 16 pixels without a bit: the kernel copies those
    mask[rows // 2, columns // 2] = 0x80
    return image, mask


def laid_out(image, pitch, offset, fill):
    rows = image.shape[0]
    raw = image.reshape(rows, -1)
    buf = np.full(offset + pitch * (rows - 1) + raw.shape[1] + GUARD, fill, np.uint8)
    for r in range(rows):
        buf[offset + r * pitch:offset + r * pitch + raw.shape[1]] = raw[r]
    return buf


def check_blend(xa, torch, ov, image, mask, cout, pad=(0, 0, 0), offset=(0, 0, 0), in_place=False, styles=STYLES):
    rows, columns = mask.shape
    cin = 1 if image.ndim == 2 else 3
    want, summary = ovs.blend(image, mask, styles, cout)
    pitch, mask_pitch, out_pitch = columns * cin + pad[0], columns + pad[1], columns * cout + pad[2]
    host_in = laid_out(image, pitch, offset[0], 0x5A)
    d_in, d_mask = upload(torch, host_in), upload(torch, laid_out(mask, mask_pitch, offset[1], 0xFF))
    if in_place:
        assert cin == cout and out_pitch == pitch
        d_out, out_at, out_fill = d_in, offset[0], 0x5A
    else:
        d_out, out_at, out_fill = upload(torch, laid_out(np.full(want.shape, FILL, np.uint8), out_pitch, offset[2], FILL)), offset[2], FILL
    d_summary = torch.full((96 + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    ov.blend_device(d_in.data_ptr() + offset[0], columns, rows, pitch, cin, d_mask.data_ptr() + offset[1], mask_pitch, styles,
                    d_out.data_ptr() + out_at, out_pitch, cout, d_summary.data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got, laid_out(want, out_pitch, out_at, out_fill))          # the image, and every byte around it as it was
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy(), host_in)
    s = d_summary.cpu().numpy()
    assert (s[96:] == FILL).all()
    s = s[:96].view(xa.OVERLAY_BLEND_SUMMARY_DTYPE)[0]
    same_summary(s, summary, ovs.BLEND_FIELDS)
    assert int(s["by_layer"].sum()) == int(s["covered"])
    return want


@pytest.mark.parametrize("cin,cout", [(1, 1), (1, 3), (3, 3)])
def test_blend_aligned_and_odd(xa, torch, ov, cin, cout):
    rng = np.random.default_rng(10 + cin + cout)
    for (columns, rows), pad, offset in (((70, 50), (0, 0, 0), (0, 0, 0)), ((301, 29), (16 - 301 * cin % 16, 16 - 301 % 16, 16 - 301 * cout % 16), (0, 0, 0)),
                                        ((301, 29), (5, 3, 7), (1, 2, 3)), ((64, 9), (0, 0, 0), (16, 32, 48)), ((1, 1), (0, 0, 0), (3, 0, 0)),
                                        ((15, 3), (1, 1, 1), (0, 0, 0)), ((2049, 5), (15 * cin, 15, 15 * cout), (16, 16, 16))):
        image, mask = blend_case(rng, columns, rows, cin)
        check_blend(xa, torch, ov, image, mask, cout, pad, offset)


def test_blend_in_place_alpha_and_overlapping_layers(xa, torch, ov):
    rng = np.random.default_rng(20)
    for cin in (1, 3):
        image, mask = blend_case(rng, 320, 40, cin)
        check_blend(xa, torch, ov, image, mask, cin, in_place=True)
        check_blend(xa, torch, ov, image, mask, cin, pad=(7, 1, 7), offset=(5, 0, 0), in_place=True)
    image = rng.integers(0, 256, (4, 64)).astype(np.uint8)
    mask = np.tile(np.array([0, 1, 2, 4, 3, 5, 6, 7, 0x80, 0x81, 0xFF, 0x40, 0x18, 0x24, 0x03, 0x00], np.uint8), (4, 4))
    for alpha in (0, 128, 255):
        styles = [(10 * k + 5, 255 - 20 * k, 30 * k, alpha) for k in range(8)]
        out = check_blend(xa, torch, ov, image, mask, 3, styles=styles)
        if alpha == 0:
            assert np.array_equal(out, np.repeat(image[:, :, None], 3, axis=2))
        if alpha == 255:
            assert out[0, 10].tolist() == [75, 115, 210] and out[0, 1].tolist() == [5, 255, 0]     # 0xFF: layer 7 wins; 1: layer 0


# ---- call forms -------------------------------------------------------------------------------------------------------------------
def test_two_draws_and_a_blend_back_to_back_between_product_and_jpeg(xa, torch, ov):
    """A 10-bit image toned by the product stage, coastline and graticule drawn into one mask, the mask blended into the toned
    image in place, the result encoded: five stages' calls on one stream with one wait at the end."""
    import jpeg_spec as js
    import product_spec as sp
    rng = np.random.default_rng(30)
    rows, columns = 90, 150
    raw = rng.integers(0, 1024, (rows, columns)).astype(np.uint16)
    coast = (np.cumsum(rng.integers(-500, 501, (400, 2)), axis=0) + (70 * 256, 40 * 256))
    lon, lat = xa.overlay_densify(*xa.overlay_graticule(30.0, 30.0), 0.5)
    grat = xa.overlay_grid_points("equirect", columns, rows, -180.0, 90.0, 2.4, 2.0, lon, lat)
    grat = np.stack([grat["qx"], grat["qy"]], axis=1)
    tone = sp.process(raw, 10, sp.EQUALISE)["tone"]
    mask, _ = ovs.draw(coast, 0, 2, 0, np.zeros((rows, columns), np.uint8))
    mask, s_grat = ovs.draw(grat, 1, 1, 75 * 256, mask)
    blended, s_blend = ovs.blend(tone, mask, STYLES, 1)
    want_file = js.encode(blended, quality=85)[0]
    assert s_blend["by_layer"][0] > 50 and s_blend["by_layer"][1] > 50
    pr, enc = xa.ImageProduct(), xa.JpegEncoder()
    enc.set_quality(85, 0)
    ov.draw(grat, 0, 1, np.zeros((rows, 152), np.uint8))                   # the scratch has its size: nothing is allocated below
    d_raw, d_coast, d_grat = upload(torch, raw), upload(torch, points_bytes(xa, coast)), upload(torch, points_bytes(xa, grat))
    d_tone = torch.zeros(rows * columns, dtype=torch.uint8, device="cuda:0")
    d_psum = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    m = Mask(torch, columns, rows, start=0x77)
    d_bsum = torch.zeros(96, dtype=torch.uint8, device="cuda:0")
    d_file = torch.full((len(want_file) + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    d_res = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    pr.process_device(d_raw.data_ptr(), columns, rows, 2 * columns, 10, d_psum.data_ptr(), tone="equalise", d_tone_ptr=d_tone.data_ptr(), stream=s.cuda_stream)
    m.draw(ov, d_coast, len(coast), 0, 2, clear=True, stream=s.cuda_stream)
    m.draw(ov, d_grat, len(grat), 1, 1, max_jump=75 * 256, stream=s.cuda_stream)
    ov.blend_device(d_tone.data_ptr(), columns, rows, columns, 1, m.d.data_ptr(), m.pitch, STYLES, d_tone.data_ptr(), columns, 1, d_bsum.data_ptr(),
                    stream=s.cuda_stream)
    enc.encode_device(d_tone.data_ptr(), columns, rows, columns, 1, d_file.data_ptr(), len(want_file), d_res.data_ptr(), stream=s.cuda_stream)
    s.synchronize()                                     # the only one
    assert np.array_equal(m.read(cleared=True), mask)
    same_summary(m.summary(xa), s_grat, ovs.DRAW_FIELDS)
    assert np.array_equal(d_tone.cpu().numpy().reshape(rows, columns), blended)
    same_summary(d_bsum.cpu().numpy().view(xa.OVERLAY_BLEND_SUMMARY_DTYPE)[0], s_blend, ovs.BLEND_FIELDS)
    got = d_file.cpu().numpy()
    assert got[:len(want_file)].tobytes() == want_file and (got[len(want_file):] == FILL).all()
    pr.close()
    enc.close()


def test_queued_behind_canvas_and_product_on_a_slot_and_in_front_of_jpeg(xa, torch, ov):
    """canvas_cases.mixed_stream through packets, files, images and canvas on one stream, and behind them with no wait in
    between, per canvas: the product call on the slot's pixels where they lie (xrit_canvas_pixels_device), two draws into one
    mask, the blend in place on the toned view, and xrit_jpeg_encode_device on it -- the file must be the specification's
    encoding of the specification's blend of the specification's toned view.  Behind that, for the 8-bit canvases, a blend in
    place on the slot itself: the slot's own pitch and base under the blend kernel."""
    import canvas_cases as cc
    import file_spec as fs
    import jpeg_spec as js
    import packet_spec as ps
    import product_spec as sp
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
    assert len(used) == 5 and {int(slots[i]["bits"]) for i in used} == {8, 10, 12}
    # what the specification makes of every canvas
    jobs = {}
    for i in used:
        _, bits, img = images[int(slots[i]["image_id"])]
        r, c = img.shape
        coast = np.cumsum(rng.integers(-300, 301, (150, 2)), axis=0) + (c * 128, r * 128)
        coast[[40, 90]] = B
        grat = np.array([p for x in range(0, c * 256, 16 * 256) for p in ((x, -500), (x + 900, r * 256 + 500), B)] +
                        [p for y in range(0, r * 256, 12 * 256) for p in ((-500, y), (c * 256 + 500, y + 300), B)])
        tone = sp.process(img, bits, sp.EQUALISE)["tone"]
        mask, _ = ovs.draw(coast, 0, 2, 0, np.zeros((r, c), np.uint8))
        mask, s_grat = ovs.draw(grat, 1, 1, 0, mask)
        blended, s_blend = ovs.blend(tone, mask, STYLES, 1)
        assert s_blend["by_layer"][0] > 0 and s_blend["by_layer"][1] > 0          # (the smallest canvas is 5 x 1)
        jobs[i] = dict(bits=bits, img=img, coast=coast, grat=grat, mask=mask, s_grat=s_grat, blended=blended, s_blend=s_blend,
                       file=js.encode(blended, quality=85)[0], slot_blend=ovs.blend(img.astype(np.uint8), mask, STYLES, 1)[0] if bits == 8 else None)
    dev = torch.device("cuda:0")
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    pa, fa, im, cv = xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder(), xa.ImageCanvas(6, cc.SLOT_BYTES)
    pr, enc = xa.ImageProduct(), xa.JpegEncoder()
    enc.set_quality(85, 0)
    n = int(off[64])
    cap = 2 * n
    mb, mp = xa.packets_max_bytes(cap), 16 * cap + 64
    b = {k: z(v) for k, v in dict(pbytes=mb, desc=mp * 32, pko=65 * 4, psum=72, fbytes=mb, pieces=mp * 32, frecs=2 * mp * 80, fsum=104, out=mp * 256,
                                  lines=mp * 32, ifiles=2 * mp * 48, isum=80, cfiles=2 * mp * 32, slots=6 * 136, csum=168).items()}
    b["vcdu"] = torch.cat([torch.from_numpy(vcdu.reshape(-1).copy()).to(dev), z((cap - n) * 892)])
    b["off"] = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
    ov.draw(np.zeros((400, 2), np.int64), 0, 1, np.zeros((4, 4), np.uint8))        # the scratch has its size: nothing is allocated below
    for i, j in jobs.items():
        r, c = j["img"].shape
        j.update(d_coast=upload(torch, points_bytes(xa, j["coast"])), d_grat=upload(torch, points_bytes(xa, j["grat"])), m=Mask(torch, c, r, start=0x33),
                 d_tone=torch.full((r * c + GUARD,), FILL, dtype=torch.uint8, device=dev), d_psum=z(64), d_bsum=z(96), d_bsum2=z(96),
                 d_file=torch.full((len(j["file"]) + GUARD,), FILL, dtype=torch.uint8, device=dev), d_res=z(16))
    q = {k: t.data_ptr() for k, t in b.items()}
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    st = s.cuda_stream
    pa.process_device(q["vcdu"], q["off"], cap, q["pbytes"], mb, q["desc"], mp, q["pko"], q["psum"], stream=st)
    fa.process_device(q["pbytes"], mb, q["desc"], q["pko"], mp, q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"], stream=st)
    im.process_device(q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"], q["out"], mp * 256, q["lines"], mp, q["ifiles"], q["isum"], stream=st)
    cv.process_device(q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"], q["out"], mp * 256, q["lines"], mp, q["ifiles"], q["isum"],
                      q["cfiles"], q["slots"], q["csum"], stream=st)
    for i, j in jobs.items():
        r, c = j["img"].shape
        assert (int(slots[i]["max_row"]), int(slots[i]["max_column"])) == (r, c)
        pitch, m = int(slots[i]["pitch"]), j["m"]
        pr.process_device(cv.pixels_device(i), c, r, pitch, j["bits"], j["d_psum"].data_ptr(), tone="equalise", d_tone_ptr=j["d_tone"].data_ptr(), stream=st)
        m.draw(ov, j["d_coast"], len(j["coast"]), 0, 2, clear=True, stream=st)
        m.draw(ov, j["d_grat"], len(j["grat"]), 1, 1, stream=st)
        ov.blend_device(j["d_tone"].data_ptr(), c, r, c, 1, m.d.data_ptr(), m.pitch, STYLES, j["d_tone"].data_ptr(), c, 1, j["d_bsum"].data_ptr(), stream=st)
        enc.encode_device(j["d_tone"].data_ptr(), c, r, c, 1, j["d_file"].data_ptr(), len(j["file"]), j["d_res"].data_ptr(), stream=st)
        if j["bits"] == 8:                              # and the slot itself, in place, at its own pitch
            ov.blend_device(cv.pixels_device(i), c, r, pitch, 1, m.d.data_ptr(), m.pitch, STYLES, cv.pixels_device(i), pitch, 1, j["d_bsum2"].data_ptr(),
                            stream=st)
    s.synchronize()                                     # the only one
    assert b["slots"].cpu().numpy().tobytes() == slots.tobytes()
    assert sum(j["bits"] == 8 for j in jobs.values()) >= 1
    for i, j in jobs.items():
        r, c = j["img"].shape
        assert np.array_equal(j["m"].read(cleared=True), j["mask"])
        same_summary(j["m"].summary(xa), j["s_grat"], ovs.DRAW_FIELDS)
        tone = j["d_tone"].cpu().numpy()
        assert np.array_equal(tone[:r * c].reshape(r, c), j["blended"]) and (tone[r * c:] == FILL).all()
        same_summary(j["d_bsum"].cpu().numpy().view(xa.OVERLAY_BLEND_SUMMARY_DTYPE)[0], j["s_blend"], ovs.BLEND_FIELDS)
        got = j["d_file"].cpu().numpy()
        assert got[:len(j["file"])].tobytes() == j["file"] and (got[len(j["file"]):] == FILL).all()
        if j["bits"] == 8:
            assert np.array_equal(cv.image(i)[1], j["slot_blend"])
        else:
            assert np.array_equal(cv.image(i)[1], j["img"])
    for x in (pa, fa, im, cv, h_pa, h_fa, h_im, h_cv, pr, enc):
        x.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_host_buffer_and_resident_forms(xa, torch, ov):
    rng = np.random.default_rng(40)
    rows, columns = 50, 70
    pts = rng.integers(-3000, 75 * 256, (60, 2))
    pts[[9, 31]] = B
    for form in (0, 1):
        ov.set_form(form)
        mask = np.full((rows, 72), 0x10, np.uint8)
        s = ov.draw_into(pts, 2, 3, mask, columns)
        want, summary = ovs.draw(pts, 2, 3, 0, np.full((rows, columns), 0x10, np.uint8))
        assert np.array_equal(mask[:, :columns], want) and (mask[:, columns:] == 0x10).all()
        same_summary(s, summary, ovs.DRAW_FIELDS)
        s = ov.draw_into(pts, 5, 1, mask, columns, max_jump=4000, clear=True)
        want, summary = ovs.draw(pts, 5, 1, 4000, want, clear=True)
        assert np.array_equal(mask[:, :columns], want) and (mask[:, columns:] == 0).all()
        same_summary(s, summary, ovs.DRAW_FIELDS)
        assert int(ov.draw([], 0, 1, np.zeros((4, 4), np.uint8))["vertices"]) == 0
    ov.set_form(1)
    # where the last host-buffer draw left the mask on the device: the resident blend takes it from there
    mask = np.zeros((rows, 72), np.uint8)
    ov.draw_into(pts, 1, 2, mask, columns)
    image = rng.integers(0, 256, (rows, columns)).astype(np.uint8)
    d_img = upload(torch, image)
    got, _ = ov.blend_resident(d_img.data_ptr(), columns, rows, columns, 1, ov.mask_device(), 72, STYLES, 3)
    assert np.array_equal(got, ovs.blend(image, mask[:, :columns], STYLES, 3)[0]) and mask.any()
    assert xa.MapOverlay().mask_device() is None
    for cin, cout in ((1, 1), (1, 3), (3, 3)):
        image, mask = blend_case(rng, columns, rows, cin)
        want, summary = ovs.blend(image, mask, STYLES, cout)
        got, s = ov.blend(image, mask, STYLES, cout)
        assert np.array_equal(got, want)
        same_summary(s, summary, ovs.BLEND_FIELDS)
        d_img, d_mask = upload(torch, image), upload(torch, mask)
        got, s = ov.blend_resident(d_img.data_ptr(), columns, rows, columns * cin, cin, d_mask.data_ptr(), columns, STYLES, cout)
        assert np.array_equal(got, want)
        same_summary(s, summary, ovs.BLEND_FIELDS)
    ov.reset()


def test_bad_arguments_leave_the_outputs_untouched(xa, torch, ov):
    d_pts = upload(torch, points_bytes(xa, [(0, 0), (5000, 5000), (9000, 100)]))
    d_mask = torch.full((72 * 50 + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    d_sum = torch.full((128,), FILL, dtype=torch.uint8, device="cuda:0")
    d_img = torch.full((70 * 50 * 3 + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((70 * 50 * 3 + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    d_quads = torch.zeros(3 * 32 + 8, dtype=torch.uint8, device="cuda:0")
    good = dict(pts=0, n=3, layer=0, width=1, mask=0, columns=70, rows=50, pitch=72, summary=0)
    bad = [dict(pts=None), dict(mask=None), dict(summary=None), dict(n=(1 << 26) + 1), dict(layer=8), dict(width=0), dict(width=9), dict(columns=0),
           dict(rows=0), dict(columns=16385, pitch=16388), dict(rows=16385), dict(pitch=68), dict(pitch=71), dict(pitch=70), dict(mask=2), dict(pts=4),
           dict(summary=4)]
    ptr = lambda t, off: None if off is None else t.data_ptr() + off
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(xa.XritError) as ei:
            ov.draw_device(ptr(d_pts, a["pts"]), a["n"], a["layer"], a["width"], 0, ptr(d_mask, a["mask"]), a["columns"], a["rows"], a["pitch"], True,
                           ptr(d_sum, a["summary"]))
        assert ei.value.code == -1, change
    good = dict(img=0, columns=70, rows=50, pitch=70, cin=1, mask=0, mask_pitch=72, styles=STYLES, out=0, out_pitch=210, cout=3, summary=0)
    bad = [dict(img=None), dict(mask=None), dict(styles=None), dict(out=None), dict(summary=None), dict(cin=0), dict(cin=2), dict(cout=2), dict(cout=4),
           dict(cin=3, pitch=210, cout=1, out_pitch=70), dict(pitch=69), dict(mask_pitch=69), dict(out_pitch=209), dict(columns=0), dict(rows=0),
           dict(summary=4), dict(columns=1 << 16, rows=1 << 16, pitch=1 << 16, mask_pitch=1 << 16, out_pitch=3 << 16), dict(bits=10)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(xa.XritError) as ei:
            if "bits" in a:
                image = ov._image(d_img.data_ptr(), 70, 50, 70)
                image["bits"] = a["bits"]
                import ctypes as C
                p = lambda x: C.c_void_p(x)
                xa._capi._check(xa.lib().xrit_overlay_blend_device(ov._h, image.ctypes.data_as(C.c_void_p), 1, p(d_mask.data_ptr()), 72,
                                                                   xa.overlay_styles(STYLES).ctypes.data_as(C.c_void_p), p(d_out.data_ptr()), 210, 3,
                                                                   p(d_sum.data_ptr()), None))
            else:
                ov.blend_device(ptr(d_img, a["img"]), a["columns"], a["rows"], a["pitch"], a["cin"], ptr(d_mask, a["mask"]), a["mask_pitch"], a["styles"],
                                ptr(d_out, a["out"]), a["out_pitch"], a["cout"], ptr(d_sum, a["summary"]))
        assert ei.value.code == -1, change
    # in place with other components or another pitch
    for cin, pitch, cout, out_pitch in ((1, 70, 3, 210), (1, 70, 1, 72)):
        with pytest.raises(xa.XritError) as ei:
            ov.blend_device(d_img.data_ptr(), 70, 50, pitch, cin, d_mask.data_ptr(), 72, STYLES, d_img.data_ptr(), out_pitch, cout, d_sum.data_ptr())
        assert ei.value.code == -1
    for change in (dict(nav=None), dict(quads=None), dict(points=None), dict(n=(1 << 26) + 1), dict(quads=4), dict(points=4)):
        a = dict(dict(nav=gs.FIXED_NAV, quads=0, n=3, points=0), **change)
        with pytest.raises(xa.XritError) as ei:
            if a["nav"] is None:
                xa._capi._check(xa.lib().xrit_overlay_map_device(ov._h, None, d_quads.data_ptr(), 3, d_out.data_ptr(), None))
            else:
                ov.map_device(a["nav"], ptr(d_quads, a["quads"]), a["n"], ptr(d_out, a["points"]))
        assert ei.value.code == -1, change
    for form in (2, 7, 1 << 31):
        with pytest.raises(xa.XritError) as ei:
            ov.set_form(form)
        assert ei.value.code == -1
    torch.cuda.synchronize()
    for t in (d_mask, d_sum, d_img, d_out):
        assert (t.cpu().numpy() == FILL).all()
    # a refused form changes nothing: the handle still draws, in form 1
    check_draw(xa, torch, ov, [(0, 0), (5000, 5000), (9000, 100)], 70, 50)


# ---- one real size --------------------------------------------------------------------------------------------------------------------
def test_one_real_size_form_1_against_form_0(xa, torch, ov):
    """5424 x 5424: a 1 degree graticule densified to 0.05 degrees on a grid that wraps, and a random walk of 200 000 vertices:
    millions of steps through the scan's second level; form 1 must leave form 0's mask and summary."""
    size = 5424
    lon, lat = xa.overlay_densify(*xa.overlay_graticule(1.0, 1.0), 0.05)
    grat = xa.overlay_grid_points("equirect", size, size, -150.0, 81.0, 162.0 / size, 162.0 / size, lon, lat)
    rng = np.random.default_rng(50)
    step = rng.integers(-600, 601, (200000, 2))
    step[::1000] = rng.integers(-(1 << 20), 1 << 20, (200, 2))
    walk = (np.cumsum(step, axis=0) + size * 128) % (size * 256 + 100000) - 50000
    both = np.concatenate([np.stack([grat["qx"], grat["qy"]], axis=1), [B], walk]).astype(np.int32)
    d_points = upload(torch, both)
    pitch = (size + 3) // 4 * 4 + 4
    results = []
    for form in (0, 1):
        ov.set_form(form)
        d_mask = torch.full((size * pitch,), FILL, dtype=torch.uint8, device="cuda:0")
        d_sum = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
        ov.draw_device(d_points.data_ptr(), len(both), 1, 2, size * 128, d_mask.data_ptr(), size, size, pitch, True, d_sum.data_ptr())
        torch.cuda.synchronize()
        results.append((d_mask, d_sum.cpu().numpy().view(xa.OVERLAY_DRAW_SUMMARY_DTYPE)[0]))
    ov.set_form(1)
    (m0, s0), (m1, s1) = results
    assert bool(torch.equal(m0, m1)) and s0.tobytes() == s1.tobytes()
    assert int(s0["vertices"]) == len(both) and int(s0["steps"]) > 2 * len(both) and int(s0["jumps"]) > 100 and int(s0["outside"]) > 0
    m = m0.cpu().numpy().reshape(size, pitch)
    assert set(np.unique(m[:, :size])) == {0, 2} and not m[:, size:].any()
    # and the specification on the walk's first vertices alone: what they draw is in the mask
    want, _ = ovs.draw(walk[:3000], 1, 2, size * 128, np.zeros((size, size), np.uint8))
    assert want.any() and np.array_equal(m[:, :size] & want, want)


# ---- the host program -------------------------------------------------------------------------------------------------------------------
def test_host_program_overlay(xa, tmp_path):
    """End to end from IQ: an 8-bit image of two segments whose first carries a navigation record and one without such a
    record -> .view.map.ppm for the first, the specification's draw and blend of its toned view, and with --project the
    .geo.view.map.ppm; a line on stderr for the other.  Everything else the run writes is what it writes without the options."""
    import canvas_spec as cs
    import image_spec as isp
    import product_spec as sp
    from test_gpu_canvas import host_capture
    rng = np.random.default_rng(81)
    a, c = cs.samples(rng, 8, 16, 64, 12), cs.samples(rng, 8, 8, 16, 4)
    nav_a = gs.nav_of(230000, -44000, 33, 7, 1, -75.2)
    seg = lambda img, bits, J, ident, key, **kw: (key,) + cs.segment_file(rng, img, bits, J, ident=ident, **kw) + (8190,)
    items = [seg(a[:7], 8, 16, (21, 1, 0, 0, 2, 64, 12), (5, 40), name=b"GOES test/full disk.lrit", extra=[(2, gs.navigation_record(nav_a)[3:])]),
             seg(a[7:], 8, 16, (21, 2, 0, 7, 2, 64, 12), (5, 41), name=b"GOES test/full disk.lrit"),
             seg(c, 8, 8, (23, 1, 0, 0, 1, 16, 4), (5, 43))]
    iq = host_capture(tmp_path, {5: [p for _, p, _ in isp.stream_of(rng, items)]}, 81)
    coast = tmp_path / "coast.txt"
    coast.write_text("> a coast\n-80 -10\n-70 5\n-60.5 20\n\n# an island\n-100 30\n-90 40\n-95 33\n-100 30\n>\n60 0\n70 10\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [os.path.join(root, "xritdemod_amd", "bin", "xrit_demod_host"), "--input", str(iq), "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null",
            "--block", "200000", "--files-decompress", "--canvas", "--canvas-slots", "6", "--canvas-mib", "1", "--products", "--project", "--project-grid",
            "-170:60:3:50:41"]
    runs = {}
    for name, extra in (("plain", []), ("map", ["--overlay", str(coast), "--graticule", "45", "--overlay-width", "2"])):
        r = subprocess.run(base + ["--files", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        runs[name] = ({nm: (tmp_path / name / nm).read_bytes() for nm in os.listdir(tmp_path / name)}, r.stderr)
    (plain, plain_err), (got, err) = runs["plain"], runs["map"]
    maps = {nm for nm in got if ".map." in nm}
    assert maps == {"GOES_test_full_disk.lrit.view.map.ppm", "GOES_test_full_disk.lrit.geo.view.map.ppm"}
    assert not [ln for ln in plain_err.splitlines() if ln.startswith("overlay:")]
    assert {nm: v for nm, v in got.items() if nm not in maps} == plain
    err = err.replace(str(tmp_path / "map"), str(tmp_path / "plain"))                # (the lines name the output directory)
    assert [ln for ln in err.splitlines() if not ln.startswith("overlay:")] == plain_err.splitlines()
    lines = [ln for ln in err.splitlines() if ln.startswith("overlay:")]
    assert len(lines) == 2 and "no image navigation record" in lines[0] and lines[1] == "overlay: 2 views written with the map (2 masks drawn), 1 skipped"
    styles = [(255, 255, 0, 255), (0, 255, 255, 160)] + [(255, 255, 255, 255)] * 6
    layers = [xa.overlay_densify(*ovs.parse_polylines(coast.read_text()), 0.05), xa.overlay_densify(*xa.overlay_graticule(45.0, 1.0), 0.05)]
    # the scan geometry: the library's quads through the specification's point rule
    mask = np.zeros((12, 64), np.uint8)
    for layer, (lon, lat) in enumerate(layers):
        mask, s = ovs.draw(ovs.points_of_quads(xa.overlay_quads(lon, lat, nav_a["sub_lon"]), nav_a), layer, 2, 0, mask)
        assert s["drawn"] > s["outside"]
    want, summary = ovs.blend(sp.process(a.astype(np.uint8), 8, sp.EQUALISE)["tone"], mask, styles, 3)
    assert summary["by_layer"][0] > 5 and summary["by_layer"][1] > 20
    assert got["GOES_test_full_disk.lrit.view.map.ppm"] == b"P6\n64 12\n255\n" + want.tobytes()
    # the grid: the library's grid points, max_jump half the grid's width
    mask = np.zeros((41, 50), np.uint8)
    for layer, (lon, lat) in enumerate(layers):
        p = xa.overlay_grid_points("equirect", 50, 41, -170.0, 60.0, 3.0, 3.0, lon, lat)
        mask, s = ovs.draw(np.stack([p["qx"], p["qy"]], axis=1), layer, 2, 50 * 128, mask)
    assert s["jumps"] == 3                              # the three parallels, where the grid's longitudes wrap
    view = np.frombuffer(got["GOES_test_full_disk.lrit.geo.view.pgm"][len(b"P5\n50 41\n255\n"):], np.uint8).reshape(41, 50)
    want, _ = ovs.blend(view, mask, styles, 3)
    assert got["GOES_test_full_disk.lrit.geo.view.map.ppm"] == b"P6\n50 41\n255\n" + want.tobytes()
