"""CPU tier of the map overlay stage: the specification of tests/overlay_spec.py against itself
(a segment's pixels do not depend on the order of its ends, are 8-connected, drawing is idempotent and two calls equal one
on the concatenation) and against an outside yardstick (Pillow's ImageDraw.line within Chebyshev distance 1, both ways);
the host helpers of the library against NumPy's trigonometry; densify and the graticule; the recorded table, and its
replay through csrc/overlay_rule.h under the sanitizers (make overlay-host-check); the ABI without a device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import geo_spec as gs
import overlay_spec as ovs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")
TABLE = os.path.join(ROOT, "tests", "golden", "overlay_rule_table.txt")

FUNCTIONS = ["xrit_overlay_create", "xrit_overlay_destroy", "xrit_overlay_reset", "xrit_overlay_set_form", "xrit_overlay_map_device",
             "xrit_overlay_draw_device", "xrit_overlay_blend_device", "xrit_overlay_map", "xrit_overlay_draw", "xrit_overlay_blend",
             "xrit_overlay_blend_resident", "xrit_overlay_mask_device", "xrit_overlay_quads", "xrit_overlay_grid_points", "xrit_overlay_densify", "xrit_overlay_graticule"]


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    return xritdemod_amd


def random_segments(rng, count, size):
    """Ends in 1/256 pixel from sub-pixel apart to longer than the image, some of them outside it."""
    p0 = rng.integers(-40 * 256, (size + 40) * 256, (count, 2))
    reach = 256 * np.array([0.3, 2, 10, 2 * size])[rng.integers(0, 4, count)]
    p1 = p0 + (rng.uniform(-1, 1, (count, 2)) * reach[:, None]).astype(np.int64)
    return p0, p1


def connected(pixels):
    """8-connected: every pixel reached from the first through neighbours in the set."""
    if not pixels:
        return True
    todo, seen = [next(iter(pixels))], set()
    while todo:
        x, y = todo.pop()
        if (x, y) in seen:
            continue
        seen.add((x, y))
        todo += [(x + dx, y + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (x + dx, y + dy) in pixels and (x + dx, y + dy) not in seen]
    return len(seen) == len(pixels)


# ---- the specification against itself ------------------------------------------------------------------------------------------
def test_a_segment_is_the_same_from_either_end_and_connected():
    rng = np.random.default_rng(1)
    size = 64
    p0, p1 = random_segments(rng, 3000, size)
    disconnected = 0
    for a, b in zip(p0, p1):
        # (an image large enough that nothing is cut: connectedness is a property of the whole line)
        shift = np.array([60 * 256, 60 * 256]) + 2 * size * 256
        fwd = ovs.segment_pixels(a + shift, b + shift, 5 * size + 120, 5 * size + 120)
        assert fwd == ovs.segment_pixels(b + shift, a + shift, 5 * size + 120, 5 * size + 120)
        disconnected += not connected(fwd)
        assert ((int(a[0] + shift[0]) + 128) >> 8, (int(a[1] + shift[1]) + 128) >> 8) in fwd
    assert disconnected == 0


def test_the_cut_of_the_range_changes_no_pixel_inside_the_image():
    rng = np.random.default_rng(2)
    p0, p1 = random_segments(rng, 400, 48)
    for width in (1, 2, 3, 8):
        for a, b in zip(p0[:100 * width], p1[:100 * width]):
            small, _ = ovs.draw([a, b], 0, width, 0, np.zeros((48, 48), np.uint8))
            off = 200 * 256
            large, _ = ovs.draw([a + off, b + off], 0, width, 0, np.zeros((448, 448), np.uint8))
            assert np.array_equal(small, large[200:248, 200:248])


def test_drawing_is_idempotent_and_two_calls_equal_one_on_the_concatenation():
    rng = np.random.default_rng(3)
    a = rng.integers(-2000, 70 * 256, (40, 2))
    b = rng.integers(-2000, 70 * 256, (25, 2))
    a[7] = b[3] = (ovs.BREAK, ovs.BREAK)
    zero = np.zeros((50, 70), np.uint8)
    once, s1 = ovs.draw(a, 2, 2, 0, zero)
    twice, s2 = ovs.draw(a, 2, 2, 0, once)
    assert np.array_equal(once, twice) and s1 == s2 and set(np.unique(once)) == {0, 4}
    both, _ = ovs.draw(b, 2, 2, 0, once)
    joined, sj = ovs.draw(np.concatenate([a, [[ovs.BREAK, ovs.BREAK]], b]), 2, 2, 0, zero)
    assert np.array_equal(both, joined)
    assert sj["hidden"] == s1["hidden"] + 2 + 2 and sj["segments"] + sj["hidden"] == sj["vertices"] - 1
    cleared, _ = ovs.draw(b, 5, 1, 0, once, clear=True)
    assert set(np.unique(cleared)) == {0, 32}


def test_summary_counts_of_a_known_list():
    pts = [(0, 0), (2560, 0), (ovs.BREAK, ovs.BREAK), (ovs.BREAK, ovs.BREAK), (ovs.LIMIT, 0), (0, 0), (0, 30000), (-5000, -5000), (-4000, -5000),
           (ovs.LIMIT - 1, ovs.LIMIT - 1)]
    mask, s = ovs.draw(pts, 0, 1, 32000, np.zeros((20, 30), np.uint8))
    # pairs: drawn (11 steps + 2), hidden x4 (two breaks, the vertex at 2^29), jump, drawn through the image, drawn outside, jump
    assert s == dict(vertices=10, segments=5, hidden=4, jumps=2, outside=1, drawn=3, steps=(2 + 11) + (2 + 20) + (2 + 0), layer=0, width=1)
    assert mask[0, :11].all() and not mask[0, 11:].any()


def test_the_line_is_pillows_within_one_pixel():
    """Ends on pixel centres: every pixel of the width-1 line within Chebyshev distance 1 of Pillow's, and the reverse.  (Not
    identity: the two round exact ties differently.)"""
    Image = pytest.importorskip("PIL.Image")
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    rng = np.random.default_rng(4)
    ends = rng.integers(0, 64, (2000, 4))

    def grown(m):
        g = np.zeros((66, 66), bool)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                g[dy:dy + 64, dx:dx + 64] |= m
        return g[1:65, 1:65]

    same = 0
    for x0, y0, x1, y1 in ends.tolist():
        im = Image.new("L", (64, 64), 0)
        ImageDraw.Draw(im).line([(x0, y0), (x1, y1)], fill=255, width=1)
        theirs = np.asarray(im) != 0
        ours = ovs.draw([(x0 * 256, y0 * 256), (x1 * 256, y1 * 256)], 0, 1, 0, np.zeros((64, 64), np.uint8))[0] != 0
        assert not (ours & ~grown(theirs)).any() and not (theirs & ~grown(ours)).any(), (x0, y0, x1, y1)
        same += np.array_equal(ours, theirs)
    assert same > 1000


def test_blend_of_the_specification():
    styles = [(255, 0, 0, 255), (0, 255, 0, 128), (0, 0, 255, 0)] + [(9, 9, 9, 9)] * 5
    img = np.array([[10, 20, 30, 40]], np.uint8)
    mask = np.array([[0, 1, 2, 7]], np.uint8)
    out, s = ovs.blend(img, mask, styles, 3)
    assert out.tolist() == [[[10, 10, 10], [255, 0, 0], [(30 * 127 + 127) // 255, (30 * 127 + 255 * 128 + 127) // 255, (30 * 127 + 127) // 255],
                             [40, 40, 40]]]
    assert s["covered"] == 3 and s["by_layer"] == [1, 1, 1, 0, 0, 0, 0, 0] and s["pixels"] == 4
    grey, _ = ovs.blend(img, mask, styles, 1)
    assert grey.tolist() == [[10, ovs.luma(255, 0, 0), ovs.mix(30, ovs.luma(0, 255, 0), 128), 40]]


# ---- the host helpers ----------------------------------------------------------------------------------------------------------
def vertices(rng, n):
    lon, lat = rng.uniform(-180, 180, n), rng.uniform(-89.5, 89.5, n)
    lon[::17] = np.nan
    lat[5::29] = np.nan
    return lon, lat


def test_quads_match_numpy_and_map_like_a_grid(xa):
    rng = np.random.default_rng(5)
    lon, lat = vertices(rng, 500)
    got, want = xa.overlay_quads(lon, lat, -75.2), ovs.quads(lon, lat, -75.2)
    brk = np.isnan(lon) | np.isnan(lat)
    assert np.isnan(got[brk]).all() and not np.isnan(got[~brk]).any()
    assert (np.abs(got[~brk] - want[~brk]) <= 1e-9 * np.abs(want[~brk])).all()
    # the quads of a grid's nodes are its tables' entries: the same formulas
    grid = (gs.EQUIRECT, 9, 7, -120.0, 60.0, 10.0, 20.0)
    A, B, C_, S = xa.geo_grid_tables(*grid, -75.2)
    glon, glat = gs.grid_lonlat(*grid)
    q = xa.overlay_quads(np.tile(glon, 7), np.repeat(np.rad2deg(glat), 9), -75.2).reshape(7, 9, 4)
    for k, t in enumerate((A[:, None], B[:, None], C_[None, :], S[None, :])):
        assert (np.abs(q[:, :, k] - t) <= 1e-12 * np.maximum(np.abs(t), 1.0)).all()
    # and through the specification's point rule they land where geo_spec.forward puts the vertex
    pts = ovs.points_of_quads(xa.overlay_quads([-75.2, -60.0, 100.0], [0.0, 30.0, 0.0], -75.2), gs.FIXED_NAV)
    assert tuple(pts[2]) == (ovs.BREAK, ovs.BREAK)
    for p, (lo, la) in zip(pts[:2], ((-75.2, 0.0), (-60.0, 30.0))):
        c, l = gs.forward(gs.FIXED_NAV, lo, la)
        assert abs(p[0] / 256 - (c - 1)) < 0.02 and abs(p[1] / 256 - (l - 1)) < 0.02


@pytest.mark.parametrize("kind", [gs.EQUIRECT, gs.MERCATOR])
def test_grid_points_match_numpy_within_one_unit(xa, kind):
    rng = np.random.default_rng(6)
    lon, lat = vertices(rng, 500)
    grid = (kind, 400, 300, -160.0, 1.3 if kind == gs.MERCATOR else 75.0, 0.4, 0.009 if kind == gs.MERCATOR else 0.5)
    got = xa.overlay_grid_points(*grid, lon, lat)
    x, y = ovs.grid_positions(kind, *grid[3:], lon, lat)
    brk = np.isnan(lon) | np.isnan(lat)
    assert (got["qx"][brk] == ovs.BREAK).all() and (got["qy"][brk] == ovs.BREAK).all() and (got["qx"][~brk] != ovs.BREAK).all()
    assert (np.abs(got["qx"][~brk] - np.floor(x[~brk] * 256 + 0.5)) <= 1).all() and (np.abs(got["qy"][~brk] - np.floor(y[~brk] * 256 + 0.5)) <= 1).all()
    # longitudes wrap into [lon0 - 180, lon0 + 180); a position that does not fit 2^29 is a break
    p = xa.overlay_grid_points(kind, 400, 300, -160.0, 0.0, 0.4, 1e-9, [-160.0, 200.0, 19.99, 20.0, 0.0], [0.0, 0.0, 0.0, 0.0, 45.0])
    assert p["qx"][:4].tolist() == [0, 0, int(np.floor(179.99 / 0.4 * 256 + 0.5)), -115200] and tuple(p[4]) == (ovs.BREAK, ovs.BREAK)


def test_densify_counts_and_breaks(xa):
    lon = np.array([0.0, 1.0, np.nan, 5.0, 5.02, 5.02, -170.0, np.nan, np.nan, 3.0])
    lat = np.array([0.0, 0.2, 1.0, 5.0, 5.0, 7.0, 80.0, 0.0, np.nan, np.nan])
    got_lon, got_lat = xa.overlay_densify(lon, lat, 0.05)
    want_lon, want_lat = ovs.densify(lon, lat, 0.05)
    assert np.array_equal(got_lon, want_lon, equal_nan=True) and np.array_equal(got_lat, want_lat, equal_nan=True)
    # the first vertex, 20 parts, a break, a vertex, 1 part, 40 parts, 3501 parts, three breaks (one of them a NaN latitude alone)
    assert len(got_lon) == 1 + 20 + 1 + 1 + 1 + 40 + 3501 + 3
    assert np.isnan(got_lon).sum() == 4 and np.array_equal(np.isnan(got_lon), np.isnan(got_lat))
    keep = ~np.isnan(got_lon)
    step = np.maximum(np.abs(np.diff(got_lon)), np.abs(np.diff(got_lat)))[keep[1:] & keep[:-1]]
    assert step.max() <= 0.05 * (1 + 1e-9)
    out = np.full((2, 10), -7.0)
    import ctypes as C
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n_out = C.c_size_t()
    rc = xa.lib().xrit_overlay_densify(p(lon), p(lat), len(lon), 0.05, p(out[0]), p(out[1]), 10, C.byref(n_out))
    assert rc == -5 and n_out.value == len(got_lon) and np.array_equal(out[0], got_lon[:10])
    for bad in (0.0, -1.0, float("nan")):
        assert xa.lib().xrit_overlay_densify(p(lon), p(lat), len(lon), bad, p(out[0]), p(out[1]), 10, C.byref(n_out)) == -1
    assert xa.lib().xrit_overlay_densify(p(np.array([0.0, 1e300])), p(np.array([0.0, 0.0])), 2, 0.05, p(out[0]), p(out[1]), 10, C.byref(n_out)) == -1


@pytest.mark.parametrize("step,vstep", [(10.0, 1.0), (30.0, 0.7), (90.0, 90.0)])
def test_graticule_lines_and_breaks(xa, step, vstep):
    lon, lat = xa.overlay_graticule(step, vstep)
    n_mer, v_mer, n_par, v_par = ovs.graticule_counts(step, vstep)
    assert len(lon) == n_mer * (v_mer + 1) + n_par * (v_par + 1)
    brk = np.isnan(lon)
    assert np.array_equal(brk, np.isnan(lat)) and brk.sum() == n_mer + n_par
    mer_lon, mer_lat = lon[:n_mer * (v_mer + 1)].reshape(n_mer, v_mer + 1), lat[:n_mer * (v_mer + 1)].reshape(n_mer, v_mer + 1)
    assert np.isnan(mer_lon[:, -1]).all() and np.array_equal(mer_lon[:, 0], -180.0 + step * np.arange(n_mer))
    assert (mer_lon[:, :-1] == mer_lon[:, :1]).all() and (mer_lat[:, 0] == -90.0).all() and (mer_lat[:, -2] == 90.0).all()
    assert (np.diff(mer_lat[:, :-1], axis=1) > 0).all() and np.diff(mer_lat[:, :-1], axis=1).max() <= vstep * (1 + 1e-9)
    par_lon, par_lat = lon[n_mer * (v_mer + 1):].reshape(n_par, v_par + 1), lat[n_mer * (v_mer + 1):].reshape(n_par, v_par + 1)
    assert np.array_equal(par_lat[:, 0], -90.0 + step * np.arange(1, n_par + 1)) and (np.abs(par_lat[:, :-1]) < 90.0).all()
    assert (par_lon[:, 0] == -180.0).all() and (par_lon[:, -2] == 180.0).all() and (np.diff(par_lon[:, :-1], axis=1) > 0).all()


def test_graticule_refuses_bad_steps(xa):
    for step, vstep in ((0.0, 0.0), (0.05, 0.01), (91.0, 1.0), (10.0, 11.0), (10.0, 0.0), (float("nan"), 1.0), (0.1, 0.001), (1.0, 0.001)):
        with pytest.raises(xa.XritError) as ei:
            xa.overlay_graticule(step, vstep)
        assert ei.value.code == -1


# ---- the rule under the sanitizers -----------------------------------------------------------------------------------------------
def test_recorded_table_is_the_specification_s():
    want = ovs.rule_table_text()
    assert open(TABLE).read() == want
    rows = [ln.split() for ln in want.splitlines()]
    assert {r[0] for r in rows} == {"0", "1", "2", "3", "4", "5", "6", "7"}
    pairs = [r for r in rows if r[0] == "1"]
    assert {r[5] for r in pairs} == {"0", "1", "2"} and {r[6] for r in pairs if r[5] == "2"} == {"0", "1"}
    assert {r[14] for r in pairs if r[5] == "2"} == {"0", "1"}                   # drawn segments that touch and that do not
    assert {int(r[3]) for r in rows if r[0] == "4"} == {0, 1, 127, 128, 254, 255}
    stamps = [r for r in rows if r[0] == "3"]
    assert {r[3] for r in stamps} == {"0", "1"}


def test_overlay_rule_host_check_under_sanitizers(tmp_path):
    """make overlay-host-check: the functions of csrc/overlay_rule.h that the kernels call, replayed over the recorded table
    in a stand-alone g++ program with -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "overlay-host-check",
                        f"OVERLAY_CHECK={tmp_path / 'overlay_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "-fsanitize=address,undefined" in r.stdout
    lines = open(TABLE).read().splitlines()
    n1, n2, n3 = (sum(ln.startswith(k) for ln in lines) for k in ("1 ", "2 ", "3 "))
    assert f"overlay_host_check: {len(lines)} rows, {n1} pairs, {n2} steps, {n3} stamps, every one the specification's: ok" in r.stdout, r.stdout


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_stage_and_the_library_exports_it(xa):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(xrit_overlay_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(FUNCTIONS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", xa.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in FUNCTIONS if f not in exported]
    assert xa.OVERLAY_DRAW_SUMMARY_DTYPE.names == ovs.DRAW_FIELDS and xa.OVERLAY_BLEND_SUMMARY_DTYPE.names == ovs.BLEND_FIELDS
    assert (xa.OVERLAY_BREAK, xa.OVERLAY_LIMIT, xa.OVERLAY_MAX_DIM, xa.OVERLAY_MAX_WIDTH, xa.OVERLAY_LAYERS, xa.OVERLAY_MAX_VERTICES) == \
        (ovs.BREAK, ovs.LIMIT, ovs.MAX_DIM, ovs.MAX_WIDTH, ovs.LAYERS, ovs.MAX_VERTICES)


def test_no_device_no_overlay(xa):
    if xa.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(xa.XritError) as ei:
        xa.MapOverlay()
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)
