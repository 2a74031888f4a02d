"""CPU tier: the projection stage's specification (tests/geo_spec.py) against an independent statement of the map with
NumPy's trigonometry, symmetries and hand-made sampling cases; the arctangent polynomial against np.arctan; the library's
host helpers (the tables of a grid, the navigation record, the inverse of the map) against NumPy; the CPU side of the ABI;
the rule (csrc/geo_rule.h) in a stand-alone program under the sanitizers, replaying a table recorded from the
specification; the host program's checks of the --project flags."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import geo_spec as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")
TABLE = os.path.join(ROOT, "tests", "golden", "geo_rule_table.txt")
HOST_BIN = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")

FUNCTIONS = ["xrit_geo_create", "xrit_geo_destroy", "xrit_geo_reset", "xrit_geo_grid_tables", "xrit_geo_set_grid", "xrit_geo_set_tables",
             "xrit_geo_tables", "xrit_geo_map_device", "xrit_geo_resample_device", "xrit_geo_project_device", "xrit_geo_project",
             "xrit_geo_project_resident", "xrit_geo_parse_navigation", "xrit_geo_pixel_to_lonlat"]


# ---- the polynomial --------------------------------------------------------------------------------------------------------
def test_polynomial_accuracy():
    t = np.linspace(-0.2, 0.2, 200001)
    err = float(np.abs(gs.atan_small(t) - np.arctan(t)).max())
    print("atan_small against np.arctan on |t| <= 0.2:", err)
    assert err <= 4e-16
    assert gs.atan_small(0.0) == 0.0 and np.array_equal(gs.atan_small(-t), -gs.atan_small(t))


# ---- the map, stated independently -----------------------------------------------------------------------------------------
def independent_map(nav, kind, columns, rows, lon0, lat0, step_lon, step_lat):
    """The map as the CGMS document writes it: x = atan(-r2 / r1), y = asin(-r3 / rn), NumPy's trigonometry throughout."""
    lon, lat = gs.grid_lonlat(kind, columns, rows, lon0, lat0, step_lon, step_lat)
    c_lat = np.arctan(0.993243 * np.tan(lat))[:, None]
    rl = 6356.5838 / np.sqrt(1.0 - 0.00675701 * np.cos(c_lat) ** 2)
    dl = np.deg2rad(lon - nav["sub_lon"])[None, :]
    r1 = 42164.0 - rl * np.cos(c_lat) * np.cos(dl)
    r2 = -rl * np.cos(c_lat) * np.sin(dl)
    r3 = rl * np.sin(c_lat) + 0.0 * dl
    rn = np.sqrt(r1 * r1 + r2 * r2 + r3 * r3)
    vis = 42164.0 * (42164.0 - r1) >= r2 * r2 + 1.006803 * r3 * r3
    x, y = np.rad2deg(np.arctan(-r2 / r1)), np.rad2deg(np.arcsin(-r3 / rn))
    fc = (nav["coff"] - nav["origin"]) + x * nav["cfac"] / 65536.0
    fl = (nav["loff"] - nav["origin"]) + y * nav["lfac"] / 65536.0
    return vis, fc * 256.0, fl * 256.0


@pytest.mark.parametrize("signs", [(1, 1), (-1, -1)], ids=["goes-signs", "msg-signs"])
def test_map_against_the_independent_statement(signs):
    nav = dict(gs.FIXED_NAV, cfac=signs[0] * gs.FIXED_NAV["cfac"], lfac=signs[1] * gs.FIXED_NAV["lfac"])
    qx, qy = gs.map_points(*gs.fixed_tables(), nav)
    vis, sx, sy = independent_map(nav, *gs.FIXED_GRID)
    on = qx != gs.OFF
    # the edge of the disc: the two statements of vis may differ only where they are within rounding of each other
    assert int(on.sum()) == 24069 and np.array_equal(on, vis) and np.array_equal(on, qy != gs.OFF)
    tie = float(np.minimum(np.abs(sx[on] + 0.5 - np.round(sx[on] + 0.5)), np.abs(sy[on] + 0.5 - np.round(sy[on] + 0.5))).min())
    print("visible pixels:", int(on.sum()), "nearest rounding tie:", tie, "of a unit")
    assert np.array_equal(qx[on], np.floor(sx[on] + 0.5).astype(np.int64)) and np.array_equal(qy[on], np.floor(sy[on] + 0.5).astype(np.int64))
    assert qx[on].min() >= 0 and qx[on].max() < 96 * 256 and qy[on].min() >= 0 and qy[on].max() < 80 * 256


def test_sub_satellite_point_and_mirror_symmetry():
    nav = gs.FIXED_NAV
    # a grid whose middle is the sub-satellite point, symmetric about it
    tables = gs.grid_tables(gs.EQUIRECT, 121, 101, nav["sub_lon"] - 60.0, 50.0, 1.0, 1.0, nav["sub_lon"])
    A, B, Cc, S = tables
    # NumPy's tables are mirror images only to rounding: make them exactly so, as the symmetry is the map's, not the tables'
    A, B = (A + A[::-1]) / 2, (B - B[::-1]) / 2
    Cc, S = (Cc + Cc[::-1]) / 2, (S - S[::-1]) / 2
    qx, qy = gs.map_points(A, B, Cc, S, nav)
    assert (qx[50, 60], qy[50, 60]) == ((nav["coff"] - nav["origin"]) * 256, (nav["loff"] - nav["origin"]) * 256)
    on = qx != gs.OFF
    assert on.sum() > 8000 and np.array_equal(on, on[:, ::-1]) and np.array_equal(on, on[::-1])
    cx, cy = 2 * int(qx[50, 60]), 2 * int(qy[50, 60])
    # floor(s + 0.5) is not odd: a mirrored position that is a tie rounds to the same side, one unit off the mirror image
    dx = (qx.astype(np.int64) + qx[:, ::-1] - cx)[on]
    dy = (qy.astype(np.int64) + qy[::-1] - cy)[on]
    assert np.isin(dx, (0, 1)).all() and np.isin(dy, (0, 1)).all() and (dx == 0).mean() > 0.99 and (dy == 0).mean() > 0.99
    assert np.array_equal(qy[on], qy[:, ::-1][on]) and np.array_equal(qx[on], qx[::-1][on])
    # east is to the right and north is up for positive cfac, negative lfac... as the factors' signs say
    assert qx[50, 90] > qx[50, 60] and (qy[20, 60] < qy[50, 60]) == (nav["lfac"] > 0)


def test_a_grid_entirely_off_the_disc():
    nav = gs.FIXED_NAV
    tables = gs.grid_tables(gs.EQUIRECT, 40, 30, nav["sub_lon"] + 100.0, 60.0, 2.0, 2.0, nav["sub_lon"])
    qx, qy = gs.map_points(*tables, nav)
    assert (qx == gs.OFF).all() and (qy == gs.OFF).all()
    out, summary = gs.resample(np.full((80, 96), 200, np.uint8), qx, qy, gs.BILINEAR)
    assert not out.any() and summary == dict(total=1200, off_disc=1200, outside=0, no_data=0, written=0, columns=40, rows=30, width=1, mode=1)


def test_positions_out_of_range_are_off_the_disc():
    A, B, Cc, S = gs.fixed_tables()
    # with int32 factors only coff and loff can carry a position to 2^30 units: here the columns some 20 pixels east of the middle do
    qx, qy = gs.map_points(A, B, Cc, S, gs.nav_of(357469, 297890, (1 << 22) - 20, 41, 0))
    visible = gs.map_points(A, B, Cc, S, gs.FIXED_NAV)[0] != gs.OFF
    on = qx != gs.OFF
    assert 0 < on.sum() < visible.sum() and not (on & ~visible).any() and (np.abs(qx[on].astype(np.int64)) < 1 << 30).all() and qx[on].max() > (1 << 30) - 300
    assert on[81, 4:100].all() and not on[81, 115:].any() and np.array_equal(on, qy != gs.OFF)
    assert (gs.map_points(A, B, Cc, S, gs.nav_of(357469, 297890, 49, -(1 << 23), 1))[0] == gs.OFF).all()
    bad = np.array([np.nan, np.inf, -np.inf, 1e300])
    for k in range(4):
        t = [A[80:84].copy(), B[80:84].copy(), Cc[84:88].copy(), S[84:88].copy()]
        assert (gs.map_points(*t, gs.FIXED_NAV)[0] != gs.OFF).all()
        t[k][1] = bad[k]
        qx, _ = gs.map_points(*t, gs.FIXED_NAV)
        hit = (qx == gs.OFF)
        assert hit[1].all() if k < 2 else hit[:, 1].all()
        assert not np.delete(hit, 1, axis=0 if k < 2 else 1).any()


# ---- the tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,sub_lon", [(gs.FIXED_GRID, -75.2), ((gs.EQUIRECT, 1800, 1800, -165.0, 90.0, 0.1, 0.1), -75.0),
                                          ((gs.MERCATOR, 700, 500, -150.0, 1.4, 0.2, 0.0056), -137.0), ((gs.EQUIRECT, 1, 1, 0.0, 0.0, 1.0, 1.0), 0.0),
                                          ((gs.MERCATOR, 16384, 3, -180.0, 3.0, 360.0 / 16384, 3.0), 140.7)])
def test_table_accuracy(grid, sub_lon):
    import xritdemod_amd as xa
    got = xa.geo_grid_tables(*grid, sub_lon)
    want = gs.grid_tables(*grid, sub_lon)
    err = [float(np.abs(g - w).max()) for g, w in zip(got, want)]
    print("max |dA|, |dB| in km, |dC|, |dS|:", err)
    assert all(g.shape == w.shape and g.dtype == np.float64 for g, w in zip(got, want))
    assert err[0] <= 1e-9 and err[1] <= 1e-9 and err[2] <= 1e-12 and err[3] <= 1e-12
    assert 6356.0 < want[0].max() <= 6378.2 and np.abs(want[2]).max() <= 1.0


def test_grid_tables_refuses_bad_grids():
    import xritdemod_amd as xa
    for grid in ((2, 4, 4, 0, 0, 1, 1), (0, 0, 4, 0, 0, 1, 1), (0, 4, 0, 0, 0, 1, 1), (0, 16385, 4, 0, 0, 1, 1), (1, 4, 16385, 0, 0, 1, 1)):
        with pytest.raises(xa.XritError) as ei:
            xa.geo_grid_tables(*grid, 0.0)
        assert ei.value.code == -1


# ---- sampling by hand --------------------------------------------------------------------------------------------------------
def one(img, qx, qy, mode):
    out, cls = gs.classify_and_sample(np.asarray(img), np.array([[qx]]), np.array([[qy]]), mode)
    return int(out[0, 0]), int(cls[0, 0])


def test_bilinear_rule_by_hand():
    img = np.array([[10, 20], [30, 40]], np.uint8)
    B, N = gs.BILINEAR, gs.NEAREST
    # all four taps: fx = 64, fy = 128: weights 192*128, 64*128, 192*128, 64*128 of 65536
    v, w = 192 * 128 * 10 + 64 * 128 * 20 + 192 * 128 * 30 + 64 * 128 * 40, 65536
    assert one(img, 64, 128, B) == ((2 * v + w) // (2 * w), gs.WRITTEN) == (23, gs.WRITTEN)
    assert one(img, 0, 0, B) == (10, gs.WRITTEN) and one(img, 256, 256, B) == (40, gs.WRITTEN)
    # one tap kept: its value whatever its weight
    holes = np.array([[0, 0], [0, 40]], np.uint8)
    assert one(holes, 1, 1, B) == (40, gs.WRITTEN) and one(holes, 255, 255, B) == (40, gs.WRITTEN)
    # W = 0: no tap with data, or the only one with data has weight 0
    assert one(holes, 0, 0, B) == (0, gs.NO_DATA) and one(holes, 255, 0, B) == (0, gs.NO_DATA) and one(np.zeros((2, 2), np.uint8), 100, 100, B) == (0, gs.NO_DATA)
    # a tap off each edge: the ones inside carry the mean
    assert one(img, -128, 0, B) == (10, gs.WRITTEN) and one(img, 0, -128, B) == (10, gs.WRITTEN)
    assert one(img, 256 + 128, 0, B) == (20, gs.WRITTEN) and one(img, 0, 256 + 128, B) == (30, gs.WRITTEN)
    assert one(img, -128, 128, B) == (20, gs.WRITTEN)                           # (10 + 30) / 2
    assert one(img, -256, 0, B) == (0, gs.NO_DATA)                              # the tap inside has weight 0
    assert one(img, -257, 0, B) == (0, gs.OUTSIDE) and one(img, 512, 0, B) == (0, gs.OUTSIDE) and one(img, 0, -257, B) == (0, gs.OUTSIDE)
    assert one(img, gs.OFF, gs.OFF, B) == (0, gs.OFF_DISC) and one(img, gs.OFF, gs.OFF, N) == (0, gs.OFF_DISC)
    # halves round up, and data never becomes 0
    assert one(np.array([[1, 2]], np.uint8), 128, 0, B) == (2, gs.WRITTEN) and one(np.array([[1, 0]], np.uint8), 255, 0, B) == (1, gs.WRITTEN)
    # 16-bit maxima: V near 2^32
    top = np.full((2, 2), 65535, np.uint16)
    assert one(top, 77, 200, B) == (65535, gs.WRITTEN)
    top[1, 1] = 65534
    assert one(top, 128, 128, B) == ((2 * (3 * 16384 * 65535 + 16384 * 65534) + 65536) // 131072, gs.WRITTEN) == (65535, gs.WRITTEN)
    assert one(top, 255, 255, B) == (65534, gs.WRITTEN)
    # nearest: halves go to the next sample
    assert one(img, 127, 0, N) == (10, gs.WRITTEN) and one(img, 128, 0, N) == (20, gs.WRITTEN) and one(img, -128, 0, N) == (10, gs.WRITTEN)
    assert one(img, -129, 0, N) == (0, gs.OUTSIDE) and one(img, 256 + 127, 256 + 127, N) == (40, gs.WRITTEN) and one(img, 256 + 128, 0, N) == (0, gs.OUTSIDE)
    assert one(holes, 0, 0, N) == (0, gs.NO_DATA)


def test_missing_rows_do_not_darken_their_neighbours():
    img = np.full((6, 6), 200, np.uint8)
    img[2:4] = 0
    qx, qy = np.meshgrid(np.arange(0, 5 * 256, 37), np.arange(0, 5 * 256, 37))
    out, summary = gs.resample(img, qx, qy, gs.BILINEAR)
    assert set(np.unique(out)) == {0, 200} and summary["no_data"] == int((out == 0).sum()) > 0 and summary["written"] + summary["no_data"] == out.size


# ---- the host helpers ------------------------------------------------------------------------------------------------------
def test_parse_navigation():
    import xritdemod_amd as xa
    nav = gs.nav_of(-781648343, -781648343, 1856, 1856, 1, 9.5)
    others = [bytes([1, 0, 9, 10, 0x0E, 0x80, 0x0E, 0x80, 0]), bytes([4, 0, 10]) + b"name.lr", bytes([128, 0, 17]) + bytes(14)]
    rec = gs.navigation_record(nav)
    good = gs.header_of(others + [rec] + [bytes([5, 0, 10]) + bytes(7)]) + b"data behind the header"
    got = xa.geo_parse_navigation(good)
    assert {k: got[k2].item() for k, k2 in zip(("cfac", "lfac", "coff", "loff", "origin", "sub_lon"),
                                                ("cfac", "lfac", "coff", "loff", "origin", "sub_lon_deg"))} == nav == gs.parse_navigation(good)
    for name, lon in ((b"GEOS(-75.2)", -75.2), (b"geos(0)", 0.0), (b"GEOS(+137)", 137.0), (b"GEOS(-135.0)   ", -135.0)):
        h = gs.header_of([gs.navigation_record(nav, name)])
        assert xa.geo_parse_navigation(h)["sub_lon_deg"] == lon == gs.parse_navigation(h)["sub_lon"]
    # the first record of type 2 and length 51 is the one
    second = gs.header_of([rec, gs.navigation_record(gs.nav_of(1, 2, 3, 4, 1, 0.0))])
    assert xa.geo_parse_navigation(second)["cfac"] == nav["cfac"]
    wrong_length = bytes([2, 0, 50]) + rec[3:50]
    bad = {"no header": b"", "no navigation record": gs.header_of(others), "a wrong length": gs.header_of(others + [wrong_length]),
           "a truncated header": good[:16 + sum(map(len, others)) + 20], "a truncated primary header": good[:15],
           "not a primary header": bytes([1]) + good[1:], "a non-GEOS name": gs.header_of([gs.navigation_record(nav, b"MERCATOR(9.5)")]),
           "a name without a number": gs.header_of([gs.navigation_record(nav, b"GEOS()")]),
           "a name without a bracket": gs.header_of([gs.navigation_record(nav, b"GEOS(9.5")]),
           "a name with text": gs.header_of([gs.navigation_record(nav, b"GEOS(east)")]),
           "a number and text": gs.header_of([gs.navigation_record(nav, b"GEOS(9.5E)")]),
           "a longitude out of range": gs.header_of([gs.navigation_record(nav, b"GEOS(400)")])}
    for what, h in bad.items():
        assert gs.parse_navigation(h) is None, what
        with pytest.raises(xa.XritError) as ei:
            xa.geo_parse_navigation(h)
        assert ei.value.code == -1, what


def test_pixel_to_lonlat_inverts_the_map():
    import xritdemod_amd as xa
    worst = 0.0
    for nav in (gs.FIXED_NAV, dict(gs.FIXED_NAV, cfac=-357469, lfac=-297890)):
        # the disc's radii in pixels: the earth's angular radii, 8.70 and 8.67 degrees, times the factors
        rx, ry = 8.70 * abs(nav["cfac"]) / 65536.0, 8.67 * abs(nav["lfac"]) / 65536.0
        inside = 0
        for line in np.arange(1, 81, 2.5):
            for column in np.arange(1, 97, 2.5):
                rho = np.hypot((column - nav["coff"]) / rx, (line - nav["loff"]) / ry)
                got = xa.geo_pixel_to_lonlat(nav, column, line)
                want = gs.pixel_to_lonlat(nav, column, line)
                assert (got is None) == (want is None)
                if rho <= 0.95:
                    assert got is not None and abs(got[0] - want[0]) < 1e-9 and abs(got[1] - want[1]) < 1e-9
                    back = gs.forward(nav, *got)
                    worst = max(worst, abs(back[0] - column), abs(back[1] - line))
                    inside += 1
                if rho >= 1.02:
                    assert got is None
        assert inside > 400
        for column, line in ((1, 1), (96, 1), (1, 80), (96, 80)):
            assert xa.geo_pixel_to_lonlat(nav, column, line) is None
    print("forward(inverse(column, line)) inside 0.95 of the radius: worst", worst, "pixel")
    assert worst <= 1e-6
    lon, lat = xa.geo_pixel_to_lonlat(gs.FIXED_NAV, 49, 41)
    assert lon == -75.2 and lat == 0.0
    east = xa.geo_pixel_to_lonlat(gs.FIXED_NAV, 60, 30)
    assert east[0] > -75.2 and (east[1] > 0) == (gs.FIXED_NAV["lfac"] > 0)
    with pytest.raises(xa.XritError):
        xa.geo_pixel_to_lonlat(gs.nav_of(0, 1, 0, 0), 1, 1)


# ---- the ABI's CPU side ------------------------------------------------------------------------------------------------------
def test_symbols_and_layouts():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(xrit_[a-z0-9_]+)\s*\(", src))
    import xritdemod_amd as xa
    from xritdemod_amd import _capi
    L = xa.lib()
    for name in FUNCTIONS:
        assert name in declared and name in _capi._SIGNATURES and hasattr(L, name), name
    assert {n for n in declared if n.startswith("xrit_geo_")} == set(FUNCTIONS)
    np_of = {"uint64_t": np.uint64, "uint32_t": np.uint32, "int32_t": np.int32, "double": np.float64}
    for struct, dtype, size in (("xrit_geo_nav", xa.GEO_NAV_DTYPE, 32), ("xrit_geo_grid", xa.GEO_GRID_DTYPE, 48), ("xrit_geo_point", xa.GEO_POINT_DTYPE, 8),
                                ("xrit_geo_summary", xa.GEO_SUMMARY_DTYPE, 56)):
        m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + r";\s*/\* (\d+) bytes", text, re.S)
        fields = []
        for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
            if decl.strip():
                ctype, names = decl.strip().split(None, 1)
                fields += [(nm.strip(), np_of[ctype]) for nm in names.split(",")]
        assert int(m.group(2)) == size == dtype.itemsize and dtype == np.dtype(fields, align=True), struct
    assert tuple(xa.GEO_SUMMARY_DTYPE.names) == gs.SUMMARY_FIELDS
    for name, value in (("EQUIRECT", gs.EQUIRECT), ("MERCATOR", gs.MERCATOR), ("NEAREST", gs.NEAREST), ("BILINEAR", gs.BILINEAR), ("MAX_DIM", gs.MAX_DIM)):
        assert re.search(r"#define XRIT_GEO_" + name + r"\s+" + str(value) + r"\b", text) and getattr(xa, "GEO_" + name) == value
    assert xa.GEO_OFF == gs.OFF == -2 ** 31 and xa.GEO_MODES == tuple(gs.MODES)


def test_bad_arguments_are_refused_before_a_device_is_asked_for():
    import xritdemod_amd as xa
    L = xa.lib()
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.xrit_geo_create(None, 0) == -1 and L.xrit_geo_reset(None) == -1 and L.xrit_geo_destroy(None) == 0
    assert L.xrit_geo_set_grid(None, p, 0.0) == -1 and L.xrit_geo_set_tables(None, 4, 4, p, p, p, p) == -1
    assert L.xrit_geo_tables(None, p, p, p, p, p, p) == -1 and L.xrit_geo_map_device(None, p, p, None) == -1
    assert L.xrit_geo_resample_device(None, p, p, 0, p, 64, p, None) == -1 and L.xrit_geo_project_device(None, p, p, 0, p, 64, p, None) == -1
    assert L.xrit_geo_project(None, p, p, 0, p, 64, p) == -1 and L.xrit_geo_project_resident(None, p, p, 0, p, 64, p) == -1
    assert L.xrit_geo_parse_navigation(None, 0, p) == -1 and L.xrit_geo_pixel_to_lonlat(None, 0.0, 0.0, p, p) == -1
    assert L.xrit_geo_grid_tables(None, 0.0, p, p, p, p) == -1


def test_no_cpu_path():
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:                   # on a GPU box the same call makes a working object (-m gpu tests it)
        xa.ImageProjector().close()
        return
    with pytest.raises(xa.XritError) as ei:
        xa.ImageProjector()
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)


# ---- the rule under the sanitizers ---------------------------------------------------------------------------------------------
def test_recorded_table_is_the_specification_s():
    want = gs.rule_table_text()
    assert open(TABLE).read() == want
    rows = [ln.split() for ln in want.splitlines()]
    assert {r[0] for r in rows} == {"0", "1", "2", "3", "4"}
    points = [r for r in rows if r[0] == "1"]
    off = sum(r[5] == str(gs.OFF) for r in points)
    assert len(points) > 250 and 0.2 < off / len(points) < 0.8 and all((r[5] == str(gs.OFF)) == (r[6] == str(gs.OFF)) for r in points)
    samples = [r for r in rows if r[0] == "3"]
    assert {(r[3], r[5]) for r in samples} == {(str(m), str(c)) for m in (0, 1) for c in (0, 1, 2, 3)} and max(int(r[4]) for r in samples) == 65535


def test_geo_rule_host_check_under_sanitizers(tmp_path):
    """make geo-host-check: the functions of csrc/geo_rule.h that the kernels call, replayed over the recorded table in a
    stand-alone g++ program with -ffp-contract=off -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "geo-host-check", f"GEO_CHECK={tmp_path / 'geo_host_check'}"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "-ffp-contract=off" in r.stdout and "-fsanitize=address,undefined" in r.stdout
    lines = open(TABLE).read().splitlines()
    n1, n3 = (sum(ln.startswith(k) for ln in lines) for k in ("1 ", "3 "))
    assert f"geo_host_check: {len(lines)} rows, {n1} map entries, {n3} samples, every one the specification's: ok" in r.stdout, r.stdout


# ---- the host program's flags ------------------------------------------------------------------------------------------------
CANVAS = ["--input", "nowhere.cf32", "--files", "nowhere", "--files-decompress", "--canvas"]


@pytest.mark.parametrize("args,says", [
    (["--input", "nowhere.cf32", "--project"], "--project needs --canvas"),
    (["--input", "nowhere.cf32", "--files", "nowhere", "--files-decompress", "--project"], "--project needs --canvas"),
    (CANVAS + ["--project-mode", "nearest"], "need --project"),
    (CANVAS + ["--project-grid", "-160:81:1:171:163"], "need --project"),
    (CANVAS + ["--project", "--project-mode", "cubic"], "--project-mode cubic: nearest or bilinear"),
    (CANVAS + ["--project", "--project-mode"], "--project-mode needs a value"),
    (CANVAS + ["--project", "--project-grid"], "--project-grid needs a value"),
    (CANVAS + ["--project", "--project-grid", "-160:81:1:171"], "--project-grid -160:81:1:171:"),
    (CANVAS + ["--project", "--project-grid", "-160:81:0:171:163"], "--project-grid -160:81:0:171:163:"),
    (CANVAS + ["--project", "--project-grid", "-160:81:1:0:163"], "--project-grid -160:81:1:0:163:"),
    (CANVAS + ["--project", "--project-grid", "-160:81:1:171:16385"], "--project-grid -160:81:1:171:16385:"),
    (CANVAS + ["--project", "--project-grid", "-160:91:1:171:163"], "--project-grid -160:91:1:171:163:"),
    (CANVAS + ["--project", "--project-grid", "-160:81:1:171:163x"], "--project-grid -160:81:1:171:163x:"),
])
def test_host_program_refuses_bad_project_flags(args, says):
    r = subprocess.run([HOST_BIN] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and says in r.stderr.splitlines()[0], r.stderr[:300]


@pytest.mark.parametrize("args", [["--project"], ["--project", "--project-mode", "nearest"], ["--project", "--project-grid", "-160.2:81:1:171:163"],
                                  ["--project", "--products", "--project-mode", "bilinear", "--project-grid", "0:0:0.01:16384:1"]])
def test_host_program_accepts_good_project_flags(args, tmp_path):
    """Past the flags, the run ends at the input file that is not there (at the device that is not there, without one)."""
    at = ["--input", str(tmp_path / "nowhere.cf32"), "--files", str(tmp_path / "out"), "--files-decompress", "--canvas"]
    r = subprocess.run([HOST_BIN] + at + args, capture_output=True, text=True, timeout=60)
    assert "usage:" not in r.stderr and r.returncode == 1 and ("nowhere.cf32" in r.stderr or "no CPU path" in r.stderr), r.stderr[:300]
