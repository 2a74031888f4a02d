"""The projection stage's specification in NumPy (include/xritdemod_amd.h, "Image projection"): what
xrit_geo_* computes -- the four tables of a grid, the map entry (qx, qy) of every output pixel, the output image of both
sampling modes and the summary.  Per pixel there is only + - * / sqrt floor on float64 arrays, one ufunc per operation in
the order the header writes them (NumPy fuses nothing), and the arctangent polynomial; the device equals every array and
every summary field exactly when it is given the same tables.  An image here is a 2-D array of samples (uint8 for
bits <= 8, uint16 above): pitch and padding are the device interface's business."""
import struct

import numpy as np

H = 42164.0
RPOL = 6356.5838
FLAT = 0.993243
E2 = 0.00675701
K = 1.006803
R2D = 57.29577951308232
LIMIT = 1073741824.0                                # 2^30
OFF = -(1 << 31)                                    # INT32_MIN
EQUIRECT, MERCATOR = 0, 1
NEAREST, BILINEAR = 0, 1
MODES = {"nearest": NEAREST, "bilinear": BILINEAR}
MAX_DIM = 16384
SUMMARY_FIELDS = ("total", "off_disc", "outside", "no_data", "written", "columns", "rows", "width", "mode")
OFF_DISC, OUTSIDE, NO_DATA, WRITTEN = 0, 1, 2, 3


def nav_of(cfac, lfac, coff, loff, origin=1, sub_lon=0.0):
    return dict(cfac=int(cfac), lfac=int(lfac), coff=int(coff), loff=int(loff), origin=int(origin), sub_lon=float(sub_lon))


def width_of(bits):
    return 1 if bits <= 8 else 2


def atan_small(t):
    """t * P(t^2): the series' first ten terms in Horner form from k = 9 down, coefficients 1.0 / (2k + 1)."""
    t = np.asarray(t, np.float64)
    z = t * t
    p = np.full(t.shape, -(1.0 / 19.0))
    for k in range(8, -1, -1):
        c = 1.0 / (2 * k + 1)
        p = (-c if k % 2 else c) + z * p
    return t * p


def grid_lonlat(kind, columns, rows, lon0, lat0, step_lon, step_lat):
    """-> (lon_j in degrees, lat_i in radians)."""
    assert kind in (EQUIRECT, MERCATOR) and 1 <= columns <= MAX_DIM and 1 <= rows <= MAX_DIM
    lon = lon0 + np.arange(columns, dtype=np.float64) * step_lon
    i = np.arange(rows, dtype=np.float64)
    lat = np.arctan(np.sinh(lat0 - i * step_lat)) if kind == MERCATOR else np.deg2rad(lat0 - i * step_lat)
    return lon, lat


def grid_tables(kind, columns, rows, lon0, lat0, step_lon, step_lat, sub_lon):
    """NumPy's tables of a grid -> (A, B of `rows` float64, C, S of `columns`)."""
    lon, lat = grid_lonlat(kind, columns, rows, lon0, lat0, step_lon, step_lat)
    c_lat = np.arctan(FLAT * np.tan(lat))
    rl = RPOL / np.sqrt(1.0 - E2 * np.cos(c_lat) ** 2)
    dl = np.deg2rad(lon - sub_lon)
    return rl * np.cos(c_lat), rl * np.sin(c_lat), np.cos(dl), np.sin(dl)


def _quantise(f):
    s = f * 256.0
    ok = (s < LIMIT) & (s > -LIMIT)
    q = np.floor(np.where(ok, s, 0.0) + 0.5).astype(np.int64)
    return ok, q


def map_points(A, B, C, S, nav):
    """The map of the grid -> (qx, qy) int32 arrays (rows, columns); OFF in both where the pixel is off the disc."""
    A, B, C, S = (np.asarray(x, np.float64) for x in (A, B, C, S))
    with np.errstate(all="ignore"):
        a, b = A[:, None], B[:, None]
        c, s = C[None, :], S[None, :]
        ac = a * c
        r1 = H - ac
        r2 = -(a * s)
        r3 = np.broadcast_to(b, ac.shape)
        r22 = r2 * r2
        vis = (r1 > 0.0) & (H * ac >= r22 + K * (r3 * r3))
        u = -r2 / r1
        v = -r3 / np.sqrt(r1 * r1 + r22)
        x = atan_small(u) * R2D
        y = atan_small(v) * R2D
        fc = float(nav["coff"] - nav["origin"]) + x * (float(nav["cfac"]) / 65536.0)
        fl = float(nav["loff"] - nav["origin"]) + y * (float(nav["lfac"]) / 65536.0)
        okx, qx = _quantise(fc)
        oky, qy = _quantise(fl)
    on = vis & okx & oky
    return np.where(on, qx, OFF).astype(np.int32), np.where(on, qy, OFF).astype(np.int32)


def classify_and_sample(img, qx, qy, mode):
    """-> (out, of img's dtype; cls, the class of every output pixel)."""
    img = np.asarray(img)
    assert img.ndim == 2 and img.dtype in (np.uint8, np.uint16) and mode in (NEAREST, BILINEAR)
    rows, columns = img.shape
    qx, qy = np.asarray(qx).astype(np.int64), np.asarray(qy).astype(np.int64)
    off = (qx == OFF) | (qy == OFF)

    def tap(x, y):
        ins = (x >= 0) & (y >= 0) & (x < columns) & (y < rows)
        return ins, np.where(ins, img[np.where(ins, y, 0), np.where(ins, x, 0)].astype(np.int64), 0)

    if mode == NEAREST:
        inside, v = tap((qx + 128) >> 8, (qy + 128) >> 8)
        out = v
        has = v != 0
    else:
        x0, y0, fx, fy = qx >> 8, qy >> 8, qx & 255, qy & 255
        W = np.zeros(qx.shape, np.int64)
        V = np.zeros(qx.shape, np.int64)
        inside = np.zeros(qx.shape, bool)
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            ins, v = tap(x0 + dx, y0 + dy)
            inside |= ins
            w = np.where(v != 0, (fx if dx else 256 - fx) * (fy if dy else 256 - fy), 0)
            W += w
            V += w * v
        has = W != 0
        out = np.where(has, (2 * V + W) // np.maximum(2 * W, 1), 0)
    cls = np.where(off, OFF_DISC, np.where(~inside, OUTSIDE, np.where(has, WRITTEN, NO_DATA)))
    return np.where(cls == WRITTEN, out, 0).astype(img.dtype), cls


def resample(img, qx, qy, mode):
    """A map applied to an image -> (out, summary dict)."""
    out, cls = classify_and_sample(img, qx, qy, mode)
    n = np.bincount(cls.reshape(-1), minlength=4)
    return out, dict(total=int(cls.size), off_disc=int(n[OFF_DISC]), outside=int(n[OUTSIDE]), no_data=int(n[NO_DATA]), written=int(n[WRITTEN]),
                     columns=cls.shape[1], rows=cls.shape[0], width=img.itemsize, mode=mode)


def project(img, tables, nav, mode):
    qx, qy = map_points(*tables, nav)
    return resample(img, qx, qy, mode)


# ---- host helpers ---------------------------------------------------------------------------------------------------------
def navigation_record(nav, name=None):
    """The image navigation record (type 2, length 51) of nav."""
    name = (b"GEOS(%s)" % repr(nav["sub_lon"]).encode()) if name is None else name
    return bytes([2]) + struct.pack(">H", 51) + name.ljust(32, b"\0")[:32] + struct.pack(">iiii", nav["cfac"], nav["lfac"], nav["coff"], nav["loff"])


def header_of(records, data_bits=0, file_type=0):
    """A primary header in front of `records`."""
    total = 16 + sum(len(r) for r in records)
    return bytes([0]) + struct.pack(">HBIQ", 16, file_type, total, data_bits) + b"".join(records)


def parse_navigation(header):
    """-> nav, or None where xrit_geo_parse_navigation says XRIT_E_INVALID."""
    b = bytes(header)
    if len(b) < 16 or b[0] != 0 or struct.unpack(">H", b[1:3])[0] != 16:
        return None
    total = struct.unpack(">I", b[4:8])[0]
    if total > len(b):
        return None
    q = 16
    while q + 3 <= total:
        t, ln = b[q], struct.unpack(">H", b[q + 1:q + 3])[0]
        if ln < 3 or q + ln > total:
            break
        if t == 2 and ln == 51:
            name = b[q + 3:q + 35]
            if name[:5] not in (b"GEOS(", b"geos(") or b")" not in name:
                return None
            try:
                lon = float(name[5:name.index(b")")].decode("ascii"))
            except ValueError:
                return None
            if not -360.0 <= lon <= 360.0:
                return None
            cfac, lfac, coff, loff = struct.unpack(">iiii", b[q + 35:q + 51])
            return nav_of(cfac, lfac, coff, loff, 1, lon)
        q += ln
    return None


def pixel_to_lonlat(nav, column, line):
    """The inverse of the map (CGMS 4.4.3.2) -> (lon_deg, lat_deg), or None for space."""
    x = np.deg2rad((column - nav["coff"]) / (nav["cfac"] / 65536.0))
    y = np.deg2rad((line - nav["loff"]) / (nav["lfac"] / 65536.0))
    cx, sx, cy, sy = np.cos(x), np.sin(x), np.cos(y), np.sin(y)
    k = cy * cy + K * sy * sy
    d = (H * cx * cy) ** 2 - k * 1737121856.0
    if not d >= 0:
        return None
    sn = (H * cx * cy - np.sqrt(d)) / k
    s1, s2, s3 = H - sn * cx * cy, sn * sx * cy, -sn * sy
    return float(np.rad2deg(np.arctan(s2 / s1)) + nav["sub_lon"]), float(np.rad2deg(np.arctan(K * s3 / np.sqrt(s1 * s1 + s2 * s2))))


def forward(nav, lon_deg, lat_deg):
    """(lon, lat) -> the fractional (column, line), numbered from nav's origin, with NumPy's trigonometry; None if hidden."""
    c_lat = np.arctan(FLAT * np.tan(np.deg2rad(lat_deg)))
    rl = RPOL / np.sqrt(1.0 - E2 * np.cos(c_lat) ** 2)
    dl = np.deg2rad(lon_deg - nav["sub_lon"])
    r1, r2, r3 = H - rl * np.cos(c_lat) * np.cos(dl), -rl * np.cos(c_lat) * np.sin(dl), rl * np.sin(c_lat)
    if not H * (H - r1) >= r2 * r2 + K * r3 * r3:
        return None
    x = np.rad2deg(np.arctan(-r2 / r1))
    y = np.rad2deg(np.arcsin(-r3 / np.sqrt(r1 * r1 + r2 * r2 + r3 * r3)))
    return float(nav["coff"] + x * nav["cfac"] / 65536.0), float(nav["loff"] + y * nav["lfac"] / 65536.0)


# ---- the fixed case of the tests -------------------------------------------------------------------------------------------
FIXED_NAV = nav_of(357469, 297890, 49, 41, 1, -75.2)
FIXED_SOURCE = (80, 96)                             # rows, columns
FIXED_GRID = (EQUIRECT, 171, 163, -160.2, 81.0, 1.0, 1.0)


def fixed_tables():
    return grid_tables(*FIXED_GRID, FIXED_NAV["sub_lon"])


# ---- the recorded table of the host check ------------------------------------------------------------------------------------
def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def rule_table_text():
    """tests/golden/geo_rule_table.txt: what csrc/geo_host_check.cpp replays through csrc/geo_rule.h.
    `0 cfac lfac coff loff origin`: a navigation.  `1 A B C S qx qy` (the doubles as their 64 bits in decimal): a map entry
    under the last navigation, OFF OFF where off the disc.  `2 columns rows v..`: a source image, row by row.
    `3 qx qy mode out class`: an output sample from the last image.  `4 t r`: atan_small(t) = r, both as bits."""
    lines = []
    A, B, C, S = fixed_tables()
    for nav in (FIXED_NAV, dict(FIXED_NAV, cfac=-FIXED_NAV["cfac"], lfac=-FIXED_NAV["lfac"]),
                nav_of((1 << 31) - 1, -(1 << 31), (1 << 22) - 20, 20 - (1 << 22), 0, 0.0)):
        lines.append("0 %d %d %d %d %d" % (nav["cfac"], nav["lfac"], nav["coff"], nav["loff"], nav["origin"]))
        rows, cols = np.arange(3, len(A), 31), np.arange(2, len(C), 23)
        qx, qy = map_points(A[rows], B[rows], C[cols], S[cols], nav)
        for a, i in enumerate(rows):
            for b, j in enumerate(cols):
                lines.append("1 %d %d %d %d %d %d" % (_bits(A[i]), _bits(B[i]), _bits(C[j]), _bits(S[j]), qx[a, b], qy[a, b]))
    # tables that hold anything
    odd = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 0.0, -0.0, 1.0, 6378.0, 5e-324])
    lines.append("0 %d %d %d %d %d" % tuple(FIXED_NAV[k] for k in ("cfac", "lfac", "coff", "loff", "origin")))
    for a, b in [(a, 100.0) for a in odd] + [(6378.0, b) for b in (np.nan, np.inf, 1e300)]:
        qx, qy = map_points([a], [b], odd, odd[::-1], FIXED_NAV)
        lines += ["1 %d %d %d %d %d %d" % (_bits(a), _bits(b), _bits(odd[j]), _bits(odd[::-1][j]), qx[0, j], qy[0, j]) for j in range(len(odd))]
    rng = np.random.default_rng(24)
    for t in np.concatenate([np.linspace(-0.2, 0.2, 21), rng.uniform(-0.2, 0.2, 10), [0.0, -0.0, 1e-300, 0.154]]):
        lines.append("4 %d %d" % (_bits(t), _bits(atan_small(t))))
    images = [np.array([[7]], np.uint8), np.array([[10, 20], [30, 40]], np.uint8), np.array([[0, 0, 5], [0, 9, 0], [255, 0, 1]], np.uint8),
              np.array([[65535, 65535], [65535, 65534]], np.uint16),
              rng.integers(0, 1024, (4, 5)).astype(np.uint16)]
    for img in images:
        r, c = img.shape
        lines.append("2 %d %d %s" % (c, r, " ".join(str(int(v)) for v in img.reshape(-1))))
        # every edge along one axis at a time, then the corners
        qs = [(x, 77) for x in (-300, -256, -129, -128, -1, 0, 1, 127, 128, 255, 256, c * 256 - 257, c * 256 - 256, c * 256 - 129, c * 256 - 128, c * 256)]
        qs += [(1, y) for y in (-257, -128, 0, 77, 128, r * 256 - 256, r * 256 - 129, r * 256 - 128, r * 256 + 3)]
        qs += [(x, y) for x in (-129, c * 256 - 129) for y in (-128, r * 256 - 128)]
        qs += [(OFF, OFF), (OFF, 0), (0, OFF), ((1 << 31) - 1, 0), (0, (1 << 31) - 1), (-(1 << 31) + 1, 5), ((1 << 30) - 1, (1 << 30) - 1)]
        qs += [(int(a), int(b)) for a, b in rng.integers(-300, 256 * 5 + 300, (8, 2))]
        qx, qy = np.array([q[0] for q in qs])[None, :], np.array([q[1] for q in qs])[None, :]
        for mode in (NEAREST, BILINEAR):
            out, cls = classify_and_sample(img, qx, qy, mode)
            lines += ["3 %d %d %d %d %d" % (qs[k][0], qs[k][1], mode, out[0, k], cls[0, k]) for k in range(len(qs))]
    return "\n".join(lines) + "\n"
