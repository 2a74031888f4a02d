"""The map overlay stage's specification (include/xritdemod_amd.h, "Map overlay"): what xrit_overlay_*
computes -- the mask a list of vertices draws, the draw's summary, the blend of a mask into an image and its summary --
in Python integers, and the host helpers in NumPy.  The device equals every array and every summary field exactly.  A
vertex list here is an (n, 2) integer array of (qx, qy) in 1/256 pixel; a mask is a 2-D uint8 array (rows, columns): pitch
and padding are the device interface's business.  The vertex map of the scan geometry is geo_spec.map_points, applied per
vertex (points_of_quads)."""
import math

import numpy as np

import geo_spec as gs

BREAK = -(1 << 31)                                  # INT32_MIN, both members of a break
LIMIT = 1 << 29                                     # a vertex at or above it in magnitude counts as a break
MAX_DIM = 16384
MAX_WIDTH = 8
LAYERS = 8
MAX_VERTICES = 1 << 26
HIDDEN, JUMP, DRAWN = 0, 1, 2
DRAW_FIELDS = ("vertices", "segments", "hidden", "jumps", "outside", "drawn", "steps", "layer", "width")
BLEND_FIELDS = ("pixels", "covered", "by_layer", "columns", "rows", "components_in", "components_out")


def is_break(p):
    return not (-LIMIT < int(p[0]) < LIMIT and -LIMIT < int(p[1]) < LIMIT)


def pixel(q):
    return (q + 128) >> 8


def before(w):
    return (w - 1) // 2


def behind(w):
    return w // 2


def setup(p0, p1, width, max_jump, columns, rows):
    """What a pair of vertices comes to -> a dict: kind; for DRAWN the end pixels, xmajor, a0, b0, da, db, the walk's m0 and
    line (the m left after the cut of rule 6) and steps = 2 + line."""
    if is_break(p0) or is_break(p1):
        return dict(kind=HIDDEN, steps=0)
    x0, y0, x1, y1 = int(p0[0]), int(p0[1]), int(p1[0]), int(p1[1])
    dx, dy = x1 - x0, y1 - y0
    if max_jump and (abs(dx) > max_jump or abs(dy) > max_jump):
        return dict(kind=JUMP, steps=0)
    xmajor = abs(dx) >= abs(dy)
    a0, b0, a1, b1 = (x0, y0, x1, y1) if xmajor else (y0, x0, y1, x1)
    if a0 > a1:
        a0, b0, a1, b1 = a1, b1, a0, b0
    s = dict(kind=DRAWN, ends=((pixel(x0), pixel(y0)), (pixel(x1), pixel(y1))), xmajor=xmajor, a0=a0, b0=b0, da=a1 - a0, db=b1 - b0, m0=0, line=0)
    if a1 > a0:
        dim = columns if xmajor else rows
        lo, hi = max(-((-a0) // 256), -behind(width)), min(a1 // 256, dim - 1 + before(width))
        if hi >= lo:
            s["m0"], s["line"] = lo, hi - lo + 1
    s["steps"] = 2 + s["line"]
    return s


def step_pixels(s):
    """The pixels (px, py) a drawn segment stamps, in step order: the two ends, then the walk."""
    out = list(s["ends"])
    for m in range(s["m0"], s["m0"] + s["line"]):
        minor = s["b0"] + (2 * (256 * m - s["a0"]) * s["db"] + s["da"]) // (2 * s["da"])
        out.append((m, pixel(minor)) if s["xmajor"] else (pixel(minor), m))
    return out


def stamp(px, py, width, columns, rows):
    """The part of a stamp inside the image -> (x0, x1, y0, y1) inclusive, or None."""
    x0, x1 = max(px - before(width), 0), min(px + behind(width), columns - 1)
    y0, y1 = max(py - before(width), 0), min(py + behind(width), rows - 1)
    return None if x1 < x0 or y1 < y0 else (x0, x1, y0, y1)


def draw(points, layer, width, max_jump, mask, clear=False):
    """One call -> (the mask afterwards, a new array; the summary dict)."""
    mask = np.array(mask, np.uint8)
    assert mask.ndim == 2 and 0 <= layer < LAYERS and 1 <= width <= MAX_WIDTH
    rows, columns = mask.shape
    assert 1 <= rows <= MAX_DIM and 1 <= columns <= MAX_DIM
    if clear:
        mask[:] = 0
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    n = len(pts)
    bit = np.uint8(1 << layer)
    c = dict(vertices=n, segments=0, hidden=0, jumps=0, outside=0, drawn=0, steps=0, layer=layer, width=width)
    for i in range(n - 1):
        s = setup(pts[i], pts[i + 1], width, max_jump, columns, rows)
        if s["kind"] == HIDDEN:
            c["hidden"] += 1
            continue
        c["segments"] += 1
        if s["kind"] == JUMP:
            c["jumps"] += 1
            continue
        c["drawn"] += 1
        c["steps"] += s["steps"]
        touched = False
        for px, py in step_pixels(s):
            st = stamp(px, py, width, columns, rows)
            if st:
                touched = True
                mask[st[2]:st[3] + 1, st[0]:st[1] + 1] |= bit
        c["outside"] += not touched
    return mask, c


def segment_pixels(p0, p1, columns, rows, width=1):
    """The set of pixels (x, y) one segment sets in an image of columns x rows."""
    s = setup(p0, p1, width, 0, columns, rows)
    out = set()
    if s["kind"] == DRAWN:
        for px, py in step_pixels(s):
            st = stamp(px, py, width, columns, rows)
            if st:
                out.update((x, y) for x in range(st[0], st[1] + 1) for y in range(st[2], st[3] + 1))
    return out


def luma(r, g, b):
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def mix(src, c, alpha):
    return (src * (255 - alpha) + c * alpha + 127) // 255


def blend(image, mask, styles, components_out):
    """image: (rows, columns) or (rows, columns, 3) uint8; styles: 8 x (r, g, b, alpha) -> (out, summary dict)."""
    image, mask = np.asarray(image, np.uint8), np.asarray(mask, np.uint8)
    cin = 1 if image.ndim == 2 else image.shape[2]
    assert cin in (1, 3) and components_out in (1, 3) and cin <= components_out and mask.shape == image.shape[:2]
    styles = np.asarray(styles, np.int64).reshape(LAYERS, 4)
    rows, columns = mask.shape
    src = image.reshape(rows, columns, cin).astype(np.int64)
    src3 = np.repeat(src, 3, axis=2) if cin == 1 else src
    top = np.zeros(mask.shape, np.int64)
    for k in range(LAYERS):
        top[(mask >> k) & 1 == 1] = k
    covered = mask != 0
    alpha = styles[top, 3]
    if components_out == 1:
        colour = luma(styles[:, 0], styles[:, 1], styles[:, 2])[top][:, :, None]
        base = src3[:, :, :1]
    else:
        colour = styles[top, :3]
        base = src3
    mixed = mix(base, colour, alpha[:, :, None])
    out = np.where(covered[:, :, None], mixed, base).astype(np.uint8)
    by_layer = [int(((top == k) & covered).sum()) for k in range(LAYERS)]
    summary = dict(pixels=rows * columns, covered=int(covered.sum()), by_layer=by_layer, columns=columns, rows=rows, components_in=cin,
                   components_out=components_out)
    return (out[:, :, 0] if components_out == 1 else out), summary


# ---- the vertex map and the host helpers, with NumPy's trigonometry ---------------------------------------------------------
def points_of_quads(quads, nav):
    """geo_spec's point rule per vertex: quads (n, 4) of A, B, C, S -> (n, 2) int32; off the disc: a break."""
    q = np.asarray(quads, np.float64).reshape(-1, 4)
    out = np.zeros((len(q), 2), np.int32)
    for i in range(0, len(q), 64):                   # (map_points is rows x columns: a vertex is a row and a column, the diagonal)
        c = q[i:i + 64]
        qx, qy = gs.map_points(c[:, 0], c[:, 1], c[:, 2], c[:, 3], nav)
        out[i:i + 64, 0], out[i:i + 64, 1] = np.diagonal(qx), np.diagonal(qy)
    return out


def quads(lon_deg, lat_deg, sub_lon_deg):
    lon, lat = np.asarray(lon_deg, np.float64), np.asarray(lat_deg, np.float64)
    with np.errstate(all="ignore"):
        c_lat = np.arctan(gs.FLAT * np.tan(np.deg2rad(lat)))
        rl = gs.RPOL / np.sqrt(1.0 - gs.E2 * np.cos(c_lat) ** 2)
        dl = np.deg2rad(lon - sub_lon_deg)
        q = np.stack([rl * np.cos(c_lat), rl * np.sin(c_lat), np.cos(dl), np.sin(dl)], axis=1)
    q[np.isnan(lon) | np.isnan(lat)] = np.nan
    return q


def grid_positions(kind, lon0, lat0, step_lon, step_lat, lon_deg, lat_deg):
    """The fractional (column, row) on a grid, float64 (NaN stays NaN)."""
    lon, lat = np.asarray(lon_deg, np.float64), np.asarray(lat_deg, np.float64)
    with np.errstate(all="ignore"):
        d = lon - lon0
        d = d - 360.0 * np.floor((d + 180.0) / 360.0)
        y = np.arcsinh(np.tan(np.deg2rad(lat))) if kind == gs.MERCATOR else lat
        return d / step_lon, (lat0 - y) / step_lat


def densify(lon_deg, lat_deg, max_step):
    lon, lat = list(map(float, lon_deg)), list(map(float, lat_deg))
    out = []
    for i in range(len(lon)):
        brk = math.isnan(lon[i]) or math.isnan(lat[i])
        if i and not brk and not (math.isnan(lon[i - 1]) or math.isnan(lat[i - 1])):
            dlon, dlat = lon[i] - lon[i - 1], lat[i] - lat[i - 1]
            k = max(int(math.ceil(max(abs(dlon), abs(dlat)) / max_step)), 1)
            out += [(lon[i - 1] + dlon * j / k, lat[i - 1] + dlat * j / k) for j in range(1, k)]
        out.append((math.nan, math.nan) if brk else (lon[i], lat[i]))
    a = np.array(out, np.float64).reshape(-1, 2)
    return a[:, 0], a[:, 1]


def graticule_counts(step, vertex_step):
    """-> (meridians, vertices of one without its break, parallels, vertices of one): what xrit_overlay_graticule writes."""
    def count(start, end, st):
        k = 0
        while start + k * st < end:
            k += 1
        return k
    return count(-180.0, 180.0, step), count(-90.0, 90.0, vertex_step) + 1, count(-90.0, 90.0, step) - 1, count(-180.0, 180.0, vertex_step) + 1


def parse_polylines(text):
    """GMT-style multi-segment text -> (lon, lat) with NaN for breaks, or ('error', line number from 1).  A line that is blank
    or begins '>' or '#' is a break; any other holds `lon lat` in degrees and nothing else."""
    lon, lat = [], []
    lines = text.split("\n")
    if lines[-1] == "":                                # nothing behind the last newline
        lines.pop()
    for k, line in enumerate(lines):
        t = line.strip()
        if t == "" or t[0] in ">#":
            lon.append(math.nan)
            lat.append(math.nan)
            continue
        w = t.split()
        try:
            if len(w) != 2:
                raise ValueError
            a, b = float(w[0]), float(w[1])
            if not (math.isfinite(a) and math.isfinite(b)):
                raise ValueError
        except ValueError:
            return ("error", k + 1)
        lon.append(a)
        lat.append(b)
    return np.array(lon), np.array(lat)


# ---- the recorded table of the host check ------------------------------------------------------------------------------------
def rule_table_text():
    """tests/golden/overlay_rule_table.txt: what csrc/overlay_host_check.cpp replays through csrc/overlay_rule.h.
    `0 columns rows width max_jump`: an image.  `1 x0 y0 x1 y1 kind xmajor a0 b0 da db m0 line steps touched`: a pair's
    set-up under the last image (the fields behind kind 0 for a pair that is not drawn).  `2 x0 y0 x1 y1 k px py`: the pixel
    of step k.  `3 px py hit x0 x1 y0 y1`: a stamp's part inside the last image.  `4 src c alpha out`: a blended byte.
    `5 r g b y`: the luminance.  `6 cin cout m s0 s1 s2 o0 o1 o2`: a pixel under mask byte m and the styles of row 7.
    `7 s0 .. s7`: the styles as r | g << 8 | b << 16 | alpha << 24."""
    rng = np.random.default_rng(28)
    L = []
    big = LIMIT - 1
    for columns, rows, width, max_jump in ((70, 50, 1, 0), (70, 50, 3, 0), (301, 203, 2, 0), (9, 7, 8, 0), (16384, 16384, 1, 0), (64, 64, 1, 4096),
                                           (1, 1, 1, 0), (1, 1, 8, 0)):
        L.append("0 %d %d %d %d" % (columns, rows, width, max_jump))
        cx, cy = columns * 256, rows * 256
        pairs = [((0, 0), (0, 0)), ((10, 10), (20, 15)), ((0, 0), (cx, cy)), ((cx, 0), (0, cy)), ((-700, 300), (cx + 700, 340)),
                 ((300, -900), (280, cy + 900)), ((-big, -big), (big, big)), ((big, -big), (-big, big)), ((-big, 100), (big, 200)),
                 ((128, 128), (129, 127)), ((127, 0), (128, 0)), ((-129, 5), (-128, 5)), ((LIMIT, 0), (0, 0)), ((0, 0), (0, -LIMIT)),
                 ((BREAK, BREAK), (0, 0)), ((5, 5), (5 + 17 * 256, 5)), ((5, 5), (5, 5 + 17 * 256)), ((-5000, -5000), (-100, -4000)),
                 ((cx + 300, 10), (cx + 9000, 4000)), ((-big, -big), (-big + 1000, -big + 10)), ((0, -3 * 256), (cx, -3 * 256)),
                 ((-4 * 256, 0), (-4 * 256, cy)), ((100, cy + 3 * 256), (cx - 100, cy + 4 * 256))]
        pairs += [(tuple(int(v) for v in rng.integers(-600, max(cx, cy) + 600, 2)), tuple(int(v) for v in rng.integers(-600, max(cx, cy) + 600, 2)))
                  for _ in range(12)]
        for p0, p1 in pairs:
            for a, b in ((p0, p1), (p1, p0)):
                s = setup(a, b, width, max_jump, columns, rows)
                if s["kind"] != DRAWN:
                    L.append("1 %d %d %d %d %d 0 0 0 0 0 0 0 0 0" % (a + b + (s["kind"],)))
                    continue
                px = step_pixels(s)
                touched = any(stamp(x, y, width, columns, rows) for x, y in px)
                L.append("1 %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (a + b + (DRAWN, s["xmajor"], s["a0"], s["b0"], s["da"], s["db"], s["m0"],
                                                                                  s["line"], s["steps"], touched)))
                ks = sorted(set([0, 1] + [int(k) for k in np.linspace(2, len(px) - 1, 7)] if len(px) > 2 else [0, 1]))
                L += ["2 %d %d %d %d %d %d %d" % (a + b + (k,) + px[k]) for k in ks]
        for px in (-9, -4, -3, -1, 0, 1, columns - 2, columns - 1, columns, columns + 3, columns + 4, columns + 9):
            for py in (-5, -4, 0, rows - 1, rows + 3, rows + 4):
                st = stamp(px, py, width, columns, rows)
                L.append("3 %d %d %d %d %d %d %d" % ((px, py, 1) + st if st else (px, py, 0, 0, 0, 0, 0)))
    for alpha in (0, 1, 127, 128, 254, 255):
        for src in (0, 1, 127, 128, 254, 255):
            for c in (0, 1, 127, 128, 254, 255):
                L.append("4 %d %d %d %d" % (src, c, alpha, mix(src, c, alpha)))
    for r, g, b in [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (1, 1, 1), (254, 254, 254)] + \
            [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(12)]:
        L.append("5 %d %d %d %d" % (r, g, b, luma(r, g, b)))
    styles = rng.integers(0, 256, (LAYERS, 4))
    styles[0, 3], styles[7, 3] = 0, 255
    L.append("7 " + " ".join(str(int(s[0]) | int(s[1]) << 8 | int(s[2]) << 16 | int(s[3]) << 24) for s in styles))
    for m in [0, 1, 2, 3, 0x80, 0x81, 0x7F, 0xFF, 0x10, 0x28]:
        for cin, cout in ((1, 1), (1, 3), (3, 3)):
            s = [int(v) for v in rng.integers(0, 256, 3)]
            img = np.array(s[:cin], np.uint8).reshape(1, 1, cin)
            out, _ = blend(img[:, :, 0] if cin == 1 else img, np.array([[m]], np.uint8), styles, cout)
            o = [int(v) for v in np.asarray(out).reshape(-1)] + [0, 0]
            L.append("6 %d %d %d %d %d %d %d %d %d" % (cin, cout, m, s[0], s[1] if cin == 3 else 0, s[2] if cin == 3 else 0, o[0], o[1], o[2]))
    return "\n".join(L) + "\n"
