"""The specification of the JPEG stage: a baseline JFIF encoder in NumPy on integers, written to be
the file libjpeg writes -- the slow-integer forward DCT (jfdctint: 13-bit constants, PASS1_BITS 2, rows then columns),
libjpeg's quantiser, quality scaling and 16-bit fixed-point RGB -> YCbCr, the Annex K Huffman tables without
optimisation, 4:4:4 only.  encode() returns the whole file and the counters of what the input exercised; the device
equals the file byte for byte (tests/test_gpu_jpeg.py), Pillow's libjpeg equals it too (tests/test_jpeg_spec.py)."""
import numpy as np

# zigzag position k -> natural index (row * 8 + column)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# Annex K.1, natural order
STD_LUMINANCE = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                          72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMINANCE = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] +
                           [99] * 32)
# Annex K.3: the number of codes of each length 1 .. 16, then the symbols in code order
DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROM_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROM_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROM_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
# in the order libjpeg writes them for a colour scan: (class, index, bits, values)
HUFFMAN = [(0, 0, DC_LUM_BITS, DC_VALS), (1, 0, AC_LUM_BITS, AC_LUM_VALS), (0, 1, DC_CHROM_BITS, DC_VALS), (1, 1, AC_CHROM_BITS, AC_CHROM_VALS)]

COUNTERS = ("stuffed", "ff_pairs", "pad_ff", "zrl", "zrl2", "zrl3", "no_eob", "dc_cat0", "dc_cat11", "ac_cat10", "one_mcu_intervals", "short_last",
            "restarts")
MAX_DIM = 65535
MAX_BLOCKS = 1 << 22            # what the device stage takes: 8 x 8 blocks of all components
BLOCK_BITS = 22 + 63 * 26       # the longest block: the longest DC code (11 bits, chrominance) and 11 bits, 63 x (16-bit code and 10 bits)


def huffman_codes(bits, vals):
    """Annex C: symbol -> (code, length)."""
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _code_arrays(bits, vals):
    code, size = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for sym, (c, n) in huffman_codes(bits, vals).items():
        code[sym], size[sym] = c, n
    return code, size


DC_CODES = [_code_arrays(DC_LUM_BITS, DC_VALS), _code_arrays(DC_CHROM_BITS, DC_VALS)]
AC_CODES = [_code_arrays(AC_LUM_BITS, AC_LUM_VALS), _code_arrays(AC_CHROM_BITS, AC_CHROM_VALS)]


def quality_entry(base, quality):
    """jpeg_quality_scaling and jpeg_add_quant_table with force_baseline."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return min(max((base * s + 50) // 100, 1), 255)


def quality_tables(quality):
    """-> (2, 64) in natural order."""
    if not 1 <= quality <= 100:
        raise ValueError("quality 1..100")
    return np.array([[quality_entry(int(b), quality) for b in t] for t in (STD_LUMINANCE, STD_CHROMINANCE)], np.int64)


def colour(rgb):
    """(..., 3) RGB -> (..., 3) YCbCr: libjpeg's rgb_ycc_convert."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr], -1)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def dct_pass(d, second):
    """One 1-D pass of jfdctint along the last axis (8 values, int64); second: the column pass's scaling."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 15 if second else 11
    o = [None] * 8
    o[0] = _descale(t10 + t11, 2) if second else (t10 + t11) << 2
    o[4] = _descale(t10 - t11, 2) if second else (t10 - t11) << 2
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def quantise(c, q):
    """libjpeg's quantiser on the transform's output (scaled by 8): divisor q << 3, halves away from zero."""
    qv = q << 3
    m = (np.abs(c) + (qv >> 1)) // qv
    return np.where(c < 0, -m, m)


def category(v):
    """-> (the number of bits of |v|, the magnitude bits: v, or v - 1 for a negative v, in that many bits)."""
    a = np.abs(v)
    cat = np.zeros(a.shape, np.int64)
    for n in range(1, 17):
        cat += a >= (1 << (n - 1))
    bits = np.where(v < 0, v - 1, v) & ((1 << cat) - 1)
    return cat, bits


def planes(image):
    """uint8 H x W or H x W x 3 -> (components, H, W) int64 samples."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3) or min(image.shape[:2]) < 1:
        raise ValueError("uint8, H x W or H x W x 3")
    if max(image.shape[:2]) > MAX_DIM:
        raise ValueError("at most 65535 rows and columns")
    if image.ndim == 2:
        return image.astype(np.int64)[None]
    return np.moveaxis(colour(image), -1, 0)


def coefficients(image, tables):
    """-> (MCUs, components, 64) quantised coefficients in zigzag order, MCUs row by row; tables (2, 64) natural order."""
    p = planes(image)
    nc, h, w = p.shape
    bh, bw = (h + 7) // 8, (w + 7) // 8
    p = np.pad(p, ((0, 0), (0, bh * 8 - h), (0, bw * 8 - w)), mode="edge") - 128
    blocks = p.reshape(nc, bh, 8, bw, 8).transpose(1, 3, 0, 2, 4)                # (bh, bw, nc, row, column)
    rows = dct_pass(blocks, False)
    both = np.swapaxes(dct_pass(np.swapaxes(rows, -1, -2), True), -1, -2)
    q = np.asarray(tables, np.int64).reshape(2, 64)[[0, 1, 1][:nc]].reshape(nc, 8, 8)
    return quantise(both, q).reshape(bh * bw, nc, 64)[:, :, ZIGZAG]


def check_tables(tables):
    t = np.asarray(tables, np.int64).reshape(-1)
    if t.shape != (128,) or t.min() < 1 or t.max() > 255:
        raise ValueError("two tables of 64 entries 1..255")
    return t.reshape(2, 64)


def header(components, columns, rows, tables, restart):
    """SOI .. SOS as libjpeg writes them; tables (2, 64) natural order."""
    if components not in (1, 3) or not (1 <= columns <= MAX_DIM and 1 <= rows <= MAX_DIM) or not 0 <= restart <= 65535:
        raise ValueError("components 1 or 3, 1..65535 columns and rows, restart 0..65535")
    tables = check_tables(tables)
    be16 = lambda v: [v >> 8, v & 255]
    out = [0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0]
    for i in range(2 if components == 3 else 1):
        out += [0xFF, 0xDB, 0, 67, i] + [int(tables[i][n]) for n in ZIGZAG]
    out += [0xFF, 0xC0] + be16(8 + 3 * components) + [8] + be16(rows) + be16(columns) + [components]
    for c in range(components):
        out += [c + 1, 0x11, 1 if c else 0]
    for cls, idx, bits, vals in HUFFMAN[:4 if components == 3 else 2]:
        out += [0xFF, 0xC4] + be16(19 + len(vals)) + [cls << 4 | idx] + list(bits) + list(vals)
    if restart:
        out += [0xFF, 0xDD, 0, 4] + be16(restart)
    out += [0xFF, 0xDA] + be16(6 + 2 * components) + [components]
    for c in range(components):
        out += [c + 1, 0x11 if c else 0x00]
    out += [0, 63, 0]
    return bytes(out)


def bound(components, columns, rows, restart):
    """The largest file any input of that shape can produce; 0 for a shape the stage does not take."""
    if components not in (1, 3) or not (1 <= columns <= MAX_DIM and 1 <= rows <= MAX_DIM) or not 0 <= restart <= 65535:
        return 0
    mcus = ((columns + 7) // 8) * ((rows + 7) // 8)
    if mcus * components > MAX_BLOCKS:
        return 0
    intervals = (mcus + restart - 1) // restart if restart else 1
    # per interval the blocks' bits rounded up to a byte, every byte stuffed; a marker between intervals; the header, EOI
    return len(header(components, 1, 1, np.ones((2, 64)), restart)) + 2 * ((mcus * components * BLOCK_BITS + 7) // 8 + intervals) + \
        2 * (intervals - 1) + 2


def scan(coef, restart):
    """coef (MCUs, components, 64) zigzag -> (the entropy-coded segment with its restart markers, the counters)."""
    coef = np.asarray(coef, np.int64)
    mcus, nc, _ = coef.shape
    ri = restart if restart else mcus
    n_int = (mcus + ri - 1) // ri
    cnt = dict.fromkeys(COUNTERS, 0)
    # DC differences per component, the predictor zero at the start of every interval
    dc = coef[:, :, 0]
    prev = np.concatenate([np.zeros((1, nc), np.int64), dc[:-1]])
    prev[np.arange(mcus) % ri == 0] = 0
    dcat, dbits = category(dc - prev)
    cnt["dc_cat0"], cnt["dc_cat11"] = int((dcat == 0).sum()), int((dcat == 11).sum())
    tab = np.array([0, 1, 1][:nc])                                              # the component's Huffman tables
    dcode = np.stack([DC_CODES[t][0][dcat[:, c]] for c, t in enumerate(tab)], 1)
    dsize = np.stack([DC_CODES[t][1][dcat[:, c]] for c, t in enumerate(tab)], 1)
    # one list of words (value, length) with a sort key (block, position in the block, order inside the position)
    nb = mcus * nc
    block = np.arange(nb)
    w_key, w_val, w_len = [block * 1024], [(dcode << dcat | dbits).reshape(-1)], [(dsize + dcat).reshape(-1)]
    ac = coef.reshape(nb, 64)
    b_idx, k_idx = np.nonzero(ac[:, 1:])
    k_idx = k_idx + 1
    first = np.concatenate([[True], b_idx[1:] != b_idx[:-1]]) if len(b_idx) else np.zeros(0, bool)
    before = np.where(first, 0, np.concatenate([[0], k_idx[:-1]]))
    run = k_idx - before - 1
    acat, abits = category(ac[b_idx, k_idx])
    cnt["ac_cat10"] = int((acat == 10).sum())
    if (acat > 10).any():
        raise ValueError("an AC coefficient beyond 10 bits")
    t_of = tab[b_idx % nc]
    codes, sizes = np.stack([AC_CODES[0][0], AC_CODES[1][0]]), np.stack([AC_CODES[0][1], AC_CODES[1][1]])
    n_zrl = run >> 4
    cnt["zrl"], cnt["zrl2"], cnt["zrl3"] = int(n_zrl.sum()), int((n_zrl == 2).sum()), int((n_zrl == 3).sum())
    for j in range(3):                                                          # up to three ZRL in front of a coefficient
        m = n_zrl > j
        w_key.append(b_idx[m] * 1024 + k_idx[m] * 8 + j)
        w_val.append(codes[t_of[m], 0xF0])
        w_len.append(sizes[t_of[m], 0xF0])
    sym = (run & 15) << 4 | acat
    w_key.append(b_idx * 1024 + k_idx * 8 + 4)
    w_val.append(codes[t_of, sym] << acat | abits)
    w_len.append(sizes[t_of, sym] + acat)
    eob = ac[:, 63] == 0
    cnt["no_eob"] = int((~eob).sum())
    w_key.append(block[eob] * 1024 + 64 * 8)
    w_val.append(codes[tab[block[eob] % nc], 0])
    w_len.append(sizes[tab[block[eob] % nc], 0])
    # the fill of every interval's last byte: 1-bits, placed behind its last block
    key, val, length = np.concatenate(w_key), np.concatenate(w_val), np.concatenate(w_len)
    order = np.argsort(key, kind="stable")
    key, val, length = key[order], val[order], length[order]
    interval = (key // 1024) // nc // ri
    bits_of = np.bincount(interval, weights=length, minlength=n_int).astype(np.int64)
    fill = -bits_of % 8
    ends = np.cumsum(np.bincount(interval, minlength=n_int))
    val, length = np.insert(val, ends, (1 << fill) - 1), np.insert(length, ends, fill)
    # words -> bits -> bytes
    total = int(length.sum())
    starts = np.cumsum(length) - length
    word = np.repeat(np.arange(len(val)), length)
    shift = length[word] - 1 - (np.arange(total) - starts[word])
    raw = np.packbits(((val[word] >> shift) & 1).astype(np.uint8))
    i_bytes = (bits_of + fill) // 8
    i_start = np.cumsum(i_bytes) - i_bytes
    ff = raw == 0xFF
    last = i_start + i_bytes - 1
    cnt["pad_ff"] = int((ff[last] & (fill > 0)).sum())
    cnt["stuffed"] = int(ff.sum()) - cnt["pad_ff"]
    pair = ff[1:] & ff[:-1]
    pair[last[:-1]] = False                                                     # not across a marker
    cnt["ff_pairs"] = int(pair.sum())
    cnt["restarts"] = n_int - 1
    cnt["one_mcu_intervals"] = n_int if ri == 1 else int(mcus % ri == 1)
    cnt["short_last"] = int(mcus % ri != 0 and n_int > 1)
    # every 0xFF gets its 0x00; RSTm between the intervals
    at = np.arange(len(raw)) + (np.cumsum(ff) - ff) + 2 * np.repeat(np.arange(n_int), i_bytes)
    out = np.zeros(len(raw) + int(ff.sum()) + 2 * (n_int - 1), np.uint8)
    out[at] = raw
    m_at = at[i_start[1:]] - 2
    out[m_at] = 0xFF
    out[m_at + 1] = 0xD0 + (np.arange(n_int - 1) & 7)
    return out.tobytes(), cnt


def encode(image, quality=None, tables=None, restart=0):
    """-> (the file, the counters).  quality 1..100 or tables: (2, 64) natural order, entries 1..255; restart in MCUs."""
    if (quality is None) == (tables is None):
        raise ValueError("quality or tables")
    tables = quality_tables(quality) if tables is None else check_tables(tables)
    image = np.asarray(image)
    rows, columns = image.shape[:2]
    nc = 1 if image.ndim == 2 else 3
    head = header(nc, columns, rows, tables, restart)
    body, cnt = scan(coefficients(image, tables), restart)
    return head + body + b"\xff\xd9", cnt


# what the device leaves in d_result: the file's length whether or not it fitted, 1 if it did not, the restart markers
RESULT_DTYPE = np.dtype([("size", np.uint64), ("status", np.uint32), ("restarts", np.uint32)])


# ---- the table csrc/jpeg_host_check.cpp replays through jpeg_rule.h ---------------------------------------------------
def rule_table_text():
    """Rows of 18 integers: the kind, then its inputs and outputs, zeros behind.  0: a transform pass (second, 8 in, 8 out);
    1: the quantiser (c, q, out); 2: the colour conversion (r, g, b, y, cb, cr); 3: category (v, bits of |v|, magnitude bits);
    4: quality scaling (base, quality, entry); 5: a Huffman code (table 0..3, symbol, code, length)."""
    rng = np.random.default_rng(2025)
    rows = []
    add = lambda kind, vals: rows.append([kind] + [int(v) for v in vals] + [0] * (17 - len(vals)))
    firsts = [np.full(8, 127), np.full(8, -128), np.array([127, -128] * 4), np.array([-128, 127] * 4), np.array([127] * 4 + [-128] * 4)]
    firsts += list(rng.integers(-128, 128, (40, 8)))
    for d in firsts:
        d = np.asarray(d, np.int64)
        o = dct_pass(d, False)
        add(0, [0] + list(d) + list(o))
        add(0, [1] + list(o) + list(dct_pass(o, True)))
    for d in rng.integers(-5800, 5801, (40, 8)):
        add(0, [1] + list(d) + list(dct_pass(np.asarray(d, np.int64), True)))
    for c, q in [(0, 1), (3, 1), (4, 1), (-4, 1), (-3, 1), (8191, 1), (-8192, 1), (8191, 255), (1019, 255), (1020, 255), (-1020, 255), (-1019, 255)] + \
            [(int(a), int(b)) for a, b in zip(rng.integers(-8192, 8192, 60), rng.integers(1, 256, 60))]:
        add(1, [c, q, quantise(np.int64(c), np.int64(q))])
    for rgb in [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)] + \
            [tuple(x) for x in rng.integers(0, 256, (60, 3))]:
        add(2, list(rgb) + list(colour(np.array(rgb))))
    for v in [0, 1, -1, 2, -2, 3, -3, 4, -4, 255, -255, 256, -256, 1023, -1023, 1024, -1024, 2047, -2047] + list(rng.integers(-2047, 2048, 30)):
        cat, bits = category(np.int64(v))
        add(3, [v, cat, bits])
    for base in (1, 10, 16, 99, 121, 255):
        for quality in (1, 2, 10, 25, 49, 50, 51, 75, 90, 95, 99, 100):
            add(4, [base, quality, quality_entry(base, quality)])
    for t, (_, _, bits, vals) in enumerate(HUFFMAN):
        for sym, (code, length) in sorted(huffman_codes(bits, vals).items()):
            add(5, [t, sym, code, length])
    return "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
