"""The specification of the JPEG decoder stage: baseline JPEG streams -> the pixels libjpeg gives
for them, in NumPy and plain Python on integers.  The header walk, the scan's cut at its markers, the SERIAL entropy walk
(whose statuses are the stage's), a model of the parallel form (subsequences walked from guessed states, rounds to a
fixpoint), DC prediction, jidctint's two passes (columns descaled by 11, rows by 18, 13-bit constants), the range limit
clip(v + 128, 0, 255) and jdcolor's 16-bit fixed-point YCbCr -> RGB.  All arithmetic behind the entropy walk is 32-bit
two's complement, so that a damaged stream that still decodes has one answer.  decode_batch() is what the device equals:
pixels, records, summary; the counters say what an input exercised."""
import numpy as np

import jpeg_spec as js

OK, UNSUPPORTED, DAMAGED, TOO_LARGE, BAD_CODE, INDEX, SHORT, INTERVALS, RST_ORDER, MARKER = range(10)
N_STATUS = 10
MAX_BLOCKS = 1 << 22
DEFAULT_BLOCKS = 1 << 16        # what the device's scratch is sized for when a call says max_blocks = 0
DEFAULT_S = 1024                # bits per subsequence of form 1
MIN_S, MAX_S = 32, 1 << 20
LANES = 64                      # subsequences per tile of form 1
LOOKAHEAD = 8                   # bits of the device's short table: longer codes go through maxcode / valptr
DEAD = 0xFFFFFFFF               # the bit position of a state behind a fault

RECORD_DTYPE = np.dtype([("offset", np.uint64), ("length", np.uint64), ("columns", np.uint32), ("rows", np.uint32), ("components", np.uint32),
                         ("restart", np.uint32), ("intervals", np.uint32), ("status", np.uint32), ("reserved", np.uint32, 6)])
SUMMARY_DTYPE = np.dtype([("images", np.uint64), ("bytes", np.uint64), ("by_status", np.uint32, N_STATUS), ("overflow", np.uint32), ("reserved", np.uint32)])
INFO_DTYPE = np.dtype([("columns", np.uint32), ("rows", np.uint32), ("components", np.uint32), ("restart", np.uint32), ("status", np.uint32),
                       ("scan_offset", np.uint32), ("blocks", np.uint32), ("intervals", np.uint32)])
assert RECORD_DTYPE.itemsize == 64 and SUMMARY_DTYPE.itemsize == 64 and INFO_DTYPE.itemsize == 32

COUNTERS = ("long_codes", "straddle", "tiles_over_one", "rounds_over_one", "max_rounds", "max_in_front", "min_in_front", "stuffed", "restarts",
            "zrl", "eob", "no_eob")


def new_counters():
    c = dict.fromkeys(COUNTERS, 0)
    return c


# ---- the header ---------------------------------------------------------------------------------------------------------
def parse_header(data):
    """The marker chain SOI .. SOS, walked serially; the first thing wrong gives the status.  -> dict: status, columns, rows,
    components, restart, scan (the first byte behind SOS), blocks, intervals (those the geometry asks for), q (components x 64,
    natural order), huff [(dc bits, dc vals, ac bits, ac vals)] per component."""
    b = bytes(data)
    n = len(b)
    h = dict(status=DAMAGED, columns=0, rows=0, components=0, restart=0, scan=0, blocks=0, intervals=0, q=None, huff=None)

    def fail(status):
        return dict(h, status=status, columns=0, rows=0, components=0, restart=0, scan=0)

    if n < 2 or b[0] != 0xFF or b[1] != 0xD8:
        return fail(DAMAGED)
    qt, ht, frame, ri, p = {}, {}, None, 0, 2
    while True:
        if p + 2 > n or b[p] != 0xFF:
            return fail(DAMAGED)
        m = b[p + 1]
        if m in (0xD8, 0xD9, 0x01, 0x00, 0xFF) or 0xD0 <= m <= 0xD7:
            return fail(DAMAGED)
        if p + 4 > n:
            return fail(DAMAGED)
        L = b[p + 2] << 8 | b[p + 3]
        end = p + 2 + L
        if L < 2 or end > n:
            return fail(DAMAGED)
        if m == 0xC0:
            if frame is not None or L < 8:
                return fail(DAMAGED)
            if b[p + 4] != 8:
                return fail(UNSUPPORTED)
            rows, columns, nf = b[p + 5] << 8 | b[p + 6], b[p + 7] << 8 | b[p + 8], b[p + 9]
            if rows == 0 or columns == 0 or L != 8 + 3 * nf:
                return fail(DAMAGED)
            if nf not in (1, 3):
                return fail(UNSUPPORTED)
            comps = [(b[p + 10 + 3 * i], b[p + 11 + 3 * i], b[p + 12 + 3 * i]) for i in range(nf)]
            if any(hv != 0x11 for _, hv, _ in comps):
                return fail(UNSUPPORTED)
            if any(tq > 3 for _, _, tq in comps):
                return fail(DAMAGED)
            frame = (rows, columns, comps)
        elif 0xC1 <= m <= 0xCF and m != 0xC4:
            return fail(UNSUPPORTED)                    # another SOF, JPG, DAC
        elif m in (0xDC, 0xDE, 0xDF):
            return fail(UNSUPPORTED)                    # DNL, DHP, EXP
        elif m == 0xC4:
            q = p + 4
            while q < end:
                if q + 17 > end:
                    return fail(DAMAGED)
                tc, th = b[q] >> 4, b[q] & 15
                if tc > 1 or th > 3:
                    return fail(DAMAGED)
                cnt = b[q + 1:q + 17]
                total = sum(cnt)
                if total > 256 or q + 17 + total > end:
                    return fail(DAMAGED)
                code = 0
                for l in range(1, 17):
                    code += cnt[l - 1]
                    if code > (1 << l):
                        return fail(DAMAGED)
                    code <<= 1
                vals = b[q + 17:q + 17 + total]
                if any((v > 11) if tc == 0 else ((v & 15) > 10) for v in vals):
                    return fail(DAMAGED)
                ht[(tc, th)] = (list(cnt), list(vals))
                q += 17 + total
        elif m == 0xDB:
            q = p + 4
            while q < end:
                pq, tq = b[q] >> 4, b[q] & 15
                if tq > 3 or pq > 1:
                    return fail(DAMAGED)
                if pq == 1:
                    return fail(UNSUPPORTED)
                if q + 65 > end:
                    return fail(DAMAGED)
                nat = [0] * 64
                for k in range(64):
                    nat[js.ZIGZAG[k]] = b[q + 1 + k]
                qt[tq] = nat
                q += 65
        elif m == 0xDD:
            if L != 4:
                return fail(DAMAGED)
            ri = b[p + 4] << 8 | b[p + 5]
        elif m == 0xDA:
            if frame is None or L < 3:
                return fail(DAMAGED)
            rows, columns, comps = frame
            ns = b[p + 4]
            if ns < 1 or ns > 4 or L != 6 + 2 * ns:
                return fail(DAMAGED)
            if ns != len(comps):
                return fail(UNSUPPORTED)                # one scan per component: several scans
            huff, q = [], []
            for i, (cid, _, tq) in enumerate(comps):
                if b[p + 5 + 2 * i] != cid:
                    return fail(UNSUPPORTED)
                td, ta = b[p + 6 + 2 * i] >> 4, b[p + 6 + 2 * i] & 15
                if td > 3 or ta > 3 or (0, td) not in ht or (1, ta) not in ht or tq not in qt:
                    return fail(DAMAGED)
                huff.append(ht[(0, td)] + ht[(1, ta)])
                q.append(qt[tq])
            if (b[p + 5 + 2 * ns], b[p + 6 + 2 * ns], b[p + 7 + 2 * ns]) != (0, 63, 0):
                return fail(UNSUPPORTED)
            mcus = ((columns + 7) // 8) * ((rows + 7) // 8)
            out = dict(h, columns=columns, rows=rows, components=ns, restart=ri, scan=end)
            if mcus * ns > MAX_BLOCKS:
                return dict(out, status=TOO_LARGE, scan=0)
            per = ri if ri else mcus
            return dict(out, status=OK, blocks=mcus * ns, intervals=(mcus + per - 1) // per, q=np.array(q, np.int64), huff=huff)
        p = end


def header_info(data):
    """What the stand-alone host function xrit_jpegdec_header returns for a stream."""
    h = parse_header(data)
    return np.array([(h["columns"], h["rows"], h["components"], h["restart"], h["status"], h["scan"], h["blocks"], h["intervals"])], INFO_DTYPE)[0]


# ---- Huffman tables -----------------------------------------------------------------------------------------------------
def derived(bits, vals):
    """libjpeg's derived table: maxcode[1 .. 16] (-1: no code of that length), valptr[1 .. 16], and the lookahead table of
    2^LOOKAHEAD entries (length << 8 | symbol, 0: a longer code or none)."""
    maxcode, valptr, look = [-1] * 18, [0] * 17, [0] * (1 << LOOKAHEAD)
    code, k = 0, 0
    for l in range(1, 17):
        valptr[l] = k - code                            # symbol index = code + valptr[l]
        if bits[l - 1]:
            if l <= LOOKAHEAD:
                for i in range(bits[l - 1]):
                    for fill in range(1 << (LOOKAHEAD - l)):
                        look[(code + i) << (LOOKAHEAD - l) | fill] = l << 8 | vals[k + i]
            code += bits[l - 1]
            k += bits[l - 1]
            maxcode[l] = code - 1
        code <<= 1
    maxcode[17] = 0xFFFFF
    return maxcode, valptr, look


def decode_step(bits, vals, window, avail):
    """One code from a 16-bit window (the bits behind the stream's end are zero) of which `avail` are the stream's:
    -> (length, symbol), or (0, SHORT) / (0, BAD_CODE).  The rule the device and the host check share."""
    maxcode, valptr, look = derived(bits, vals)
    e = look[window >> (16 - LOOKAHEAD)]
    if e:
        l, sym = e >> 8, e & 255
    else:
        l = LOOKAHEAD + 1
        while l <= 16 and (window >> (16 - l)) > maxcode[l]:
            l += 1
        if l > 16:
            return (0, BAD_CODE if avail >= 16 else SHORT)
        sym = vals[(window >> (16 - l)) + valptr[l]]
    return (l, sym) if l <= avail else (0, SHORT)


def _full_lut(bits, vals):
    """code length and symbol for every 16-bit window (0: no code)."""
    length, symbol = np.zeros(1 << 16, np.int64), np.zeros(1 << 16, np.int64)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            if code < (1 << l):
                length[code << (16 - l):(code + 1) << (16 - l)] = l
                symbol[code << (16 - l):(code + 1) << (16 - l)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return length.tolist(), symbol.tolist()


# ---- the scan's bytes ---------------------------------------------------------------------------------------------------
def cut_scan(b, begin):
    """The bytes from `begin`: FF 00 -> FF, FF Dm ends an interval, any other FF xx (or a lone FF at the end) ends the scan.
    -> (the unstuffed bytes of every interval found, the m of every RSTm, 'eoi' / 'marker' / 'end', stuffed bytes)."""
    a = np.frombuffer(bytes(b[begin:]), np.uint8)
    n = len(a)
    nxt = np.concatenate([a[1:], [0x01]]).astype(np.int64) if n else np.zeros(0, np.int64)
    is_ff = a == 0xFF
    rst = is_ff & (nxt >= 0xD0) & (nxt <= 0xD7)
    term = is_ff & (nxt != 0) & ~rst
    stop = int(np.argmax(term)) if term.any() else n
    kind = "end"
    if stop < n:
        kind = "end" if stop + 1 >= n else ("eoi" if a[stop + 1] == 0xD9 else "marker")
    prev_ff = np.concatenate([[False], is_ff[:-1]])
    drop = rst | (prev_ff & ((a == 0) | ((a >= 0xD0) & (a <= 0xD7))))
    keep = ~drop
    keep[stop:] = False
    at = np.nonzero(rst[:stop])[0]
    kept_before = np.cumsum(keep) - keep
    bounds = [0] + [int(kept_before[i]) for i in at] + [int(keep.sum())]
    un = a[keep]
    return [un[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1)], [int(a[i + 1]) & 7 for i in at], kind, int((prev_ff & (a == 0))[:stop].sum())


# ---- the entropy walk ---------------------------------------------------------------------------------------------------
class Interval:
    """The bits of one restart interval and the tables of its components."""

    def __init__(self, data, luts):
        bits = np.unpackbits(np.asarray(data, np.uint8))
        self.nbits = len(bits)
        pad = np.concatenate([bits, np.zeros(32, np.uint8)]).astype(np.int64)
        w = np.zeros(self.nbits + 1, np.int64)
        for i in range(16):
            w += pad[i:i + self.nbits + 1] << (15 - i)
        self.w16 = w.tolist()
        self.luts = luts                                # per component (dc length, dc symbol, ac length, ac symbol)
        self.comps = len(luts)


def walk(iv, state, end, limit, first_block, sink, cnt):
    """Symbols that begin in front of bit `end`, from state (bit, component, zigzag index), at most `limit` blocks.
    sink(block, zigzag index, value) takes what is decoded (the DC as its difference).  -> (state behind, blocks completed,
    fault): a fault's state is (DEAD, 0, 0)."""
    p, c, z = state
    if p == DEAD:
        return (DEAD, 0, 0), 0, OK
    w16, nbits, done = iv.w16, iv.nbits, 0
    while p < end and done < limit:
        dl, ds, al, asym = iv.luts[c]
        w = w16[p]
        l = (dl if z == 0 else al)[w]
        avail = nbits - p
        if l == 0 or l > avail:
            return (DEAD, 0, 0), done, (BAD_CODE if l == 0 and avail >= 16 else SHORT)
        if cnt is not None and l > LOOKAHEAD:
            cnt["long_codes"] += 1
        sym = (ds if z == 0 else asym)[w]
        p += l
        if z == 0:
            r, s = 0, sym
        else:
            r, s = sym >> 4, sym & 15
            if s == 0:
                if r == 15:
                    if z + 16 > 64:
                        return (DEAD, 0, 0), done, INDEX
                    z += 16
                    if cnt is not None:
                        cnt["zrl"] += 1
                else:
                    z = 64
                    if cnt is not None:
                        cnt["eob"] += 1
                if z == 64:
                    z, c, done = 0, (c + 1) % iv.comps, done + 1
                continue
            z += r
            if z > 63:
                return (DEAD, 0, 0), done, INDEX
        if p + s > nbits:
            return (DEAD, 0, 0), done, SHORT
        v = w16[p] >> (16 - s) if s else 0
        if s and v < (1 << (s - 1)):
            v -= (1 << s) - 1
        p += s
        if sink is not None:
            sink(first_block + done, z, v)
        z += 1
        if z == 64:
            if cnt is not None:
                cnt["no_eob"] += 1
            z, c, done = 0, (c + 1) % iv.comps, done + 1
    return (p, c, z), done, OK


def serial_walk(iv, blocks, sink, cnt):
    """Form 0 and the arbiter of the statuses: -> the interval's fault."""
    _, done, fault = walk(iv, (0, 0, 0), iv.nbits, blocks, 0, sink, cnt)
    return fault if fault else (SHORT if done < blocks else OK)


def parallel_walk(iv, blocks, sink, S, cnt):
    """Form 1 as the device runs it: tiles of LANES subsequences of S bits; in a round every lane whose entry state changed
    walks again, then lane i + 1 takes lane i's exit; a round that changes nothing ends the tile.  Lane 0's entry is the
    carried, settled state, so after round r lanes 0 .. r - 1 have the serial walk's states: at most LANES rounds.  Then
    every lane walks once more from its settled entry with its block index and stores.  -> the interval's fault."""
    nsub = (iv.nbits + S - 1) // S
    carry, index = (0, 0, 0), 0
    if nsub > LANES:
        cnt["tiles_over_one"] += 1
    for t0 in range(0, nsub, LANES):
        subs = list(range(t0, min(t0 + LANES, nsub)))
        ends = [min((s + 1) * S, iv.nbits) for s in subs]
        entry = [carry] + [(s * S, 0, 0) for s in subs[1:]]
        out, dirty, rounds = [None] * len(subs), [True] * len(subs), 0
        while any(dirty):
            rounds += 1
            for i in range(len(subs)):
                if dirty[i]:
                    out[i] = walk(iv, entry[i], ends[i], 1 << 60, 0, None, None)
            dirty = [False] * len(subs)
            for i in range(len(subs) - 1):
                if out[i][0] != entry[i + 1]:
                    entry[i + 1], dirty[i + 1] = out[i][0], True
        assert rounds <= len(subs) + 1
        cnt["max_rounds"] = max(cnt["max_rounds"], rounds)
        cnt["rounds_over_one"] += rounds > 1
        for i in range(len(subs)):
            first = index + sum(o[1] for o in out[:i])
            if entry[i][0] == DEAD or first >= blocks:
                break
            state, done, fault = walk(iv, entry[i], ends[i], blocks - first, first, sink, cnt)
            if fault:
                return fault
            if state[2] != 0 and first + done < blocks:
                cnt["straddle"] += 1                    # the block goes on in the next subsequence
        index += sum(o[1] for o in out)
        carry = out[-1][0]
        if index >= blocks or carry[0] == DEAD:
            break
    return SHORT if index < blocks else OK


# ---- inverse DCT, range limit, colour -------------------------------------------------------------------------------------
def _i32(x):
    return np.asarray(x).astype(np.int64).astype(np.int32)


def idct_pass(d, shift):
    """One 1-D pass of jidctint along the last axis (8 values), in 32-bit two's complement; shift 11 (columns) or 18 (rows)."""
    with np.errstate(over="ignore"):
        d = [_i32(d[..., i]) for i in range(8)]
        k = lambda v: np.int32(v)
        z2, z3 = d[2], d[6]
        z1 = (z2 + z3) * k(4433)
        t2 = z1 + z3 * k(-15137)
        t3 = z1 + z2 * k(6270)
        t0 = (d[0] + d[4]) << k(13)
        t1 = (d[0] - d[4]) << k(13)
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * k(9633)
        t0, t1, t2, t3 = t0 * k(2446), t1 * k(16819), t2 * k(25172), t3 * k(12299)
        z1, z2, z3, z4 = z1 * k(-7373), z2 * k(-20995), z3 * k(-16069) + z5, z4 * k(-3196) + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        half = k(1 << (shift - 1))
        o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
        return np.stack([(v + half) >> k(shift) for v in o], -1)


def range_limit(v):
    """The sample of a value in front of the range limit: saturating (libjpeg's table wraps beyond 10 bits; its SIMD saturates)."""
    with np.errstate(over="ignore"):
        return np.clip(_i32(v) + np.int32(128), 0, 255)


def colour_terms(x):
    """jdcolor's four tables at sample value x: Cr -> R, Cb -> B, Cr -> G, Cb -> G (the last two in 16-bit fixed point)."""
    x = np.asarray(x, np.int64) - 128
    return (91881 * x + 32768) >> 16, (116130 * x + 32768) >> 16, -46802 * x, -22554 * x + 32768


def colour(ycc):
    """(..., 3) YCbCr samples -> (..., 3) RGB: libjpeg's ycc_rgb_convert."""
    y, cb, cr = (ycc[..., i].astype(np.int64) for i in range(3))
    crr, _, crg, _ = colour_terms(cr)
    _, cbb, _, cbg = colour_terms(cb)
    return np.clip(np.stack([y + crr, y + ((cbg + crg) >> 16), y + cbb], -1), 0, 255)


def samples(coef, q, cnt=None):
    """coef (blocks, 64) zigzag order, q (blocks, 64) natural order -> (blocks, 8, 8) samples 0 .. 255."""
    nat = np.zeros(coef.shape, np.int64)
    nat[:, js.ZIGZAG] = coef
    with np.errstate(over="ignore"):
        x = (_i32(nat) * _i32(q)).reshape(-1, 8, 8)
    cols = np.swapaxes(idct_pass(np.swapaxes(x, -1, -2), 11), -1, -2)
    v = idct_pass(cols, 18)
    if cnt is not None and v.size:
        cnt["max_in_front"] = max(cnt["max_in_front"], int(v.max()) + 128)
        cnt["min_in_front"] = min(cnt["min_in_front"], int(v.min()) + 128)
    return range_limit(v)


# ---- one image, a batch ---------------------------------------------------------------------------------------------------
def decode(data, form=0, S=DEFAULT_S, cnt=None):
    """One stream -> (status, pixels uint8 rows x columns [x 3] or None, the header's dict, intervals found)."""
    status, s, h, found = block_samples(data, form, S, cnt)
    if h["status"] != OK:
        return status, None, h, 0
    nc, columns, rows = h["components"], h["columns"], h["rows"]
    if status:
        return status, np.zeros((rows, columns) if nc == 1 else (rows, columns, 3), np.uint8), h, found
    bw, bh = (columns + 7) // 8, (rows + 7) // 8
    planes = s.reshape(bh, bw, nc, 8, 8).transpose(2, 0, 3, 1, 4).reshape(nc, bh * 8, bw * 8)[:, :rows, :columns]
    pixels = planes[0] if nc == 1 else colour(np.moveaxis(planes, 0, -1))
    return OK, pixels.astype(np.uint8), h, found


def checksum(data):
    """(status, sum of sample * (1 + its index in block order) mod 2^32): what csrc/jpegdec_host_check.cpp computes for a stream."""
    status, s, _, _ = block_samples(data)
    if status:
        return status, 0
    s = s.reshape(-1).astype(np.uint64)
    return OK, int((s * (np.arange(len(s), dtype=np.uint64) + 1)).sum() % (1 << 32))


def block_samples(data, form=0, S=DEFAULT_S, cnt=None):
    """One stream -> (status, samples (MCUs, components, 8, 8) or None, the header's dict, intervals found)."""
    cnt = new_counters() if cnt is None else cnt
    h = parse_header(data)
    if h["status"] != OK:
        return h["status"], None, h, 0
    nc, columns, rows = h["components"], h["columns"], h["rows"]
    mcus = h["blocks"] // nc
    per = h["restart"] if h["restart"] else mcus
    parts, ms, kind, stuffed = cut_scan(bytes(data), h["scan"])
    cnt["stuffed"] += stuffed
    cnt["restarts"] += len(ms)
    luts = [_full_lut(*hf[:2]) + _full_lut(*hf[2:]) for hf in h["huff"]]
    coef = np.zeros((h["blocks"], 64), np.int64)

    def sink_at(base):
        def sink(block, z, v):
            coef[base + block, z] = v
        return sink

    status = OK
    for k in range(h["intervals"]):
        if k >= len(parts):
            status = MARKER if kind == "marker" else INTERVALS
            break
        blocks = (min((k + 1) * per, mcus) - k * per) * nc
        iv = Interval(parts[k], luts)
        status = serial_walk(iv, blocks, sink_at(k * per * nc), cnt) if form == 0 else parallel_walk(iv, blocks, sink_at(k * per * nc), S, cnt)
        if status:
            break
        if k + 1 < h["intervals"] and k < len(ms) and ms[k] != (k & 7):
            status = RST_ORDER
            break
    if not status:
        status = INTERVALS if len(parts) > h["intervals"] else (MARKER if kind == "marker" else OK)
    if status:
        return status, None, h, len(parts)
    # DC prediction: per component a running sum that starts anew with every interval, kept in 16 bits
    dc = coef[:, 0].reshape(mcus, nc)
    total = np.cumsum(dc, 0)
    start = (np.arange(mcus) // per) * per              # the interval's first MCU
    before = np.where((start > 0)[:, None], total[np.maximum(start, 1) - 1], 0)
    coef[:, 0] = (total - before).astype(np.int16).reshape(-1)
    q = np.tile(h["q"], (mcus, 1))
    return OK, samples(coef, q, cnt).reshape(mcus, nc, 8, 8), h, len(parts)


def decode_batch(buf, items, cap=None, max_blocks=MAX_BLOCKS, max_scan=None, form=0, S=DEFAULT_S, cnt=None, cache=None):
    """buf: the bytes; items: (offset, length) per stream.  -> (pixels: the output buffer's bytes that the call writes, as a
    list of (offset, bytes) with the padding, records, summary).  An item that reaches outside buf is damaged.  max_scan:
    the scratch's room for scan bytes (the device: n_bytes), max_blocks: for blocks; the item that brings the call's running
    total of either above it, and every sound item behind it, is too large."""
    buf = bytes(buf)
    max_scan = len(buf) if max_scan is None else max_scan
    records, writes = np.zeros(len(items), RECORD_DTYPE), []
    summary = np.zeros(1, SUMMARY_DTYPE)[0]
    at, blocks_sum, scan_sum = 0, 0, 0
    for i, (offset, length) in enumerate(items):
        r = records[i]
        if offset > len(buf) or length > len(buf) - offset:
            r["status"] = DAMAGED
            continue
        data = buf[offset:offset + length]
        h = parse_header(data)
        if h["status"] == OK:
            blocks_sum += h["blocks"]
            scan_sum += length - h["scan"]
            if blocks_sum > max_blocks or scan_sum > max_scan:
                h = dict(h, status=TOO_LARGE)
        r["status"] = h["status"]
        r["columns"], r["rows"], r["components"], r["restart"] = h["columns"], h["rows"], h["components"], h["restart"]
        if h["status"] != OK:
            continue
        if cache is not None and data in cache:         # (a test's: the same stream many times)
            status, pixels, found = cache[data]
        else:
            status, pixels, _, found = decode(data, form, S, cnt)
            if cache is not None:
                cache[data] = (status, pixels, found)
        n = pixels.size
        padded = (n + 3) & ~3
        r["status"], r["offset"], r["length"], r["intervals"] = status, at, n, found
        if cap is None or at + padded <= cap:
            writes.append((at, pixels.tobytes() + bytes(padded - n)))
        else:
            summary["overflow"] = 1
        at += padded
    summary["bytes"] = at
    summary["images"] = int((records["status"] == OK).sum())
    summary["by_status"] = np.bincount(records["status"], minlength=N_STATUS)
    return writes, records, summary


# ---- the table csrc/jpegdec_host_check.cpp replays through jpegdec_rule.h -------------------------------------------------
def rule_table_text(optimised, files):
    """Lines of integers, the kind first.  0: an inverse-DCT pass (shift, 8 in, 8 out); 1: the range limit (the first value,
    n, the samples of n consecutive values); 2: the colour terms (the first x, n, four values per x); 3: a pixel (y, cb, cr,
    r, g, b); 4: a Huffman table (id, 16 counts, n, n symbols); 5: decode steps of a table (id, then window, avail, length,
    symbol or fault per step): per code one with the bits behind it random and, in the short tables, one with a bit too few,
    then all ones; 6: a
    stream (id, n, n bytes); 9: a stream that is stream 0 but for some bytes (id, then offset, value per byte); 7: the header
    of the first `cut` bytes of a stream for every cut in a range (id, first cut, last cut, xrit_jpegdec_info's eight fields);
    8: a stream decoded (id, status, the checksum of its samples).  optimised: (bits, vals) of a table that is not Annex K's;
    files: streams for the header parser, each cut at every byte."""
    rng = np.random.default_rng(2027)
    rows = []
    add = lambda kind, vals: rows.append(" ".join(str(int(v)) for v in [kind] + list(vals)))
    ins = [np.full(8, 1023 * 8), np.full(8, -1024 * 8), np.array([8191, -8192] * 4), np.array([-8192, 8191] * 4), np.array([2047 * 255] * 8),
           np.array([-2048 * 255, 2047 * 255] * 4), np.array([32767 * 255] * 8), np.array([-32768 * 255, 0, 0, 0, 32767 * 255, 0, 0, 1]), np.zeros(8), np.array([1] + [0] * 7)]
    ins += list(rng.integers(-2048, 2048, (8, 8))) + list(rng.integers(-(1 << 23), 1 << 23, (4, 8)))
    for d in ins:
        o = idct_pass(np.asarray(d, np.int64), 11)
        add(0, [11] + list(d) + list(o))
        add(0, [18] + list(o) + list(idct_pass(o, 18)))
    for d in rng.integers(-(1 << 20), 1 << 20, (4, 8)):
        add(0, [18] + list(d) + list(idct_pass(np.asarray(d, np.int64), 18)))
    add(1, [-640, 1281] + list(range_limit(np.arange(-640, 641))))
    for v in (-(1 << 31), (1 << 31) - 1, (1 << 31) - 128, (1 << 31) - 129, -(1 << 20), 1 << 20):
        add(1, [v, 1, range_limit(np.int64(v))])
    add(2, [0, 256] + [int(t) for x in range(256) for t in colour_terms(x)])
    for ycc in [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (128, 128, 128)] + \
            [tuple(v) for v in rng.integers(0, 256, (40, 3))]:
        add(3, list(ycc) + list(colour(np.array(ycc))))
    tables = [(b, v) for _, _, b, v in js.HUFFMAN] + [optimised]
    for t, (bits, vals) in enumerate(tables):
        add(4, [t] + list(bits) + [len(vals)] + list(vals))
        steps, code = [], 0
        for l in range(1, 17):
            for _ in range(bits[l - 1]):
                for fill, avail in ((int(rng.integers(0, 1 << (16 - l))), 16), (0, l - 1))[:2 if len(vals) < 100 else 1]:
                    w = code << (16 - l) | fill
                    steps += [w, avail] + list(decode_step(bits, vals, w, avail))
                code += 1
            code <<= 1
        for avail in (16, 15, 3, 0):                    # all ones: no code of Annex K's, the longest of a full table
            steps += [0xFFFF, avail] + list(decode_step(bits, vals, 0xFFFF, avail))
        add(5, [t] + steps)
    for i, f in enumerate(files):
        diff = [k for k in range(len(f)) if f[k] != files[0][k]] if i and len(f) == len(files[0]) else None
        if diff is not None and len(diff) <= 16:
            add(9, [i] + [v for k in diff for v in (k, f[k])])
        else:
            add(6, [i, len(f)] + list(f))
        add(8, [i] + list(checksum(f)))
        infos = [[int(v) for v in header_info(f[:cut]).tolist()] for cut in range(len(f) + 1)]
        first = 0
        for cut in range(1, len(f) + 2):
            if cut > len(f) or infos[cut] != infos[first]:
                add(7, [i, first, cut - 1] + infos[first])
                first = cut
    return "\n".join(rows) + "\n"
