"""Python specification of the image stage (xrit_images_*, ImageDecoder) on top of file_spec and
rice_spec, and a generator of streams of image files for it (test infrastructure).

One call takes one files call's outputs and decodes every Rice-coded line of every image in it; per (vcid, apid) it
carries whether a rice-coded image is open, its key_serial and its lines and faults so far.  `process` is the serial
statement, one record at a time, and the device must equal it byte for byte.  Like the two layers below, this one is
our reading of the documents; no recorded downlink was at hand."""
import numpy as np

import file_spec as fs
import rice_spec as rs

LINE_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint32), ("row", np.uint32), ("file", np.uint32), ("piece", np.uint32),
    ("samples", np.uint16), ("bits", np.uint8), ("status", np.uint8), ("reserved", np.uint8, (4,))])
assert LINE_DTYPE.itemsize == 32
FILE_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint64), ("first_line", np.uint32), ("n_lines", np.uint32), ("first_row", np.uint32),
    ("faults", np.uint32), ("lines_total", np.uint32), ("faults_total", np.uint32), ("columns", np.uint16), ("bits", np.uint8),
    ("rice", np.uint8), ("reserved", np.uint8, (4,))])
assert FILE_DTYPE.itemsize == 48
COUNTERS = ("images_begun", "images_completed", "images_aborted", "total_lines", "total_faults", "total_bytes")
MAX_LINE_BYTES = 131072           # 65535 samples of two bytes, padded to a multiple of 4


# ---- the serial statement ------------------------------------------------------------------------------------------
class Key:
    """What one (vcid, apid) carries."""

    def __init__(self):
        self.open = self.key_serial = self.lines = self.faults = 0

    def as_tuple(self):
        return (self.open, self.key_serial, self.lines, self.faults)


class State:
    def __init__(self):
        self.keys = {}
        for c in COUNTERS:
            setattr(self, c, 0)

    def key(self, v, a):
        return self.keys.setdefault((v, a), Key())


def params_ok(r):
    """Bits per pixel, block size and columns inside the Rice decoder's ranges (is_rice_coded without the header link)."""
    return (1 <= int(r["bits_per_pixel"]) <= 16 and int(r["columns"]) >= 1 and int(r["pixels_per_block"]) in rs.BLOCK_SIZES)


def padded(r):
    return (int(r["columns"]) * (1 if int(r["bits_per_pixel"]) <= 8 else 2) + 3) & ~3


def mark(r, first_length, first_index, k):
    """The decision for one record from the record, its first piece of the call and the key's state before the call
    -> dict(rice, continued, n_lines, first_row, base_lines, base_faults)."""
    begins = bool(int(r["flags"]) & fs.BEGINS)
    if begins:
        rice, cont = int(r["n_pieces"]) >= 1 and fs.is_rice_coded(r, first_length), False
    else:
        rice = cont = bool(k.open and k.key_serial == int(r["key_serial"]) and params_ok(r))
    m = dict(rice=int(rice), continued=int(cont), n_lines=0, first_row=0, base_lines=0, base_faults=0)
    if not rice:
        return m
    m["n_lines"] = int(r["n_pieces"]) - (1 if begins else 0)
    if cont:
        m["base_lines"], m["base_faults"] = k.lines, k.faults
    m["first_row"] = 0 if begins else ((first_index - 1 if first_index else 0) if int(r["n_pieces"]) else m["base_lines"])
    return m


def after(r, m, faults):
    """The key's state after a call whose last record of that key is r -> (open, key_serial, lines, faults)."""
    if not m["rice"]:
        return (0, int(r["key_serial"]), 0, 0)
    return (int(not int(r["flags"]) & (fs.ENDS | fs.ABORTED)), int(r["key_serial"]), m["base_lines"] + m["n_lines"],
            m["base_faults"] + faults)


def process(state, data, pieces, files, table=None):
    """One call on a files call's bytes, PIECE_DTYPE and RECORD_DTYPE.  Returns (bytes, lines, image_files, summary):
    the decoded lines back to back (uint8 or little-endian uint16, each padded with zeros to a multiple of 4 bytes),
    their LINE_DTYPE, one FILE_DTYPE per record, and a dict with the call's counts and the state's counters after it.
    table, a list: one row per record of what the rule was given and what it said (the host check's table)."""
    raw = np.asarray(data, np.uint8).tobytes()
    lines, chunks = [], []
    out_f = np.zeros(len(files), FILE_DTYPE)
    nbytes = images = 0
    last = {}
    for f, r in enumerate(files):
        key = (int(r["vcid"]), int(r["apid"]))
        k = state.key(*key)                                 # (as the call found it: the keys are rewritten behind the loop)
        first, count = int(r["first_piece"]), int(r["n_pieces"])
        mine = pieces[first:first + count]
        flen, fidx = (int(mine[0]["length"]), int(mine[0]["index_in_file"])) if count else (0, 0)
        m = mark(r, flen, fidx, k)
        faults = 0
        if m["rice"]:
            begins = int(r["flags"]) & fs.BEGINS
            n, J, S = int(r["bits_per_pixel"]), int(r["pixels_per_block"]), int(r["columns"])
            width, pad = (1 if n <= 8 else 2), padded(r)
            o = out_f[f]
            o["rice"], o["offset"], o["first_line"], o["n_lines"], o["first_row"] = 1, nbytes, len(lines), m["n_lines"], m["first_row"]
            o["columns"], o["bits"] = S, n
            for j in range(m["n_lines"]):
                p = first + (1 if begins else 0) + j
                pc = pieces[p]
                if int(pc["offset"]) + int(pc["length"]) > len(raw):        # a piece outside the bytes: nothing read, all 0
                    x, status = np.zeros(S, np.int64), 2
                else:
                    x, status = rs.decode(raw[int(pc["offset"]):int(pc["offset"]) + int(pc["length"])], n, J, S)
                body = x.astype("<u1" if n <= 8 else "<u2").tobytes()
                lines.append((nbytes, S * width, int(pc["index_in_file"]) - 1, f, p, S, n, status))
                chunks.append(body + bytes(pad - len(body)))
                nbytes += pad
                faults += status != 0
            o["length"] = m["n_lines"] * pad
            o["faults"], o["lines_total"], o["faults_total"] = faults, m["base_lines"] + m["n_lines"], m["base_faults"] + faults
            images += 1
            state.images_begun += bool(begins)
            state.images_completed += bool(int(r["flags"]) & fs.ENDS)
            state.images_aborted += bool(int(r["flags"]) & fs.ABORTED)
            state.total_lines += m["n_lines"]
            state.total_faults += faults
            state.total_bytes += m["n_lines"] * pad
        nxt = after(r, m, faults)
        last[key] = nxt
        if table is not None:
            table.append([int(r[c]) for c in TABLE_RECORD] + [flen, fidx] + list(k.as_tuple()) + [m[c] for c in TABLE_MARK] +
                         [padded(r) if m["rice"] else 0, faults] + list(nxt))
    for key, nxt in last.items():
        k = state.key(*key)
        k.open, k.key_serial, k.lines, k.faults = nxt
    out_l = np.zeros(len(lines), LINE_DTYPE)
    for i, ln in enumerate(lines):
        out_l[i] = ln + ([0] * 4,)
    summary = {"lines": len(lines), "bytes": nbytes, "images": images}
    for c in COUNTERS:
        summary[c] = int(getattr(state, c))
    return np.frombuffer(b"".join(chunks), np.uint8), out_l, out_f, summary


# the columns of the host check's table (tests/golden/image_rule_table.txt): the record's fields, the first piece's length
# and index_in_file, the key before (open, key_serial, lines, faults); then what the rule says: the mark, the padded line
# length, and -- given the faults -- the key after
TABLE_RECORD = ("flags", "n_pieces", "key_serial", "header_length", "header_state", "file_type", "compression", "bits_per_pixel",
                "columns", "pixels_per_block")
TABLE_MARK = ("rice", "continued", "n_lines", "first_row", "base_lines", "base_faults")


class Rows:
    """What a host does with the outputs of consecutive calls: places every line by (vcid, apid, key_serial, row)."""

    def __init__(self):
        self.rows = {}              # (vcid, apid, key_serial, row) -> (samples, status)

    def add(self, data, lines, files):
        raw = np.asarray(data, np.uint8)
        for ln in lines:
            r = files[int(ln["file"])]
            key = (int(r["vcid"]), int(r["apid"]), int(r["key_serial"]), int(ln["row"]))
            assert key not in self.rows, key
            a = raw[int(ln["offset"]):int(ln["offset"]) + int(ln["length"])]
            self.rows[key] = ((a if ln["bits"] <= 8 else a.view("<u2")).astype(np.int64), int(ln["status"]))

    def image(self, v, a, serial):
        """(samples (rows, columns), status (rows,)) of one image: its rows 0, 1, ... as far as they came."""
        got = []
        while (v, a, serial, len(got)) in self.rows:
            got.append(self.rows[(v, a, serial, len(got))])
        return np.stack([g[0] for g in got]), np.array([g[1] for g in got])


# ---- generator ------------------------------------------------------------------------------------------------------
def image_file(rng, n, J, cols, rows, kinds=rs.KINDS, spoil=None, force=None, coded=None):
    """A rice-coded image file -> (samples (rows, cols), file bytes, cuts): the cuts put the headers alone into the first
    packet and one coded line into each one behind it.  spoil(rng, line) damages a coded line before it is packed;
    force is rs.encode's.  coded: the `rows` lines to pack instead of rs.encode's (lines of another encoder); no
    samples are drawn then and None is returned for them."""
    if coded is None:
        img = np.stack([rs.samples(rng, kinds[int(rng.integers(0, len(kinds)))], n, J, cols) for _ in range(rows)])
        coded = [rs.encode(row, n, J, force=force) for row in img]
    else:
        assert len(coded) == rows and force is None
        img, coded = None, list(coded)
    if spoil is not None:
        coded = [spoil(rng, c) for c in coded]
    head = fs.lrit_file(b"", image=(n, cols, rows, 1), rice=(int(rng.integers(0, 65536)), J, 1),
                        declared_data_bits=8 * sum(len(c) for c in coded))
    cuts = [int(c) for c in np.cumsum([len(head)] + [len(c) for c in coded])[:-1]]
    return img, head + b"".join(coded), cuts


def stream_of(rng, items, seq_start=None, run=6):
    """items: (key, file bytes, cuts or None, max_user) in the order they are sent per key -> (vcid, packet, tag) entries,
    the keys interleaved at packet granularity; tag = (vcid, apid, serial on the key, index in file, packets of the file)."""
    queues, seq, serial = {}, {}, {}
    for key, data, cuts, max_user in items:
        s = seq.setdefault(key, int(rng.integers(0, 1 << 14)) if seq_start is None else seq_start)
        pk, seq[key] = fs.packetise(data, key[1], s, int(rng.integers(0, 65536)), cuts=cuts, max_user=max_user)
        n = serial.get(key, 0)
        serial[key] = n + 1
        queues.setdefault(key, []).extend((key[0], p, key + (n, i, len(pk))) for i, p in enumerate(pk))
    stream, live, pos = [], list(queues), {k: 0 for k in queues}
    while live:
        k = live[int(rng.integers(0, len(live)))]
        step = int(rng.integers(1, run))
        stream.extend(queues[k][pos[k]:pos[k] + step])
        pos[k] += step
        if pos[k] >= len(queues[k]):
            live.remove(k)
    return stream


def random_stream(rng, n_images, keys, n_other=0, max_cols=400, max_rows=12, spoil=None):
    """n_images rice-coded images of random (n, J, columns, rows) and n_other fs.random_file files over the keys ->
    (stream, images): images {(vcid, apid, serial): samples}."""
    order = ["image"] * n_images + ["other"] * n_other
    rng.shuffle(order)
    items, images, serial = [], {}, {}
    for what in order:
        key = keys[int(rng.integers(0, len(keys)))]
        n = serial.get(key, 0)
        serial[key] = n + 1
        if what == "image":
            img, data, cuts = image_file(rng, int(rng.integers(1, 17)), int(rng.choice(rs.BLOCK_SIZES)), int(rng.integers(1, max_cols)),
                                         int(rng.integers(1, max_rows)), spoil=spoil)
            images[key + (n,)] = img
            items.append((key, data, cuts, 8190))
        else:
            items.append((key, fs.random_file(rng, 3000), None, int(rng.choice([200, 1000]))))
    return stream_of(rng, items), images


def run_files(state, part):
    """The specification's files call on a piece of stream -> (bytes, pieces, files, summary dict)."""
    return fs.process(state, *fs.stage_input(part))


# ---- large calls from small ones ------------------------------------------------------------------------------------
def tiling_base(seed=50):
    """A small stream on one key, (0, 0), made to be tiled: a file that is no image, an 8-bit image (J = 8, 11 columns,
    2 rows, the second one truncated) and a 12-bit image (J = 16, 12 columns, 3 rows, the first one truncated) ->
    (stream, cut, images by serial): stream[:cut] ends inside the last image, two packets before its end, so a first
    call leaves it open with one line and one fault, and a second call holds nothing but its continuation."""
    rng = np.random.default_rng(seed)
    row = [0]

    def spoil(r, line):
        row[0] += 1
        return rs.truncate(r, line) if row[0] in (2, 3) else line

    plain = fs.lrit_file(rng.integers(0, 256, 50, dtype=np.uint8).tobytes(), file_type=2)
    img8, d8, c8 = image_file(rng, 8, 8, 11, 2, kinds=("uniform", "walk3"), spoil=spoil)
    img12, d12, c12 = image_file(rng, 12, 16, 12, 3, kinds=("uniform", "walk3"), spoil=spoil)
    stream = stream_of(rng, [((0, 0), plain, None, 40), ((0, 0), d8, c8, 8190), ((0, 0), d12, c12, 8190)])
    return stream, len(stream) - 2, {1: img8, 2: img12}



def tile_call(files_out, copies):
    """A files call (bytes, pieces, records, summary) whose records all sit on one key, repeated over `copies` distinct
    keys: copy c on (c // 2048, c % 2048), its bytes, pieces and records behind those of copy c - 1.  The result is
    ordered by (vcid, apid, stream order) like every files call; every count of the summary is the base's times
    `copies` (the counters too: what a stream with that many keys leaves when every call of it is tiled alike)."""
    data, pieces, files, summ = files_out
    data, pieces, files = np.asarray(data, np.uint8), np.asarray(pieces), np.asarray(files)
    assert 1 <= copies <= fs.N_VC * fs.N_APID
    assert len({(int(r["vcid"]), int(r["apid"])) for r in files}) <= 1 and int(summ["files"]) == len(files)
    assert int(summ["pieces"]) == len(pieces) and int(summ["bytes"]) == len(data)
    c = np.arange(copies, dtype=np.uint64)
    per_piece, per_file = np.repeat(c, len(pieces)), np.repeat(c, len(files))
    out_p, out_f = np.tile(pieces, copies), np.tile(files, copies)
    out_p["offset"] += per_piece * np.uint64(len(data))
    out_p["file"] += (per_piece * np.uint64(len(files))).astype(np.uint32)
    out_f["offset"] += per_file * np.uint64(len(data))
    out_f["first_piece"] += (per_file * np.uint64(len(pieces))).astype(np.uint32)
    for a, per in ((out_p, per_piece), (out_f, per_file)):
        a["vcid"], a["apid"] = per // np.uint64(fs.N_APID), per % np.uint64(fs.N_APID)
    return np.tile(data, copies), out_p, out_f, {k: int(v) * copies for k, v in summ.items()}


def head_of_call(call, n_records):
    """The first n_records records of a files call with exactly their pieces and bytes (records, pieces and bytes lie in
    the same order, so each is a prefix) -> (bytes, pieces, records, summary: the three counts of the call alone)."""
    data, pieces, files, _ = call
    assert 0 <= n_records <= len(files)
    head = files[:n_records]
    n_pieces = int(head[-1]["first_piece"]) + int(head[-1]["n_pieces"]) if n_records else 0
    n_bytes = int(head[-1]["offset"]) + int(head[-1]["length"]) if n_records else 0
    assert n_pieces <= len(pieces) and n_bytes <= len(data)
    return data[:n_bytes], pieces[:n_pieces], head, {"files": n_records, "pieces": n_pieces, "bytes": n_bytes}
