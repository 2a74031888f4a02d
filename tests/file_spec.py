"""Python specification of the file assembler (xrit_files_*, FileAssembler) and a generator of
packet streams for it (test infrastructure).

The reference decoder ends at the VCDU, so this layer is specified here, from the LRIT/HRIT global specification (CGMS
03: the transport file's 10-byte header -- file counter and length in bits -- in front of the session layer's file, the
primary header record, the image structure record) and the GOES mission specific record 131 (Rice compression).  The
field offsets are as we read those documents; no recorded downlink was at hand (DESIGN.md lists what is unverified).
`process` is the serial statement, one packet at a time, and the device must equal it byte for byte."""
import copy

import numpy as np

import packet_spec as ps

N_VC = 64
N_APID = 2048
BEGINS, ENDS, ABORTED, LENGTH_MATCH = 1, 2, 4, 8

PIECE_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint32), ("index_in_file", np.uint32), ("file", np.uint32),
    ("seq_count", np.uint16), ("apid", np.uint16), ("vcid", np.uint8), ("seq_flags", np.uint8), ("reserved", np.uint8, (6,))])
assert PIECE_DTYPE.itemsize == 32

HEADER_FIELDS = ("data_bits", "header_length", "columns", "lines", "rice_flags", "file_type", "header_state",
                 "bits_per_pixel", "compression", "pixels_per_block", "lines_per_packet")
RECORD_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint64), ("file_offset", np.uint64), ("declared_bits", np.uint64),
    ("data_bits", np.uint64),
    ("header_length", np.uint32), ("first_piece", np.uint32), ("n_pieces", np.uint32), ("key_serial", np.uint32),
    ("file_counter", np.uint16), ("apid", np.uint16), ("columns", np.uint16), ("lines", np.uint16), ("rice_flags", np.uint16),
    ("vcid", np.uint8), ("flags", np.uint8), ("file_type", np.uint8), ("header_state", np.uint8),
    ("bits_per_pixel", np.uint8), ("compression", np.uint8), ("pixels_per_block", np.uint8), ("lines_per_packet", np.uint8),
    ("reserved", np.uint8, (6,))])
assert RECORD_DTYPE.itemsize == 80

COUNTERS = ("files_begun", "files_completed", "files_aborted", "bad_packets", "seq_gaps", "short_first", "orphans",
            "total_pieces", "total_bytes")


def be(b):
    return int.from_bytes(bytes(b), "big")


# ---- the serial statement ------------------------------------------------------------------------------------------
class Key:
    """What one (vcid, apid) carries."""

    def __init__(self):
        self.open = 0
        self.next_seq = 0
        self.key_serial = 0
        self.file_bytes = 0
        self.n_pieces = 0
        self.file_counter = 0
        self.declared_bits = 0
        for f in HEADER_FIELDS:
            setattr(self, f, 0)

    def as_tuple(self):
        return (self.open, self.next_seq, self.key_serial, self.file_bytes, self.n_pieces, self.file_counter,
                self.declared_bits) + tuple(getattr(self, f) for f in HEADER_FIELDS)


class State:
    def __init__(self):
        self.keys = {}
        for c in COUNTERS:
            setattr(self, c, 0)

    def key(self, v, a):
        return self.keys.setdefault((v, a), Key())

    def open_files(self):
        return sum(k.open for k in self.keys.values())


def parse_header(k, p):
    """The header fields of a file from its first piece's payload, into k.  Fields found before the walk stops are kept."""
    for f in HEADER_FIELDS:
        setattr(k, f, 0)
    n = len(p)
    if not (n >= 16 and p[0] == 0 and be(p[1:3]) == 16):
        return
    k.file_type, k.header_length, k.data_bits = p[3], be(p[4:8]), be(p[8:16])
    H = k.header_length
    k.header_state = 1
    if H > n:
        return
    q, image, rice = 16, False, False
    while q + 3 <= H:
        t, l = p[q], be(p[q + 1:q + 3])
        if l < 3 or q + l > H:
            return
        if t == 1 and l == 9 and not image:
            image = True
            k.bits_per_pixel, k.columns, k.lines, k.compression = p[q + 3], be(p[q + 4:q + 6]), be(p[q + 6:q + 8]), p[q + 8]
        if t == 131 and l == 7 and not rice:
            rice = True
            k.rice_flags, k.pixels_per_block, k.lines_per_packet = be(p[q + 3:q + 5]), p[q + 5], p[q + 6]
        q += l
    if q == H:
        k.header_state = 2


def process(state, data, desc, pkt_offsets):
    """One call: the packet assembler's bytes, PACKET_DTYPE descriptors and pkt_offsets (65,).  Returns (bytes, pieces,
    files, summary): the emitted payloads back to back, their PIECE_DTYPE and the RECORD_DTYPE of every file touched,
    all ordered by (vcid, apid, stream order), and a dict with the call's counts and the state's counters after it."""
    raw = np.asarray(data, np.uint8).tobytes()
    offs = [int(x) for x in np.asarray(pkt_offsets).reshape(N_VC + 1)]
    pieces, records, chunks = [], [], []
    nbytes = 0
    for v in range(N_VC):
        idx = np.arange(offs[v], offs[v + 1])
        if not len(idx):
            continue
        apids = desc["apid"][idx].astype(np.int64) & (N_APID - 1)
        for i in idx[np.argsort(apids, kind="stable")]:
            d = desc[i]
            a = int(d["apid"]) & (N_APID - 1)
            k = state.key(v, a)
            rec = getattr(k, "_rec", None)

            def touch(begins=False):
                r = {"offset": nbytes, "length": 0, "file_offset": k.file_bytes, "first_piece": len(pieces), "n_pieces": 0,
                     "flags": BEGINS if begins else 0, "key": k, "vcid": v, "apid": a}
                records.append(r)
                k._rec = len(records) - 1
                return r

            def current():
                return records[k._rec] if getattr(k, "_rec", None) is not None else touch()

            def abort():
                r = current()
                r["flags"] |= ABORTED
                r["snap"] = snapshot(k)
                k.open = 0
                k._rec = None
                state.files_aborted += 1

            off, length = int(d["offset"]), int(d["length"])
            if d["crc_ok"] == 0 or length < 8 or off + length > len(raw):
                state.bad_packets += 1
                if k.open:
                    abort()
                continue
            seq, flags = int(d["seq_count"]), int(d["seq_flags"]) & 3
            if k.open and seq != k.next_seq:
                state.seq_gaps += 1
                abort()
            u = raw[off + 6:off + length - 2]
            if flags in (1, 3):
                if k.open:
                    abort()
                if len(u) < 10:
                    state.short_first += 1
                    continue
                payload = u[10:]
                k.file_counter, k.declared_bits = be(u[0:2]), be(u[2:10])
                k.file_bytes, k.n_pieces = 0, 0
                k.key_serial += 1
                state.files_begun += 1
                parse_header(k, payload)
                r = touch(begins=True)
                k.open = 1
            else:
                if not k.open:
                    state.orphans += 1
                    continue
                payload = u
                r = current()
            pieces.append((nbytes, len(payload), k.n_pieces, k._rec, seq, a, v, flags))
            chunks.append(payload)
            nbytes += len(payload)
            r["length"] += len(payload)
            r["n_pieces"] += 1
            k.file_bytes += len(payload)
            k.n_pieces += 1
            k.next_seq = (seq + 1) & 0x3FFF
            state.total_pieces += 1
            state.total_bytes += len(payload)
            if flags in (2, 3):
                r["flags"] |= ENDS
                if 8 * k.file_bytes == k.declared_bits:
                    r["flags"] |= LENGTH_MATCH
                r["snap"] = snapshot(k)
                k.open = 0
                k._rec = None
                state.files_completed += 1
    for k in state.keys.values():           # a file that stays open: its record of this call is closed, the file is not
        if getattr(k, "_rec", None) is not None:
            records[k._rec]["snap"] = snapshot(k)
            k._rec = None
    out_p = np.zeros(len(pieces), PIECE_DTYPE)
    for i, p in enumerate(pieces):
        out_p[i] = p + ([0] * 6,)
    out_r = np.zeros(len(records), RECORD_DTYPE)
    for i, r in enumerate(records):
        s = r["snap"]
        for f in ("offset", "length", "file_offset", "first_piece", "n_pieces", "flags", "vcid", "apid"):
            out_r[i][f] = r[f]
        for f, val in s.items():
            out_r[i][f] = val
    summary = {"pieces": len(pieces), "bytes": nbytes, "files": len(records)}
    for c in COUNTERS:
        summary[c] = getattr(state, c)
    return np.frombuffer(b"".join(chunks), np.uint8), out_p, out_r, summary


def snapshot(k):
    s = {f: getattr(k, f) for f in HEADER_FIELDS}
    s.update(declared_bits=k.declared_bits, file_counter=k.file_counter, key_serial=k.key_serial - 1)
    return s


def is_rice_coded(rec, first_piece_length):
    """The link between the two stages (our convention): the file is an image whose pieces 1, 2, ... are one
    Rice-coded line each."""
    return (int(rec["header_state"]) == 2 and int(rec["file_type"]) == 0 and int(rec["compression"]) == 1 and
            1 <= int(rec["bits_per_pixel"]) <= 16 and int(rec["columns"]) >= 1 and
            int(rec["pixels_per_block"]) in (8, 16, 32, 64) and int(rec["header_length"]) == int(first_piece_length))


class Collector:
    """What a host does with the outputs of consecutive calls: appends every file's pieces, keeps the finished files,
    drops the aborted ones."""

    def __init__(self):
        self.partial = {}           # (vcid, apid, key_serial) -> bytearray
        self.done = []              # (vcid, apid, key_serial, bytes, record)
        self.aborted = []

    def add(self, data, pieces, files):
        raw = np.asarray(data, np.uint8).tobytes()
        for r in files:
            key = (int(r["vcid"]), int(r["apid"]), int(r["key_serial"]))
            buf = self.partial.setdefault(key, bytearray())
            assert len(buf) == int(r["file_offset"]), key
            buf += raw[int(r["offset"]):int(r["offset"]) + int(r["length"])]
            ps_ = pieces[int(r["first_piece"]):int(r["first_piece"]) + int(r["n_pieces"])]
            assert int(ps_["length"].sum()) == int(r["length"])
            if r["flags"] & ABORTED:
                self.aborted.append(key)
                del self.partial[key]
            elif r["flags"] & ENDS:
                self.done.append(key + (bytes(buf), r.copy()))
                del self.partial[key]


# ---- generator ------------------------------------------------------------------------------------------------------
def space_packet(apid, seq, flags, user, good_crc=True, header_bits=0):
    """A space packet around the given user data, CRC-16 behind it."""
    n = len(user) + 2 - 1
    assert n <= 65535
    head = bytes([(header_bits & 31) << 3 | apid >> 8, apid & 255, (flags & 3) << 6 | (seq >> 8) & 0x3F, seq & 255,
                  n >> 8, n & 255])
    crc = ps.crc16_fast(user) ^ (0 if good_crc else 0x0100)
    return head + bytes(user) + bytes([crc >> 8, crc & 255])


def record(t, body):
    return bytes([t]) + (len(body) + 3).to_bytes(2, "big") + bytes(body)


def lrit_file(data, file_type=0, image=None, rice=None, extra=(), declared_data_bits=None):
    """A session-layer file: primary header, optional image structure record (bits, columns, lines, compression),
    optional Rice record (flags, pixels per block, lines per packet), further records (type, body), then the data."""
    recs = b""
    if image is not None:
        bpp, cols, lines, comp = image
        recs += record(1, bytes([bpp]) + cols.to_bytes(2, "big") + lines.to_bytes(2, "big") + bytes([comp]))
    for t, body in extra:
        recs += record(t, body)
    if rice is not None:
        fl, ppb, lpp = rice
        recs += record(131, fl.to_bytes(2, "big") + bytes([ppb, lpp]))
    total = 16 + len(recs)
    bits = 8 * len(data) if declared_data_bits is None else declared_data_bits
    return bytes([0, 0, 16, file_type]) + total.to_bytes(4, "big") + bits.to_bytes(8, "big") + recs + bytes(data)


def packetise(file_bytes, apid, seq, counter, cuts=None, max_user=8190, declared_bits=None):
    """The packets of one file from sequence count `seq`: the 10-byte transport header in front, cut at the given file
    offsets (default: every max_user bytes of transport data).  -> (packets, next seq)."""
    bits = 8 * len(file_bytes) if declared_bits is None else declared_bits
    tp = counter.to_bytes(2, "big") + bits.to_bytes(8, "big") + bytes(file_bytes)
    if cuts is None:
        edges = list(range(0, len(tp), max_user))[1:]
    else:
        edges = [10 + c for c in cuts]
    parts = [tp[a:b] for a, b in zip([0] + edges, edges + [len(tp)])]
    out = []
    for i, part in enumerate(parts):
        flags = 3 if len(parts) == 1 else (1 if i == 0 else (2 if i == len(parts) - 1 else 0))
        out.append(space_packet(apid, seq, flags, part))
        seq = (seq + 1) & 0x3FFF
    return out, seq


def random_file(rng, max_bytes=30000):
    """A file with a well-formed header chain and random data; now and then an image or a Rice record in it."""
    data = rng.integers(0, 256, int(rng.integers(0, max_bytes)), dtype=np.uint8).tobytes()
    image = (int(rng.integers(1, 17)), int(rng.integers(1, 3000)), int(rng.integers(1, 3000)), int(rng.integers(0, 3))) \
        if rng.random() < 0.6 else None
    rice = (int(rng.integers(0, 65536)), int(rng.choice([8, 16, 32, 64, 5])), 1) if rng.random() < 0.4 else None
    extra = [(int(rng.choice([2, 3, 4, 5, 128, 129, 130])), rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8).tobytes())
             for _ in range(int(rng.integers(0, 4)))]
    return lrit_file(data, file_type=int(rng.choice([0, 0, 1, 2, 130])), image=image, rice=rice, extra=extra)


def random_stream(rng, n_files, keys, max_bytes=30000, max_user=None, seq_start=None):
    """n_files files over the given (vcid, apid) keys, interleaved at packet granularity.  -> (stream, files): stream a
    list of (vcid, packet bytes, tag) with tag = (vcid, apid, serial, index in file, pieces in file); files
    {(vcid, apid, serial): bytes}."""
    queues, files = {}, {}
    seq = {k: (int(rng.integers(0, 1 << 14)) if seq_start is None else seq_start) for k in keys}
    serial = {k: 0 for k in keys}
    for _ in range(n_files):
        k = keys[int(rng.integers(0, len(keys)))]
        f = random_file(rng, max_bytes)
        mu = int(rng.choice([50, 200, 1000, 8190])) if max_user is None else max_user
        pk, seq[k] = packetise(f, k[1], seq[k], int(rng.integers(0, 65536)), max_user=mu)
        files[k + (serial[k],)] = f
        queues.setdefault(k, []).extend((k[0], p, k + (serial[k], i, len(pk))) for i, p in enumerate(pk))
        serial[k] += 1
    stream = []
    live = [k for k in queues]
    pos = {k: 0 for k in live}
    while live:
        k = live[int(rng.integers(0, len(live)))]
        run = int(rng.integers(1, 6))
        stream.extend(queues[k][pos[k]:pos[k] + run])
        pos[k] += run
        if pos[k] >= len(queues[k]):
            live.remove(k)
    return stream, files


def stage_input(stream):
    """(bytes, PACKET_DTYPE descriptors, pkt_offsets) as the packet assembler hands them on, from (vcid, packet, ...)
    entries in stream order: VCID ascending, stream order within a VCID."""
    order = sorted(range(len(stream)), key=lambda i: stream[i][0])
    desc = np.zeros(len(order), ps.PACKET_DTYPE)
    pko = np.zeros(N_VC + 1, np.uint32)
    off = 0
    chunks = []
    for j, i in enumerate(order):
        v, pkt = stream[i][0], stream[i][1]
        total = len(pkt)
        computed = carried = ok = 0
        if total >= 8:
            computed = ps.crc16_fast(pkt[6:total - 2])
            carried = pkt[total - 2] << 8 | pkt[total - 1]
            ok = int(computed == carried)
        desc[j] = (off, total, 0, (pkt[0] & 7) << 8 | pkt[1], (pkt[2] & 0x3F) << 8 | pkt[3], computed, carried, v,
                   pkt[2] >> 6, ok, pkt[0] >> 3, [0] * 4)
        pko[v + 1] += 1
        chunks.append(pkt)
        off += total
    pko[1:] = np.cumsum(pko[1:])
    return np.frombuffer(b"".join(chunks), np.uint8), desc, pko


def cut_calls(rng, stream, k):
    """The stream in calls of 0 .. k packets."""
    pos = 0
    while pos < len(stream):
        n = int(rng.integers(0, k + 1))
        yield stream[pos:pos + n]
        pos += n


# ---- damage ----------------------------------------------------------------------------------------------------------
def remove(stream, i):
    return stream[:i] + stream[i + 1:]


def repeat(stream, i):
    return stream[:i + 1] + stream[i:]


def bad_crc(stream, i):
    v, p, *rest = stream[i]
    q = bytearray(p)
    q[-1] ^= 1
    return stream[:i] + [(v, bytes(q), *rest)] + stream[i + 1:]


def wrong_flags(stream, i, flags):
    v, p, *rest = stream[i]
    q = bytearray(p)
    q[2] = (q[2] & 0x3F) | flags << 6
    return stream[:i] + [(v, bytes(q), *rest)] + stream[i + 1:]


def short_first(stream, i, rng, n_user=None):
    """Entry i replaced by a first packet (same key and sequence count) with fewer than 10 bytes of user data."""
    v, p, *rest = stream[i]
    n_user = int(rng.integers(0, 10)) if n_user is None else n_user
    apid, seq = (p[0] & 7) << 8 | p[1], (p[2] & 0x3F) << 8 | p[3]
    return stream[:i] + [(v, space_packet(apid, seq, 1, rng.integers(0, 256, n_user, dtype=np.uint8).tobytes()), *rest)] + stream[i + 1:]


def random_packets(rng, count, vcids, apids=(0, 1, 64, 700, 2046)):
    """Packets of random bytes with consistent descriptors' worth of header (the walk must follow garbage exactly):
    random flags, sequence counts that mostly continue, user data whose first bytes often look like a primary header."""
    out = []
    seq = {}
    for _ in range(count):
        v, a = int(vcids[rng.integers(0, len(vcids))]), int(apids[rng.integers(0, len(apids))])
        s = seq.get((v, a), int(rng.integers(0, 1 << 14)))
        if rng.random() < 0.05:
            s = int(rng.integers(0, 1 << 14))
        seq[(v, a)] = (s + 1) & 0x3FFF
        user = bytearray(rng.integers(0, 256, int(rng.choice([0, 3, 9, 10, 11, 25, 26, 27, 40, 200, 900])), dtype=np.uint8).tobytes())
        if len(user) >= 26 and rng.random() < 0.8:
            user[10:13] = b"\x00\x00\x10"
            user[14:18] = int(rng.integers(0, len(user))).to_bytes(4, "big")
            if rng.random() < 0.7:
                q = 26
                while q + 3 <= len(user) and rng.random() < 0.8:
                    l = int(rng.choice([0, 3, 7, 9, 9, 12]))
                    user[q:q + 3] = bytes([int(rng.choice([1, 131, 2])), 0, l])
                    q += max(l, 1)
                if rng.random() < 0.5:
                    user[14:18] = (q - 10).to_bytes(4, "big")
        out.append((v, space_packet(a, s, int(rng.choice([0, 0, 1, 2, 3])), bytes(user), good_crc=rng.random() < 0.95)))
    return out


def damage(rng, stream, share=0.02):
    """About `share` of the entries hit, each by one kind drawn at random: removed, CRC broken, repeated, flags
    overwritten, replaced by a short first packet."""
    out = []
    for i, e in enumerate(stream):
        if rng.random() >= share:
            out.append(e)
            continue
        kind = int(rng.integers(0, 5))
        one = [e]
        if kind == 0:
            continue
        if kind == 1:
            one = bad_crc(one, 0)
        elif kind == 2:
            one = repeat(one, 0)
        elif kind == 3:
            one = wrong_flags(one, 0, int(rng.integers(0, 4)))
        else:
            one = short_first(one, 0, rng)
        out.extend(one)
    return out


# ---- generators that reach what the random ones leave to chance -------------------------------------------------------
MANY = [(v, a) for v in (0, 1, 5, 30, 62) for a in (0, 1, 2, 63, 64, 65, 700, 1023, 1024, 2046, 2047)]
# user data per packet: on either side of the device's 2048-byte gather step and of two such steps, what real LRIT
# packets carry (8190), and close to the most a space packet can (65534)
LONG_USERS = (2047, 2048, 2049, 4095, 4096, 4097, 8190, 65524)


def long_piece_stream(seed=0, count=600, keys=tuple(MANY[6:12]), share=0.01):
    """`count` packets of generated files over the keys, lightly damaged, every batch of six files cut every LONG_USERS[i]
    bytes and long enough to span several such packets.  -> (stream, the generated files as a set of bytes)."""
    rng = np.random.default_rng([seed, 5])
    stream, files, i = [], set(), 0
    while len(stream) < count + count // 8 + 8:
        mu = LONG_USERS[i % len(LONG_USERS)]
        i += 1
        s, f = random_stream(rng, 6, list(keys), max_bytes=6 * mu, max_user=mu)
        stream += s
        files |= set(f.values())
    return damage(rng, stream, share)[:count], files


def many_pieces_stream(seed=0, count=60000, share=0.005, tail=4000, long_keys=tuple(MANY[-6:])):
    """`count` packets of generated files over MANY, lightly damaged, 60 bytes of user data each, so that one call emits
    far more pieces than the device's gather grid takes in one pass (4096 workgroups of 8); among the last `tail` packets
    files cut every 8190 bytes on keys that sort last: long pieces for the second pass."""
    rng = np.random.default_rng([seed, 6])
    stream = []
    while len(stream) < count - tail:
        stream += random_stream(rng, 12, MANY, max_bytes=12000, max_user=60)[0]
    stream = stream[:count - tail]
    while len(stream) < count + count // 8:
        stream += random_stream(rng, 3, MANY, max_bytes=12000, max_user=60)[0]
        stream += random_stream(rng, 8, list(long_keys), max_bytes=50000, max_user=8190)[0]
    return damage(rng, stream, share)[:count]


_CACHE = {}


def many_pieces_case():
    """The stage's input for many_pieces_stream() and what the specification makes of it in one call and in the same call
    once more behind it: (args, [(result, state after it)] for the two calls), computed once for all the tests."""
    if "many" not in _CACHE:
        args = stage_input(many_pieces_stream())
        st, runs = State(), []
        for _ in range(2):
            res = process(st, *args)
            runs.append((res, copy.deepcopy(st)))
        _CACHE["many"] = (args, runs)
    return _CACHE["many"]
