"""Python specification of the packet assembler (xrit_packets_*, PacketAssembler) and a generator
of VCDU streams for it (test infrastructure).

The reference decoder ends at the VCDU, so this layer is specified here, from the CCSDS AOS space data link
recommendation (the M_PDU and its first header pointer), the space packet recommendation (the 6-byte primary header) and
the LRIT/HRIT global specification (the CP_PDU's CRC-16 over its data field): `process` is the serial statement, one
row at a time, and the device must equal it byte for byte."""
import binascii

import numpy as np

import ccsds

VCDU_BYTES = 892
ZONE = 884                       # the M_PDU packet zone: VCDU bytes 8 .. 892
N_VC = 64
FILL_VC = 63                     # fill VCDUs: ignored entirely
FHP_NONE = 2047                  # no packet header starts in this zone
FHP_IDLE = 2046                  # idle data only
APID_FILL = 2047
PACKET_MAX = 65542

PACKET_DTYPE = np.dtype([
    ("offset", np.uint64), ("length", np.uint32), ("first_counter", np.uint32),
    ("apid", np.uint16), ("seq_count", np.uint16), ("crc_computed", np.uint16), ("crc_carried", np.uint16),
    ("vcid", np.uint8), ("seq_flags", np.uint8), ("crc_ok", np.uint8), ("header_bits", np.uint8),
    ("reserved", np.uint8, (4,))])
assert PACKET_DTYPE.itemsize == 32

COUNTERS = ("packets", "crc_failures", "fill_packets", "discarded", "bad_fhp", "rows")


# ---- CRC-16/CCITT-FALSE ------------------------------------------------------------------------------------------
def crc16(data, reg=0xFFFF):
    """Polynomial 0x1021, initial value 0xFFFF, MSB first, no reflection, no final XOR: the definition, bit by bit."""
    for b in bytes(data):
        reg ^= b << 8
        for _ in range(8):
            reg = ((reg << 1) ^ 0x1021) & 0xFFFF if reg & 0x8000 else (reg << 1) & 0xFFFF
    return reg


def crc16_fast(data):
    """The same through the C library's table (binascii.crc_hqx is this polynomial, MSB first; test_packet_spec holds
    it against crc16)."""
    return binascii.crc_hqx(bytes(data), 0xFFFF)


def gf_mul(a, b):
    """a * b modulo x^16 + x^12 + x^5 + 1 over GF(2)."""
    r = 0
    for i in range(15, -1, -1):
        r <<= 1
        if r & 0x10000:
            r ^= 0x11021
        if (b >> i) & 1:
            r ^= a
    return r


def x_pow8(n):
    """x^(8 n) modulo the polynomial: what n zero bytes do to the CRC register."""
    r, p = 1, 0x100
    while n:
        if n & 1:
            r = gf_mul(r, p)
        p = gf_mul(p, p)
        n >>= 1
    return r


def crc_combine(crc_a, crc0_b, len_b):
    """crc(A | B) from crc(A) and the zero-start CRC of B: shift(crc(A), |B|) ^ crc0(B)."""
    return gf_mul(crc_a, x_pow8(len_b)) ^ crc0_b


# ---- the serial statement ------------------------------------------------------------------------------------------
class State:
    """What one handle carries: per channel the last counter, the pending bytes and where they began; the counters."""

    def __init__(self):
        self.last = [-1] * N_VC
        self.pending = [b""] * N_VC
        self.first_counter = [0] * N_VC
        for k in COUNTERS:
            setattr(self, k, [0] * N_VC)

    def total(self, name):
        return sum(getattr(self, name))


def _total(p):
    return 7 + (p[4] << 8 | p[5])


def _finish(s, v, pkt, first_counter, out):
    if ((pkt[0] & 7) << 8 | pkt[1]) == APID_FILL:
        s.fill_packets[v] += 1
        return
    s.packets[v] += 1
    total = len(pkt)
    computed = carried = ok = 0
    if total >= 8:
        computed = crc16_fast(pkt[6:total - 2])
        carried = pkt[total - 2] << 8 | pkt[total - 1]
        ok = int(computed == carried)
    if not ok:
        s.crc_failures[v] += 1
    out.append((v, first_counter, pkt, computed, carried, ok))


def _discard(s, v):
    if s.pending[v]:
        s.discarded[v] += 1
        s.pending[v] = b""


def _row(s, v, row, out):
    c = row[2] << 16 | row[3] << 8 | row[4]
    fhp = (row[6] & 7) << 8 | row[7]
    zone = row[8:VCDU_BYTES]
    # 1: continuity
    if s.last[v] >= 0 and c != (s.last[v] + 1) & 0xFFFFFF:
        _discard(s, v)
    s.last[v] = c
    s.rows[v] += 1
    # 2: the bytes in front of the first header
    if fhp == FHP_NONE:
        if not s.pending[v]:
            return
        p = s.pending[v] + zone
        if len(p) >= 6 and len(p) > _total(p):
            s.pending[v] = p
            _discard(s, v)
        elif len(p) >= 6 and len(p) == _total(p):
            s.pending[v] = b""
            _finish(s, v, p, s.first_counter[v], out)
        else:
            s.pending[v] = p
        return
    if fhp >= ZONE:
        if fhp != FHP_IDLE:
            s.bad_fhp[v] += 1
        _discard(s, v)
        return
    if s.pending[v]:
        p = s.pending[v] + zone[:fhp]
        if len(p) >= 6 and len(p) == _total(p):
            s.pending[v] = b""
            _finish(s, v, p, s.first_counter[v], out)
        else:
            _discard(s, v)
    # 3: the packets that begin in this zone
    p = fhp
    while p < ZONE:
        if ZONE - p < 6:
            s.pending[v], s.first_counter[v] = zone[p:], c
            break
        total = _total(zone[p:p + 6])
        if p + total <= ZONE:
            _finish(s, v, zone[p:p + total], c, out)
            p += total
        else:
            s.pending[v], s.first_counter[v] = zone[p:], c
            break


def process(state, vcdu, offsets):
    """One call: vcdu rows (n, 892) grouped by VCID, offsets (65,).  Returns (bytes, packets, pkt_offsets, summary):
    the emitted packets back to back as uint8, their PACKET_DTYPE descriptors, the exclusive prefix of the per-channel
    packet counts (65 entries) and a dict with the call's packets / bytes and the handle's counters after it."""
    vcdu = np.ascontiguousarray(vcdu, np.uint8).reshape(-1, VCDU_BYTES)
    offsets = [int(x) for x in np.asarray(offsets).reshape(N_VC + 1)]
    out = []
    pkt_offsets = np.zeros(N_VC + 1, np.uint32)
    for v in range(N_VC):
        pkt_offsets[v] = len(out)
        if v == FILL_VC:
            continue
        for r in range(offsets[v], offsets[v + 1]):
            _row(state, v, vcdu[r].tobytes(), out)
    pkt_offsets[N_VC] = len(out)
    desc = np.zeros(len(out), PACKET_DTYPE)
    off = 0
    for i, (v, fc, pkt, computed, carried, ok) in enumerate(out):
        desc[i] = (off, len(pkt), fc, (pkt[0] & 7) << 8 | pkt[1], (pkt[2] & 0x3F) << 8 | pkt[3], computed, carried, v,
                   pkt[2] >> 6, ok, pkt[0] >> 3, [0] * 4)
        off += len(pkt)
    data = np.frombuffer(b"".join(o[2] for o in out), np.uint8)
    summary = {"packets": len(out), "bytes": off, "total_packets": state.total("packets")}
    for k in COUNTERS[1:]:
        summary[k] = state.total(k)
    return data, desc, pkt_offsets, summary


def packets_of(data, desc):
    raw = np.asarray(data, np.uint8).tobytes()
    return [raw[int(o):int(o) + int(n)] for o, n in zip(desc["offset"], desc["length"])]


# ---- generator ------------------------------------------------------------------------------------------------------
SIZES = [7, 8] + list(range(9, 65)) + list(range(876, 893)) + [8198, PACKET_MAX]


def make_packet(apid, seq_count, total, rng, header_bits=0, seq_flags=3, good_crc=True):
    """A space packet of `total` bytes: primary header, random data field, CRC-16 of the data field in front of it in the
    last two bytes (a packet of 7 bytes has no room for one)."""
    assert 7 <= total <= PACKET_MAX
    n = total - 7
    head = bytes([(header_bits & 31) << 3 | apid >> 8, apid & 255, (seq_flags & 3) << 6 | (seq_count >> 8) & 0x3F,
                  seq_count & 255, n >> 8, n & 255])
    if total < 8:
        return head + rng.integers(0, 256, 1, dtype=np.uint8).tobytes()
    data = rng.integers(0, 256, total - 8, dtype=np.uint8).tobytes()
    crc = crc16_fast(data) ^ (0 if good_crc else 0x0100)
    return head + data + bytes([crc >> 8, crc & 255])


def random_packets(rng, count, vcids, sizes=None, weights=None):
    """`count` packets (vcid, bytes) on the given channels, sizes drawn from `sizes` (default: SIZES, the two long ones
    rare), a sequence count per (vcid, apid)."""
    sizes = SIZES if sizes is None else sizes
    if weights is None:
        weights = np.array([0.02 if s > 1000 else 1.0 for s in sizes])
    weights = np.asarray(weights, float) / np.sum(weights)
    seq = {}
    out = []
    for _ in range(count):
        v = int(vcids[rng.integers(0, len(vcids))])
        apid = int(rng.choice([0, 1, 64, 700, 2046]))
        k = seq.get((v, apid), 0)
        seq[(v, apid)] = (k + 1) & 0x3FFF
        total = int(sizes[rng.choice(len(sizes), p=weights)])
        out.append((v, make_packet(apid, k, total, rng, header_bits=int(rng.integers(0, 32)),
                                   seq_flags=int(rng.integers(0, 4)))))
    return out


class Stream:
    """The rows of one channel and where every generated packet lies in them."""

    def __init__(self, vcid):
        self.vcid = vcid
        self.rows = []            # 892-byte rows as bytearrays
        self.packets = []         # (bytes, first row, last row)
        self.headers = []         # (row, offset in the zone) of every header that lies in one zone


def build_stream(vcid, packets, rng, scid=0x8C, start_counter=None, fill=0.15, idle=0.1):
    """M_PDU zones for one channel: the packets back to back, now and then a fill packet (APID 2047) between two of them
    or an idle zone (fhp = 2046) where a packet ends exactly at a zone's end; a fill packet completes the last zone."""
    st = Stream(vcid)
    body = bytearray()
    starts = []                   # (position in body, packet index or -1)
    marks = []                    # body positions (multiples of ZONE) in front of which an idle zone goes
    for i, pkt in enumerate(packets):
        if rng.random() < fill:
            n = int(rng.integers(7, 300))
            starts.append((len(body), -1))
            body += make_packet(APID_FILL, 0, n, rng)
        if len(body) % ZONE == 0 and rng.random() < idle:
            marks.append(len(body))
        starts.append((len(body), i))
        body += pkt
    rest = -len(body) % ZONE
    if rest:
        starts.append((len(body), -1))
        body += make_packet(APID_FILL, 0, rest if rest >= 7 else rest + ZONE, rng)
    nz = len(body) // ZONE
    fhp = [FHP_NONE] * nz
    for pos, _ in reversed(starts):
        fhp[pos // ZONE] = pos % ZONE
    counter = int(rng.integers(0, 1 << 24)) if start_counter is None else start_counter
    zone_row = []                 # body zone -> row index
    for z in range(nz):
        if z * ZONE in marks:
            st.rows.append(_row_bytes(scid, vcid, counter, FHP_IDLE, rng.integers(0, 256, ZONE, dtype=np.uint8).tobytes(), rng))
            counter = (counter + 1) & 0xFFFFFF
        zone_row.append(len(st.rows))
        st.rows.append(_row_bytes(scid, vcid, counter, fhp[z], bytes(body[z * ZONE:(z + 1) * ZONE]), rng))
        counter = (counter + 1) & 0xFFFFFF
    for pos, i in starts:
        if pos % ZONE <= ZONE - 6:
            st.headers.append((zone_row[pos // ZONE], pos % ZONE))
        if i >= 0:
            st.packets.append((bytes(packets[i]), zone_row[pos // ZONE], zone_row[(pos + len(packets[i]) - 1) // ZONE]))
    return st


def _row_bytes(scid, vcid, counter, fhp, zone, rng):
    spare = int(rng.integers(0, 32)) << 3          # the five spare bits are ignored
    return bytearray(ccsds.vcdu_header(scid, vcid, counter).tobytes() + bytes([spare | fhp >> 8, fhp & 255]) + zone)


def build_streams(packets, rng, **kw):
    """{vcid: Stream} from a list of (vcid, bytes) packets."""
    by_vc = {}
    for v, pkt in packets:
        by_vc.setdefault(v, []).append(pkt)
    return {v: build_stream(v, by_vc[v], rng, **kw) for v in sorted(by_vc)}


def damage(st, rng, remove=0.0, repeat=0.0, wrong_fhp=0.0, bad_length=0.0, flip=0.0):
    """The rows of a Stream after damage, as a list of bytes: each kind hits about the given share of the rows.  Returns
    (rows, removed): `removed` holds the indices (in st.rows) of the rows taken out."""
    rows = [bytearray(r) for r in st.rows]
    n = len(rows)
    for r, off in st.headers:
        if rng.random() < bad_length * n / max(len(st.headers), 1):
            rows[r][8 + off + 4 + int(rng.integers(0, 2))] ^= 1 << int(rng.integers(0, 8))
    for r in range(n):
        if rng.random() < wrong_fhp:
            f = int(rng.integers(0, 2048))
            rows[r][6], rows[r][7] = (rows[r][6] & 0xF8) | f >> 8, f & 255
        if rng.random() < flip:
            rows[r][8 + int(rng.integers(0, ZONE))] ^= 1 << int(rng.integers(0, 8))
    removed = set(r for r in range(n) if rng.random() < remove)
    out = []
    for r in range(n):
        if r in removed:
            continue
        out.append(bytes(rows[r]))
        if rng.random() < repeat:
            out.append(bytes(rows[r]))
    return out, removed


def group(rows_by_vc):
    """(vcdu, offsets) as the demux hands them on: the channels' rows in ascending VCID order."""
    offsets = np.zeros(N_VC + 1, np.uint32)
    parts = []
    for v in range(N_VC):
        rows = rows_by_vc.get(v, [])
        offsets[v + 1] = offsets[v] + len(rows)
        parts.extend(rows)
    vcdu = np.frombuffer(b"".join(bytes(r) for r in parts), np.uint8).reshape(-1, VCDU_BYTES) if parts else \
        np.zeros((0, VCDU_BYTES), np.uint8)
    return vcdu, offsets


# ---- generators that reach what the random ones leave to chance -------------------------------------------------------
# (total, zone offset of the long packet's first byte): ten rows; the longest packet with one byte in its last row, so
# that a cut in front of that row leaves 65541 bytes pending; the longest packet beginning 1, 3, 4, 5 bytes before a
# zone's end: the header split by the rows' joint, with 5 the length field itself
LONG_CASES = {"ten_rows": (8198, 300), "one_byte_last": (PACKET_MAX, 759), "tail_1": (PACKET_MAX, ZONE - 1),
              "tail_3": (PACKET_MAX, ZONE - 3), "tail_4": (PACKET_MAX, ZONE - 4), "tail_5": (PACKET_MAX, ZONE - 5)}


def long_packet_stream(case, vcid=5, seed=0):
    """-> (Stream, index of the long packet in its .packets): one channel without fill packets between the packets or
    idle zones: three short packets that end where the long one is to begin, the long one, three short ones."""
    total, start = LONG_CASES[case]
    rng = np.random.default_rng([seed, total, start, vcid])
    front = start if start >= 21 else start + ZONE
    sizes = [front // 3, front // 3, front - 2 * (front // 3)] + [total] + [40, 60, 80]
    pkts = [make_packet(20 + i % 3, i, n, rng) for i, n in enumerate(sizes)]
    st = build_stream(vcid, pkts, rng, fill=0.0, idle=0.0)
    assert [p for p, _, _ in st.packets] == pkts and st.packets[3][1] == front // ZONE
    return st, 3


def rows_of(st):
    return [bytes(r) for r in st.rows]


def with_fhp(row, fhp):
    """The row under another first header pointer (the spare bits kept)."""
    r = bytearray(row)
    r[6], r[7] = (r[6] & 0xF8) | fhp >> 8, fhp & 255
    return bytes(r)


def with_counter(row, counter):
    r = bytearray(row)
    r[2], r[3], r[4] = counter >> 16 & 255, counter >> 8 & 255, counter & 255
    return bytes(r)


def counter_of(row):
    return row[2] << 16 | row[3] << 8 | row[4]


def run_calls(calls, state=None):
    """The calls ({vcid: rows} each) through the specification.  -> (state, [(result of process, the pending lengths
    after the call)])."""
    state = State() if state is None else state
    out = []
    for part in calls:
        res = process(state, *group(part))
        out.append((res, [len(p) for p in state.pending]))
    return state, out


def joint_damage(case, vcid=5):
    """[(name, first call, second call)] as row lists: a long packet's rows cut at a handful of places, the second call
    beginning with a row that does not continue what the first one left pending."""
    st, k = long_packet_stream(case, vcid)
    rows = rows_of(st)
    _, a, b = st.packets[k]
    out = []
    for c in sorted({a + 1, a + 2, (a + b) // 2, b}):
        head, rest = rows[:c], rows[c:]
        if len(rest) > 1:
            out.append((f"{c}_skipped_counter", head, rest[1:]))
        out.append((f"{c}_repeated_row", head, [rows[c - 1]] + rest))
        for fhp in (0, 400, FHP_IDLE, 1000, 2045):
            out.append((f"{c}_fhp_{fhp}", head, [with_fhp(rest[0], fhp)] + rest[1:]))
        if c < b:
            # the packet's last row, with its right pointer and the next counter, in front of the zones it needs
            moved = with_counter(rows[b], counter_of(rows[c]))
            out.append((f"{c}_early_end", head, [moved] + [with_counter(r, (counter_of(r) + 1) & 0xFFFFFF) for r in rest]))
    _, start = LONG_CASES[case]
    if ZONE - start < 6:
        # the length field's low byte lies in the second row's zone: the right pointer (2047), another length
        at = 8 + 5 - (ZONE - start)
        for flip in (0x01, 0x80):
            r = bytearray(rows[a + 1])
            r[at] ^= flip
            out.append((f"{a + 1}_length_{flip}", rows[:a + 1], [bytes(r)] + rows[a + 2:]))
    return out


def three_call_cases(seed=0, count=30):
    """[(c1, c2, calls)], calls three {vcid: rows}: channel 5 carries LONG_CASES["one_byte_last"] cut in front of rows
    c1 <= c2 that both lie inside the long packet, so the first call leaves it pending, the second brings only rows
    with pointer 2047 (none where c1 == c2) and the third ends it; channel 9 carries "tail_5" cut likewise at places of
    its own, always with rows in the middle call; channel 63 has rows in every call.  -> (cases, {vcid: Stream})."""
    rng = np.random.default_rng([seed, 3])
    sa, ka = long_packet_stream("one_byte_last", 5)
    sb, kb = long_packet_stream("tail_5", 9)
    ra, rb = rows_of(sa), rows_of(sb)
    (_, a0, a1), (_, b0, b1) = sa.packets[ka], sb.packets[kb]
    pairs = [(a0 + 1, a0 + 1), (a1, a1), (a0 + 1, a1), (a0 + 1, a0 + 2), (a1 - 1, a1), (a0 + 37, a0 + 37)]
    while len(pairs) < count:
        c1 = int(rng.integers(a0 + 1, a1 + 1))
        pairs.append((c1, c1 if rng.random() < 0.15 else int(rng.integers(c1, a1 + 1))))
    cases = []
    for c1, c2 in pairs:
        d1 = int(rng.integers(b0 + 1, b1))
        d2 = int(rng.integers(d1 + 1, b1 + 1))
        junk = [[bytes(r) for r in rng.integers(0, 256, (int(rng.integers(1, 4)), VCDU_BYTES), dtype=np.uint8)] for _ in range(3)]
        cases.append((c1, c2, [{5: ra[:c1], 9: rb[:d1], 63: junk[0]}, {5: ra[c1:c2], 9: rb[d1:d2], 63: junk[1]},
                               {5: ra[c2:], 9: rb[d2:], 63: junk[2]}]))
    return cases, {5: sa, 9: sb}


def chunks_of(total):
    """The 4096-byte steps in which the device runs a packet's CRC (they end where the CRC's two bytes begin)."""
    return -(-(total - 2) // 4096) if total >= 8 else 0


# every total around the first two chunk edges: the zeroed header and the initial value's XOR on data bytes 6 and 7 fall
# on either side of them; the two-byte CRC on either side of a step's end
LADDER_EDGES = list(range(4097, 4108)) + list(range(8193, 8204))
# one total per chunk count 4 .. 16: the first chunk holding 1, 6, 7, 8 bytes, an exact edge, the others anywhere
LADDER_STEPS = [4096 * 3 + 2 + 1, 4096 * 5 + 2, 4096 * 5 + 2 + 6, 4096 * 6 + 2 + 7, 4096 * 7 + 2 + 8] + \
    [4096 * (m - 1) + 2 + (977 * m) % 4096 for m in range(9, 17)]
LADDER = LADDER_EDGES + LADDER_STEPS + [PACKET_MAX - 1]
assert [chunks_of(t) for t in LADDER_STEPS] == list(range(4, 17))


def crc_ladder(flip=False, seed=0):
    """-> ({vcid: Stream}, long): a good-CRC packet of every total in LADDER on channels 5 and 30, short packets between
    them so that they begin at varied zone offsets; `long` the generated long packets.  With flip, the same packets with
    one bit of one data byte of every long packet changed (the first data bytes, the last, the bytes on either side of the
    last chunk's beginning, one in the middle, in turn)."""
    rng = np.random.default_rng([seed, 4])
    totals = [LADDER[i] for i in rng.permutation(len(LADDER))]
    packets, long = [], []
    for i, total in enumerate(totals):
        v = (5, 30)[i % 2]
        for _ in range(int(rng.integers(1, 4))):
            packets.append((v, make_packet(1 + i % 5, len(packets), int(rng.integers(7, 300)), rng)))
        p = make_packet(100 + i % 7, i, total, rng)
        if flip:
            e = total - 2
            at = min(max((6, 7, e - 1, e - 4096, e - 4097, (6 + e) // 2)[i % 6], 6), e - 1)
            p = p[:at] + bytes([p[at] ^ 1 << (i % 8)]) + p[at + 1:]
        long.append(p)
        packets.append((v, p))
    return build_streams(packets, rng, fill=0.0, idle=0.0), long


_LADDER_CRC = {}


def ladder_crcs():
    """{packet: the CRC of its data field by the definition, bit by bit} for crc_ladder()'s long packets, computed once
    for all the tests."""
    if not _LADDER_CRC:
        _LADDER_CRC.update({p: crc16(p[6:-2]) for p in crc_ladder()[1]})
    return _LADDER_CRC


def block_of(vcdu_row):
    """The 1020-byte RS block around a given VCDU (ccsds.make_block fills its own with random bytes)."""
    data = np.frombuffer(bytes(vcdu_row), np.uint8)
    return ccsds.interleave([ccsds.encode_ccsds(data[k::4]) for k in range(4)])
