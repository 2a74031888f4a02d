"""CPU tier: the specification of the packet assembler (tests/packet_spec.py) -- the CRC and the identity the kernel's
lane slices rely on, every branch of the serial rule on hand-made rows, the round trip through the generator with and
without lost rows, calls cut at random -- and the CPU side of the ABI (header, ctypes signatures, dtypes, no CPU path)."""
import os
import re

import numpy as np
import pytest

import ccsds
import packet_spec as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")


# ---- CRC -----------------------------------------------------------------------------------------------------------
def test_crc_check_values():
    assert ps.crc16(b"123456789") == 0x29B1
    assert ps.crc16(b"") == 0xFFFF
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 3, 17, 884, 5000):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert ps.crc16_fast(d) == ps.crc16(d)


def test_crc_slices_combine():
    rng = np.random.default_rng(2)
    for _ in range(200):
        n = int(rng.integers(0, 600))
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        cuts = sorted(int(x) for x in rng.integers(0, n + 1, int(rng.integers(1, 6))))
        parts = [d[a:b] for a, b in zip([0] + cuts, cuts + [n])]
        # every slice from a zero register, combined left to right; the initial value shifted over the whole length
        reg = 0
        for part in parts:
            reg = ps.crc_combine(reg, ps.crc16(part, 0), len(part))
        assert reg ^ ps.gf_mul(0xFFFF, ps.x_pow8(n)) == ps.crc16(d)
        # zeros in front of the data change nothing from a zero register; the initial value is an XOR on the first two bytes
        if n >= 2:
            folded = bytes([d[0] ^ 0xFF, d[1] ^ 0xFF]) + d[2:]
            assert ps.crc16(bytes(int(rng.integers(0, 9))) + folded, 0) == ps.crc16(d)
    assert ps.x_pow8(0) == 1 and ps.x_pow8(1) == 0x100
    assert ps.crc16(b"\x00" * 7, 0x1234) == ps.gf_mul(0x1234, ps.x_pow8(7))


# ---- hand-made rows ------------------------------------------------------------------------------------------------
RNG = np.random.default_rng(3)


def row(counter, fhp, zone, vcid=5):
    zone = bytes(zone)
    assert len(zone) == ps.ZONE
    return ccsds.vcdu_header(0x8C, vcid, counter).tobytes() + bytes([fhp >> 8, fhp & 255]) + zone


def pkt(total, apid=100, seq=0, good=True):
    return ps.make_packet(apid, seq, total, RNG, good_crc=good)


def junk(n):
    return RNG.integers(0, 256, n, dtype=np.uint8).tobytes()


def fill_to(n):
    """Fill packets of exactly n bytes in all (n = 0 or n >= 7)."""
    assert n == 0 or n >= 7
    return ps.make_packet(ps.APID_FILL, 0, n, RNG) if n else b""


def run(rows, state=None, vcid=5):
    state = state or ps.State()
    vcdu, off = ps.group({vcid: rows})
    data, desc, pko, summary = ps.process(state, vcdu, off)
    return ps.packets_of(data, desc), desc, state, summary


def zones(body, first=1000, fhps=None):
    """Rows from a byte string that is a whole number of zones; fhps given per zone."""
    assert len(body) % ps.ZONE == 0
    return [row((first + z) & 0xFFFFFF, fhps[z], body[z * ps.ZONE:(z + 1) * ps.ZONE]) for z in range(len(body) // ps.ZONE)]


def test_packet_inside_one_zone():
    a, b = pkt(100), pkt(8)
    got, desc, st, _ = run([row(7, 10, junk(10) + a + b + fill_to(ps.ZONE - 118))])
    assert got == [a, b] and (desc["crc_ok"] == 1).all() and (desc["first_counter"] == 7).all()
    assert list(desc["offset"]) == [0, 100] and st.fill_packets[5] == 1 and st.pending[5] == b""
    assert desc["apid"][0] == 100 and desc["vcid"][0] == 5 and desc["seq_flags"][0] == 3


@pytest.mark.parametrize("nrows", [2, 11])
def test_packet_spanning_rows(nrows):
    total = ps.ZONE * (nrows - 1) + 100 - 50            # starts at 50 in the first zone, ends at 100 in the last
    a = pkt(total)
    body = fill_to(50) + a + fill_to(ps.ZONE - 100)
    fh = [0] + [ps.FHP_NONE] * (nrows - 2) + [100]
    got, desc, st, _ = run(zones(body, fhps=fh))
    assert got == [a] and desc["crc_ok"][0] == 1 and desc["first_counter"][0] == 1000 and st.discarded[5] == 0
    assert st.fill_packets[5] == 2 and st.rows[5] == nrows


def test_packet_ending_exactly_at_a_zone_end():
    a, b = pkt(ps.ZONE + 84), pkt(20)
    body = fill_to(800) + a + b + fill_to(ps.ZONE - 20)
    got, desc, st, _ = run(zones(body, fhps=[0, ps.FHP_NONE, 0]))
    assert got == [a, b] and st.discarded[5] == 0
    # ... and when the row that ends it has fhp = 2047 as its last word: the packet is finished by that row
    got, _, st, _ = run(zones(body, fhps=[0, ps.FHP_NONE, 0])[:2])
    assert got == [a] and st.pending[5] == b""


@pytest.mark.parametrize("cut", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("long", [False, True])
def test_header_split_across_rows(cut, long):
    # the packet starts `cut` bytes before the first zone's end
    end = 300 if long else 484                          # ... and ends there in the second (third) zone
    a = pkt(cut + (ps.ZONE if long else 0) + end)
    b = pkt(30)
    lead = ps.ZONE - cut
    body = fill_to(lead) + a + b
    body += fill_to(-len(body) % ps.ZONE if -len(body) % ps.ZONE >= 7 else 0)
    if len(body) % ps.ZONE:
        body += fill_to(-len(body) % ps.ZONE + ps.ZONE)
    nz = len(body) // ps.ZONE
    fh = [0, ps.FHP_NONE, end] if long else [0, end]
    fh += [ps.FHP_NONE] * (nz - len(fh))
    got, desc, st, _ = run(zones(body, fhps=fh))
    assert got[:2] == [a, b] and desc["first_counter"][0] == 1000 and st.discarded[5] == 0
    # a tail shorter than a header and a first header pointer that leaves it shorter than one: dropped
    rows = zones(body, fhps=fh)
    short = row(1001, 0, rows[1][8:])
    got, _, st, _ = run([rows[0], short])
    assert a not in got and st.discarded[5] == 1


def test_lost_row_under_a_spanning_packet():
    a, b, c = pkt(3 * ps.ZONE), pkt(40), pkt(50)
    body = fill_to(400) + a + b + c
    body += fill_to(-len(body) % ps.ZONE)
    rows = zones(body, fhps=[0, ps.FHP_NONE, ps.FHP_NONE, 400, ][:len(body) // ps.ZONE])
    got, _, st, _ = run(rows)
    assert got == [a, b, c]
    got, desc, st, _ = run(rows[:2] + rows[3:])
    assert got == [b, c] and st.discarded[5] == 1 and (desc["first_counter"] == 1003).all()


def test_counter_wrap_is_continuous_and_a_repeat_is_not():
    a = pkt(ps.ZONE + 20)
    body = fill_to(300) + a + fill_to(ps.ZONE - 320)
    rows = zones(body, first=0xFFFFFF, fhps=[0, 320])
    assert [bytes(r[2:5]) for r in rows] == [b"\xff\xff\xff", b"\x00\x00\x00"]
    got, desc, st, _ = run(rows)
    assert got == [a] and desc["first_counter"][0] == 0xFFFFFF
    again = row(0xFFFFFF, 320, rows[1][8:])              # the second row under the first one's counter
    got, _, st, _ = run([rows[0], again])
    assert got == [] and st.discarded[5] == 1


def test_fhp_contradicting_the_pending_length():
    a = pkt(ps.ZONE + 20)
    body = fill_to(300) + a + fill_to(ps.ZONE - 320)
    r0, r1 = zones(body, fhps=[0, 320])
    for wrong in (319, 321, 0):
        got, _, st, _ = run([r0, row(1001, wrong, r1[8:])])
        assert a not in got and st.discarded[5] == 1
    # 2047 where the packet should have ended: it grows past its length
    got, _, st, _ = run([r0, row(1001, ps.FHP_NONE, r1[8:])])
    assert got == [] and st.discarded[5] == 1 and st.pending[5] == b""


def test_idle_and_invalid_pointers():
    a, b = pkt(ps.ZONE + 20), pkt(60)
    body = fill_to(300) + a + fill_to(ps.ZONE - 320)
    r0, r1 = zones(body, fhps=[0, 320])
    nxt = row(1002, 0, b + fill_to(ps.ZONE - 60))
    got, _, st, _ = run([r0, row(1001, ps.FHP_IDLE, r1[8:]), nxt])
    assert got == [b] and st.discarded[5] == 1 and st.bad_fhp[5] == 0
    got, _, st, _ = run([r0, row(1001, 1000, r1[8:]), nxt])
    assert got == [b] and st.discarded[5] == 1 and st.bad_fhp[5] == 1
    got, _, st, _ = run([row(1001, 884, r1[8:]), row(1002, 2045, r1[8:]), nxt])
    assert got == [b] and st.discarded[5] == 0 and st.bad_fhp[5] == 2


def test_shortest_and_longest_packets():
    a = pkt(7)
    got, desc, st, _ = run([row(1, 0, a + pkt(8) + fill_to(ps.ZONE - 15))])
    assert got[0] == a and desc["crc_ok"][0] == 0 and desc["crc_computed"][0] == 0 and desc["crc_carried"][0] == 0
    assert desc["crc_ok"][1] == 1 and desc["crc_computed"][1] == 0xFFFF and st.crc_failures[5] == 1
    big = pkt(ps.PACKET_MAX)
    body = big + fill_to(-ps.PACKET_MAX % ps.ZONE)
    nz = len(body) // ps.ZONE
    got, desc, st, _ = run(zones(body, fhps=[0] + [ps.FHP_NONE] * (nz - 2) + [ps.PACKET_MAX % ps.ZONE]))
    assert got == [big] and desc["crc_ok"][0] == 1 and desc["length"][0] == 65542 and nz == 75
    bad = pkt(200, good=False)
    got, desc, st, _ = run([row(1, 0, bad + fill_to(ps.ZONE - 200))])
    assert got == [bad] and desc["crc_ok"][0] == 0 and st.crc_failures[5] == 1 and st.packets[5] == 1


def test_fill_packets_and_fill_channel():
    a = pkt(90)
    z = fill_to(100) + a + fill_to(ps.ZONE - 190)
    got, _, st, summary = run([row(1, 0, z)])
    assert got == [a] and st.fill_packets[5] == 2 and summary["fill_packets"] == 2
    got, _, st, summary = run([row(1, 0, z, vcid=63)], vcid=63)
    assert got == [] and summary["rows"] == 0 and st.last[63] == -1


# ---- round trips -----------------------------------------------------------------------------------------------------
def test_round_trip_without_damage():
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        packets = ps.random_packets(rng, int(rng.integers(1, 60)), [0, 5, 62])
        streams = ps.build_streams(packets, rng)
        vcdu, off = ps.group({v: s.rows for v, s in streams.items()})
        st = ps.State()
        data, desc, pko, _ = ps.process(st, vcdu, off)
        want = [p for v in sorted(streams) for p, _, _ in streams[v].packets]
        assert ps.packets_of(data, desc) == want, seed
        assert (desc["crc_ok"][desc["length"] >= 8] == 1).all() and st.total("discarded") == 0
        assert [int(pko[v + 1] - pko[v]) for v in (0, 5, 62)] == [len(streams[v].packets) if v in streams else 0 for v in (0, 5, 62)]


def test_round_trip_with_rows_removed():
    for seed in range(60):
        rng = np.random.default_rng(5000 + seed)
        packets = ps.random_packets(rng, int(rng.integers(20, 120)), [3, 40])
        streams = ps.build_streams(packets, rng)
        rows, want = {}, []
        for v, s in streams.items():
            rows[v], removed = ps.damage(s, rng, remove=0.1)
            want += [p for p, a, b in s.packets if not any(r in removed for r in range(a, b + 1))]
        vcdu, off = ps.group(rows)
        data, desc, _, _ = ps.process(ps.State(), vcdu, off)
        assert ps.packets_of(data, desc) == want, seed


def test_calls_cut_at_random_equal_one_call():
    rng = np.random.default_rng(77)
    packets = ps.random_packets(rng, 400, [1, 2, 30])
    streams = ps.build_streams(packets, rng)
    rows = {v: ps.damage(s, rng, remove=0.03, repeat=0.01, wrong_fhp=0.02, bad_length=0.02, flip=0.02)[0]
            for v, s in streams.items()}
    one = ps.State()
    data, desc, _, _ = ps.process(one, *ps.group(rows))
    whole = {v: [p for p, d in zip(ps.packets_of(data, desc), desc) if d["vcid"] == v] for v in rows}
    many = ps.State()
    got = {v: [] for v in rows}
    pos = {v: 0 for v in rows}
    while any(pos[v] < len(rows[v]) for v in rows):
        part = {}
        for v in rows:
            k = int(rng.integers(0, 6))
            part[v] = rows[v][pos[v]:pos[v] + k]
            pos[v] += k
        d, ds, _, _ = ps.process(many, *ps.group(part))
        for p, e in zip(ps.packets_of(d, ds), ds):
            got[int(e["vcid"])].append(p)
    assert got == whole
    for k in ps.COUNTERS:
        assert getattr(many, k) == getattr(one, k), k
    assert many.pending == one.pending and many.last == one.last


# ---- the ABI, CPU side -------------------------------------------------------------------------------------------------
PACKET_FUNCTIONS = ["xrit_packets_create", "xrit_packets_destroy", "xrit_packets_process", "xrit_packets_process_device",
                    "xrit_packets_reset", "xrit_packets_stats"]


def test_packet_assembler_abi():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xrit_[a-z0-9_]+)\s*\(", src))
    import xritdemod_amd as xa
    from xritdemod_amd import _capi
    for name in PACKET_FUNCTIONS:
        assert name in declared, name
        assert name in _capi._SIGNATURES, name
    assert xa.PACKET_DTYPE.itemsize == 32 and xa.PACKET_DTYPE == ps.PACKET_DTYPE
    assert xa.PACKETS_SUMMARY_DTYPE.itemsize == 72 and xa.PACKETS_STATS_DTYPE.itemsize == 4144
    assert "CCSDS 732.0" in open(HEADER).read() and "CCSDS 133.0" in open(HEADER).read()


def test_packet_assembler_has_no_cpu_path():
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(xa.XritError) as ei:
        xa.PacketAssembler()
    assert ei.value.code == -2 and "no CPU path" in str(ei.value)
