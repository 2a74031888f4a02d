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


# ---- the generators of the GPU tier reach what they are there for ------------------------------------------------------
@pytest.mark.parametrize("case", list(ps.LONG_CASES))
def test_long_packet_cut_at_every_row(case):
    total, start = ps.LONG_CASES[case]
    st, k = ps.long_packet_stream(case)
    rows = ps.rows_of(st)
    long, a, b = st.packets[k]
    assert len(long) == total and b - a + 1 == -(-(start + total) // ps.ZONE) and len(rows) == b + 1
    want = [p for p, _, _ in st.packets]
    pending = []
    for c in range(1, len(rows)):
        state, ((r1, p1), (r2, p2)) = ps.run_calls([{5: rows[:c]}, {5: rows[c:]}])
        assert ps.packets_of(r1[0], r1[1]) + ps.packets_of(r2[0], r2[1]) == want
        assert (r1[1]["crc_ok"] == 1).all() and (r2[1]["crc_ok"] == 1).all() and state.total("discarded") == 0
        assert p2[5] == 0
        pending.append(p1[5])
    # the first call holds the packet's head and whole zones behind it: every length the packet passes through
    first = ps.ZONE - start
    assert pending[a:b] == [first + ps.ZONE * i for i in range(b - a)]
    assert max(pending) > 4096 + ps.ZONE
    if case == "one_byte_last":
        assert pending[b - 1] == ps.PACKET_MAX - 1 == 65541
    if case.startswith("tail_"):
        assert pending[a] == int(case[5:]) < 6


def test_three_calls_grow_the_pending_state_in_the_middle():
    cases, streams = ps.three_call_cases()
    want = {v: [p for p, _, _ in s.packets] for v, s in streams.items()}
    assert len(cases) >= 30 and sum(c1 == c2 for c1, c2, _ in cases) >= 4 and sum(c2 - c1 >= 5 for c1, c2, _ in cases) >= 5
    for c1, c2, calls in cases:
        state, ((r1, p1), (r2, p2), (r3, p3)) = ps.run_calls(calls)
        assert all(len(c[63]) > 0 for c in calls) and state.rows[63] == 0
        assert p1[5] > 0 and p1[9] > 0 and p1[5] != p1[9]                       # two channels pending at once
        assert int(r2[2][6] - r2[2][5]) == 0 and int(r2[2][10] - r2[2][9]) == 0 and len(r2[1]) == 0
        assert p2[5] == p1[5] + ps.ZONE * (c2 - c1) and len(calls[1][5]) == c2 - c1
        assert p2[9] > p1[9] and (p2[9] - p1[9]) % ps.ZONE == 0
        assert all(ps.with_fhp(r, ps.FHP_NONE) == r for v in (5, 9) for r in calls[1][v])
        assert p3[5] == 0 and p3[9] == 0 and state.total("discarded") == 0
        got = {v: [] for v in want}
        for res, _ in ((r1, 0), (r2, 0), (r3, 0)):
            for p, d in zip(ps.packets_of(res[0], res[1]), res[1]):
                got[int(d["vcid"])].append(p)
                assert d["crc_ok"] == 1
        assert got == want


@pytest.mark.parametrize("case", ["ten_rows", "one_byte_last", "tail_5", "tail_1"])
def test_joint_damage_drops_the_long_packet(case):
    st, k = ps.long_packet_stream(case)
    long = st.packets[k][0]
    cases = ps.joint_damage(case)
    names = [n for n, _, _ in cases]
    assert len(set(names)) == len(names) >= 20
    kinds = {n.split("_", 1)[1] for n in names}
    assert {"skipped_counter", "repeated_row", "fhp_0", "fhp_400", "fhp_2046", "fhp_1000", "early_end"} <= kinds
    assert case.startswith("tail_") == ("length_1" in kinds)
    for name, head, rest in cases:
        state, ((r1, p1), (r2, p2)) = ps.run_calls([{5: head}, {5: rest}])
        assert p1[5] > 0, name
        got = ps.packets_of(r1[0], r1[1]) + ps.packets_of(r2[0], r2[1])
        assert state.discarded[5] >= 1, name
        # (the row the packet begins in, repeated: dropped and begun again)
        assert (long in got) == (name == f"{st.packets[k][1] + 1}_repeated_row"), name
        assert state.bad_fhp[5] == (1 if name.endswith(("fhp_1000", "fhp_2045")) else 0), name


def test_crc_ladder_has_every_chunk_count():
    streams, long = ps.crc_ladder()
    assert sorted(len(p) for p in long) == sorted(ps.LADDER)
    assert set(range(4097, 4108)) | set(range(8193, 8204)) | {65541} <= set(ps.LADDER)
    assert any((t - 2) % 4096 == 0 for t in ps.LADDER_STEPS)
    state, ((res, _),) = ps.run_calls([{v: s.rows for v, s in streams.items()}])
    got = ps.packets_of(res[0], res[1])
    assert got == [p for v in sorted(streams) for p, _, _ in streams[v].packets] and (res[1]["crc_ok"] == 1).all()
    assert {ps.chunks_of(int(n)) for n in res[1]["length"]} == set(range(1, 18))
    where = {}                      # the long packets begin all over the zone
    for v, s in streams.items():
        for p, a, _ in s.packets:
            if len(p) > 4096:
                where[p] = a
    assert len(where) == len(ps.LADDER)
    bitwise = ps.ladder_crcs()
    assert set(bitwise) == set(long)
    for p, d in zip(got, res[1]):
        if len(p) > 4096:
            assert int(d["crc_computed"]) == bitwise[p]
    # flipped: the same stream but for one bit in every long packet, which the CRC sees
    flipped, bad = ps.crc_ladder(flip=True)
    assert [len(p) for p in bad] == [len(p) for p in long] and all(sum(x != y for x, y in zip(p, q)) == 1 for p, q in zip(long, bad))
    state, ((res2, _),) = ps.run_calls([{v: s.rows for v, s in flipped.items()}])
    assert np.array_equal(res2[1]["length"], res[1]["length"])
    is_long = res[1]["length"] > 4096
    assert (res2[1]["crc_ok"][is_long] == 0).all() and (res2[1]["crc_ok"][~is_long] == 1).all()
    assert (res2[1]["crc_carried"] == res[1]["crc_carried"]).all() and state.total("crc_failures") == len(ps.LADDER)


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
