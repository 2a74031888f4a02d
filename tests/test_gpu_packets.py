"""GPU tier: the packet assembler (xrit_packets_*, PacketAssembler) against the specification of tests/packet_spec.py --
generator streams with lost, repeated and damaged rows at tile-edge sizes and VCID mixes, rows of random bytes, calls
cut at random, a long packet cut at every row and carried over three calls, damage at the joint, every count of CRC
chunks, reset, several handles, the capacities, the row bound, the device path behind decoder and demultiplexer, the chain from
IQ and the host program.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import ccsds
import file_spec as fs
import packet_spec as ps
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = [0, 1, 2, 3, 4, 6, 7, 9, 13, 20, 21, 30, 31, 32, 40, 41, 50, 60, 62, 63]     # test_gpu_demux's skewed mix


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


def rows_per_channel(rng, nf, mix):
    if mix == "one":
        vc = np.full(nf, 5)
    elif mix == "all":
        vc = rng.integers(0, 64, nf)
    else:
        vc = np.where(rng.random(nf) < 0.9, 5, np.array(OTHERS)[rng.integers(0, len(OTHERS), nf)])
    return np.bincount(vc, minlength=64)


def random_rows(rng, n, vcid=None):
    """Rows of random bytes under consecutive counters (the walk must follow garbage lengths as the specification does);
    with a VCID, under that channel's VCDU header."""
    a = rng.integers(0, 256, (n, 892), dtype=np.uint8)
    if vcid is not None:
        a[:, 0:2] = ccsds.vcdu_header(0x8C, vcid, 0)[:2]
    c = (int(rng.integers(0, 1 << 24)) + np.arange(n)) & 0xFFFFFF
    a[:, 2], a[:, 3], a[:, 4] = c >> 16, (c >> 8) & 255, c & 255
    return [bytes(r) for r in a]


def make_case(rng, nf, mix):
    """(vcdu, offsets) of nf rows: per channel a generator stream with about 3 % of the rows removed and 1 % damaged in
    each of the other ways, cut to the channel's share; channel 63 carries random bytes."""
    counts = rows_per_channel(rng, nf, mix)
    sizes = ps.SIZES
    weights = np.array([(0.6 if nf >= 10000 else 0.02) if s > 1000 else 1.0 for s in sizes])   # long runs: fewer, longer packets
    rows = {}
    for v in np.nonzero(counts)[0]:
        n = int(counts[v])
        if v == 63:
            rows[63] = random_rows(rng, n)
            continue
        got = []
        while len(got) < n:                                     # (a stream per round; the counters restart: one more break)
            want_bytes = (n - len(got)) * ps.ZONE * 1.2 + 2000
            packets, have = [], 0
            while have < want_bytes:
                p = ps.random_packets(rng, 8, [int(v)], sizes, weights)
                packets += p
                have += sum(len(x[1]) for x in p)
            st = ps.build_stream(int(v), [p for _, p in packets], rng)
            got += ps.damage(st, rng, remove=0.03, repeat=0.01, wrong_fhp=0.01, bad_length=0.01, flip=0.01)[0]
        rows[int(v)] = got[:n]
    return ps.group(rows)


def same(got, want):
    data, desc, pko, summary = got
    wdata, wdesc, wpko, wsum = want
    assert np.array_equal(pko, wpko)
    assert desc.tobytes() == wdesc.tobytes()
    assert np.array_equal(data, wdata)
    for k, w in wsum.items():
        assert int(summary[k]) == w, k
    assert int(summary["overflow"]) == 0


def same_state(xa, pa, st):
    s = pa.stats()
    for k in ps.COUNTERS:
        assert [int(x) for x in s["vc_" + k]] == getattr(st, k), k
        assert int(s[k]) == st.total(k)
    assert [int(x) for x in s["last_counter"]] == st.last
    assert [int(x) for x in s["pending_bytes"]] == [len(p) for p in st.pending]
    assert [int(x) for x, p in zip(s["pending_first_counter"], st.pending) if p] == \
        [c for c, p in zip(st.first_counter, st.pending) if p]


@pytest.mark.parametrize("mix", ["one", "all", "skewed"])
@pytest.mark.parametrize("nf", [1, 2, 63, 64, 65, 1023, 1024, 1025, 100000])
def test_one_call_matches_spec(xa, nf, mix):
    rng = np.random.default_rng(nf * 5 + len(mix))
    vcdu, off = make_case(rng, nf, mix)
    assert int(off[64]) == nf
    pa = xa.PacketAssembler()
    st = ps.State()
    same(pa.process(vcdu, off), ps.process(st, vcdu, off))
    same_state(xa, pa, st)
    pa.close()


@pytest.mark.parametrize("n", [1, 700, 30000])
def test_rows_of_random_bytes(xa, n):
    rng = np.random.default_rng(n)
    rows = {0: random_rows(rng, n), 17: random_rows(rng, n // 2 + 1)}
    # a second channel where the garbage is followed further: many pointers say "no header here", lengths are short
    a = np.frombuffer(b"".join(rows[17]), np.uint8).reshape(-1, 892).copy()
    a[rng.random(len(a)) < 0.5, 6:8] = (7, 255)
    a[rng.random(len(a)) < 0.5, 6] = 0
    a[:, 12::97] &= 1
    rows[17] = [bytes(r) for r in a]
    vcdu, off = ps.group(rows)
    pa = xa.PacketAssembler()
    st = ps.State()
    same(pa.process(vcdu, off), ps.process(st, vcdu, off))
    same_state(xa, pa, st)
    # ... and once more behind itself: the pending state in front of the same rows
    same(pa.process(vcdu, off), ps.process(st, vcdu, off))
    same_state(xa, pa, st)
    pa.close()


def cut_stream(rng, rows, k):
    """The channels' rows in calls of 0 .. k rows per channel."""
    pos = {v: 0 for v in rows}
    while any(pos[v] < len(rows[v]) for v in rows):
        part = {}
        for v in rows:
            n = int(rng.integers(0, k + 1))
            part[v] = rows[v][pos[v]:pos[v] + n]
            pos[v] += n
        yield ps.group(part)


def damaged_streams(rng, count, vcids):
    streams = ps.build_streams(ps.random_packets(rng, count, vcids), rng)
    return {v: ps.damage(s, rng, remove=0.03, repeat=0.01, wrong_fhp=0.02, bad_length=0.02, flip=0.02)[0]
            for v, s in streams.items()}


def test_random_cuts_equal_one_call(xa):
    rng = np.random.default_rng(21)
    rows = damaged_streams(rng, 1500, [1, 2, 30, 62])
    one, many = xa.PacketAssembler(), xa.PacketAssembler()
    data, desc, _, _ = one.process(*ps.group(rows))
    whole = {v: [p for p, d in zip(one.split(data, desc), desc) if d["vcid"] == v] for v in rows}
    st = ps.State()
    got = {v: [] for v in rows}
    for k in (5, 80):
        for vcdu, off in cut_stream(rng, rows, k):
            res = many.process(vcdu, off)
            same(res, ps.process(st, vcdu, off))
            for p, d in zip(many.split(res[0], res[1]), res[1]):
                got[int(d["vcid"])].append(p)
        if k == 5:
            assert got == whole
            assert many.stats().tobytes() == one.stats().tobytes()
    same_state(xa, many, st)
    one.close()
    many.close()


def test_reset_and_two_handles_interleaved(xa):
    rng = np.random.default_rng(22)
    ra, rb = damaged_streams(rng, 600, [4, 9]), damaged_streams(rng, 600, [4, 9])
    a, b = xa.PacketAssembler(), xa.PacketAssembler()
    sa, sb = ps.State(), ps.State()
    for (va, oa), (vb, ob) in zip(cut_stream(rng, ra, 40), cut_stream(rng, rb, 40)):
        same(a.process(va, oa), ps.process(sa, va, oa))
        same(b.process(vb, ob), ps.process(sb, vb, ob))
    same_state(xa, a, sa)
    same_state(xa, b, sb)
    assert int(a.stats()["packets"]) > 0
    a.reset()
    fresh = xa.PacketAssembler()
    assert a.stats().tobytes() == fresh.stats().tobytes()
    want = ps.process(ps.State(), *ps.group(rb))
    same(a.process(*ps.group(rb)), want)
    same(fresh.process(*ps.group(rb)), want)
    for h in (a, b, fresh):
        h.close()


def test_capacity(xa):
    rng = np.random.default_rng(23)
    rows = damaged_streams(rng, 400, [3, 8])
    first = {v: r[:len(r) // 2] for v, r in rows.items()}
    second = {v: r[len(r) // 2:] for v, r in rows.items()}
    st = ps.State()
    w1 = ps.process(st, *ps.group(first))
    w2 = ps.process(st, *ps.group(second))
    n, nb = len(w1[1]), len(w1[0])
    assert n > 10
    for cap_p, cap_b in ((n - 1, None), (None, nb - 1), (n - 1, nb - 1), (0, 0)):
        pa = xa.PacketAssembler()
        with pytest.raises(xa.XritError) as ei:
            pa.process(*ps.group(first), max_packets=cap_p, max_bytes=cap_b)
        assert ei.value.code == -5
        data, desc, pko, summary = ei.value.partial
        assert int(summary["packets"]) == n and int(summary["bytes"]) == nb and int(summary["overflow"]) == 1
        assert np.array_equal(pko, w1[2])
        kp = n if cap_p is None else cap_p
        assert desc.tobytes() == w1[1][:kp].tobytes()
        ends = (w1[1]["offset"] + w1[1]["length"]).astype(np.int64)
        kb = nb if cap_b is None else int(max([0] + [e for e in ends if e <= cap_b]))
        assert np.array_equal(data[:kb], w1[0][:kb]) and len(data) >= kb
        same(pa.process(*ps.group(second)), w2)                 # the state advanced as if everything had fitted
        same_state(xa, pa, st)
        pa.close()
    # exactly enough is enough
    pa = xa.PacketAssembler()
    same(pa.process(*ps.group(first), max_packets=n, max_bytes=nb), w1)
    pa.close()


# ---- a long packet across calls, the CRC's chunks, the row bound (generators and what they reach: packet_spec.py, checked
# in test_packet_spec.py) ------------------------------------------------------------------------------------------------
def run_calls(xa, pa, calls):
    """A reset handle through the calls ({vcid: rows} each), after every one against the specification.  -> (the
    packets emitted per channel, their descriptors, the specification's state)."""
    pa.reset()
    st = ps.State()
    got, descs = {}, []
    for part in calls:
        vcdu, off = ps.group(part)
        res = pa.process(vcdu, off)
        same(res, ps.process(st, vcdu, off))
        same_state(xa, pa, st)
        for p, d in zip(pa.split(res[0], res[1]), res[1]):
            got.setdefault(int(d["vcid"]), []).append(p)
        descs.append(res[1])
    return got, np.concatenate(descs), st


@pytest.mark.parametrize("case", list(ps.LONG_CASES))
def test_long_packet_cut_at_every_row(xa, case):
    stream, k = ps.long_packet_stream(case)
    rows = ps.rows_of(stream)
    want = [p for p, _, _ in stream.packets]
    pa = xa.PacketAssembler()
    longest = 0
    for c in range(1, len(rows)):
        got, desc, st = run_calls(xa, pa, [{5: rows[:c]}, {5: rows[c:]}])
        assert got == {5: want} and (desc["crc_ok"] == 1).all(), c          # the generated packets, byte for byte
        assert int(desc["first_counter"][k]) == ps.counter_of(rows[stream.packets[k][1]])
        longest = max(longest, int(desc["length"].max()))
    assert longest == ps.LONG_CASES[case][0]
    pa.close()


def test_long_packets_over_three_calls(xa):
    cases, streams = ps.three_call_cases()
    want = {v: [p for p, _, _ in s.packets] for v, s in streams.items()}
    pa = xa.PacketAssembler()
    for c1, c2, calls in cases:
        got, desc, st = run_calls(xa, pa, calls)
        assert got == want and (desc["crc_ok"] == 1).all(), (c1, c2)
    pa.close()


@pytest.mark.parametrize("case", ["ten_rows", "one_byte_last", "tail_5", "tail_1"])
def test_damage_at_the_joint(xa, case):
    stream, k = ps.long_packet_stream(case)
    first_row = stream.packets[k][1]
    pa = xa.PacketAssembler()
    for name, head, rest in ps.joint_damage(case):
        got, desc, st = run_calls(xa, pa, [{5: head}, {5: rest}])
        assert st.discarded[5] >= 1, name
        assert (stream.packets[k][0] in got.get(5, [])) == (name == f"{first_row + 1}_repeated_row"), name
    pa.close()


def ladder_input(flip):
    streams, long = ps.crc_ladder(flip=flip)
    return ps.group({v: s.rows for v, s in streams.items()}), long


def test_crc_ladder(xa):
    (vcdu, off), long = ladder_input(False)
    pa = xa.PacketAssembler()
    st = ps.State()
    res, want = pa.process(vcdu, off), ps.process(st, vcdu, off)
    same(res, want)
    same_state(xa, pa, st)
    data, desc = res[0], res[1]
    assert (desc["crc_ok"] == 1).all() and sorted(int(n) for n in desc["length"] if n > 4096) == sorted(ps.LADDER)
    assert {ps.chunks_of(int(n)) for n in desc["length"]} == set(range(1, 18))
    packets = pa.split(data, desc)
    assert sorted(p for p in packets if len(p) > 4096) == sorted(long)      # the generated packets, byte for byte
    bitwise = ps.ladder_crcs()                                  # the definition, bit by bit
    for p, d in zip(packets, desc):
        if len(p) > 4096:
            assert int(d["crc_computed"]) == bitwise[p], len(p)
    # one bit of every long packet changed: the computed CRC follows the data, the carried one stays
    (vcdu2, off2), bad = ladder_input(True)
    pa.reset()
    st = ps.State()
    res2, want2 = pa.process(vcdu2, off2), ps.process(st, vcdu2, off2)
    same(res2, want2)
    same_state(xa, pa, st)
    is_long = res2[1]["length"] > 4096
    assert is_long.sum() == len(ps.LADDER) and (res2[1]["crc_ok"][is_long] == 0).all() and (res2[1]["crc_ok"][~is_long] == 1).all()
    assert np.array_equal(res2[1]["crc_computed"], want2[1]["crc_computed"])
    assert np.array_equal(res2[1]["crc_carried"], desc["crc_carried"])
    assert (res2[1]["crc_computed"][is_long] != desc["crc_computed"][is_long]).all()
    pa.close()


def test_more_rows_than_the_bound_changes_nothing(xa):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(27)
    sa, ka = ps.long_packet_stream("ten_rows", 5)
    sb, _ = ps.long_packet_stream("tail_5", 9)
    ra, rb = ps.rows_of(sa), ps.rows_of(sb)
    # an earlier call: pending bytes on two channels, counters; the file assembler behind has seen a call too
    pa, fa = xa.PacketAssembler(), xa.FileAssembler()
    st = ps.State()
    earlier = ps.group({5: ra[:4], 9: rb[:30], 63: random_rows(rng, 3)})
    same(pa.process(*earlier), ps.process(st, *earlier))
    same_state(xa, pa, st)
    assert st.pending[5] and st.pending[9] and st.total("packets") > 0
    files_in = fs.stage_input(fs.random_stream(rng, 6, [(5, 20), (9, 21)], max_bytes=3000, max_user=500)[0][:-2])
    fst = fs.State()
    want_f = fs.process(fst, *files_in)
    got_f = fa.process(*files_in)
    assert got_f[1].tobytes() == want_f[1].tobytes() and got_f[2].tobytes() == want_f[2].tobytes()
    before, files_before = pa.stats().tobytes(), fa.stats().tobytes()
    assert int(fa.stats()["open_files"]) > 0 and int(fa.stats()["total_pieces"]) > 0

    vcdu, off = ps.group({5: ra[4:], 9: rb[30:], 63: random_rows(rng, 2)})
    n = int(off[64])
    want = ps.process(st, vcdu, off)
    assert len(want[1]) >= 8
    dev = torch.device("cuda:0")
    ee = lambda nbytes: torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
    d_vcdu = torch.from_numpy(vcdu.copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
    max_bytes, max_packets = xa.packets_max_bytes(n), 64
    d_bytes, d_desc, d_pko, d_sum = ee(max_bytes), ee(max_packets * 32), ee(260), ee(72)
    d_fbytes, d_pieces, d_frecs, d_fsum = ee(max_bytes), ee(max_packets * 32), ee(2 * max_packets * 80), ee(104)

    def call(bound):
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            pa.process_device(d_vcdu.data_ptr(), d_off.data_ptr(), bound, d_bytes.data_ptr(), max_bytes, d_desc.data_ptr(),
                              max_packets, d_pko.data_ptr(), d_sum.data_ptr(), stream=s.cuda_stream)
            fa.process_device(d_bytes.data_ptr(), max_bytes, d_desc.data_ptr(), d_pko.data_ptr(), max_packets,
                              d_fbytes.data_ptr(), max_bytes, d_pieces.data_ptr(), max_packets, d_frecs.data_ptr(),
                              2 * max_packets, d_fsum.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        return d_sum.cpu().numpy().view(xa.PACKETS_SUMMARY_DTYPE)[0], d_fsum.cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)[0]

    summ, fsum = call(n - 1)
    assert int(summ["overflow"]) == 2 and int(summ["packets"]) == 0 and int(summ["bytes"]) == 0
    assert (d_bytes.cpu().numpy() == 0xEE).all() and (d_desc.cpu().numpy() == 0xEE).all()
    assert (d_pko.cpu().numpy() == 0).all()                     # the one thing written besides the summary: no packets
    assert pa.stats().tobytes() == before
    # the file assembler queued behind it saw an empty call
    assert [int(fsum[k]) for k in ("pieces", "bytes", "files", "overflow")] == [0, 0, 0, 0]
    assert (d_pieces.cpu().numpy() == 0xEE).all() and (d_frecs.cpu().numpy() == 0xEE).all() and (d_fbytes.cpu().numpy() == 0xEE).all()
    assert fa.stats().tobytes() == files_before
    # the true bound: the call as if the refused one had not been
    summ, fsum = call(n)
    got = (d_bytes.cpu().numpy()[:int(summ["bytes"])], d_desc.cpu().numpy().view(xa.PACKET_DTYPE)[:int(summ["packets"])],
           d_pko.cpu().numpy().view(np.uint32), summ)
    same(got, want)
    same_state(xa, pa, st)
    assert sa.packets[ka][0] in pa.split(got[0], got[1])
    # ... and the file assembler behind it the packets of that call (unsegmented ones: a file each)
    want_f = fs.process(fst, d_bytes.cpu().numpy(), got[1], got[2])
    assert int(fsum["overflow"]) == 0 and want_f[3]["files_completed"] >= 8
    for key, w in want_f[3].items():
        assert int(fsum[key]) == w, key
    assert d_pieces.cpu().numpy().view(xa.FILE_PIECE_DTYPE)[:len(want_f[1])].tobytes() == want_f[1].tobytes()
    assert d_frecs.cpu().numpy().view(xa.FILE_RECORD_DTYPE)[:len(want_f[2])].tobytes() == want_f[2].tobytes()
    assert np.array_equal(d_fbytes.cpu().numpy()[:len(want_f[0])], want_f[0])
    for x in (pa, fa):
        x.close()
    del d_vcdu, d_off, d_bytes, d_desc, d_pko, d_sum, d_fbytes, d_pieces, d_frecs, d_fsum
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def interleave(rows):
    """The channels' rows in a transmission order: round robin while they last."""
    out, k = [], 0
    while any(k < len(r) for r in rows.values()):
        for v in sorted(rows):
            if k < len(rows[v]):
                out.append((v, rows[v][k]))
        k += 1
    return out


def cadus_of(sent):
    blocks = np.stack([ps.block_of(r) for _, r in sent])
    return blocks, np.stack([ccsds.cadu_from_block(b) for b in blocks])


def test_device_path_behind_decoder_and_demux_on_a_side_stream(xa):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(24)
    sizes = [40, 300, 700, 880, 884, 890, 1500, 2700]
    streams = ps.build_streams(ps.random_packets(rng, 70, [0, 7], sizes, np.ones(len(sizes))), rng)
    rows = {v: [bytes(r) for r in s.rows][:16] for v, s in streams.items()}
    rows[63] = random_rows(rng, 16, 63)
    for v in (0, 7):
        assert len(rows[v]) == 16
    sent = interleave(rows)
    n = len(sent)
    _, cadus = cadus_of(sent)
    clean = ccsds.coded_symbols(cadus).reshape(n, ccsds.FRAME_SYMBOLS).astype(np.int16)
    frames = np.clip(clean + rng.normal(0, 60, clean.shape).round(), -128, 127).astype(np.int8)
    lost = 19                                                    # a frame of channel 7 that does not decode
    assert sent[lost][0] == 7
    frames[lost] = rng.integers(-128, 128, ccsds.FRAME_SYMBOLS)
    valid = np.ones(n, np.uint8)
    hits = np.zeros((n, 4), np.uint32)
    hits[:, 2] = 60
    # the expectation: the specification on the rows that were sent and decoded, one call; and the generated packets
    good = {v: [r for i, (u, r) in enumerate(sent) if u == v and i != lost] for v in rows}
    want = ps.process(ps.State(), *ps.group(good))
    k_lost = [i for i, (u, _) in enumerate(sent) if u == 7].index(lost)
    survivors = [p for v in (0, 7) for p, a, b in streams[v].packets if b < 16 and not (v == 7 and a <= k_lost <= b)]
    assert ps.packets_of(want[0], want[1]) == survivors and len(survivors) > 10

    dev = torch.device("cuda:0")
    d_frames = torch.from_numpy(frames.view(np.uint8)).to(dev)
    d_valid = torch.from_numpy(valid).to(dev)
    d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1)).to(dev)
    d_cadu = torch.zeros((n, 1024), dtype=torch.uint8, device=dev)
    d_block = torch.zeros((n, 1020), dtype=torch.uint8, device=dev)
    d_info = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    d_vcdu = torch.zeros((n, 892), dtype=torch.uint8, device=dev)
    d_off = torch.zeros(2 * 65 * 4, dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(n * 88, dtype=torch.uint8, device=dev)
    max_bytes, max_packets = xa.packets_max_bytes(n), 200
    d_bytes = torch.zeros(2 * max_bytes, dtype=torch.uint8, device=dev)
    d_desc = torch.zeros(2 * max_packets * 32, dtype=torch.uint8, device=dev)
    d_pko = torch.zeros(2 * 65 * 4, dtype=torch.uint8, device=dev)
    d_sum = torch.zeros(2 * 72, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    dec, dm, pa = xa.FrameDecoder("lrit"), xa.ChannelDemux(), xa.PacketAssembler()
    h = n // 2
    with torch.cuda.stream(s):
        for k, (a, b) in enumerate(((0, h), (h, n))):
            dec.decode_device(d_frames[a:].data_ptr(), d_valid[a:].data_ptr(), b - a, d_cadu[a:].data_ptr(),
                              d_block[a:].data_ptr(), d_info[a * 40:].data_ptr(), stream=s.cuda_stream)
            dm.process_device(d_hits[a * 16:].data_ptr(), d_cadu[a:].data_ptr(), d_block[a:].data_ptr(),
                              d_info[a * 40:].data_ptr(), b - a, d_vcdu[a:].data_ptr(), d_off[k * 260:].data_ptr(),
                              d_rec[a * 88:].data_ptr(), stream=s.cuda_stream)
            pa.process_device(d_vcdu[a:].data_ptr(), d_off[k * 260:].data_ptr(), b - a, d_bytes[k * max_bytes:].data_ptr(),
                              max_bytes, d_desc[k * max_packets * 32:].data_ptr(), max_packets,
                              d_pko[k * 260:].data_ptr(), d_sum[k * 72:].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    summ = d_sum.cpu().numpy().view(xa.PACKETS_SUMMARY_DTYPE)
    desc = d_desc.cpu().numpy().view(xa.PACKET_DTYPE).reshape(2, max_packets)
    raw = d_bytes.cpu().numpy().reshape(2, max_bytes)
    pko = d_pko.cpu().numpy().view(np.uint32).reshape(2, 65)
    assert (summ["overflow"] == 0).all()
    # each call against the specification on the rows the demultiplexer handed over, byte for byte
    offs = d_off.cpu().numpy().view(np.uint32).reshape(2, 65)
    vc = d_vcdu.cpu().numpy()
    st = ps.State()
    got = []
    for k, a in enumerate((0, h)):
        d = desc[k][:int(summ[k]["packets"])]
        same((raw[k][:int(summ[k]["bytes"])], d, pko[k], summ[k]), ps.process(st, vc[a:a + int(offs[k][64])], offs[k]))
        got.append(pa.split(raw[k], d))
    same_state(xa, pa, st)
    # ... and together against the one-call run on the rows that were sent and decoded: the generated packets
    assert int(summ[1]["rows"]) == 31                           # (channel 63 aside) every frame but the lost one
    by_vc = {v: [p for k in range(2) for p, e in zip(got[k], desc[k]) if e["vcid"] == v] for v in (0, 7)}
    assert by_vc[0] + by_vc[7] == survivors
    assert int(summ[1]["total_packets"]) == len(survivors) and int(summ[1]["discarded"]) == want[3]["discarded"] >= 1
    for x in (dec, dm, pa):
        x.close()
    del d_frames, d_valid, d_hits, d_cadu, d_block, d_info, d_vcdu, d_off, d_rec, d_bytes, d_desc, d_pko, d_sum
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def fixed_stream(vcid, totals, rng, counter):
    pkts = [ps.make_packet(10 + i % 3, i, t, rng) for i, t in enumerate(totals)]
    return ps.build_stream(vcid, pkts, rng, start_counter=counter, fill=0.0, idle=0.0)


def iq_of(cadus, seed):
    sym = ccsds.coded_symbols(cadus, amplitude=1).astype(np.float64)
    p = synth.SynthParams(fs_in=1.25e6, seed=seed, esn0_db=12.0)
    return synth.generate(p, int((len(sym) + 64) * p.sps_in), symbols=sym)


def test_chain_from_iq_drops_the_packet_under_the_missing_frame(xa):
    rng = np.random.default_rng(25)
    nrow = 10
    s5 = fixed_stream(5, [400, 600, 500, 700, 2100, 300, 800, 900, 350, 650, 500, 700, 800], rng, 70)
    s2 = fixed_stream(2, [90, 1200, 64, 884, 2000, 7, 450, 1000, 1300, 800, 700, 300, 600], rng, 500)
    rows = {2: [bytes(r) for r in s2.rows][:nrow], 5: [bytes(r) for r in s5.rows][:nrow], 63: random_rows(rng, nrow, 63)}
    assert len(rows[2]) == nrow and len(rows[5]) == nrow
    victim = next((p, a, b) for p, a, b in s5.packets if b - a == 2 and a >= 2 and b < nrow - 1)
    sent = interleave(rows)
    skip = next(i for i, (v, r) in enumerate(sent) if v == 5 and r == rows[5][victim[1] + 1])
    sent = sent[:skip] + sent[skip + 1:]                      # one CADU left out, in the middle of that packet
    blocks, cadus = cadus_of(sent)
    x = iq_of(cadus, 25)
    q = xa.Demodulator(xa.Demodulator.config("lrit", 1.25e6, 1))
    s8 = q.quantize_i8(q.process(x))
    hits = np.asarray(xa.sync_correlate(s8))
    frames, valid = xa.sync_fix_frames(s8, hits)
    cadu, block, info = xa.FrameDecoder("lrit").decode(frames, valid)
    a = 3                                                     # after acquisition
    assert (info["ok"][a:] == 1).all()
    dm, pa = xa.ChannelDemux(), xa.PacketAssembler()
    vcdu, off, _ = dm.process(hits[a:], cadu[a:], block[a:], info[a:])
    first = next(i for i in range(len(sent)) if np.array_equal(blocks[i, :892], block[a, :892]))
    assert first <= a and skip > first + 3
    received = {}
    for v in (2, 5, 63):
        tx = [r for u, r in sent[first:] if u == v]
        got = [bytes(r) for r in vcdu[off[v]:off[v + 1]]]
        assert len(tx) - 1 <= len(got) <= len(tx) and got == tx[:len(got)], v
        received[v] = got
    res = pa.process(vcdu, off)
    st = ps.State()
    same(res, ps.process(st, *ps.group(received)))
    same_state(xa, pa, st)
    assert st.total("discarded") == 1 and st.discarded[5] == 1
    out5 = [p for p, d in zip(pa.split(res[0], res[1]), res[1]) if d["vcid"] == 5]
    have = set(received[5])
    whole = [p for p, i, j in s5.packets if j < nrow and all(r in have for r in rows[5][i:j + 1])]
    assert out5 == whole and victim[0] not in out5              # the only one missing of those whose other rows arrived
    assert rows[5][victim[1]] in have and rows[5][victim[2]] in have
    around = [p for p, i, j in s5.packets if p != victim[0] and (i <= victim[1] <= j or i <= victim[2] <= j)]
    assert len(around) >= 2 and all(p in out5 for p in around)  # the packets in the frames around it
    assert (res[1]["crc_ok"][res[1]["length"] >= 8] == 1).all()
    dm.close()
    pa.close()


def run_host(tmp_path, extra, tag):
    host_bin = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
    r = subprocess.run([host_bin, "--input", str(tmp_path / "iq.cf32"), "--mode", "lrit", "--sample-rate", "1250000",
                        "--sink", "null", "--block", "200000"] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (tag, r.stderr)
    return r.stderr


def test_host_program_packets(xa, tmp_path):
    rng = np.random.default_rng(26)
    nrow = 8
    s0 = fixed_stream(0, [100, 950, 30, 884, 1800, 7, 500, 640, 1200, 760, 900], rng, 0xFFFFFC)
    s5 = fixed_stream(5, [2500, 80, 610, 8, 1400, 333, 1500, 900], rng, 9)
    bad = s5.headers[3]                                       # one packet's payload damaged: CRC failure, not written
    s5.rows[bad[0]][8 + bad[1] + 6] ^= 0x10
    rows = {0: [bytes(r) for r in s0.rows][:nrow], 5: [bytes(r) for r in s5.rows][:nrow], 63: random_rows(rng, nrow, 63)}
    _, cadus = cadus_of(interleave(rows))
    iq_of(cadus, 26).tofile(tmp_path / "iq.cf32")
    plain = run_host(tmp_path, ["--decode", str(tmp_path / "a.bin"), "--channels", str(tmp_path / "ch")], "channels")
    both = run_host(tmp_path, ["--decode", str(tmp_path / "b.bin"), "--channels", str(tmp_path / "ch2"),
                               "--packets", str(tmp_path / "pk")], "channels and packets")
    only = run_host(tmp_path, ["--packets", str(tmp_path / "pk2")], "packets only")
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes()
    for tag in ("decode:", "demux:"):
        line = [ln for ln in plain.splitlines() if ln.startswith(tag)]
        assert line and line == [ln for ln in both.splitlines() if ln.startswith(tag)]
    assert "packets:" not in plain
    names = sorted(os.listdir(tmp_path / "ch"))
    assert names == sorted(os.listdir(tmp_path / "ch2")) and "channel_5.bin" in names
    received = {}
    for nm in names:
        raw = (tmp_path / "ch" / nm).read_bytes()
        assert raw == (tmp_path / "ch2" / nm).read_bytes()
        received[int(nm[len("channel_"):-len(".bin")])] = [raw[i:i + 892] for i in range(0, len(raw), 892)]
    st = ps.State()
    data, desc, _, summary = ps.process(st, *ps.group(received))
    files = {}
    for p, d in zip(ps.packets_of(data, desc), desc):
        if d["crc_ok"]:
            key = f"vc{d['vcid']}_apid{d['apid']}.bin"
            files[key] = files.get(key, b"") + p
    assert len(files) >= 4 and st.total("crc_failures") >= 1
    for d in ("pk", "pk2"):
        assert sorted(os.listdir(tmp_path / d)) == sorted(files)
        for key, want in files.items():
            assert (tmp_path / d / key).read_bytes() == want, (d, key)
    line = f"packets: {st.total('packets')} emitted, {st.total('crc_failures')} CRC failures, " \
           f"{st.total('discarded')} discarded, {st.total('fill_packets')} fill"
    assert line in both.splitlines() and line in only.splitlines()
