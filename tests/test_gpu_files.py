"""GPU tier: the file assembler (xrit_files_*, FileAssembler) against the specification of tests/file_spec.py -- generator
streams with every kind of damage at tile-edge packet counts over one key and many, pieces longer than a gather step, more
pieces than one pass of the gather grid, packets of random bytes, calls cut
at random with the state compared after every call, reset, several handles, every capacity, the device path behind
decoder, demultiplexer and packet assembler on one stream.  Every comparison is exact."""
import numpy as np
import pytest

import ccsds
import file_spec as fs
import packet_spec as ps

pytestmark = pytest.mark.gpu

MANY = fs.MANY


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


def make_stream(rng, count, keys, share=0.02):
    """`count` packets of generated files over the keys, damaged."""
    if count == 0:
        return []
    stream = []
    while len(stream) < count + count // 8 + 8:
        s, _ = fs.random_stream(rng, 12, keys, max_bytes=12000, max_user=int(rng.choice([60, 200, 900])))
        stream += s
    return fs.damage(rng, stream, share)[:count]


def same(got, want):
    data, pieces, files, summary = got
    wdata, wpieces, wfiles, wsum = want
    for k, w in wsum.items():
        assert int(summary[k]) == w, k
    assert int(summary["overflow"]) == 0
    assert pieces.tobytes() == wpieces.tobytes()
    assert files.tobytes() == wfiles.tobytes()
    assert np.array_equal(data, wdata)


def same_state(fa, st):
    s = fa.stats()
    for c in fs.COUNTERS:
        assert int(s[c]) == getattr(st, c), c
    assert int(s["open_files"]) == st.open_files()
    for (v, a), k in st.keys.items():
        d = fa.key(v, a)
        got = (int(d["open"]), int(d["next_seq"]), int(d["key_serial"]), int(d["file_bytes"]), int(d["n_pieces"]),
               int(d["file_counter"]), int(d["declared_bits"])) + tuple(int(d[f]) for f in fs.HEADER_FIELDS)
        assert got == k.as_tuple(), (v, a)


@pytest.mark.parametrize("keys", ["one", "many"])
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 30000])
def test_one_call_matches_spec(xa, count, keys):
    rng = np.random.default_rng(count * 3 + len(keys))
    stream = make_stream(rng, count, [(5, 700)] if keys == "one" else MANY)
    assert len(stream) == count
    args = fs.stage_input(stream)
    fa, st = xa.FileAssembler(), fs.State()
    same(fa.process(*args), fs.process(st, *args))
    same_state(fa, st)
    # ... and once more behind itself: open files and sequence counts in front of the same packets
    same(fa.process(*args), fs.process(st, *args))
    same_state(fa, st)
    fa.close()


def test_keys_on_either_side_of_a_tile_edge(xa):
    """One call whose packets lie on the keys (v, 2047) and (v + 1, 0) alone, several files on each: the last key of one
    tile of 2048 keys and the first of the next, so the second key's bases are all the first tile's sums."""
    rng = np.random.default_rng(2047)
    v, stream = 5, []
    for key in [(v, 2047), (v + 1, 0)]:
        stream += fs.random_stream(rng, 3, [key], max_bytes=4000, max_user=200)[0]
    args = fs.stage_input(stream)
    fa, st = xa.FileAssembler(), fs.State()
    want = fs.process(st, *args)
    for key in [(v, 2047), (v + 1, 0)]:
        assert int(((want[2]["vcid"] == key[0]) & (want[2]["apid"] == key[1])).sum()) >= 2, key
    same(fa.process(*args), want)
    same_state(fa, st)
    fa.close()


def test_long_pieces_in_one_call_and_in_cut_calls(xa):
    """Pieces on either side of the gather's 2048-byte step and of two steps, of 8190 bytes and of 65524 (the generator
    and what it reaches: file_spec.long_piece_stream, checked in test_file_spec.py)."""
    stream, generated = fs.long_piece_stream()
    args = fs.stage_input(stream)
    fa, st = xa.FileAssembler(), fs.State()
    res = fa.process(*args)
    same(res, fs.process(st, *args))
    same_state(fa, st)
    assert int(res[1]["length"].max()) == 65524 and int((res[1]["length"] > 2048).sum()) >= 250
    one = fs.Collector()
    one.add(*res[:3])
    fa.reset()
    st, col = fs.State(), fs.Collector()
    rng = np.random.default_rng(37)
    for part in fs.cut_calls(rng, stream, 40):
        args = fs.stage_input(part)
        res = fa.process(*args)
        same(res, fs.process(st, *args))
        same_state(fa, st)
        col.add(*res[:3])
    # the files that came through whole are generated ones, cut or not
    for c in (one, col):
        whole = [d[3] for d in c.done if d[4]["flags"] & fs.LENGTH_MATCH]
        assert len(whole) >= 100 and all(f in generated for f in whole)
    assert sorted(d[:4] for d in col.done) == sorted(d[:4] for d in one.done)
    fa.close()


def test_more_pieces_than_one_pass_of_the_gather_grid(xa):
    """A call of more than 4096 x 8 pieces, long ones among those beyond (file_spec.many_pieces_case, checked in
    test_file_spec.py), and the same call once more behind itself."""
    args, runs = fs.many_pieces_case()
    assert runs[0][0][3]["pieces"] >= 40000
    fa = xa.FileAssembler()
    for want, st in runs:
        same(fa.process(*args), want)
        same_state(fa, st)
    fa.close()


@pytest.mark.parametrize("count", [1, 700, 20000])
def test_packets_of_random_bytes(xa, count):
    rng = np.random.default_rng(count)
    args = fs.stage_input(fs.random_packets(rng, count, [0, 17, 40], apids=(0, 1, 64, 700, 2046, 2047)))
    fa, st = xa.FileAssembler(), fs.State()
    want = fs.process(st, *args)
    same(fa.process(*args), want)
    same_state(fa, st)
    if count >= 700:
        assert {int(x) for x in want[2]["header_state"]} == {0, 1, 2} and want[3]["files_aborted"] > 0
    same(fa.process(*args), fs.process(st, *args))
    same_state(fa, st)
    fa.close()


def test_random_cuts_state_after_every_call(xa):
    rng = np.random.default_rng(31)
    stream = make_stream(rng, 4000, MANY[:12], share=0.01)
    fa, st = xa.FileAssembler(), fs.State()
    got, want = fs.Collector(), fs.Collector()
    for k in (3, 40, 400):
        for part in fs.cut_calls(rng, stream, k):
            args = fs.stage_input(part)
            res, exp = fa.process(*args), fs.process(st, *args)
            same(res, exp)
            same_state(fa, st)
            got.add(*res[:3])
            want.add(*exp[:3])
    assert len(got.done) > 30 and [d[:4] for d in got.done] == [d[:4] for d in want.done]
    assert got.aborted == want.aborted and got.partial == want.partial
    # the files that came through whole are the generated ones: cut or not, one call gives the same
    one = xa.FileAssembler()
    col = fs.Collector()
    for _ in range(3):
        col.add(*one.process(*fs.stage_input(stream))[:3])
    assert sorted(d[:4] for d in col.done) == sorted(d[:4] for d in got.done)
    assert one.stats().tobytes() == fa.stats().tobytes()
    one.close()
    fa.close()


def test_reset_and_two_handles_interleaved(xa):
    rng = np.random.default_rng(32)
    sa, sb = make_stream(rng, 1500, MANY[:6]), make_stream(rng, 1500, MANY[:6])
    a, b = xa.FileAssembler(), xa.FileAssembler()
    ta, tb = fs.State(), fs.State()
    for pa, pb in zip(fs.cut_calls(rng, sa, 300), fs.cut_calls(rng, sb, 300)):
        ia, ib = fs.stage_input(pa), fs.stage_input(pb)
        same(a.process(*ia), fs.process(ta, *ia))
        same(b.process(*ib), fs.process(tb, *ib))
    same_state(a, ta)
    same_state(b, tb)
    assert int(a.stats()["files_begun"]) > 0
    a.reset()
    fresh = xa.FileAssembler()
    assert a.stats().tobytes() == fresh.stats().tobytes()
    for v, ap in MANY[:6]:
        assert a.key(v, ap).tobytes() == fresh.key(v, ap).tobytes() == bytes(56)
    args = fs.stage_input(sb)
    want = fs.process(fs.State(), *args)
    same(a.process(*args), want)
    same(fresh.process(*args), want)
    for h in (a, b, fresh):
        h.close()


def test_each_capacity(xa):
    rng = np.random.default_rng(33)
    stream = make_stream(rng, 900, MANY[:5])
    first, second = fs.stage_input(stream[:450]), fs.stage_input(stream[450:])
    st = fs.State()
    w1 = fs.process(st, *first)
    w2 = fs.process(st, *second)
    nb, npc, nf = len(w1[0]), len(w1[1]), len(w1[2])
    assert npc > 100 and nf > 5
    for cap in ({"max_bytes": nb - 1}, {"max_pieces": npc - 1}, {"max_files": nf - 1},
                {"max_bytes": nb // 2, "max_pieces": npc // 2, "max_files": nf // 2}, {"max_bytes": 0, "max_pieces": 0, "max_files": 0}):
        fa = xa.FileAssembler()
        with pytest.raises(xa.XritError) as ei:
            fa.process(*first, **cap)
        assert ei.value.code == -5
        data, pieces, files, summary = ei.value.partial
        assert (int(summary["pieces"]), int(summary["bytes"]), int(summary["files"]), int(summary["overflow"])) == (npc, nb, nf, 1)
        for k in fs.COUNTERS:
            assert int(summary[k]) == w1[3][k]
        kp, kf, cb = cap.get("max_pieces", npc), cap.get("max_files", nf), cap.get("max_bytes", nb)
        assert pieces.tobytes() == w1[1][:kp].tobytes() and files.tobytes() == w1[2][:kf].tobytes()
        # a piece's bytes are written iff it fits whole
        ends = (w1[1]["offset"] + w1[1]["length"]).astype(np.int64)
        kb = int(max([0] + [e for e in ends[:kp] if e <= cb])) if kp else 0
        assert len(data) == (nb if cb >= nb else kb) and np.array_equal(data[:kb], w1[0][:kb])
        same(fa.process(*second), w2)                           # the state advanced as if everything had fitted
        same_state(fa, st)
        fa.close()
    fa = xa.FileAssembler()
    same(fa.process(*first, max_bytes=nb, max_pieces=npc, max_files=nf), w1)     # exactly enough is enough
    fa.close()


def test_more_packets_than_the_bound_changes_nothing(xa):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(34)
    data, desc, pko = fs.stage_input(make_stream(rng, 100, MANY[:3]))
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(data.copy()).to(dev)
    d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(dev)
    d_pko = torch.from_numpy(pko.view(np.uint8).copy()).to(dev)
    d_bytes = torch.zeros(len(data), dtype=torch.uint8, device=dev)
    d_pieces = torch.full((100 * 32,), 0xEE, dtype=torch.uint8, device=dev)
    d_files = torch.full((200 * 80,), 0xEE, dtype=torch.uint8, device=dev)
    d_sum = torch.zeros(104, dtype=torch.uint8, device=dev)
    fa = xa.FileAssembler()
    fa.process_device(d_in.data_ptr(), len(data), d_desc.data_ptr(), d_pko.data_ptr(), 99, d_bytes.data_ptr(), len(data),
                      d_pieces.data_ptr(), 100, d_files.data_ptr(), 200, d_sum.data_ptr())
    torch.cuda.synchronize()
    summ = d_sum.cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)[0]
    assert int(summ["overflow"]) == 2 and int(summ["pieces"]) == 0 and int(summ["files_begun"]) == 0
    assert (d_pieces.cpu().numpy() == 0xEE).all() and (d_files.cpu().numpy() == 0xEE).all()
    assert fa.stats().tobytes() == bytes(80)
    fa.process_device(d_in.data_ptr(), len(data), d_desc.data_ptr(), d_pko.data_ptr(), 100, d_bytes.data_ptr(), len(data),
                      d_pieces.data_ptr(), 100, d_files.data_ptr(), 200, d_sum.data_ptr())
    torch.cuda.synchronize()
    summ = d_sum.cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)[0]
    want = fs.process(fs.State(), data, desc, pko)
    same((d_bytes.cpu().numpy()[:int(summ["bytes"])], d_pieces.cpu().numpy().view(xa.FILE_PIECE_DTYPE)[:int(summ["pieces"])],
          d_files.cpu().numpy().view(xa.FILE_RECORD_DTYPE)[:int(summ["files"])], summ), want)
    fa.close()


def test_device_path_behind_decoder_demux_and_packets_one_synchronisation(xa):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(35)
    # fifteen small files on three keys of two channels, sequence counts wrapping on the way
    stream, files = [], {}
    for key in ((0, 10), (0, 11), (7, 10)):
        s, f = fs.random_stream(rng, 5, [key], max_bytes=2500, max_user=700, seq_start=16380)
        stream += s
        files.update(f)
    by_vc = {}
    for v, p, *_ in stream:
        by_vc.setdefault(v, []).append(p)
    streams = {v: ps.build_stream(v, pk, rng, fill=0.0, idle=0.0) for v, pk in by_vc.items()}
    rows = {v: [bytes(r) for r in s.rows] for v, s in streams.items()}
    sent = []
    k = 0
    while any(k < len(r) for r in rows.values()):
        sent += [(v, rows[v][k]) for v in sorted(rows) if k < len(rows[v])]
        k += 1
    n = len(sent)
    blocks = np.stack([ps.block_of(r) for _, r in sent])
    cadus = np.stack([ccsds.cadu_from_block(b) for b in blocks])
    clean = ccsds.coded_symbols(cadus).reshape(n, ccsds.FRAME_SYMBOLS).astype(np.int16)
    frames = np.clip(clean + rng.normal(0, 50, clean.shape).round(), -128, 127).astype(np.int8)
    valid = np.ones(n, np.uint8)
    hits = np.zeros((n, 4), np.uint32)
    hits[:, 2] = 60

    dev = torch.device("cuda:0")
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    d_frames = torch.from_numpy(frames.view(np.uint8).reshape(-1)).to(dev)
    d_valid = torch.from_numpy(valid).to(dev)
    d_hits = torch.from_numpy(hits.view(np.uint8).reshape(-1)).to(dev)
    d_cadu, d_block, d_info, d_vcdu, d_rec = z(n * 1024), z(n * 1020), z(n * 40), z(n * 892), z(n * 88)
    max_bytes, max_packets = xa.packets_max_bytes(n), 400
    h = n // 2
    d_off, d_pko, d_psum = z(2 * 260), z(2 * 260), z(2 * 72)
    d_pbytes, d_desc = z(2 * max_bytes), z(2 * max_packets * 32)
    d_fbytes, d_pieces, d_frecs, d_fsum = z(2 * max_bytes), z(2 * max_packets * 32), z(2 * 2 * max_packets * 80), z(2 * 104)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    dec, dm, pa, fa = xa.FrameDecoder("lrit"), xa.ChannelDemux(), xa.PacketAssembler(), xa.FileAssembler()
    with torch.cuda.stream(s):
        for k, (a, b) in enumerate(((0, h), (h, n))):
            dec.decode_device(d_frames[a * 16384:].data_ptr(), d_valid[a:].data_ptr(), b - a, d_cadu[a * 1024:].data_ptr(),
                              d_block[a * 1020:].data_ptr(), d_info[a * 40:].data_ptr(), stream=s.cuda_stream)
            dm.process_device(d_hits[a * 16:].data_ptr(), d_cadu[a * 1024:].data_ptr(), d_block[a * 1020:].data_ptr(),
                              d_info[a * 40:].data_ptr(), b - a, d_vcdu[a * 892:].data_ptr(), d_off[k * 260:].data_ptr(),
                              d_rec[a * 88:].data_ptr(), stream=s.cuda_stream)
            pa.process_device(d_vcdu[a * 892:].data_ptr(), d_off[k * 260:].data_ptr(), b - a, d_pbytes[k * max_bytes:].data_ptr(),
                              max_bytes, d_desc[k * max_packets * 32:].data_ptr(), max_packets, d_pko[k * 260:].data_ptr(),
                              d_psum[k * 72:].data_ptr(), stream=s.cuda_stream)
            fa.process_device(d_pbytes[k * max_bytes:].data_ptr(), max_bytes, d_desc[k * max_packets * 32:].data_ptr(),
                              d_pko[k * 260:].data_ptr(), max_packets, d_fbytes[k * max_bytes:].data_ptr(), max_bytes,
                              d_pieces[k * max_packets * 32:].data_ptr(), max_packets, d_frecs[k * 2 * max_packets * 80:].data_ptr(),
                              2 * max_packets, d_fsum[k * 104:].data_ptr(), stream=s.cuda_stream)
    s.synchronize()                                             # the only one
    psum = d_psum.cpu().numpy().view(xa.PACKETS_SUMMARY_DTYPE)
    fsum = d_fsum.cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)
    assert (psum["overflow"] == 0).all() and (fsum["overflow"] == 0).all()
    desc = d_desc.cpu().numpy().view(xa.PACKET_DTYPE).reshape(2, max_packets)
    pko = d_pko.cpu().numpy().view(np.uint32).reshape(2, 65)
    pbytes = d_pbytes.cpu().numpy().reshape(2, max_bytes)
    fbytes = d_fbytes.cpu().numpy().reshape(2, max_bytes)
    pieces = d_pieces.cpu().numpy().view(xa.FILE_PIECE_DTYPE).reshape(2, max_packets)
    frecs = d_frecs.cpu().numpy().view(xa.FILE_RECORD_DTYPE).reshape(2, 2 * max_packets)
    st = fs.State()
    col = fs.Collector()
    for k in range(2):
        # (the specification sees the whole input buffer: a packet is bad only where it lies outside it)
        want = fs.process(st, pbytes[k], desc[k][:int(psum[k]["packets"])], pko[k])
        got = (fbytes[k][:int(fsum[k]["bytes"])], pieces[k][:int(fsum[k]["pieces"])], frecs[k][:int(fsum[k]["files"])], fsum[k])
        same(got, want)
        col.add(*got[:3])
    same_state(fa, st)
    # ... and together: the generated files (the last of each channel may end in the fill packet's row: all rows were sent)
    assert {d[:3]: d[3] for d in col.done} == files and not col.aborted
    assert int(fsum[1]["files_completed"]) == len(files) == 15
    for x in (dec, dm, pa, fa):
        x.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_host_program_files_and_decompress(xa, tmp_path):
    """End to end: a rice-coded image file (headers by the specification's generator, lines by its encoder) and a plain
    file, packetised, put into VCDUs, coded, modulated, and through the host program from IQ: the .lrit files are the
    generated files, the .img is the generated image; a file whose end never comes stays .part."""
    import os
    import subprocess
    import rice_spec as rs
    import synth
    rng = np.random.default_rng(36)
    n, J, cols, nlines = 8, 16, 600, 16
    img = np.stack([rs.samples(rng, rs.KINDS[i % len(rs.KINDS)], n, J, cols) for i in range(nlines)])
    coded = [rs.encode(row, n, J) for row in img]
    head = fs.lrit_file(b"", image=(n, cols, nlines, 1), rice=(49, J, 1), extra=[(2, b"synthetic image")],
                        declared_data_bits=8 * sum(len(c) for c in coded))
    image_file = head + b"".join(coded)
    cuts = [int(c) for c in np.cumsum([len(head)] + [len(c) for c in coded])[:-1]]
    image_packets, _ = fs.packetise(image_file, 40, 16375, 1, cuts=cuts)
    assert len(image_packets) == nlines + 1
    plain_file = fs.lrit_file(rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), file_type=2, extra=[(4, b"\x01" * 7)])
    plain_packets, _ = fs.packetise(plain_file, 41, 7, 2, max_user=900)
    open_packets, _ = fs.packetise(fs.lrit_file(bytes(1500)), 42, 0, 3, max_user=400)

    def dummies(count, seq):                                  # unsegmented one-packet files: what acquisition may eat, what flushes the end
        return [fs.space_packet(99, seq + i, 3, rng.integers(0, 256, 600, dtype=np.uint8).tobytes()) for i in range(count)]

    streams = {5: ps.build_stream(5, dummies(7, 0) + image_packets + dummies(6, 7), rng, start_counter=100, fill=0.0, idle=0.0),
               0: ps.build_stream(0, dummies(7, 0) + plain_packets + open_packets[:-1] + dummies(6, 7), rng, start_counter=0xFFFFFA,
                                  fill=0.0, idle=0.0)}
    rows = {v: [bytes(r) for r in s.rows] for v, s in streams.items()}
    sent, k = [], 0
    while any(k < len(r) for r in rows.values()):
        sent += [rows[v][k] for v in sorted(rows) if k < len(rows[v])]
        k += 1
    cadus = np.stack([ccsds.cadu_from_block(ps.block_of(r)) for r in sent])
    sym = ccsds.coded_symbols(cadus, amplitude=1).astype(np.float64)
    p = synth.SynthParams(fs_in=1.25e6, seed=36, esn0_db=12.0)
    synth.generate(p, int((len(sym) + 64) * p.sps_in), symbols=sym).tofile(tmp_path / "iq.cf32")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host_bin = os.path.join(root, "xritdemod_amd", "bin", "xrit_demod_host")
    out = tmp_path / "files"
    r = subprocess.run([host_bin, "--input", str(tmp_path / "iq.cf32"), "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null",
                        "--block", "200000", "--files", str(out), "--files-decompress"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    names = set(os.listdir(out))
    assert (out / "vc5_apid40_0.lrit").read_bytes() == image_file
    assert (out / "vc5_apid40_0.img").read_bytes() == img.astype(np.uint8).tobytes()
    assert (out / "vc0_apid41_0.lrit").read_bytes() == plain_file and "vc0_apid41_0.img" not in names
    assert "vc0_apid42_0.lrit.part" in names and "vc0_apid42_0.lrit" not in names
    assert (out / "vc0_apid42_0.lrit.part").read_bytes() == fs.lrit_file(bytes(1500))[:sum(len(q) - 8 for q in open_packets[:-1]) - 10]
    assert not [nm for nm in names if nm.endswith(".img.part")] and len([nm for nm in names if nm.endswith(".img")]) == 1
    assert f"rice: {nlines} lines decoded, 0 faulted" in r.stderr.splitlines()
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("files:")]
    assert len(line) == 1 and " 0 aborted" in line[0]
    assert not os.path.exists(tmp_path / "pk")                  # --files writes no packet dumps
