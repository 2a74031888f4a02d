"""GPU tier: the image stage (xrit_images_*, ImageDecoder) against the specification of tests/image_spec.py -- images of
mixed (bits, block, columns) in one call, streams cut into small calls with the state compared after every call, two
files on one key in one call, damaged streams and lines, every capacity, the refused call, reset, two handles, the device
path behind lock, demultiplexer, packet and file assembler on one stream, the per-record decode that existed before, and
pieces that lie outside the bytes; calls tiled over up to 65 537 keys (image_spec.tile_call) with 63 to 524 289
records -- full waves and tiles, second tiles, every kernel's grid cap and the stride behind it, a second round of the
scan over the tiles --, two such calls on one handle, the device-pointer path with bounds four times the counts,
capacities that cut in a later tile, lines with long codes, and image files whose lines libaec encoded
(tests/golden/rice_libaec_lines.npz) against the samples they were made from.
Every comparison is exact."""
import functools

import numpy as np
import pytest

import ccsds
import file_spec as fs
import image_spec as isp
import packet_spec as ps
import rice_spec as rs

pytestmark = pytest.mark.gpu

# (bits, block, columns, rows): 8- and 16-bit lines adjacent, a 5-byte line padded to 8, a one-sample line
MIXED = [(8, 16, 300, 20), (10, 64, 1000, 7), (8, 8, 5, 3), (16, 32, 33, 2), (1, 8, 1, 4)]
MIXED_KEYS = [(2, 100), (2, 101), (5, 100), (5, 101), (5, 100)]


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


def mixed_stream():
    """The five images on four keys of two channels, an image file that is not compressed and a rice-coded one whose
    first packet also carries data (so header_length is not the first piece's length) -> (stream, images)."""
    rng = np.random.default_rng(41)
    items, images, serial = [], {}, {}
    for (n, J, cols, rows), key in zip(MIXED, MIXED_KEYS):
        img, data, cuts = isp.image_file(rng, n, J, cols, rows)
        images[key + (serial.get(key, 0),)] = img
        serial[key] = serial.get(key, 0) + 1
        items.append((key, data, cuts, 8190))
    items.append(((2, 100), fs.lrit_file(rng.integers(0, 256, 700, dtype=np.uint8).tobytes(), image=(8, 35, 20, 0)), None, 300))
    _, data, _ = isp.image_file(rng, 8, 16, 64, 4)
    items.append(((5, 102), data, None, 100))
    return isp.stream_of(rng, items, seq_start=16370), images


@pytest.fixture(scope="module")
def mixed():
    """The stream, its images, and the specification's one call on it (shared, never changed)."""
    stream, images = mixed_stream()
    fst, ist = fs.State(), isp.State()
    files_out = isp.run_files(fst, stream)
    want = isp.process(ist, *files_out[:3])
    rows = isp.Rows()
    rows.add(want[0], want[1], files_out[2])
    return dict(stream=stream, images=images, files_out=files_out, want=want, rows=rows, state=ist)


def files_summary(xa, summ, overflow=0):
    """A FILES_SUMMARY_DTYPE record from the specification's dict."""
    s = np.zeros(1, xa.FILES_SUMMARY_DTYPE)
    for k, v in summ.items():
        s[0][k] = v
    s[0]["overflow"] = overflow
    return s


def same(got, want):
    data, lines, ifiles, summary = got
    wdata, wlines, wfiles, wsum = want
    for k, w in wsum.items():
        assert int(summary[k]) == w, k
    assert int(summary["overflow"]) == 0
    assert lines.tobytes() == wlines.tobytes()
    assert ifiles.tobytes() == wfiles.tobytes()
    assert np.array_equal(data, wdata)


def same_state(im, st):
    s = im.stats()
    for c in isp.COUNTERS:
        assert int(s[c]) == getattr(st, c), c
    for (v, a), k in st.keys.items():
        d = im.key(v, a)
        assert (int(d["open"]), int(d["key_serial"]), int(d["lines"]), int(d["faults"])) == k.as_tuple(), (v, a)
        assert not d["reserved"].any()


def both(xa, im, ist, fst, part):
    """The specification's files call on a piece of stream, then device and specification on its outputs."""
    data, pieces, files, summ = isp.run_files(fst, part)
    got = im.process(data, pieces, files, files_summary(xa, summ))
    want = isp.process(ist, data, pieces, files)
    return files, got, want


def same_rows(a, b):
    assert a.rows.keys() == b.rows.keys()
    for key, (x, status) in a.rows.items():
        assert status == b.rows[key][1] and np.array_equal(x, b.rows[key][0]), key


def test_mixed_parameters_in_one_call(xa, mixed):
    data, pieces, files, summ = mixed["files_out"]
    want = mixed["want"]
    assert [int(x) for x in want[2]["rice"]] == [1, 0, 1, 1, 1, 1, 0] and want[3]["lines"] == 36
    bits = want[1]["bits"].astype(int)
    assert ((bits[:-1] <= 8) & (bits[1:] > 8)).any() and ((bits[:-1] > 8) & (bits[1:] <= 8)).any()
    assert {(5, 8), (1, 4)} <= {(int(l), int(b - a)) for l, a, b in zip(want[1]["length"], want[1]["offset"],
                                                                        list(want[1]["offset"][1:]) + [want[3]["bytes"]])}
    im = xa.ImageDecoder()
    got = im.process(data, pieces, files, files_summary(xa, summ))
    same(got, want)
    same_state(im, mixed["state"])
    rows = isp.Rows()
    rows.add(got[0], got[1], files)
    for (v, a, serial), img in mixed["images"].items():
        x, status = rows.image(v, a, serial)
        assert not status.any() and np.array_equal(x, img), (v, a, serial)
    assert [r.tolist() for r in xa.ImageDecoder.rows(got[0], got[1])] == [rows.rows[k][0].tolist() for k in sorted(
        rows.rows, key=lambda k: (k[0], k[1], k[2], k[3]))]
    im.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cut_streams(xa, mixed, seed):
    rng = np.random.default_rng(seed)
    im, ist, fst = xa.ImageDecoder(), isp.State(), fs.State()
    rows = isp.Rows()
    calls = 0
    for part in fs.cut_calls(rng, mixed["stream"], 3):
        files, got, want = both(xa, im, ist, fst, part)
        same(got, want)
        same_state(im, ist)
        rows.add(got[0], got[1], files)
        calls += 1
    assert calls > len(mixed["stream"]) // 3
    same_rows(rows, mixed["rows"])
    assert im.stats().tobytes() == np.array([tuple(getattr(mixed["state"], c) for c in isp.COUNTERS)], xa.IMAGES_STATS_DTYPE).tobytes()
    im.close()


def test_two_files_on_one_key_in_one_call(xa):
    rng = np.random.default_rng(42)
    img, data, cuts = isp.image_file(rng, 12, 16, 50, 5)
    plain = fs.lrit_file(rng.integers(0, 256, 300, dtype=np.uint8).tobytes(), file_type=2)
    key = (9, 77)
    for order in ("image first", "image last"):
        items = [(key, data, cuts, 8190), (key, plain, None, 100)]
        stream = isp.stream_of(rng, items if order == "image first" else items[::-1])
        n_img, cut = 6, 3
        im, ist, fst = xa.ImageDecoder(), isp.State(), fs.State()
        # the first call ends inside the first file, the second holds the rest of it and the whole other file
        for part in (stream[:cut], stream[cut:]):
            files, got, want = both(xa, im, ist, fst, part)
            same(got, want)
            same_state(im, ist)
        assert len(files) == 2 and [int(x) for x in got[2]["rice"]] == ([1, 0] if order == "image first" else [0, 1])
        assert ist.keys[key].as_tuple() == ((0, 1, 0, 0) if order == "image first" else (0, 1, 5, 0))
        assert ist.total_lines == n_img - 1 and ist.images_completed == 1
        im.close()
    # an image left open by the call before; its only record in this call is the bare ABORTED one
    stream = isp.stream_of(rng, [(key, data, cuts, 8190)])
    im, ist, fst = xa.ImageDecoder(), isp.State(), fs.State()
    for part, flags in ((stream[:3], fs.BEGINS), (stream[4:5], fs.ABORTED)):
        files, got, want = both(xa, im, ist, fst, part)
        assert len(files) == 1 and int(files[0]["flags"]) == flags
        same(got, want)
        same_state(im, ist)
    assert int(files[0]["n_pieces"]) == 0 and int(got[2][0]["rice"]) == 1 and int(got[2][0]["lines_total"]) == 2
    assert ist.keys[key].as_tuple() == (0, 0, 2, 0) and ist.images_aborted == 1 and len(got[1]) == 0
    im.close()


def damaged_stream():
    """Fourteen images over five keys: a tenth of the coded lines truncated and a tenth with a flipped bit before they are
    packed (the CRCs are the damaged lines'), then one packet removed inside an image, one CRC broken, one packet
    repeated -> the stream."""
    rng = np.random.default_rng(43)

    def spoil(r, line):
        u = r.random()
        return rs.truncate(r, line) if u < 0.1 else rs.flip(r, line) if u < 0.2 else line

    stream, images = isp.random_stream(rng, 14, [(0, 1), (0, 2), (3, 1), (3, 700), (40, 2047)], n_other=3, max_cols=200, max_rows=14,
                                  spoil=spoil)
    inside = [i for i, e in enumerate(stream) if e[2][:3] in images and 2 <= e[2][3] < e[2][4] - 2]
    a, b, c = (inside[int(len(inside) * f)] for f in (0.2, 0.5, 0.8))
    assert len({stream[i][2][:3] for i in (a, b, c)}) == 3          # three different files
    stream = fs.repeat(stream, c)
    stream = fs.bad_crc(stream, b)
    return fs.remove(stream, a)


def test_damage(xa):
    stream = damaged_stream()
    rng = np.random.default_rng(44)
    # from the specification alone, before the GPU is touched: the case holds what it is for
    fst, ist = fs.State(), isp.State()
    files_out = isp.run_files(fst, stream)
    want = isp.process(ist, *files_out[:3])
    status = want[1]["status"]
    print("lines", len(status), "ok", int((status == 0).sum()), "faulted", int((status == 1).sum()), "aborted", ist.images_aborted)
    assert 2 * int((status == 0).sum()) >= len(status) and int((status == 1).sum()) >= 10 and ist.images_aborted >= 1
    assert ist.images_begun >= 12
    im = xa.ImageDecoder()
    same(im.process(files_out[0], files_out[1], files_out[2], files_summary(xa, files_out[3])), want)
    same_state(im, ist)
    im.close()
    # ... and cut into calls: the same rows, the state after every call
    im, ist2, fst = xa.ImageDecoder(), isp.State(), fs.State()
    rows, whole = isp.Rows(), isp.Rows()
    whole.add(want[0], want[1], files_out[2])
    for part in fs.cut_calls(rng, stream, 9):
        files, got, exp = both(xa, im, ist2, fst, part)
        same(got, exp)
        same_state(im, ist2)
        rows.add(got[0], got[1], files)
    same_rows(rows, whole)
    for c in isp.COUNTERS:
        assert getattr(ist2, c) == getattr(ist, c), c
    im.close()


def test_each_capacity(xa, mixed):
    stream = mixed["stream"]
    half = len(stream) // 2
    fst, ist = fs.State(), isp.State()
    f1, f2 = isp.run_files(fst, stream[:half]), isp.run_files(fst, stream[half:])
    w1 = isp.process(ist, *f1[:3])
    w2 = isp.process(ist, *f2[:3])
    nb, nl = len(w1[0]), len(w1[1])
    assert nl > 8 and w2[3]["lines"] > 0
    ends = (w1[1]["offset"] + ((w1[1]["length"].astype(np.uint64) + 3) & ~np.uint64(3))).astype(np.int64)
    for cap in ({"max_lines": nl - 1}, {"max_bytes": nb - 1}, {"max_lines": nl // 2, "max_bytes": nb // 2}, {"max_lines": 0, "max_bytes": 0}):
        im = xa.ImageDecoder()
        with pytest.raises(xa.XritError) as ei:
            im.process(f1[0], f1[1], f1[2], files_summary(xa, f1[3]), **cap)
        assert ei.value.code == -5
        data, lines, ifiles, summary = ei.value.partial
        assert (int(summary["lines"]), int(summary["bytes"]), int(summary["images"]), int(summary["overflow"])) == \
               (nl, nb, w1[3]["images"], 1)
        for k in isp.COUNTERS:
            assert int(summary[k]) == w1[3][k], k
        kl, cb = cap.get("max_lines", nl), cap.get("max_bytes", nb)
        assert lines.tobytes() == w1[1][:kl].tobytes() and ifiles.tobytes() == w1[2].tobytes()
        # a line's samples are written iff it fits whole, padding included
        fit = [int(e) for e in ends[:kl] if e <= cb]
        kb = max([0] + fit)
        assert len(data) == (nb if cb >= nb else kb)
        for ln in w1[1][:kl]:
            a, b = int(ln["offset"]), int(ln["offset"]) + ((int(ln["length"]) + 3) & ~3)
            if b <= cb:
                assert np.array_equal(data[a:b], w1[0][a:b])
        same(im.process(f2[0], f2[1], f2[2], files_summary(xa, f2[3])), w2)          # the state advanced as if everything had fitted
        same_state(im, ist)
        im.close()
    im = xa.ImageDecoder()
    same(im.process(f1[0], f1[1], f1[2], files_summary(xa, f1[3]), max_lines=nl, max_bytes=nb), w1)       # exactly enough is enough
    im.close()


def test_refused_calls_change_nothing(xa, mixed):
    torch = pytest.importorskip("torch")
    stream = mixed["stream"]
    half = len(stream) // 2
    fst, ist = fs.State(), isp.State()
    f1, f2 = isp.run_files(fst, stream[:half]), isp.run_files(fst, stream[half:])
    im = xa.ImageDecoder()
    same(im.process(f1[0], f1[1], f1[2], files_summary(xa, f1[3])), isp.process(ist, *f1[:3]))
    stats, keys = im.stats().tobytes(), [im.key(v, a).tobytes() for v, a in MIXED_KEYS]
    assert any(im.key(v, a)["open"] for v, a in MIXED_KEYS)
    data, pieces, files, summ = f2
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_data, d_pieces, d_files = up(data), up(pieces), up(files)
    nb = xa.images_max_bytes(files)
    for how in ("files overflow", "pieces bound", "files bound"):
        d_fsum = up(files_summary(xa, summ, overflow=1 if how == "files overflow" else 0))
        d_out, d_lines = (torch.full((n,), 0xA5, dtype=torch.uint8, device=dev) for n in (nb, len(pieces) * 32))
        d_ifiles, d_sum = (torch.full((n,), 0xA5, dtype=torch.uint8, device=dev) for n in (len(files) * 48, 80))
        im.process_device(d_data.data_ptr(), len(data), d_pieces.data_ptr(), len(pieces) - (how == "pieces bound"), d_files.data_ptr(),
                          len(files) - (how == "files bound"), d_fsum.data_ptr(), d_out.data_ptr(), nb, d_lines.data_ptr(), len(pieces),
                          d_ifiles.data_ptr(), d_sum.data_ptr())
        torch.cuda.synchronize()
        s = d_sum.cpu().numpy().view(xa.IMAGES_SUMMARY_DTYPE)[0]
        assert int(s["overflow"]) == 2 and int(s["lines"]) == int(s["bytes"]) == int(s["images"]) == 0, how
        assert bytes(s.tobytes()[24:72]) == stats                   # the handle's counters as they were
        for t in (d_out, d_lines, d_ifiles):
            assert (t.cpu().numpy() == 0xA5).all(), how
        assert im.stats().tobytes() == stats and [im.key(v, a).tobytes() for v, a in MIXED_KEYS] == keys, how
    # the host-buffer call says so too
    with pytest.raises(xa.XritError) as ei:
        im.process(data, pieces, files, files_summary(xa, summ, overflow=1))
    assert ei.value.code == -1 and int(ei.value.partial[3]["overflow"]) == 2 and len(ei.value.partial[1]) == 0
    with pytest.raises(xa.XritError) as ei:
        im.process(data, pieces[:-1], files, files_summary(xa, summ))
    assert ei.value.code == -1 and int(ei.value.partial[3]["overflow"]) == 2
    assert im.stats().tobytes() == stats and [im.key(v, a).tobytes() for v, a in MIXED_KEYS] == keys
    # ... and the call that is not refused goes on from the unchanged state
    same(im.process(data, pieces, files, files_summary(xa, summ)), isp.process(ist, data, pieces, files))
    same_state(im, ist)
    im.close()


def test_reset_and_two_handles_interleaved(xa, mixed):
    rng = np.random.default_rng(45)
    sa = mixed["stream"]
    sb, _ = isp.random_stream(rng, 6, [(2, 100), (5, 100), (11, 3)], n_other=2, max_cols=90, max_rows=6)
    a, b = xa.ImageDecoder(), xa.ImageDecoder()
    ta, tb, fa, fb = isp.State(), isp.State(), fs.State(), fs.State()
    for pa, pb in zip(fs.cut_calls(rng, sa, 8), fs.cut_calls(rng, sb, 8)):
        _, got, want = both(xa, a, ta, fa, pa)
        same(got, want)
        _, got, want = both(xa, b, tb, fb, pb)
        same(got, want)
    same_state(a, ta)
    same_state(b, tb)
    assert int(a.stats()["images_begun"]) > 0 and int(b.stats()["images_begun"]) > 0
    # reset in the middle of an image: that image's later lines are nobody's, the next image is decoded
    img1, d1, c1 = isp.image_file(rng, 8, 16, 40, 6)
    img2, d2, c2 = isp.image_file(rng, 9, 32, 40, 3)
    stream = isp.stream_of(rng, [((1, 1), d1, c1, 8190), ((1, 1), d2, c2, 8190)])
    im, fst = xa.ImageDecoder(), fs.State()
    f1, f2 = isp.run_files(fst, stream[:4]), isp.run_files(fst, stream[4:])
    same(im.process(f1[0], f1[1], f1[2], files_summary(xa, f1[3])), isp.process(isp.State(), *f1[:3]))
    assert int(im.key(1, 1)["open"]) == 1 and int(im.stats()["total_lines"]) == 3
    im.reset()
    fresh = xa.ImageDecoder()
    assert im.stats().tobytes() == fresh.stats().tobytes() == bytes(48) and im.key(1, 1).tobytes() == bytes(16)
    ist = isp.State()
    want = isp.process(ist, *f2[:3])
    got = im.process(f2[0], f2[1], f2[2], files_summary(xa, f2[3]))
    same(got, want)
    same_state(im, ist)
    assert [int(x) for x in got[2]["rice"]] == [0, 1] and int(got[3]["lines"]) == 3
    assert np.array_equal(np.stack(xa.ImageDecoder.rows(got[0], got[1])), img2)
    for h in (a, b, im, fresh):
        h.close()


def test_device_path_behind_lock_demux_packets_and_files_one_synchronisation(xa):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(46)
    items, images = [], {}
    for key, (n, J, cols, rows) in (((4, 20), (8, 16, 900, 16)), ((6, 21), (11, 32, 600, 14))):
        img, data, cuts = isp.image_file(rng, n, J, cols, rows, kinds=("uniform", "scaled"))
        images[key + (0,)] = img
        items.append((key, data, cuts, 8190))
    stream = isp.stream_of(rng, items)
    by_vc = {}
    for v, p, *_ in stream:
        by_vc.setdefault(v, []).append(p)
    # (unsegmented one-packet files in front and behind: what flushes the last row of a channel)
    dummies = lambda count: [fs.space_packet(99, i, 3, rng.integers(0, 256, 800, dtype=np.uint8).tobytes()) for i in range(count)]
    streams = {v: ps.build_stream(v, dummies(2) + pk + dummies(3), rng, fill=0.0, idle=0.0) for v, pk in by_vc.items()}
    rows = {v: [bytes(r) for r in s.rows] for v, s in streams.items()}
    sent, k = [], 0
    while any(k < len(r) for r in rows.values()):
        sent += [rows[v][k] for v in sorted(rows) if k < len(rows[v])]
        k += 1
    n = len(sent)
    assert 25 <= n <= 60
    cadus = np.stack([ccsds.cadu_from_block(ps.block_of(r)) for r in sent])
    sym = ccsds.coded_symbols(cadus, amplitude=40).reshape(-1).astype(np.int8)
    third = len(sym) // 3 + 1000
    pushes = [sym[:third], sym[third:2 * third], sym[2 * third:]]

    dev = torch.device("cuda:0")
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    lock, dm, pa, fa, im = xa.FrameLock("lrit"), xa.ChannelDemux(), xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder()
    d_sym = [torch.from_numpy(p.view(np.uint8).copy()).to(dev) for p in pushes]
    bufs = []
    for p in pushes:
        cap = lock.rows(len(p))
        mb, mp = xa.packets_max_bytes(cap), 16 * cap + 64
        sizes = dict(frames=cap * 16384, valid=cap, hits=cap * 16, start=cap * 8, mode=cap, cadu=cap * 1024, block=cap * 1020,
                     info=cap * 40, count=8, vcdu=cap * 892, off=65 * 4, rec=cap * 88, pbytes=mb, desc=mp * 32, pko=65 * 4, psum=72,
                     fbytes=mb, pieces=mp * 32, frecs=2 * mp * 80, fsum=104, out=mp * 1400, lines=mp * 32, ifiles=2 * mp * 48, isum=80)
        bufs.append((cap, mb, mp, {k_: z(v) for k_, v in sizes.items()}))
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for d, p, (cap, mb, mp, b) in zip(d_sym, pushes, bufs):
            q = {k_: t.data_ptr() for k_, t in b.items()}
            lock.push_device(d.data_ptr(), len(p), q["frames"], q["valid"], q["hits"], q["start"], q["mode"], q["cadu"], q["block"],
                             q["info"], q["count"], stream=s.cuda_stream)
            dm.process_device(q["hits"], q["cadu"], q["block"], q["info"], cap, q["vcdu"], q["off"], q["rec"], stream=s.cuda_stream)
            pa.process_device(q["vcdu"], q["off"], cap, q["pbytes"], mb, q["desc"], mp, q["pko"], q["psum"], stream=s.cuda_stream)
            fa.process_device(q["pbytes"], mb, q["desc"], q["pko"], mp, q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"],
                              stream=s.cuda_stream)
            im.process_device(q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"], q["out"], mp * 1400, q["lines"], mp,
                              q["ifiles"], q["isum"], stream=s.cuda_stream)
    s.synchronize()                                             # the only one of this test's own
    # the host-buffer path, stage by stage
    h_lock, h_dm, h_pa, h_fa, h_im = xa.FrameLock("lrit"), xa.ChannelDemux(), xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder()
    got_rows, want_rows = isp.Rows(), isp.Rows()
    total = 0
    for p, (cap, mb, mp, b) in zip(pushes, bufs):
        frames, valid, hits, start, mode, cadu, block, info = h_lock.push(p)
        vcdu, off = h_dm.process(hits, cadu, block, info)[:2]
        pdata, pdesc, pko = h_pa.process(vcdu, off)[:3]
        fdata, fpieces, ffiles, fsum = h_fa.process(pdata, pdesc, pko)
        want = h_im.process(fdata, fpieces, ffiles, fsum)
        isum = b["isum"].cpu().numpy().view(xa.IMAGES_SUMMARY_DTYPE)[0]
        d_fsum = b["fsum"].cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)[0]
        assert d_fsum.tobytes() == fsum.tobytes() and int(isum["overflow"]) == 0
        assert isum.tobytes() == want[3].tobytes()
        nl, nbytes, nfiles = int(isum["lines"]), int(isum["bytes"]), int(fsum["files"])
        lines = b["lines"].cpu().numpy().view(xa.IMAGE_LINE_DTYPE)[:nl]
        ifiles = b["ifiles"].cpu().numpy().view(xa.IMAGE_FILE_DTYPE)[:nfiles]
        out = b["out"].cpu().numpy()[:nbytes]
        assert lines.tobytes() == want[1].tobytes() and ifiles.tobytes() == want[2].tobytes() and np.array_equal(out, want[0])
        got_rows.add(out, lines, ffiles)
        want_rows.add(want[0], want[1], ffiles)
        total += nl
    assert total == 30 and im.stats().tobytes() == h_im.stats().tobytes() and int(im.stats()["images_completed"]) == 2
    for (v, a, serial), img in images.items():
        x, status = got_rows.image(v, a, serial)
        assert not status.any() and np.array_equal(x, img)
    for x in (lock, dm, pa, fa, im, h_lock, h_dm, h_pa, h_fa, h_im):
        x.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_equals_decode_file_lines_per_record(xa, mixed):
    data, pieces, files, summ = mixed["files_out"]
    im = xa.ImageDecoder()
    out, lines, ifiles, _ = im.process(data, pieces, files, files_summary(xa, summ))
    seen = 0
    for f, rec in enumerate(files):
        old = xa.decode_file_lines(rec, pieces, data)
        if old is None:
            assert int(ifiles[f]["rice"]) == 0
            continue
        samples, status = old
        mine = lines[int(ifiles[f]["first_line"]):int(ifiles[f]["first_line"]) + int(ifiles[f]["n_lines"])]
        assert int(ifiles[f]["rice"]) == 1 and len(mine) == len(samples) and (mine["file"] == f).all()
        assert np.array_equal(mine["status"], status)
        new = np.stack(xa.ImageDecoder.rows(out, mine))
        assert new.dtype == samples.dtype and np.array_equal(new, samples)
        seen += 1
    assert seen == 5
    im.close()


def test_pieces_outside_the_bytes_are_status_2(xa, mixed):
    """The guard of the Rice decoder, per line: a piece that does not lie inside the bytes handed over is not read; its
    line is all zero with status 2 and counts as a fault."""
    data, pieces, files, summ = mixed["files_out"]
    cut = int(pieces[len(pieces) // 2]["offset"]) + 1                # inside a piece: it and everything behind it lie outside
    want = isp.process(isp.State(), data[:cut], pieces, files)
    status = want[1]["status"]
    assert (status == 2).sum() > 5 and (status == 0).sum() > 5 and want[3]["total_faults"] == int((status == 2).sum())
    im = xa.ImageDecoder()
    same(im.process(data[:cut], pieces, files, files_summary(xa, summ)), want)
    im.close()


def test_image_files_of_lines_encoded_by_libaec(xa):
    """An 8-bit and a 10-bit image file whose lines libaec 1.0.4 encoded (tests/golden/rice_libaec_lines.npz; columns no
    multiple of the block, so the last block of every line is padded libaec's way), through the file assembler and this
    stage: the host-buffer form, and the device form on a side stream.  The rows are the samples the lines were made
    from; neither rs.encode nor rs.decode is in the chain."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(47)
    groups = [g for g in rs.libaec_groups() if g[3] == 0]
    items, images = [], {}
    for key, bits in (((3, 8), 8), ((3, 10), 10)):
        n, J, S, _, lines, samples = next(g for g in groups if g[0] == bits and g[2] > 1 and max(len(ln) for ln in g[4]) <= 8190)
        assert S % J and len(lines) >= 20
        _, data, cuts = isp.image_file(rng, n, J, S, len(lines), coded=lines)
        items.append((key, data, cuts, 8190))
        images[key] = samples
    stream = isp.stream_of(rng, items)
    fa, im = xa.FileAssembler(), xa.ImageDecoder()
    data, pieces, files, fsum = fa.process(*fs.stage_input(stream))
    assert len(files) == 2 and (files["flags"] == fs.BEGINS | fs.ENDS | fs.LENGTH_MATCH).all()
    got = im.process(data, pieces, files, fsum)

    def rows_are_the_fixture_s(out, lines):
        assert len(lines) == sum(len(s) for s in images.values()) and not lines["status"].any()
        rows = isp.Rows()
        rows.add(out, lines, files)
        for (v, a), samples in images.items():
            x, status = rows.image(v, a, 0)
            assert not status.any() and np.array_equal(x, samples), (v, a)

    assert [int(x) for x in got[2]["rice"]] == [1, 1] and int(got[3]["images_completed"]) == 2 and int(got[3]["total_faults"]) == 0
    rows_are_the_fixture_s(got[0], got[1])
    # the device form on a side stream: the same bytes
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.atleast_1d(a)).view(np.uint8).reshape(-1).copy()).to(dev)
    d_data, d_pieces, d_files, d_fsum = up(data), up(pieces), up(files), up(fsum)
    nb = xa.images_max_bytes(files)
    d_out, d_lines = (torch.full((k,), 0xA5, dtype=torch.uint8, device=dev) for k in (nb, len(pieces) * 32))
    d_ifiles, d_sum = (torch.full((k,), 0xA5, dtype=torch.uint8, device=dev) for k in (len(files) * 48, 80))
    im2 = xa.ImageDecoder()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        im2.process_device(d_data.data_ptr(), len(data), d_pieces.data_ptr(), len(pieces), d_files.data_ptr(), len(files),
                           d_fsum.data_ptr(), d_out.data_ptr(), nb, d_lines.data_ptr(), len(pieces), d_ifiles.data_ptr(),
                           d_sum.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    isum = d_sum.cpu().numpy().view(xa.IMAGES_SUMMARY_DTYPE)[0]
    assert isum.tobytes() == got[3].tobytes()
    nl, nbytes = int(isum["lines"]), int(isum["bytes"])
    lines = d_lines.cpu().numpy().view(xa.IMAGE_LINE_DTYPE)[:nl]
    assert lines.tobytes() == got[1].tobytes() and d_ifiles.cpu().numpy().tobytes() == got[2].tobytes()
    assert np.array_equal(d_out.cpu().numpy()[:nbytes], got[0])
    rows_are_the_fixture_s(d_out.cpu().numpy()[:nbytes], lines)
    for h in (fa, im, im2):
        h.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- calls beyond one tile ---------------------------------------------------------------------------------------------
# Record indices at which the device's work changes hands: the waves of a tile (64), the tiles (IMAGES_TILE = 1024), the
# records kernel's grid (4096 workgroups of 4 waves: 16384 records, a stride behind them), the rounds of 64 tiles in the
# scan over the tiles (65536), the grids of the mark kernel (1024 x 256 records) and of the tile kernel (512 tiles).
BOUNDARIES = (64, 1024, 16384, 65536, 262144, 524288)
DECODE_GRID = 8192 * 4            # pieces: the decode kernel strides behind them


@functools.lru_cache(maxsize=None)
def tiling():
    """The files calls that the large calls are tiled from (image_spec.tiling_base and one more image on its key):
    first -- a file that is no image, an 8-bit image with a truncated line, a 12-bit image left open --, second -- the
    rest of that image, nothing else --, third -- a 10-bit image left open after two lines --, fourth -- its rest."""
    stream, cut, _ = isp.tiling_base()
    rng = np.random.default_rng(52)
    _, data, cuts = isp.image_file(rng, 10, 32, 7, 4, kinds=("uniform", "sparse"))
    more = isp.stream_of(rng, [((0, 0), data, cuts, 8190)])
    fst = fs.State()
    return tuple(isp.run_files(fst, part) for part in (stream[:cut], stream[cut:], more[:3], more[3:]))


@functools.lru_cache(maxsize=None)
def large_call(records):
    """`records` records of the tiled first call -> (files call, the specification's outputs, its state behind the
    call); shared, never changed."""
    first = tiling()[0]
    call = isp.head_of_call(isp.tile_call(first, -(-records // len(first[2]))), records)
    st = isp.State()
    return call, isp.process(st, *call[:3]), st


def holds_what_it_is_for(call, want):
    """From the specification alone: faults, records that are rice-coded images and records that are not, and at every
    boundary inside the call both kinds among the three records in front of it, a rice-coded record with lines ON it
    (its first line and offset are sums over everything in front) and, where the call goes on, both kinds behind it."""
    rice = want[2]["rice"].astype(bool)
    n = len(rice)
    assert want[3]["total_faults"] > 0 and rice.any() and not rice.all() and want[3]["lines"] > 0
    inside = [b for b in BOUNDARIES if b < n]
    for b in inside:
        assert rice[b - 3:b].any() and not rice[b - 3:b].all(), b
        assert rice[b] and int(want[2]["n_lines"][b]) > 0 and int(want[2]["first_line"][b]) > 0 and int(want[2]["offset"][b]) > 0, b
        if n >= b + 3:
            assert not rice[b:b + 3].all(), b
    return inside


def sampled_keys(files, seed=0):
    """The first and the last key, the keys of the records on both sides of every boundary, and fifty drawn."""
    n = len(files)
    idx = {0, n - 1} | {i for b in BOUNDARIES for i in (b - 1, b) if i < n}
    idx |= {int(i) for i in np.random.default_rng(seed).integers(0, n, 50)}
    return sorted({(int(files[i]["vcid"]), int(files[i]["apid"])) for i in idx})


def same_state_sampled(im, st, keys):
    """same_state with the keys read back a sample (every key read waits for the device once)."""
    s = im.stats()
    for c in isp.COUNTERS:
        assert int(s[c]) == getattr(st, c), c
    for v, a in keys:
        d = im.key(v, a)
        assert (int(d["open"]), int(d["key_serial"]), int(d["lines"]), int(d["faults"])) == st.keys[(v, a)].as_tuple(), (v, a)
        assert not d["reserved"].any()


@pytest.mark.parametrize("records", [63, 64, 65, 1023, 1024, 1025, 2049, 16383, 16385, 65537, "pieces"])
def test_one_call_matches_spec(xa, records):
    """One call of that many records, tiled from the small one; "pieces": the smallest whole number of copies with more
    pieces than the decode kernel's grid has waves."""
    if records == "pieces":
        first = tiling()[0]
        records = len(first[2]) * (DECODE_GRID // len(first[1]) + 1)
    (data, pieces, files, summ), want, st = large_call(records)
    assert len(files) == records == summ["files"]
    inside = holds_what_it_is_for((data, pieces, files, summ), want)
    assert inside == [b for b in BOUNDARIES if b < records]
    if len(pieces) > DECODE_GRID:
        assert int(want[1]["piece"].max()) > DECODE_GRID and int(want[1]["piece"].min()) < DECODE_GRID
    keys = sampled_keys(files, records)
    assert (keys[0], keys[-1]) == ((0, 0), ((records - 1) // 3 // 2048, (records - 1) // 3 % 2048))
    assert any(st.keys[k].open and st.keys[k].faults for k in keys)
    im = xa.ImageDecoder()
    same(im.process(data, pieces, files, files_summary(xa, summ)), want)
    same_state_sampled(im, st, keys)
    im.close()


def test_two_calls_at_scale_and_the_state_is_usable(xa):
    """51 000 records on 17 000 keys, then 17 000 records that are all continuations of the images the first call left
    open (image_mark's `continued` branch for every key), then two small ordinary calls on five of those keys."""
    copies = 17000
    first, second, third, fourth = tiling()
    calls = [isp.tile_call(first, copies), isp.tile_call(second, copies), isp.tile_call(third, 5), isp.tile_call(fourth, 5)]
    assert len(calls[0][2]) > 16384 and len(calls[1][2]) > 16384
    ist, im = isp.State(), xa.ImageDecoder()
    for i, (data, pieces, files, summ) in enumerate(calls):
        want = isp.process(ist, data, pieces, files)
        if i == 0:
            assert all(k.open for k in ist.keys.values()) and len(ist.keys) == copies
        if i == 1:
            assert not (files["flags"] & fs.BEGINS).any() and want[2]["rice"].all() and (want[2]["first_row"] == 1).all()
            assert (want[2]["lines_total"] == 3).all() and not any(k.open for k in ist.keys.values())
            assert ist.total_faults == 2 * copies and (want[2]['faults_total'] == 1).all() and want[3]["lines"] == 2 * copies
        if i == 2:
            assert (files["flags"] == fs.BEGINS).all() and want[3]["lines"] == 10
        if i == 3:
            assert (want[2]["first_row"] == 2).all() and (want[2]["lines_total"] == 4).all() and ist.images_completed == 2 * copies + 5
        same(im.process(data, pieces, files, files_summary(xa, summ)), want)
        same_state_sampled(im, ist, sampled_keys(calls[0][2], i))
    im.close()


def test_device_pointers_with_bounds_four_times_the_counts(xa):
    """The 65 537-record call through process_device: bounds equal to the counts, then four times the counts (grids
    sized by the bounds, most workgroups find nothing); the same bytes as the host-buffer call, nothing written
    beyond the true counts."""
    torch = pytest.importorskip("torch")
    (data, pieces, files, summ), want, st = large_call(65537)
    host = xa.ImageDecoder()
    got = host.process(data, pieces, files, files_summary(xa, summ))
    same(got, want)
    host.close()
    dev = torch.device("cuda:0")
    nb, nl, nf = len(want[0]), len(want[1]), len(files)
    cap_b = xa.images_max_bytes(files) + 4096
    assert cap_b > nb + 1024
    keys = sampled_keys(files)
    for times in (1, 4):
        def up(a, room):
            t = torch.full((room,), 0xA5, dtype=torch.uint8, device=dev)
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            t[:len(raw)] = torch.from_numpy(raw.copy()).to(dev)
            return t
        bp, bf = times * len(pieces), times * nf
        d_data, d_pieces, d_files = up(data, len(data) + 8), up(pieces, bp * 32), up(files, bf * 80)
        d_fsum = up(files_summary(xa, summ), 104)
        d_out, d_lines, d_ifiles, d_sum = (torch.full((n,), 0xA5, dtype=torch.uint8, device=dev) for n in (cap_b, bp * 32, bf * 48, 80))
        im = xa.ImageDecoder()
        im.process_device(d_data.data_ptr(), len(data), d_pieces.data_ptr(), bp, d_files.data_ptr(), bf, d_fsum.data_ptr(),
                          d_out.data_ptr(), cap_b, d_lines.data_ptr(), bp, d_ifiles.data_ptr(), d_sum.data_ptr())
        torch.cuda.synchronize()
        out, lines, ifiles, s = (t.cpu().numpy() for t in (d_out, d_lines, d_ifiles, d_sum))
        assert s.tobytes() == got[3].tobytes(), times
        assert np.array_equal(out[:nb], got[0]) and (out[nb:] == 0xA5).all(), times
        assert lines[:nl * 32].tobytes() == got[1].tobytes() and (lines[nl * 32:] == 0xA5).all(), times
        assert ifiles[:nf * 48].tobytes() == got[2].tobytes() and (ifiles[nf * 48:] == 0xA5).all(), times
        same_state_sampled(im, st, keys)
        im.close()
    torch.cuda.empty_cache()


def test_capacity_cut_in_a_later_tile(xa):
    """test_each_capacity's rules with the cut far from the start: inside the second tile of records, behind line 1024,
    and inside a record's lines."""
    copies = 683                                                    # 2049 records
    first, second = tiling()[:2]
    f1, f2 = isp.tile_call(first, copies), isp.tile_call(second, copies)
    ist = isp.State()
    w1 = isp.process(ist, *f1[:3])
    w2 = isp.process(ist, *f2[:3])
    nb, nl = len(w1[0]), len(w1[1])
    assert nl == 3 * copies and nb == 48 * copies
    ends = (w1[1]["offset"] + ((w1[1]["length"].astype(np.uint64) + 3) & ~np.uint64(3))).astype(np.int64)
    keys = sampled_keys(f1[2])
    for cap in ({"max_lines": 1501}, {"max_bytes": 48 * 520 + 17}, {"max_lines": 1700, "max_bytes": 48 * 400 + 30}):
        kl, cb = cap.get("max_lines", nl), cap.get("max_bytes", nb)
        # (the cut lies behind line 1024, inside a record's lines or inside a line, in a record of the second tile)
        cut_line = min(kl, int(np.searchsorted(ends, cb, side="right")))
        assert cut_line > 1024 and int(w1[1]["file"][cut_line]) > 1024
        assert cb not in ends if cut_line < kl else w1[1]["file"][cut_line - 1] == w1[1]["file"][cut_line]
        im = xa.ImageDecoder()
        with pytest.raises(xa.XritError) as ei:
            im.process(f1[0], f1[1], f1[2], files_summary(xa, f1[3]), **cap)
        assert ei.value.code == -5
        data, lines, ifiles, summary = ei.value.partial
        assert (int(summary["lines"]), int(summary["bytes"]), int(summary["images"]), int(summary["overflow"])) == \
               (nl, nb, w1[3]["images"], 1)
        for k in isp.COUNTERS:
            assert int(summary[k]) == w1[3][k], k
        assert lines.tobytes() == w1[1][:kl].tobytes() and ifiles.tobytes() == w1[2].tobytes()
        # a line's samples are written iff it fits whole, padding included
        fit = ends[:kl][ends[:kl] <= cb]
        assert len(data) == (nb if cb >= nb else int(fit.max()))
        assert np.array_equal(data, w1[0][:len(data)])
        same(im.process(f2[0], f2[1], f2[2], files_summary(xa, f2[3])), w2)          # the state advanced as if everything had fitted
        same_state_sampled(im, ist, keys)
        im.close()


def test_strides_of_the_mark_and_tile_kernels(xa):
    """524 289 records: beyond the mark kernel's grid (262 144 records) and the tile kernel's (512 tiles), nine rounds of
    the scan over the tiles.  Sixteen records a key, fourteen of them one-packet files that are no images (the
    specification's time goes with the lines; most of this test's seconds are the specification's)."""
    rng = np.random.default_rng(51)
    plain = lambda: ((0, 0), fs.lrit_file(rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), file_type=2), None, 8190)
    good = isp.image_file(rng, 10, 8, 9, 1, kinds=("uniform",))
    bad = isp.image_file(rng, 8, 16, 7, 1, kinds=("uniform",), spoil=rs.truncate)
    items = [((0, 0), good[1], good[2], 8190)] + [plain() for _ in range(13)] + [((0, 0), bad[1], bad[2], 8190), plain()]
    base = isp.run_files(fs.State(), isp.stream_of(rng, items))
    assert len(base[2]) == 16 and len(base[1]) == 18
    records = 524289
    data, pieces, files, summ = call = isp.head_of_call(isp.tile_call(base, -(-records // 16)), records)
    st = isp.State()
    want = isp.process(st, data, pieces, files)
    assert holds_what_it_is_for(call, want) == list(BOUNDARIES) and want[3]["lines"] == 65537 == 2 * want[3]["total_faults"] + 1
    im = xa.ImageDecoder()
    same(im.process(data, pieces, files, files_summary(xa, summ)), want)
    same_state_sampled(im, st, sampled_keys(files))
    im.close()


def test_long_codes_through_the_image_stage(xa):
    """decode_line_wave as this stage instantiates it, for uint8 and for uint16, on lines of uniform samples under a
    forced k: zero runs across the 64-bit windows (8 bits, J = 64, k = 0) and single codes longer than a 4096-bit chunk
    (16 bits, J = 8, k = 3).  Every line fits a packet."""
    for seed in range(53, 73):                                      # (the first seed whose 16-bit lines all fit a packet)
        rng = np.random.default_rng(seed)
        img8, d8, c8 = isp.image_file(rng, 8, 64, 192, 3, kinds=("uniform",), force=0)
        img16, d16, c16 = isp.image_file(rng, 16, 8, 16, 3, kinds=("uniform",), force=3)
        if max(np.diff(c16 + [len(d16)])) <= 8190:
            break
    stream = isp.stream_of(rng, [((1, 8), d8, c8, 8190), ((1, 16), d16, c16, 8190)])
    data, pieces, files, summ = isp.run_files(fs.State(), stream)
    st = isp.State()
    want = isp.process(st, data, pieces, files)
    assert want[3]["lines"] == 6 and not want[1]["status"].any() and int(pieces["length"].max()) <= 8190
    for ln in want[1]:
        pc = pieces[int(ln["piece"])]
        run = rs.longest_zero_run(data[int(pc["offset"]):int(pc["offset"]) + int(pc["length"])].tobytes())
        print("bits", int(ln["bits"]), "bytes", int(pc["length"]), "longest zero run", run)
        assert run > (64 if ln["bits"] == 8 else 4096)
    im = xa.ImageDecoder()
    got = im.process(data, pieces, files, files_summary(xa, summ))
    same(got, want)
    same_state(im, st)
    assert np.array_equal(np.stack(xa.ImageDecoder.rows(got[0], got[1][:3])), img8)
    assert np.array_equal(np.stack(xa.ImageDecoder.rows(got[0], got[1][3:])), img16)
    im.close()
