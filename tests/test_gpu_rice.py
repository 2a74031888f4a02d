"""GPU tier: the Rice decoder (xrit_rice_*, RiceDecoder) against the specification of tests/rice_spec.py -- batches that
mix every option at both ID lengths, on both kernel forms (one lane per line, one wave per line), forced options, the shortest and longest lines, a stated share of truncated and
damaged lines (status and kept prefix), descriptors outside the bytes, the stride form fed with file-piece and packet
descriptor arrays, the device-pointer path, and decode_file_lines on the file assembler's output; valid lines with long
codes (uniform samples under a forced low k: zero runs across 64-bit windows, 4096-bit chunks and many chunks; codes
that end on a chunk's edge and on the line's last bit; values at the limit; second-extension codes up to 2^23) and the
line limit of 2^20 bytes; lines encoded by libaec and libsz, not by rice_spec (tests/golden/rice_libaec_lines.npz),
against the samples they were made from, and damaged copies of them against the specification.  Every comparison is
exact."""
import functools

import numpy as np
import pytest

import file_spec as fs
import rice_spec as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


@pytest.fixture(params=["lane", "wave"], autouse=True)
def form(request, xa):
    """Every test of this file runs on both kernel forms."""
    xa.rice_form(request.param)
    yield request.param
    xa.rice_form("default")


def check(xa, lines, n, J, S, desc_dtype=None):
    data, desc = rs.pack(lines)
    if desc_dtype is not None:
        d = np.zeros(len(desc), desc_dtype)
        d["offset"], d["length"] = desc["offset"], desc["length"]
        for f in d.dtype.names:                                 # whatever else the record holds is not looked at
            if f not in ("offset", "length") and d.dtype[f].shape == ():
                d[f] = 0xA5
        desc = d
    out, status = xa.RiceDecoder(n, J, S).decode(data, desc)
    want, wstatus = rs.decode_batch(lines, n, J, S)
    assert out.dtype == want.dtype and out.shape == want.shape
    assert np.array_equal(status, wstatus)
    assert np.array_equal(out, want)
    return wstatus


@pytest.mark.parametrize("n,J,S", [(8, 16, 2000), (7, 8, 333), (8, 64, 64 * 70 + 1), (1, 32, 900), (12, 32, 1500), (16, 8, 8 * 130),
                                   (9, 64, 63), (10, 16, 1)])
def test_batches_mixing_every_option(xa, n, J, S):
    rng = np.random.default_rng(n * 100 + J)
    stats = {}
    lines = [rs.random_line(rng, n, J, S, kind=rs.KINDS[i % len(rs.KINDS)], stats=stats)[1] for i in range(200)]
    kmax = (1 << rs.id_bits(n)) - 3
    for force in list(range(kmax + 1)) + [rs.SE, rs.RAW, "nozero"]:
        lines.append(rs.encode(rs.samples(rng, "sparse", n, J, S), n, J, force=force))
    status = check(xa, lines, n, J, S)
    assert not status.any()
    if S >= 900 and n >= 7:
        assert {rs.ZERO, rs.SE, rs.RAW, 0, 1, 2} <= set(stats), stats


def test_every_option_id_at_both_lengths_in_one_batch_each(xa):
    for n, seed in ((8, 1), (16, 2)):
        rng = np.random.default_rng(seed)
        stats, lines = {}, []
        for i in range(150):
            lines.append(rs.random_line(rng, n, 16, 1600, kind=rs.KINDS[i % len(rs.KINDS)], stats=stats)[1])
        kmax = (1 << rs.id_bits(n)) - 3
        assert set(stats) >= {rs.ZERO, "rest", rs.SE, rs.RAW, *range(kmax + 1)}, stats
        assert not check(xa, lines, n, 16, 1600).any()


def test_shortest_and_longest_lines(xa):
    rng = np.random.default_rng(3)
    # S = 1 and S = 65535, lines of 0 and of 65533 bytes
    for n, J in ((8, 8), (16, 64)):
        x1, l1 = rs.random_line(rng, n, J, 1, kind="uniform")
        assert check(xa, [l1, b"", l1[:1], rng.integers(0, 256, 65533, dtype=np.uint8).tobytes()], n, J, 1)[1] == 1
    for n, J, kind in ((8, 16, "walk3"), (16, 8, "scaled"), (12, 64, "uniform")):
        x, ln = rs.random_line(rng, n, J, 65535, kind=kind)
        junk = rng.integers(0, 256, 65533, dtype=np.uint8).tobytes()
        zeros = bytes(65533)
        padded = ln + rng.integers(0, 256, 65533 - len(ln), dtype=np.uint8).tobytes() if len(ln) < 65533 else ln
        status = check(xa, [ln, b"", junk, zeros, padded, ln[:len(ln) // 2]], n, J, 65535)
        assert list(status[[0, 1, 4, 5]]) == [0, 1, 0, 1]


@pytest.mark.parametrize("n,J,S", [(8, 16, 1200), (10, 32, 700), (16, 64, 3000), (4, 8, 100)])
def test_a_quarter_truncated_a_tenth_damaged(xa, n, J, S):
    rng = np.random.default_rng(S)
    lines, cut = [], 0
    for i in range(400):
        ln = rs.random_line(rng, n, J, S)[1]
        u = rng.random()
        if u < 0.25:
            ln = rs.truncate(rng, ln)
            cut += 1
        elif u < 0.35:
            ln = rs.flip(rng, ln, int(rng.integers(1, 4)))
        elif u < 0.40:
            ln = rng.integers(0, 256, int(rng.integers(0, 2 * len(ln) + 2)), dtype=np.uint8).tobytes()
        lines.append(ln)
    status = check(xa, lines, n, J, S)
    assert cut > 60 and int(status.sum()) >= cut                # every cut line faults; the kept prefixes were compared


def test_stride_forms_and_descriptors_outside_the_bytes(xa):
    rng = np.random.default_rng(5)
    lines = [rs.random_line(rng, 8, 16, 500)[1] for _ in range(70)]
    for dt in (xa.FILE_PIECE_DTYPE, xa.PACKET_DTYPE, fs.RECORD_DTYPE):          # 32, 32 and 80 bytes apart
        assert not check(xa, lines, 8, 16, 500, desc_dtype=dt).any()
    data, desc = rs.pack(lines)
    want, _ = rs.decode_batch(lines, 8, 16, 500)
    bad = desc.copy()
    bad["offset"][3] = len(data) - 2                            # runs past the end
    bad["offset"][7] = 1 << 40
    bad["length"][9] = 0xFFFFFFFF
    out, status = xa.RiceDecoder(8, 16, 500).decode(data, bad)
    assert list(np.flatnonzero(status)) == [3, 7, 9] and (status[[3, 7, 9]] == 2).all()
    assert not out[[3, 7, 9]].any()
    keep = np.ones(70, bool)
    keep[[3, 7, 9]] = False
    assert np.array_equal(out[keep], want[keep])
    out, status = xa.RiceDecoder(8, 16, 500).decode(data, desc[:0])
    assert out.shape == (0, 500) and status.shape == (0,)
    for args in ((0, 16, 500), (8, 24, 500), (8, 16, 0), (17, 16, 500), (8, 16, 65536)):
        with pytest.raises(xa.XritError) as ei:
            xa.RiceDecoder(*args)
        assert ei.value.code == -1


def test_device_pointers_on_a_side_stream(xa):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(6)
    n, J, S = 12, 32, 777
    lines = [rs.truncate(rng, rs.random_line(rng, n, J, S)[1]) if i % 5 == 0 else rs.random_line(rng, n, J, S)[1] for i in range(300)]
    data, desc = rs.pack(lines)
    dev = torch.device("cuda:0")
    d_data = torch.from_numpy(data.copy()).to(dev)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_out = torch.full((300 * S * 2,), 0xEE, dtype=torch.uint8, device=dev)
    d_status = torch.full((300,), 0xEE, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        xa.RiceDecoder(n, J, S).decode_device(d_data.data_ptr(), len(data), d_desc.data_ptr(), 16, 300, d_out.data_ptr(),
                                              d_status.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    want, wstatus = rs.decode_batch(lines, n, J, S)
    assert np.array_equal(d_status.cpu().numpy(), wstatus) and wstatus.sum() == 60
    assert np.array_equal(d_out.cpu().numpy().view(np.uint16).reshape(300, S), want)


def image_file(rng, n, J, columns, lines, kind="walk3"):
    """(file bytes, image (lines, columns), cuts): a rice-coded image file by the link rule -- the headers, then one
    coded line per piece."""
    img = np.stack([rs.samples(rng, kind, n, J, columns) for _ in range(lines)])
    coded = [rs.encode(row, n, J) for row in img]
    head = fs.lrit_file(b"", image=(n, columns, lines, 1), rice=(49, J, 1), extra=[(2, b"annotation")],
                        declared_data_bits=8 * sum(len(c) for c in coded))
    cuts = list(np.cumsum([len(head)] + [len(c) for c in coded])[:-1])
    return head + b"".join(coded), img, [int(c) for c in cuts]


def test_decode_file_lines_on_the_assembler_s_output(xa):
    rng = np.random.default_rng(7)
    stream, images = [], {}
    for key, (n, J, cols, rows) in (((2, 40), (8, 16, 300, 20)), ((2, 41), (10, 64, 1000, 7)), ((9, 40), (8, 8, 5, 3))):
        f, img, cuts = image_file(rng, n, J, cols, rows)
        pk, _ = fs.packetise(f, key[1], 16380, 3, cuts=cuts)
        assert len(pk) == rows + 1
        stream += [(key[0], p) for p in pk]
        images[key] = (f, img)
    plain, _ = fs.packetise(fs.lrit_file(bytes(500), image=(8, 10, 50, 0)), 42, 0, 4, max_user=100)    # not compressed
    stream += [(2, p) for p in plain]
    args = fs.stage_input(stream)
    fa = xa.FileAssembler()
    data, pieces, files, summary = fa.process(*args)
    want = fs.process(fs.State(), *args)
    assert files.tobytes() == want[2].tobytes() and np.array_equal(data, want[0])
    assert len(files) == 4 and (files["flags"] == fs.BEGINS | fs.ENDS | fs.LENGTH_MATCH).all()
    seen = 0
    for r in files:
        key = (int(r["vcid"]), int(r["apid"]))
        res = xa.decode_file_lines(r, pieces, data)
        if key not in images:
            assert res is None
            continue
        f, img = images[key]
        assert data[int(r["offset"]):int(r["offset"]) + int(r["length"])].tobytes() == f
        out, status = res
        assert not status.any() and np.array_equal(out, img) and out.dtype == (np.uint8 if r["bits_per_pixel"] <= 8 else np.uint16)
        seen += 1
    assert seen == 3
    fa.close()


# ---- long codes: valid lines that the generators' cheapest options never produce --------------------------------------
@pytest.mark.parametrize("case", rs.FORCED_LOW_K, ids=lambda c: "n%d-J%d-S%d-k%d" % c[:4])
def test_forced_low_k_on_uniform_samples(xa, case):
    """Codes across the wave form's 64-bit windows, a block's codes across its 4096-bit chunks, single codes across many
    chunks with chunks that hold no one (the lane form: zero runs longer than its 64-bit buffer)."""
    n, J, S, k, run = case
    x, line = rs.forced_low_k_line(case)
    y, status = rs.decode(line, n, J, S)
    zeros = rs.longest_zero_run(line)
    print("bytes", len(line), "longest zero run", zeros)
    assert status == 0 and np.array_equal(x, y) and zeros > run     # from the specification, before the device is compared
    # the line, the line with bytes behind it (ignored) and the line without its last byte (a fault: whole blocks kept)
    status = check(xa, [line, line + b"\xa5\xff\x01", line[:-1]], n, J, S)
    assert list(status[:2]) == [0, 0]


def test_codes_that_end_on_chunk_edges_and_values_at_the_limit(xa):
    edges = rs.chunk_edge_lines()
    for line, x, at in edges:
        y, status = rs.decode(line, 16, 8, 8)
        assert status == 0 and np.array_equal(x, y) and rs.longest_zero_run(line) >= at - 4, at
    assert not check(xa, [line for line, _, _ in edges], 16, 8, 8).any()
    (n, J, line, x, status), at_limit, beyond = rs.limit_lines()
    # a line whose last code ends on its last bit: alone, and with a line of ones behind it (reading on would go unnoticed); without its last bit
    assert 8 * len(line) == 32 and rs.decode(line, n, J, 8)[1] == 0 and rs.decode(line[:3] + bytes([line[3] & 0xFE]), n, J, 8)[1] == 1
    assert list(check(xa, [line, b"\xff" * 8, line, line[:3] + bytes([line[3] & 0xFE]), line], n, J, 8)[[0, 2, 3, 4]]) == [0, 0, 1, 0]
    assert list(check(xa, [at_limit[2], beyond[2], at_limit[2]], 12, 8, 8)) == [0, 1, 0]
    out, _ = xa.RiceDecoder(12, 8, 8).decode(*rs.pack([beyond[2]]))
    assert not out.any()


def test_second_extension_with_large_codes(xa):
    """beta up to 4094: from 2896 on 8 g + 1 is beyond 2^24 and the float root is only a guess.  (With a correctly rounded
    float32 square root the guess is right for every g below 2^23 -- checked exhaustively on the host --, so the two
    fix-up loops behind it never act and no line can tell whether they are there.)  One batch, so that the megabyte
    lines are decoded once per form."""
    lines = rs.se_long_lines()
    for line, x, g in lines:
        y, status = rs.decode(line, 16, 8, 8)
        assert status == 0 and np.array_equal(x, y) and rs.longest_zero_run(line) == max(g, 6), g
    assert max(g for _, _, g in lines) > (1 << 23) - 4096 and max(len(ln) for ln, _, _ in lines) < rs.MAX_LINE
    assert not check(xa, [line for line, _, _ in lines], 16, 8, 8).any()
    out, _ = xa.RiceDecoder(16, 8, 8).decode(*rs.pack([line for line, _, _ in lines]))
    assert np.array_equal(out, np.stack([x for _, x, _ in lines]))


# ---- lines that our own encoder did not make -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def libaec_groups():
    """tests/golden/rice_libaec_lines.npz (shared, never changed): lines encoded by libaec 1.0.4 and by its libsz under
    mask 49, with the samples they were made from.  Two fifths of them are other bytes than rs.encode's."""
    return rs.libaec_groups()


def test_lines_encoded_by_libaec(xa):
    """libaec -> kernel, with neither rs.encode nor rs.decode in the chain: one batch per group of the fixture against
    the fixture's samples.  Both ID lengths, n = 1 and 4, every J, lines whose last block libaec padded, S = 1, lines of
    more than 64 blocks, the line of 4096 blocks."""
    groups = libaec_groups()
    assert len(groups) >= 11 and max(-(-S // J) for _, J, S, *_ in groups) == 4096
    for n, J, S, source, lines, samples in groups:
        out, status = xa.RiceDecoder(n, J, S).decode(*rs.pack(lines))
        assert out.dtype == (np.uint8 if n <= 8 else np.uint16) and out.shape == samples.shape, (n, J, S, source)
        assert not status.any(), (n, J, S, source, np.flatnonzero(status))
        assert np.array_equal(out, samples), (n, J, S, source, np.flatnonzero((out != samples).any(1)))


def test_libaec_lines_truncated_and_damaged(xa):
    """Each group's lines in one batch with a truncated copy and a copy with one to three flipped bits of each: statuses
    and kept prefixes against the specification."""
    rng = np.random.default_rng(8)
    faults = 0
    for n, J, S, source, lines, samples in libaec_groups():
        batch = list(lines) + [rs.truncate(rng, ln) for ln in lines] + [rs.flip(rng, ln, int(rng.integers(1, 4))) for ln in lines]
        status = check(xa, batch, n, J, S)
        assert not status[:len(lines)].any() and status[len(lines):2 * len(lines)].all(), (n, J, S)     # every cut line faults
        faults += int(status.sum())
    assert faults > 200


def test_the_line_limit(xa):
    """A descriptor of exactly 2^20 bytes is decoded (here: a valid line that needs 1 048 324 of them, and the same bytes
    from one byte on, whatever the specification says to those); one byte more is refused, status 2 and zeros."""
    line, x, g = rs.se_long_lines()[-1]
    data = np.frombuffer(line + b"\xa5" * (rs.MAX_LINE + 1 - len(line)), np.uint8)
    assert len(data) == rs.MAX_LINE + 1
    desc = rs.pack([b""] * 3)[1]
    desc["offset"], desc["length"] = [0, 0, 1], [rs.MAX_LINE, rs.MAX_LINE + 1, rs.MAX_LINE]
    want = [rs.decode(data[o:o + rs.MAX_LINE].tobytes(), 16, 8, 8) for o in (0, 1)]
    assert want[0][1] == 0 and np.array_equal(want[0][0], x)
    out, status = xa.RiceDecoder(16, 8, 8).decode(data, desc)
    assert list(status) == [0, 2, want[1][1]]
    assert np.array_equal(out[0], x) and not out[1].any() and np.array_equal(out[2], want[1][0])
