"""CPU tier: the specification of the Rice decoder (tests/rice_spec.py) -- the round trip through its own encoder over
randomised parameters, every option reached at both ID lengths, forced options, damaged input, the prefix a faulted line
keeps."""
import numpy as np
import pytest

import rice_spec as rs


def test_round_trip_random_parameters():
    rng = np.random.default_rng(1)
    cases = [(n, J, S) for n in (1, 8, 9, 16) for J, S in ((8, 1), (64, 5), (16, 16), (32, 33), (8, 8 * 64 + 3), (16, 16 * 130))]
    cases += [(int(rng.integers(1, 17)), int(rng.choice(rs.BLOCK_SIZES)), int(rng.integers(1, 3000))) for _ in range(150)]
    for t, (n, J, S) in enumerate(cases):
        x, line = rs.random_line(rng, n, J, S, kind=rs.KINDS[t % len(rs.KINDS)])
        y, status = rs.decode(line, n, J, S)
        assert status == 0 and np.array_equal(x, y), (n, J, S)
        y, status = rs.decode(line + b"\xa5\x00\xff", n, J, S)          # trailing bits are ignored
        assert status == 0 and np.array_equal(x, y), (n, J, S)


def test_longest_line_and_single_sample():
    rng = np.random.default_rng(2)
    for n, J, S, kind in ((8, 16, 65535, "walk3"), (16, 64, 65535, "scaled"), (8, 8, 1, "uniform"), (12, 32, 1, "uniform")):
        x, line = rs.random_line(rng, n, J, S, kind=kind)
        y, status = rs.decode(line, n, J, S)
        assert status == 0 and np.array_equal(x, y)


def option_stats(n_values, seed):
    rng = np.random.default_rng(seed)
    stats = {}
    for t in range(120):
        n = int(n_values[t % len(n_values)])
        J = int(rs.BLOCK_SIZES[(t // 2) % 4])
        S = int(rng.integers(200, 6000))
        x, line = rs.random_line(rng, n, J, S, kind=rs.KINDS[t % len(rs.KINDS)], stats=stats)
        y, status = rs.decode(line, n, J, S)
        assert status == 0 and np.array_equal(x, y)
    return stats


def test_generators_reach_every_option_at_both_id_lengths():
    short, long_ = option_stats((7, 8), 3), option_stats((12, 16), 4)
    for k in [rs.ZERO, "rest", rs.SE, rs.RAW] + list(range(6)):
        assert short.get(k, 0) > 0, ("L = 3", k, short)
    for k in [rs.ZERO, "rest", rs.SE, rs.RAW] + list(range(14)):
        assert long_.get(k, 0) > 0, ("L = 4", k, long_)
    assert set(short) <= {rs.ZERO, "rest", rs.SE, rs.RAW, *range(6)}


@pytest.mark.parametrize("n", [1, 5, 8, 9, 16])
def test_forced_options_decode(n):
    rng = np.random.default_rng(5 + n)
    kmax = (1 << rs.id_bits(n)) - 3
    for J in rs.BLOCK_SIZES:
        S = int(rng.integers(1, 700))
        x = rs.samples(rng, "sparse", n, J, S)
        for force in list(range(kmax + 1)) + [rs.SE, rs.RAW, "nozero"]:
            stats = {}
            line = rs.encode(x, n, J, force=force, stats=stats)
            if force != "nozero":
                assert set(stats) == {force}
            assert rs.ZERO not in stats
            y, status = rs.decode(line, n, J, S)
            assert status == 0 and np.array_equal(x, y), (n, J, S, force)
        u = rs.samples(rng, "uniform", n, J, S)                     # raw on noise, forced
        y, status = rs.decode(rs.encode(u, n, J, force=rs.RAW), n, J, S)
        assert status == 0 and np.array_equal(u, y)


def test_zero_block_codes_by_hand():
    # n = 8, J = 8: ID 000, zero-block flag 0, reference 0x55, then FS codes; every sample equals the reference
    def line(bits):
        bits += "0" * (-len(bits) % 8)
        return int(bits, 2).to_bytes(len(bits) // 8, "big")
    head = "000" + "0" + "01010101"
    for v, blocks in ((0, 1), (3, 4), (5, 5), (9, 9)):
        y, status = rs.decode(line(head + "0" * v + "1"), 8, 8, 8 * blocks)
        assert status == 0 and (y == 0x55).all()
        y, status = rs.decode(line(head + "0" * v + "1"), 8, 8, 8 * blocks - 8 if blocks > 1 else 8)
        assert status == (1 if blocks > 1 else 0)                   # a run past the line's end
        if blocks > 1:
            assert not y.any()
    # the rest-of-segment code: to block 64, or to the line's end where that comes first
    for blocks in (5, 64, 70):
        rest = head + "00001"
        if blocks > 64:
            rest += "000" + "0" + "0" * (blocks - 64 - 1 if blocks - 64 <= 4 else blocks - 64) + "1"
        y, status = rs.decode(line(rest), 8, 8, 8 * blocks)
        assert status == 0 and (y == 0x55).all() and len(y) == 8 * blocks
    # a second extension in block 0 whose stand-in is not zero: gamma = 1 is the pair (1, 0)
    y, status = rs.decode(line("000" + "1" + "01010101" + "01" + "1" * 3), 8, 8, 8)
    assert status == 1 and not y.any()
    y, status = rs.decode(line("000" + "1" + "01010101" + "001" + "1" * 3), 8, 8, 8)     # gamma = 2: the pair (0, 1)
    assert status == 0 and list(y) == [0x55, 0x54] + [0x54] * 6


def test_damaged_input_returns_a_status_and_keeps_whole_blocks():
    rng = np.random.default_rng(6)
    faults = clean = 0
    for t in range(300):
        n = int(rng.choice([1, 2, 7, 8, 9, 10, 12, 16]))
        J = int(rng.choice(rs.BLOCK_SIZES))
        S = int(rng.integers(1, 2500))
        x, line = rs.random_line(rng, n, J, S, kind=rs.KINDS[t % len(rs.KINDS)])
        cut = rs.truncate(rng, line)
        y, status = rs.decode(cut, n, J, S)
        assert status in (0, 1) and len(y) == S
        if status == 0:
            clean += 1
            assert np.array_equal(y, x)
        else:
            faults += 1
            # the prefix of whole blocks, then zeros: the blocks kept are those of the whole line
            diff = np.flatnonzero(y != x)
            keep = (int(diff[0]) if len(diff) else S) // J * J
            assert np.array_equal(y[:keep], x[:keep]) and not y[keep:].any()
        for junk in (rs.flip(rng, line, 3), rng.integers(0, 256, int(rng.integers(0, 400)), dtype=np.uint8).tobytes(), b""):
            y, status = rs.decode(junk, n, J, S)
            assert status in (0, 1) and len(y) == S and y.min() >= 0 and y.max() < (1 << n)
    assert faults > 100                                             # (a cut always takes a needed bit: clean stays 0)
    assert rs.decode(b"", 8, 8, 10)[1] == 1


def test_batch_types_and_bad_parameters():
    rng = np.random.default_rng(7)
    lines = [rs.random_line(rng, 8, 16, 100)[1] for _ in range(5)]
    out, status = rs.decode_batch(lines, 8, 16, 100)
    assert out.dtype == np.uint8 and out.shape == (5, 100) and not status.any()
    assert rs.decode_batch([b""], 9, 8, 3)[0].dtype == np.uint16
    data, desc = rs.pack(lines)
    assert desc.itemsize == 16 and int(desc["offset"][-1] + desc["length"][-1]) == len(data)
    for bad in ((0, 8, 1), (17, 8, 1), (8, 12, 1), (8, 8, 0), (8, 8, 65536)):
        with pytest.raises(ValueError):
            rs.decode(b"\x00", *bad)


def test_forced_low_k_lines_hold_the_long_codes_they_are_for():
    """Uniform samples under a forced low k: valid lines with zero runs longer than the wave form's 64-bit windows, with
    a block's codes longer than its 4096-bit chunks, and with single codes longer than one and than two chunks."""
    for case in rs.FORCED_LOW_K:
        n, J, S, k, run = case
        x, line = rs.forced_low_k_line(case)
        stats = {}
        assert rs.encode(x, n, J, force=k, stats=stats) == line and set(stats) == {k}
        y, status = rs.decode(line, n, J, S)
        assert status == 0 and np.array_equal(x, y), case
        assert rs.longest_zero_run(line) > run, case
        assert 8 * len(line) > 4096 * (S // J), case               # every case: more than a chunk of codes per block on average
    assert rs.longest_zero_run(b"\x00\x80\x00\x01") == 22 and rs.longest_zero_run(bytes(3)) == 0


def test_hand_made_lines_decode_to_what_they_were_built_from():
    edges = rs.chunk_edge_lines()
    assert sorted({at for _, _, at in edges}) == list(rs.CHUNK_EDGES) and len(edges) == 12
    for line, x, at in edges:
        # (the codes begin behind the 4-bit ID and the 16-bit reference)
        assert np.unpackbits(np.frombuffer(line, np.uint8))[20 + at] == 1 and rs.longest_zero_run(line) >= at - 4
        y, status = rs.decode(line, 16, 8, 8)
        assert status == 0 and np.array_equal(x, y), at
        assert x.min() >= 0 and x.max() <= 65535 and len(set(x.tolist())) > 4
    (n, J, line, x, status), at_limit, beyond = rs.limit_lines()
    assert len(line) == 4 and rs.decode(line, n, J, 8)[1] == 0 and np.array_equal(rs.decode(line, n, J, 8)[0], x)
    assert rs.decode(line[:3], n, J, 8)[1] == 1                     # (its last bit is needed)
    for n, J, line, x, status in (at_limit, beyond):
        y, got = rs.decode(line, n, J, 8)
        assert got == status and np.array_equal(x, y)
    assert at_limit[4] == 0 and at_limit[3].any() and beyond[4] == 1 and not beyond[3].any()
    # the mapper's inverse by search is the decoder's on a line the encoder wrote
    rng = np.random.default_rng(8)
    x = rs.samples(rng, "uniform", 12, 8, 8)
    assert np.array_equal(rs.samples_of(x[0], rs.map_residuals(x, 12)[1:], 12), x)


def test_second_extension_with_large_codes():
    lines = rs.se_long_lines()
    assert len(lines) == 2 * len(rs.SE_BETAS) and max(len(ln) for ln, _, _ in lines) == 1048324 < rs.MAX_LINE
    assert sum(8 * g + 1 > 1 << 24 for _, _, g in lines) == 6      # where a float32 root of 8 g + 1 is only a start
    for (line, x, g), beta in zip(lines, np.repeat(rs.SE_BETAS, 2)):
        assert rs.longest_zero_run(line) == max(g, 6) and g - beta * (beta + 1) // 2 in (0, beta)
        y, status = rs.decode(line, 16, 8, 8)
        assert status == 0 and np.array_equal(x, y), g
