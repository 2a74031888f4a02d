"""CPU tier: the Rice specification (tests/rice_spec.py) held against libaec 1.0.4 and its SZIP-compatible libsz
(tests/aec_ref.py) -- libaec's lines through rs.decode, rs.encode's lines under every forced
option through libaec's decoder, zero-block runs at the segment ends, the hand-made long-code lines, damaged lines
wherever both sides accept them, single scanlines of libsz under the option masks, and the fixture of libaec's lines
that the GPU tier decodes (tests/golden/rice_libaec_lines.npz).  The tests of the fixture alone always run; the others
need the library and skip without it.  Every comparison is exact."""
import functools
import os
import sys

import numpy as np
import pytest

import aec_ref
import rice_spec as rs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_rice_golden as mg  # noqa: E402

GRID_N = (1, 2, 3, 4, 5, 7, 8, 9, 10, 12, 15, 16)
MASKS = (49, 48, 53, 41, 177)     # GOES's ALLOW_K13 | MSB | NN; without K13; with EC; LSB samples; with RAW


@pytest.fixture(scope="module")
def aec():
    if not aec_ref.available():
        pytest.skip("libaec and libsz (libaec 1.0.4: libaec.so, libsz.so) were not found")
    return aec_ref


def grid_sizes(J):
    return (J, 3 * J, 5 * J - 3, 64 * J, 70 * J, 131 * J + 1, 1)


@functools.lru_cache(maxsize=None)
def grid(n):
    """The samples of one n: every J, seven S, the five generators -> [(J, S, x)]; shared, never changed."""
    rng = np.random.default_rng(1000 + n)
    return [(J, S, rs.samples(rng, kind, n, J, S)) for J in rs.BLOCK_SIZES for S in grid_sizes(J) for kind in rs.KINDS]


# ---- libaec's encoder, our decoder -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", GRID_N)
def test_libaec_lines_through_the_specification(aec, n):
    other = 0
    for J, S, x in grid(n):
        line = aec.encode(x, n, J)
        y, status = rs.decode(line, n, J, S)
        assert status == 0 and np.array_equal(x, y), (n, J, S)
        other += line != rs.encode(x, n, J)
    print("n", n, "lines", len(grid(n)), "other bytes than rs.encode", other)


def test_the_line_of_4096_blocks_through_the_specification(aec):
    x = mg.line_samples(np.random.default_rng(5), 8, 8, aec_ref.MAX_RSI * 8, 0)
    line = aec.encode(x, 8, 8)
    stats = {}
    y, status = rs.decode(line, 8, 8, len(x), stats=stats)
    assert status == 0 and np.array_equal(x, y) and {rs.ZERO, "rest", rs.SE, rs.RAW, 0, 1, 2, 3, 4, 5} <= set(stats), stats
    with pytest.raises(ValueError):
        aec.encode(np.zeros(aec_ref.MAX_RSI * 8 + 1, np.int64), 8, 8)


# ---- our encoder, libaec's decoder -------------------------------------------------------------------------------------
def through_libaec(aec, line, n, J, x):
    rc, y, written = aec.decode(line, n, J, len(x))
    assert rc == aec_ref.AEC_OK and written == len(x) and np.array_equal(x, y), (n, J, len(x), rc, written)


@pytest.mark.parametrize("n", GRID_N)
def test_specification_lines_through_libaec(aec, n):
    for J, S, x in grid(n):
        through_libaec(aec, rs.encode(x, n, J), n, J, x)


@pytest.mark.parametrize("n", [8, 16])
def test_every_forced_option_through_libaec(aec, n):
    """The encoder that every GPU test of the Rice decoder, the image stage and the canvas is built on, under each of its
    `force` values at both ID lengths.  Small residuals for every option; jumps (the constant line's rare zeros) for all
    but the second extension, whose codes libaec refuses above 90; uniform samples too where the
    longest code stays below 1024 bits."""
    rng = np.random.default_rng(n)
    kmax = (1 << rs.id_bits(n)) - 3
    xmax = (1 << n) - 1
    for force in [None, "nozero", rs.SE, rs.RAW] + list(range(kmax + 1)):
        kinds = ["sparse", "walk3"] + ([] if force == rs.SE else ["constant"])
        if force == rs.RAW or (isinstance(force, int) and xmax >> force <= 1024):
            kinds += ["uniform", "scaled"]
        met = {}
        for J in rs.BLOCK_SIZES:
            for S in (3 * J, 5 * J - 3, 70 * J, 1):
                for kind in kinds:
                    x = rs.samples(rng, kind, n, J, S)
                    through_libaec(aec, rs.encode(x, n, J, force=force, stats=met), n, J, x)
        if force not in (None, "nozero"):
            assert set(met) == {force}, (force, met)


def zero_run_line(rng, n, J, B, first, run):
    """B blocks of noise in which blocks first .. first + run - 1 repeat the sample in front of them."""
    x = rng.integers(0, 1 << n, B * J)
    x[first * J:(first + run) * J] = x[first * J - 1] if first else x[0]
    return x.astype(np.int64)


def test_zero_block_runs_at_the_segment_ends(aec):
    """Runs of 1, 2, 3, 4, 5 and 64 all-zero blocks that end on a 64-block segment end and that lie across one, in both
    directions: our codes through libaec, libaec's through the specification.  Both encoders must have used the
    rest-of-segment code and the plain code of a long run."""
    rng = np.random.default_rng(64)
    ours, theirs = {}, {}
    for n, J in ((8, 8), (10, 16)):
        for run in (1, 2, 3, 4, 5, 64):
            # in front of the end of the first or second segment; across the first end; at the start of the line
            for first in {rs.SEGMENT * (2 if run == 64 else 1) - run, rs.SEGMENT - (run + 1) // 2, 0}:
                x = zero_run_line(rng, n, J, 140, first, run)
                line = rs.encode(x, n, J)
                through_libaec(aec, line, n, J, x)
                rs.decode(line, n, J, len(x), stats=ours)
                y, status = rs.decode(aec.encode(x, n, J), n, J, len(x), stats=theirs)
                assert status == 0 and np.array_equal(x, y), (n, J, run, first)
    print("rs.encode", ours, "libaec", theirs)
    assert ours["rest"] >= 4 and ours["long"] >= 4 and theirs["rest"] >= 4 and theirs["long"] >= 4


# ---- the hand-made lines of rice_spec ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rs.FORCED_LOW_K, ids=lambda c: "n%d-J%d-S%d-k%d" % c[:4])
def test_forced_low_k_lines_through_libaec(aec, case):
    n, J, S, k, _ = case
    x, line = rs.forced_low_k_line(case)
    through_libaec(aec, line, n, J, x)


def test_chunk_edge_and_limit_lines_through_libaec(aec):
    for line, x, at in rs.chunk_edge_lines():
        through_libaec(aec, line, 16, 8, x)
    seen = 0
    for n, J, line, x, status in rs.limit_lines():
        if status == 0:
            through_libaec(aec, line, n, J, x)
            seen += 1
    assert seen == 2


SE_LIMIT = 90                     # libaec's: the code of the pairs (12, 0) .. (0, 12); beyond it AEC_DATA_ERROR


def test_second_extension_lines_through_libaec(aec):
    """Every second-extension code that libaec takes, 0 .. 90: the pairing and its order.  Of se_long_lines (the 1 MiB
    line included) libaec decodes those of beta 1 and 2 and refuses every longer code with AEC_DATA_ERROR, slack or
    not: its decoder looks the pair up in a table of 91 entries.  The specification and the device decode them; that
    they are valid is our reading of the recommendation alone."""
    for g in range(SE_LIMIT + 1):
        beta = (int(np.sqrt(8 * g + 1)) - 1) // 2
        c = g - beta * (beta + 1) // 2
        through_libaec(aec, rs.se_line(16, 8, 12345, [0, g, 3, 0]), 16, 8, rs.samples_of(12345, [0, beta - c, c, 2, 0, 0, 0], 16))
    lines = rs.se_long_lines()
    assert len(lines) == 2 * len(rs.SE_BETAS) and max(len(ln) for ln, _, _ in lines) > 1000000
    taken = 0
    for line, x, g in lines:
        if g <= SE_LIMIT:
            through_libaec(aec, line, 16, 8, x)
            taken += 1
        else:
            assert aec.decode(line, 16, 8, 8)[0] == aec_ref.AEC_DATA_ERROR, g
    assert taken == 4


# ---- damaged lines -------------------------------------------------------------------------------------------------------
DAMAGED = 2000
DAMAGED_SEED = 7


def damaged_lines(aec):
    """2000 lines: even ones from rs.encode, odd ones from libaec; every third cut at a random byte, the others with one to
    three bits flipped -> [(n, J, S, bytes)]."""
    rng = np.random.default_rng(DAMAGED_SEED)
    out = []
    for i in range(DAMAGED):
        n, J = int(rng.choice([1, 4, 8, 10, 16])), int(rng.choice(rs.BLOCK_SIZES))
        S = int(rng.choice([J, 5 * J - 3, 9 * J, 70 * J + 1]))
        x = rs.samples(rng, rs.KINDS[int(rng.integers(0, len(rs.KINDS)))], n, J, S)
        line = rs.encode(x, n, J) if i % 2 == 0 else aec.encode(x, n, J)
        line = rs.truncate(rng, line) if i % 3 == 0 else rs.flip(rng, line, int(rng.integers(1, 4)))
        out.append((n, J, S, line))
    return out


def test_damaged_lines_that_both_accept_are_equal(aec):
    """Wherever the specification reports status 0 and libaec returns AEC_OK having written all S samples, the samples are
    equal.  Measured with libaec 1.0.4 and the slack of aec_ref.decode: 617 of the 2000 lines (30.9 %) reach the
    comparison (at least a tenth must, from the reference alone); 144 are accepted by libaec alone and none by the
    specification alone -- counted and printed, not asserted on: libaec does not enforce the value range as section 16
    does, and behind a cut line it reads the slack."""
    compared = only_spec = only_libaec = 0
    for n, J, S, line in damaged_lines(aec):
        y, status = rs.decode(line, n, J, S)
        rc, z, written = aec.decode(line, n, J, S)
        theirs = rc == aec_ref.AEC_OK and written == S
        if status == 0 and theirs:
            compared += 1
            assert np.array_equal(y, z), (n, J, S, line.hex())
        only_spec += status == 0 and not theirs
        only_libaec += status != 0 and theirs
    print("compared", compared, "accepted by the specification alone", only_spec, "by libaec alone", only_libaec, "of", DAMAGED)
    assert 10 * compared >= DAMAGED


# ---- libsz and the option mask --------------------------------------------------------------------------------------------
def sz_cases():
    rng = np.random.default_rng(49)
    for n in (1, 4, 8, 10, 16):
        for J in (8, 16, 32):
            for S in (5 * J, 5 * J + 3):
                for kind in ("uniform", "walk3", "scaled"):
                    yield n, J, S, kind, rs.samples(rng, kind, n, J, S)


@pytest.mark.parametrize("mask", MASKS)
def test_libsz_scanlines_through_the_specification(aec, mask):
    for n, J, S, kind, x in sz_cases():
        line = aec.sz_encode(x, n, J, mask)
        y, status = rs.decode(line, n, J, S)
        assert status == 0 and np.array_equal(x, y), (mask, n, J, S, kind)
        if mask == aec_ref.SZ_GOES and S % J == 0:
            assert line == aec.encode(x, n, J), (n, J, S, kind)


def test_a_mask_without_the_nn_bit_is_another_stream(aec):
    """Mask 17, ALLOW_K13 | MSB: no predictor.  The image stage reports rice_flags and does not act on it, so such a file
    would be decoded as if mask 49 had made it: here, for uniform samples, to other samples (or a fault)."""
    wrong = 0
    for n, J, S, kind, x in sz_cases():
        line = aec.sz_encode(x, n, J, 17)
        assert line != aec.sz_encode(x, n, J, aec_ref.SZ_GOES), (n, J, S, kind)
        if kind == "uniform":
            y, status = rs.decode(line, n, J, S)
            assert status != 0 or not np.array_equal(x, y), (n, J, S)
            wrong += status == 0
    print("uniform lines decoded to other samples with status 0:", wrong)


# ---- the fixture --------------------------------------------------------------------------------------------------------
def test_fixture_is_current(aec):
    arrays, report = mg.make()
    mg.check(report)
    with np.load(rs.LIBAEC_LINES) as z:
        assert sorted(z.files) == sorted(arrays)
        for k, a in arrays.items():
            assert z[k].dtype == a.dtype and np.array_equal(z[k], a), k


def test_fixture_holds_what_it_is_for():
    """From the committed file alone: its size, the groups the GPU tier relies on, every line through the specification,
    every option at both ID lengths, and the share of lines whose bytes are not rs.encode's."""
    assert os.path.getsize(rs.LIBAEC_LINES) <= mg.MAX_BYTES
    groups = rs.libaec_groups()
    assert [(n, J, S, len(lines), source) for n, J, S, source, lines, _ in groups] == list(mg.GROUPS)
    met = {3: {}, 4: {}}
    total = differ = 0
    for n, J, S, source, lines, samples in groups:
        assert samples.shape == (len(lines), S) and samples.dtype == np.uint16
        for line, x in zip(lines, samples):
            y, status = rs.decode(line, n, J, S, stats=met[rs.id_bits(n)])
            assert status == 0 and np.array_equal(x, y), (n, J, S)
            differ += line != rs.encode(x, n, J)
            total += 1
    print("lines", total, "other bytes than rs.encode", differ)
    mg.check(dict(met=met, lines=total, differ=differ))
    shapes = {(n, J, S) for n, J, S, *_ in groups}
    assert {J for _, J, _ in shapes} == set(rs.BLOCK_SIZES) and {1, 4, 8, 10, 16} <= {n for n, _, _ in shapes}
    assert any(S == 1 for _, _, S in shapes) and any(S % J for _, J, S in shapes if S > 1)
    assert any(-(-S // J) == aec_ref.MAX_RSI for _, J, S in shapes)
    assert {source for _, _, _, source, _, _ in groups} == {mg.LIBAEC, mg.LIBSZ}
