"""CPU tier: the specification of the file assembler (tests/file_spec.py) -- generated files over several keys in calls
cut at random, every kind of damage with the record flags and counters it must leave, the header record walk, the
sequence count's wrap."""
import numpy as np
import pytest

import file_spec as fs

KEYS = [(0, 5), (0, 700), (3, 5), (3, 6), (62, 2046), (7, 0)]


def run(stream, state=None, cuts=None, rng=None, col=None):
    """The stream through the specification, in one call or in calls of 0 .. cuts packets.  -> (collector, state,
    all records, last summary)."""
    state = fs.State() if state is None else state
    col = fs.Collector() if col is None else col
    recs, summary = [], None
    calls = [stream] if cuts is None else fs.cut_calls(rng, stream, cuts)
    for part in calls:
        data, pieces, files, summary = fs.process(state, *fs.stage_input(part))
        assert len(data) == summary["bytes"] == int(pieces["length"].sum())
        assert len(data) <= sum(len(e[1]) for e in part)
        col.add(data, pieces, files)
        recs.extend(files)
    return col, state, recs, summary


@pytest.mark.parametrize("cuts", [None, 1, 7, 60])
def test_generated_files_come_back(cuts):
    rng = np.random.default_rng(11)
    stream, files = fs.random_stream(rng, 60, KEYS)
    col, state, recs, summary = run(stream, cuts=cuts, rng=rng)
    got = {k[:3]: k[3] for k in col.done}
    assert got == files and not col.aborted and not col.partial
    for v, a, s, data, r in col.done:
        assert r["flags"] & fs.ENDS and r["flags"] & fs.LENGTH_MATCH and int(r["declared_bits"]) == 8 * len(data)
        assert int(r["header_state"]) in (1, 2) and int(r["header_length"]) <= len(data)      # 1: headers over several packets
        assert int(r["data_bits"]) == 8 * (len(data) - int(r["header_length"]))
    assert summary["files_begun"] == summary["files_completed"] == 60
    assert all(summary[c] == 0 for c in ("files_aborted", "bad_packets", "seq_gaps", "short_first", "orphans"))
    assert summary["total_pieces"] == len(stream) and state.open_files() == 0
    if cuts is None:
        assert [(int(r["vcid"]), int(r["apid"])) for r in recs] == sorted((int(r["vcid"]), int(r["apid"])) for r in recs)
        assert (np.array(recs)["flags"] == (fs.BEGINS | fs.ENDS | fs.LENGTH_MATCH)).all()


def test_cut_calls_equal_one_call_state():
    rng = np.random.default_rng(12)
    stream, _ = fs.random_stream(rng, 40, KEYS)
    stream = stream[:len(stream) * 2 // 3]                           # files left open at the end
    _, one, _, s1 = run(stream)
    _, many, _, s2 = run(stream, cuts=9, rng=rng)
    assert one.open_files() > 0
    assert {k: v.as_tuple() for k, v in one.keys.items()} == {k: v.as_tuple() for k, v in many.keys.items()}
    assert {c: s1[c] for c in fs.COUNTERS} == {c: s2[c] for c in fs.COUNTERS}


def one_file(rng, n_pieces=6, key=(3, 5), seq=100):
    f = fs.lrit_file(rng.integers(0, 256, 100 * n_pieces - 40, dtype=np.uint8).tobytes(), image=(8, 10, 10, 0))
    pk, _ = fs.packetise(f, key[1], seq, 77, max_user=100)
    assert len(pk) == n_pieces
    return [(key[0], p) for p in pk], f


def test_each_damage_kind():
    rng = np.random.default_rng(13)
    stream, f = one_file(rng)
    col, st, recs, s = run(stream)
    assert col.done[0][3] == f and int(recs[0]["file_counter"]) == 77 and int(recs[0]["n_pieces"]) == 6

    # a removed packet in the middle: a gap aborts the file, the rest are orphans
    col, st, recs, s = run(fs.remove(stream, 2))
    assert len(recs) == 1 and recs[0]["flags"] == fs.BEGINS | fs.ABORTED and int(recs[0]["n_pieces"]) == 2
    assert (s["seq_gaps"], s["files_aborted"], s["orphans"], s["files_completed"]) == (1, 1, 3, 0)
    assert not col.done and col.aborted == [(3, 5, 0)]
    # the first packet removed: orphans only, no record
    col, st, recs, s = run(fs.remove(stream, 0))
    assert not recs and (s["orphans"], s["files_begun"], s["seq_gaps"]) == (5, 0, 0)
    # the last packet removed: the file stays open; the next file's first packet aborts it
    nxt, f2 = one_file(rng, 3, seq=105)           # (the count the lost packet had: no gap)
    col, st, recs, s = run(fs.remove(stream, 5) + nxt)
    assert [int(r["flags"]) for r in recs] == [fs.BEGINS | fs.ABORTED, fs.BEGINS | fs.ENDS | fs.LENGTH_MATCH]
    assert [int(r["key_serial"]) for r in recs] == [0, 1] and col.done[0][3] == f2
    assert (s["files_aborted"], s["files_completed"], s["seq_gaps"]) == (1, 1, 0)
    # ... in the next call: a record of that call with no pieces
    state = fs.State()
    col = run(fs.remove(stream, 5), state)[0]
    _, _, recs, s = run(nxt, state, col=col)
    assert [int(r["flags"]) for r in recs] == [fs.ABORTED, fs.BEGINS | fs.ENDS | fs.LENGTH_MATCH]
    assert int(recs[0]["n_pieces"]) == 0 and int(recs[0]["length"]) == 0 and int(recs[0]["file_offset"]) == 5 * 100 - 10
    assert int(recs[0]["columns"]) == 10 and int(recs[0]["key_serial"]) == 0

    # a bad CRC: the packet is not emitted, the open file is aborted
    col, st, recs, s = run(fs.bad_crc(stream, 3))
    assert recs[0]["flags"] == fs.BEGINS | fs.ABORTED and int(recs[0]["n_pieces"]) == 3
    assert (s["bad_packets"], s["files_aborted"], s["orphans"], s["seq_gaps"]) == (1, 1, 2, 0)
    # ... with no file open it is only counted
    _, _, recs, s = run(fs.bad_crc(stream, 0))
    assert not recs and (s["bad_packets"], s["files_aborted"], s["orphans"]) == (1, 0, 5)

    # a repeated packet: its sequence count is not the expected one
    col, st, recs, s = run(fs.repeat(stream, 1))
    assert recs[0]["flags"] == fs.BEGINS | fs.ABORTED and int(recs[0]["n_pieces"]) == 2
    assert (s["seq_gaps"], s["orphans"]) == (1, 5)
    # a repeated first packet: the gap aborts, the packet itself begins the file again
    col, st, recs, s = run(fs.repeat(stream, 0))
    assert [int(r["flags"]) for r in recs] == [fs.BEGINS | fs.ABORTED, fs.BEGINS | fs.ENDS | fs.LENGTH_MATCH]
    assert col.done[0][3] == f and col.done[0][2] == 1 and (s["seq_gaps"], s["files_aborted"]) == (1, 1)

    # wrong flags: a continuation marked last ends the file early (the length no longer matches) ...
    col, st, recs, s = run(fs.wrong_flags(stream, 2, 2))
    assert recs[0]["flags"] == fs.BEGINS | fs.ENDS and (s["files_completed"], s["orphans"]) == (1, 3)
    assert col.done[0][3] == f[:290]
    # ... marked first it aborts the file and begins another, marked unsegmented that one ends at once
    col, st, recs, s = run(fs.wrong_flags(stream, 2, 1))
    assert [int(r["flags"]) for r in recs] == [fs.BEGINS | fs.ABORTED, fs.BEGINS | fs.ENDS]
    assert (s["files_begun"], s["files_aborted"], s["files_completed"]) == (2, 1, 1) and int(recs[1]["header_state"]) == 0
    col, st, recs, s = run(fs.wrong_flags(stream, 2, 3))
    assert [int(r["flags"]) for r in recs] == [fs.BEGINS | fs.ABORTED, fs.BEGINS | fs.ENDS] and s["orphans"] == 3
    # the last marked continuation: the file stays open
    col, st, recs, s = run(fs.wrong_flags(stream, 5, 0))
    assert recs[0]["flags"] == fs.BEGINS and st.open_files() == 1 and bytes(col.partial[(3, 5, 0)]) == f

    # a first packet shorter than the transport header
    for n_user in (0, 9):
        col, st, recs, s = run(fs.short_first(stream, 0, rng, n_user))
        assert not recs and (s["short_first"], s["orphans"], s["files_begun"]) == (1, 5, 0)
    col, st, recs, s = run(fs.short_first(stream, 3, rng))
    assert recs[0]["flags"] == fs.BEGINS | fs.ABORTED and (s["short_first"], s["files_aborted"], s["orphans"]) == (1, 1, 2)
    # exactly ten bytes: a file with an empty first piece
    col, st, recs, s = run([(3, fs.space_packet(5, 0, 3, bytes(10)))])
    assert recs[0]["flags"] == fs.BEGINS | fs.ENDS | fs.LENGTH_MATCH and int(recs[0]["n_pieces"]) == 1 and s["bytes"] == 0


def header_state_of(payload):
    k = fs.Key()
    fs.parse_header(k, bytes(payload))
    return k


def test_header_record_chains():
    img = fs.record(1, bytes([8, 0, 100, 0, 50, 1]))
    rice = fs.record(131, bytes([0, 49, 16, 1]))
    good = fs.lrit_file(b"", image=(8, 100, 50, 1), rice=(49, 16, 1))
    k = header_state_of(good + b"data")
    assert (k.header_state, k.header_length, k.bits_per_pixel, k.columns, k.lines, k.compression, k.rice_flags,
            k.pixels_per_block, k.lines_per_packet) == (2, 16 + 9 + 7, 8, 100, 50, 1, 49, 16, 1)
    assert header_state_of(good).header_state == 2                  # the headers alone
    assert header_state_of(good[:-1]).header_state == 1             # the headers continue in a later packet
    assert header_state_of(good[:15]).header_state == 0
    assert header_state_of(b"\x01" + good[1:]).header_state == 0    # not a primary header
    assert header_state_of(good[:2] + b"\x11" + good[3:]).header_state == 0

    def chain(recs, total=None):
        body = b"".join(recs)
        total = 16 + len(body) if total is None else total
        return bytes([0, 0, 16, 0]) + total.to_bytes(4, "big") + bytes(8) + body

    assert header_state_of(chain([])).header_state == 2
    assert header_state_of(chain([], total=12)).header_state == 1   # shorter than the primary header itself
    assert header_state_of(chain([img, b"\x05\x00\x02"])).header_state == 1          # a record shorter than its own head
    k = header_state_of(chain([img, b"\x05\x00\x20", rice]))        # a record that runs past the headers
    assert (k.header_state, k.columns, k.pixels_per_block) == (1, 100, 0)
    assert header_state_of(chain([img, b"\x05\x00"])).header_state == 1              # two stray bytes at the end
    k = header_state_of(chain([fs.record(1, bytes(7)), fs.record(131, bytes(5)), img, rice, fs.record(1, bytes([1] * 6))]))
    assert (k.header_state, k.bits_per_pixel, k.columns, k.rice_flags) == (2, 8, 100, 49)   # wrong lengths skipped; the first fit counts
    k = header_state_of(chain([img, rice]) + bytes(50))
    assert k.header_state == 2 and k.header_length == 32

    rec = np.zeros(1, fs.RECORD_DTYPE)[0]
    for f, v in (("header_state", 2), ("compression", 1), ("bits_per_pixel", 8), ("columns", 100), ("pixels_per_block", 16),
                 ("header_length", 32)):
        rec[f] = v
    assert fs.is_rice_coded(rec, 32) and not fs.is_rice_coded(rec, 33)
    for f, v in (("header_state", 1), ("file_type", 2), ("compression", 0), ("bits_per_pixel", 17), ("bits_per_pixel", 0),
                 ("columns", 0), ("pixels_per_block", 12)):
        bad = rec.copy()
        bad[f] = v
        assert not fs.is_rice_coded(bad, 32), f


def test_sequence_count_wraps():
    rng = np.random.default_rng(14)
    stream, f = one_file(rng, 6, seq=16381)
    assert [(p[2] & 0x3F) << 8 | p[3] for _, p in stream] == [16381, 16382, 16383, 0, 1, 2]
    col, st, recs, s = run(stream, cuts=2, rng=rng)
    assert col.done[0][3] == f and s["seq_gaps"] == 0 and s["files_completed"] == 1


def test_random_packets_never_raise_and_stay_within_the_input():
    rng = np.random.default_rng(15)
    stream = fs.random_packets(rng, 3000, [1, 9])
    col, st, recs, s = run(stream, cuts=50, rng=rng)
    assert s["files_begun"] > 50 and s["files_aborted"] > 10 and s["orphans"] > 10 and s["short_first"] > 10
    assert s["bad_packets"] > 50 and {int(r["header_state"]) for r in recs} == {0, 1, 2}


# ---- the generators of the GPU tier reach what they are there for ------------------------------------------------------
def test_long_piece_stream_has_pieces_around_the_gather_steps():
    stream, files = fs.long_piece_stream()
    assert len(stream) == 600
    col, state, recs, s = run(stream)
    data, pieces, _, _ = fs.process(fs.State(), *fs.stage_input(stream))
    lengths = {int(x) for x in pieces["length"]}
    assert {2047, 2048, 2049, 4095, 4096, 4097, 8190, 65524} <= lengths and max(lengths) == 65524
    assert len(pieces) >= 500 and int((pieces["length"] > 2048).sum()) >= 250 and len(data) > 2_000_000
    # the files that came through whole are generated ones, and there are many of them, over several pieces
    whole = [d for d in col.done if d[4]["flags"] & fs.LENGTH_MATCH]
    assert len(whole) >= 100 and all(d[3] in files for d in whole)
    assert sum(len(d[3]) > 3 * 2048 for d in whole) >= 50
    # ... and in calls cut at random the same ones
    col2 = run(stream, cuts=40, rng=np.random.default_rng(16))[0]
    assert sorted(d[:4] for d in col2.done) == sorted(d[:4] for d in col.done)


def test_many_pieces_stream_emits_more_than_one_gather_pass():
    args, runs = fs.many_pieces_case()
    assert len(args[1]) == 60000
    for (data, pieces, files, summary), state in runs:
        assert summary["pieces"] == len(pieces) >= 40000 > 4096 * 8
        # the second pass moves long pieces too
        assert int((pieces["length"][4096 * 8:] > 2048).sum()) >= 100 and int(pieces["length"][4096 * 8:].max()) == 8190
    assert runs[1][1].total_pieces == runs[0][0][3]["pieces"] + runs[1][0][3]["pieces"] and runs[0][1].open_files() > 0
