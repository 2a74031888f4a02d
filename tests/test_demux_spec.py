"""CPU tier: the demultiplexer's specification (tests/demux_spec.py) on hand-worked cases of newdecoder.cpp:309-395 --
gaps, counter wraps, repeats, first frames, corrupted and invalid frames, the C truncations -- and its wire record."""
import struct

import numpy as np

import demux_spec as ds
from xritdemod_amd import FRAME_INFO_DTYPE, FRAME_STATS_DTYPE, DECODER_STATS_DTYPE, STATISTICS_WIRE_BYTES

BAD = (-1, -1, -1, -1)


def call(rows, state=None):
    """rows: (vcid, counter[, rs_errors[, viterbi_errors[, valid]]]); rs_errors BAD makes a corrupted frame."""
    nf = len(rows)
    info = np.zeros(nf, FRAME_INFO_DTYPE)
    block = np.zeros((nf, 1020), np.uint8)
    cadu = np.zeros((nf, 1024), np.uint8)
    hits = np.zeros((nf, 4), np.uint32)
    for f, r in enumerate(rows):
        vcid, counter = r[0], r[1]
        rs = r[2] if len(r) > 2 else (0, 0, 0, 0)
        verr = r[3] if len(r) > 3 else 0
        valid = r[4] if len(r) > 4 else 1
        info[f] = (valid, 0 if tuple(rs) == BAD or not valid else 1, verr, rs, 0x8C, vcid, counter)
        block[f, :892] = (f * 7 + np.arange(892)) % 251
        cadu[f, :4] = (0x1A, 0xCF, 0xFC, 0x1D)
        hits[f] = (f & 1, 0, 60 + f, 0)
    st = state if state is not None else ds.State(start_time=1234)
    return st, ds.process(st, hits, cadu, block, info)


def test_record_layouts():
    assert ds.WIRE_SIZE == STATISTICS_WIRE_BYTES == 4167
    assert ds.RECORD_DTYPE == FRAME_STATS_DTYPE and FRAME_STATS_DTYPE.itemsize == 88
    assert DECODER_STATS_DTYPE.itemsize == 6192


def test_gap_loses_the_missing_counters():
    st, (vcdu, off, rec, wire) = call([(5, 5), (5, 8)])
    assert rec["lost_packets"].tolist() == [0, 2] and rec["lost_vc"].tolist() == [0, 2]
    assert st.lost == 2 and st.lost_vc[5] == 2 and st.last[5] == 8 and st.received[5] == 2
    assert off[5] == 0 and off[6] == 2 and off[64] == 2


def test_first_frame_of_a_channel_loses_nothing():
    st, (_, _, rec, _) = call([(1, 1000), (2, 7), (1, 1001)])
    assert rec["lost_packets"].tolist() == [0, 0, 0]
    assert rec["received_vc"].tolist() == [1, 1, 2]


def test_counter_wrap_adds_minus_2_pow_24():
    st, (_, _, rec, wire) = call([(3, 0xFFFFFF), (3, 0)])
    assert st.lost == (1 << 64) - (1 << 24) and st.lost_vc[3] == -(1 << 24)
    assert int(rec["lost_packets"][1]) == (1 << 64) - (1 << 24) and int(rec["lost_vc"][1]) == -(1 << 24)
    d = ds.unpack(wire[1])
    assert d["lostPackets"] == (1 << 64) - (1 << 24) and d["lostPacketsPerChannel"][3] == -(1 << 24)


def test_repeated_counter_adds_minus_one():
    st, (_, _, rec, _) = call([(4, 10), (4, 10), (4, 11)])
    assert rec["lost_vc"].tolist() == [0, -1, -1]
    assert st.lost == (1 << 64) - 1 and st.received[4] == 3


def test_corrupted_frame():
    st, (vcdu, off, rec, wire) = call([(2, 50, (1, 0, 0, 2), 300), (9, 77, BAD, 900), (2, 51)])
    r = rec[1]
    assert (r["scid"], r["vcid"], r["packet_number"], r["signal_quality"], r["phase_correction"]) == (0, 0, 0, 0, 0)
    assert r["frame_lock"] == 0 and r["valid"] == 1 and r["dropped_packets"] == 1 and r["total_packets"] == 2
    assert r["rs_errors"].tolist() == [-1] * 4 and r["vit_errors"] == 900
    assert r["sync_correlation"] == 61 and r["sync_word"].tolist() == [0x1A, 0xCF, 0xFC, 0x1D]
    assert st.dropped == 1 and st.received[9] == -1 and st.last[9] == -1
    assert off[64] == 2 and rec["frame_lock"].tolist() == [1, 0, 1]
    assert rec["lost_packets"].tolist() == [0, 0, 0]
    d = ds.unpack(wire[1])
    assert d["frameLock"] == 0 and d["vcid"] == 0 and d["droppedPackets"] == 1 and d["receivedPacketsPerChannel"][2] == 1
    # averages: (300 + 900) / 2 and 3 / 2, truncated
    assert r["average_vit_corrections"] == 600 and r["average_rs_corrections"] == 1


def test_invalid_frames_do_not_exist():
    st, (vcdu, off, rec, wire) = call([(1, 1), (1, 5, (0, 0, 0, 0), 0, 0), (1, 2)])
    assert len(wire) == 2 and rec["valid"].tolist() == [1, 0, 1]
    assert rec[1].tobytes() == bytes(88)
    assert st.frames == 2 and st.lost == 0 and off[64] == 2


def test_average_rs_truncates_to_uint8():
    # a frame adds at most 64 RS corrections, so the uint8 cast of the uint64 quotient bites on a state that carries a
    # large sum; set one up directly
    st = ds.State()
    st.sum_rs, st.frames = 1000, 1
    st, (_, _, rec, _) = call([(0, 1, (16, 16, 16, 16))], st)
    assert int(rec["average_rs_corrections"][0]) == (1064 // 2) & 0xFF == 20
    st2 = ds.State()
    st2.sum_vit, st2.frames = 70000 * 3, 2
    st2, (_, _, rec2, _) = call([(0, 1, (0, 0, 0, 0), 0)], st2)
    assert int(rec2["average_vit_corrections"][0]) == 70000 & 0xFFFF


def test_received_stays_minus_one_and_arrays_are_256_wide():
    st, (_, _, _, wire) = call([(0, 1), (63, 9)])
    d = ds.unpack(wire[-1])
    assert len(d["receivedPacketsPerChannel"]) == 256 and len(d["lostPacketsPerChannel"]) == 256
    assert d["receivedPacketsPerChannel"][0] == 1 and d["receivedPacketsPerChannel"][63] == 1
    assert all(x == -1 for i, x in enumerate(d["receivedPacketsPerChannel"]) if i not in (0, 63))
    assert all(x == 0 for x in d["lostPacketsPerChannel"])
    assert d["startTime"] == 1234 and d["frameBits"] == 8192 and d["totalPackets"] == 2


def test_vcid_grouping_is_stable_and_keeps_fill():
    rows = [(63, 1), (2, 1), (63, 2), (0, 1), (2, 2)]
    st, (vcdu, off, rec, _) = call(rows)
    assert off[:3].tolist() == [0, 1, 1] and off[3] == 3 and off[63] == 3 and off[64] == 5
    order = [3, 1, 4, 0, 2]
    want = np.stack([(f * 7 + np.arange(892)) % 251 for f in order]).astype(np.uint8)
    assert np.array_equal(vcdu, want)


def test_signal_quality_and_phase():
    assert ds.signal_quality(0) == 100 and ds.signal_quality(8256) == 0 and ds.signal_quality(83) == 89
    st, (_, _, rec, _) = call([(1, 1, (0, 0, 0, 0), 83), (1, 2, (0, 0, 0, 0), 900)])
    assert rec["signal_quality"].tolist() == [89, 0]
    assert rec["phase_correction"].tolist() == [0, 180]


def test_wire_record_packing():
    st, (_, _, _, wire) = call([(7, 100, (1, 2, 3, 4), 5)])
    raw = wire[0]
    assert len(raw) == 4167
    assert raw[0] == 0x8C and raw[1] == 7 and struct.unpack_from("<Q", raw, 2)[0] == 100
    assert struct.unpack_from("<HH4i", raw, 10) == (5, 8192, 1, 2, 3, 4)
    assert raw[-7:-3] == bytes((0x1A, 0xCF, 0xFC, 0x1D)) and raw[-3:] == bytes((1, 0, 0))
