"""NumPy / Python specification of the channel demultiplexer and the decoder's packet accounting: a literal
transcription of decoder/src/newdecoder.cpp:309-395 (the statistics of a frame, ChannelWriter::writeChannel) with the
reference's C integer types, and a `struct` packer of its wire record (Statistics_st, Statistics.h:14-36, packed,
little-endian).  DESIGN.md section 13 is the contract; the device stage (xrit_demux_*, ChannelDemux) must reproduce it
exactly."""
import struct

import numpy as np

VCDU_BYTES = 892                       # FRAMESIZE - RSPARITYBLOCK - SYNCWORDSIZE / 8 (newdecoder.cpp:356)
FRAME_BITS = 8192                      # FRAMEBITS
VITERBI_BITS = 8256                    # the length Viterbi27 is built with (newdecoder.cpp:80)
N_VC = 64                              # vcid has 6 bits
WIRE_FORMAT = "<BBQHH4iBBBQHBQ256q256qQI4sBBB"
WIRE_SIZE = struct.calcsize(WIRE_FORMAT)
assert WIRE_SIZE == 4167

U64 = (1 << 64) - 1

# xrit_frame_stats: one compact record per frame (include/xritdemod_amd.h)
RECORD_DTYPE = np.dtype([
    ("packet_number", np.uint64), ("lost_packets", np.uint64), ("dropped_packets", np.uint64),
    ("total_packets", np.uint64), ("received_vc", np.int64), ("lost_vc", np.int64),
    ("rs_errors", np.int32, (4,)),
    ("vit_errors", np.uint16), ("frame_bits", np.uint16), ("average_vit_corrections", np.uint16),
    ("scid", np.uint8), ("vcid", np.uint8), ("signal_quality", np.uint8), ("sync_correlation", np.uint8),
    ("phase_correction", np.uint8), ("average_rs_corrections", np.uint8), ("sync_word", np.uint8, (4,)),
    ("frame_lock", np.uint8), ("valid", np.uint8), ("reserved", np.uint8, (6,))])
assert RECORD_DTYPE.itemsize == 88


def signal_quality(viterbi_errors):
    """newdecoder.cpp:289-291 in float32, GetPercentBER() taken as 100 * BER / 8256 (unverified)."""
    p = np.float32(100) * np.float32(viterbi_errors) / np.float32(VITERBI_BITS)
    s = np.float32(100) - p * np.float32(10)
    return 0 if s < 0 else int(s)


class State:
    """The counters main() keeps across frames (newdecoder.cpp:44-53, 133-137)."""

    def __init__(self, start_time=0):
        self.dropped = 0           # droppedPackets, uint64
        self.sum_rs = 0            # averageRSCorrections, uint64
        self.sum_vit = 0           # averageVitCorrections, uint64
        self.frames = 0            # frameCount, uint64
        self.lost = 0              # lostPackets, uint64
        self.lost_vc = [0] * 256   # lostPacketsPerFrame, int64
        self.last = [-1] * 256     # lastPacketCount, int64
        self.received = [-1] * 256  # receivedPacketsPerFrame, int64
        self.start_time = start_time


def _u64(x):
    return x & U64


def _int(x):
    """C (int) of a 64-bit value."""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def process(state, hits, cadu, block, info, wire=True):
    """One call's frames through the loop body.  hits: rows (word, position, correlation[, reserved]) as the correlator
    returned them; cadu (nf, >= 4) uint8; block (nf, >= 892) uint8 (or (nf, 0) to skip the VCDUs); info:
    xrit_frame_info rows.  Returns (vcdu, offsets, records, wire): the good frames' VCDUs grouped by VCID in ascending
    order (frame order within a VCID), the exclusive prefix of the per-VCID counts (65 entries), one RECORD_DTYPE row
    per frame, and the Statistics_st the reference would send after every valid frame (a list of WIRE_SIZE-byte
    strings; empty when wire is False)."""
    hits = np.asarray(hits)
    nf = len(info)
    cols = {k: np.asarray(info[k]).tolist() for k in ("valid", "viterbi_errors", "rs_errors", "scid", "vcid", "counter")}
    words, corrs = hits[:, 0].tolist(), hits[:, 2].tolist()
    sync = [bytes(r) for r in np.asarray(cadu)[:, :4]]
    rows = [None] * nf
    out = []
    per_vc = [[] for _ in range(N_VC)]
    s = state
    for f in range(nf):
        if not cols["valid"][f]:
            continue                                        # :244-247, no record
        verr = int(cols["viterbi_errors"][f])
        derrors = [int(x) for x in cols["rs_errors"][f]]
        word, corr = int(words[f]), int(corrs[f])
        sync_word = sync[f]                                 # :302
        sq = signal_quality(verr)
        s.sum_vit = _u64(s.sum_vit + verr)
        s.frames = _u64(s.frames + 1)
        corrupted = derrors == [-1, -1, -1, -1]
        if corrupted:
            s.dropped = _u64(s.dropped + 1)
        else:
            for e in derrors:
                s.sum_rs = _u64(s.sum_rs + (e if e != -1 else 0))
        scid, vcid, counter = cols["scid"][f] & 0xFF, cols["vcid"][f] & 0xFF, cols["counter"][f] & 0xFFFFFF
        phase = 180 if word != 0 else 0
        avg_vit = (s.sum_vit // s.frames) & 0xFFFF
        avg_rs = (s.sum_rs // s.frames) & 0xFF
        if not corrupted:
            per_vc[vcid].append(f)
            if s.last[vcid] + 1 != counter and s.last[vcid] > -1:
                lost = _int(counter - s.last[vcid] - 1)
                s.lost = _u64(s.lost + lost)
                s.lost_vc[vcid] += lost
            s.last[vcid] = counter
            s.received[vcid] = 1 if s.received[vcid] == -1 else s.received[vcid] + 1
            fields = (scid, vcid, counter, verr & 0xFFFF, FRAME_BITS, derrors, sq, corr & 0xFF, phase, True)
            rvc, lvc = s.received[vcid], s.lost_vc[vcid]
        else:
            fields = (0, 0, 0, verr & 0xFFFF, FRAME_BITS, derrors, 0, corr & 0xFF, 0, False)
            rvc, lvc = 0, 0
        scid_o, vcid_o, pn, vit16, fbits, rs, sq_o, corr8, phase_o, lock = fields
        rows[f] = (pn, s.lost, s.dropped, s.frames, rvc, lvc, rs, vit16, fbits, avg_vit, scid_o, vcid_o, sq_o, corr8,
                   phase_o, avg_rs, list(sync_word), int(lock), 1, [0] * 6)
        if wire:
            out.append(pack(scid=scid_o, vcid=vcid_o, packetNumber=pn, vitErrors=vit16, frameBits=fbits, rsErrors=rs,
                            signalQuality=sq_o, syncCorrelation=corr8, phaseCorrection=phase_o, lostPackets=s.lost,
                            averageVitCorrections=avg_vit, averageRSCorrections=avg_rs, droppedPackets=s.dropped,
                            receivedPacketsPerChannel=s.received, lostPacketsPerChannel=s.lost_vc,
                            totalPackets=s.frames, startTime=s.start_time, syncWord=sync_word, frameLock=lock))
    zero = (0, 0, 0, 0, 0, 0, [0] * 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, [0] * 4, 0, 0, [0] * 6)
    rec = np.array([r if r is not None else zero for r in rows], RECORD_DTYPE)
    counts = [len(x) for x in per_vc]
    offsets = np.zeros(N_VC + 1, np.uint32)
    offsets[1:] = np.cumsum(counts)
    order = np.array([f for x in per_vc for f in x], np.int64)
    block = np.asarray(block)
    vcdu = block[order, :VCDU_BYTES] if len(order) else np.zeros((0, min(block.shape[1], VCDU_BYTES)), np.uint8)
    return vcdu, offsets, rec, out


def pack(scid, vcid, packetNumber, vitErrors, frameBits, rsErrors, signalQuality, syncCorrelation, phaseCorrection,
         lostPackets, averageVitCorrections, averageRSCorrections, droppedPackets, receivedPacketsPerChannel,
         lostPacketsPerChannel, totalPackets, startTime, syncWord, frameLock, demodulatorFifoUsage=0, decoderFifoUsage=0):
    """Statistics_st as the dispatcher sends it: packed, little-endian, Statistics.h's field order."""
    return struct.pack(WIRE_FORMAT, scid, vcid, packetNumber, vitErrors, frameBits, *rsErrors, signalQuality,
                       syncCorrelation, phaseCorrection, lostPackets, averageVitCorrections, averageRSCorrections,
                       droppedPackets, *receivedPacketsPerChannel, *lostPacketsPerChannel, totalPackets, startTime,
                       bytes(syncWord), int(bool(frameLock)), demodulatorFifoUsage, decoderFifoUsage)


def unpack(raw):
    """One wire record back into a dict of Statistics_st's fields."""
    v = struct.unpack(WIRE_FORMAT, raw)
    names = ["scid", "vcid", "packetNumber", "vitErrors", "frameBits"]
    d = dict(zip(names, v[:5]))
    d["rsErrors"] = list(v[5:9])
    for i, n in enumerate(["signalQuality", "syncCorrelation", "phaseCorrection", "lostPackets", "averageVitCorrections",
                           "averageRSCorrections", "droppedPackets"]):
        d[n] = v[9 + i]
    d["receivedPacketsPerChannel"] = list(v[16:272])
    d["lostPacketsPerChannel"] = list(v[272:528])
    for i, n in enumerate(["totalPackets", "startTime", "syncWord", "frameLock", "demodulatorFifoUsage",
                           "decoderFifoUsage"]):
        d[n] = v[528 + i]
    return d
