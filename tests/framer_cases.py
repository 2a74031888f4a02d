"""Streams and cuttings the frame synchroniser's tests share (tests/test_framer_spec.py, tests/test_gpu_framer.py)."""
import numpy as np

import ccsds

F = ccsds.FRAME_SYMBOLS


def coded_frames(n, rng, hrit=False, amplitude=100):
    """(n, F) int8: n CADUs of random VCDUs, coded as one stream."""
    cadus = [ccsds.cadu_from_block(ccsds.make_block(0x8C, (5, 7, 63)[i % 3], 100 + i // 3, rng)) for i in range(n)]
    return ccsds.coded_symbols(cadus, hrit=hrit, amplitude=amplitude).reshape(n, F), cadus


def drifting_stream(offset=16300, n=40, inserts=(10, 20), seed=1, hrit=False):
    """n coded frames behind `offset` symbols of noise, one symbol inserted after each frame of `inserts`: (stream, the
    frames as sent, where each begins, the CADUs)."""
    rng = np.random.default_rng(seed)
    frames, cadus = coded_frames(n, rng, hrit=hrit)
    parts, starts, at = [rng.integers(-20, 21, offset).astype(np.int8)], [], offset
    for i in range(n):
        starts.append(at)
        parts.append(frames[i])
        at += F
        if i in inserts:
            parts.append(np.array([0], np.int8))
            at += 1
    return np.concatenate(parts), frames, np.array(starts, np.uint64), cadus


def cuttings(length, frame, word_at, frame_end, count=20, seed=7):
    """`count` random cuttings of a stream of `length` symbols, each a sorted list of cut positions; every one also holds
    cuts at 0, 1, frame - 1, frame, inside a sync word (word_at + 31) and at the last byte of a frame (frame_end - 1)."""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, frame - 1, frame, word_at + 31, frame_end - 1]
    out = []
    for _ in range(count):
        k = int(rng.integers(1, 9))
        cuts = sorted(set(fixed) | set(int(v) for v in rng.integers(0, length + 1, k)))
        out.append([c for c in cuts if 0 <= c <= length])
    return out
