"""Writes tests/golden/rice_libaec_lines.npz: lines encoded by libaec 1.0.4 (flags MSB | PREPROCESS, one
reference-sample interval a line), a few by its libsz under option mask 49, and the samples they were made from -- the
streams that the GPU tier feeds the Rice decoder and the image stage without our own encoder in the chain.  Needs
tests/aec_ref.py's libraries; seeded, deterministic:  python tests/golden/make_rice_golden.py

The file holds, per group, n, J, S, the source (0 libaec, 1 libsz) and the index of its first line; the lines' bytes
back to back with their offsets; the samples back to back (S per line, uint16).  tests/rice_spec.py's libaec_groups
reads it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import aec_ref  # noqa: E402
import rice_spec as rs  # noqa: E402

PATH = os.path.join(HERE, "rice_libaec_lines.npz")
SEED = 121
MAX_BYTES = 256 * 1024
LIBAEC, LIBSZ = 0, 1
# (n, J, S, lines, source).  Both ID lengths; n = 1 and 4; every J; S no multiple of J (libaec's own padding of the last
# block); S = 1; 70 and 131 blocks and a sample (J = 8: zero-block runs meet the ends of the 64-block segments); one
# line of 4096 blocks, libaec's most.  The first 8-bit and the 10-bit group also make the image files of
# tests/test_gpu_images.py: every line of theirs fits a packet.
GROUPS = ((8, 16, 600, 24, LIBAEC), (10, 32, 500, 24, LIBAEC), (16, 8, 70 * 8, 30, LIBAEC), (8, 8, 131 * 8 + 1, 24, LIBAEC),
          (1, 32, 5 * 32 - 3, 12, LIBAEC), (4, 64, 70 * 64, 18, LIBAEC), (8, 8, 1, 6, LIBAEC), (10, 16, 1, 6, LIBAEC),
          (8, 8, 4096 * 8, 1, LIBAEC), (8, 16, 320, 8, LIBSZ), (10, 32, 500, 8, LIBSZ))
KINDS = rs.KINDS + ("noise",)


def noise(rng, n, J, S):
    """Uniform noise around mid-range whose width in bits is drawn per block from 0 .. n - 1: split-sample options of
    every k, next to one another."""
    xmax = (1 << n) - 1
    half = 1 << np.repeat(rng.integers(0, n, -(-S // J)), J)[:S]
    return np.clip(xmax // 2 + (rng.random(S) * (2 * half + 1)).astype(np.int64) - half, 0, xmax).astype(np.int64)


def line_samples(rng, n, J, S, i):
    """Line i of a group: the generators of rice_spec.samples and the noise above in turn.  The 4096-block line is
    pieces of all of them."""
    if S > 8192:
        cuts = np.linspace(0, S, 2 * len(KINDS) + 1).astype(int)
        return np.concatenate([line_samples(rng, n, J, int(b - a), j) for j, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))])
    kind = KINDS[i % len(KINDS)]
    return noise(rng, n, J, S) if kind == "noise" else rs.samples(rng, kind, n, J, S)


def make():
    """-> (arrays of the file, report: options met per ID length, lines, lines whose bytes differ from rs.encode's)."""
    rng = np.random.default_rng(SEED)
    lines, samples, first = [], [], []
    met = {3: {}, 4: {}}
    differ = 0
    for n, J, S, count, source in GROUPS:
        first.append(len(lines))
        for i in range(count):
            x = line_samples(rng, n, J, S, i)
            line = aec_ref.encode(x, n, J) if source == LIBAEC else aec_ref.sz_encode(x, n, J, aec_ref.SZ_GOES)
            y, status = rs.decode(line, n, J, S, stats=met[rs.id_bits(n)])
            assert status == 0 and np.array_equal(x, y), (n, J, S, i)
            differ += line != rs.encode(x, n, J)
            lines.append(line)
            samples.append(x.astype(np.uint16))
    g = np.array(GROUPS)
    arrays = dict(n=g[:, 0].astype(np.uint8), J=g[:, 1].astype(np.uint8), S=g[:, 2].astype(np.uint32), source=g[:, 4].astype(np.uint8),
                  first=np.array(first + [len(lines)], np.uint32),
                  offsets=np.cumsum([0] + [len(ln) for ln in lines]).astype(np.uint32),
                  data=np.frombuffer(b"".join(lines), np.uint8), samples=np.concatenate(samples))
    return arrays, dict(met=met, lines=len(lines), differ=int(differ))


def check(report):
    """What the fixture is for: every option somewhere, every k at both ID lengths, and a fifth of the lines other bytes
    than our own encoder's."""
    for bits, met in report["met"].items():
        kmax = (1 << bits) - 3
        missing = {rs.ZERO, "rest", rs.SE, rs.RAW, *range(kmax + 1)} - set(met)
        assert not missing, (bits, missing, met)
    assert 5 * report["differ"] >= report["lines"], report


if __name__ == "__main__":
    arrays, report = make()
    print("lines %d, other bytes than rs.encode %d (%.1f %%)" % (report["lines"], report["differ"], 100.0 * report["differ"] / report["lines"]))
    for bits, met in report["met"].items():
        print("ID of %d bits:" % bits, {str(k): v for k, v in sorted(met.items(), key=lambda kv: str(kv[0]))})
    check(report)
    np.savez_compressed(PATH, **arrays)
    size = os.path.getsize(PATH)
    print(PATH, size, "bytes")
    assert size <= MAX_BYTES, size
