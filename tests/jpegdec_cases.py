"""Inputs of the JPEG decoder's tests, shared by the CPU tier (tests/test_jpegdec_spec.py), the GPU tier
(tests/test_gpu_jpegdec.py) and the fixture's generator (tests/golden/make_jpegdec_golden.py).  The Pillow-written streams
and Pillow's pixels for them are recorded in tests/golden/jpegdec_pil.npz; everything else is made here from those or
from nothing: the streams Pillow cannot write (12-bit, arithmetic, 16-bit tables), the damaged set, the adversarial one."""
import os

import numpy as np

import jpeg_cases as jc
import jpeg_spec as js
import jpegdec_spec as ds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pillow_cases():
    """(name, image, Pillow's save arguments, bytes appended behind EOI).  At most 64, shapes up to 64 x 72 but for the row of
    75 blocks.  What tests/golden/jpeg_pil_files.npz lacks: optimised tables, restart intervals 0, 1, 2, 7, a block row and
    beyond the image, qtables=, COM and APPn segments, trailing bytes."""
    own = [[int(v) for v in row] for row in np.stack([np.arange(1, 65), np.arange(64, 0, -1) * 3])]
    out = []
    add = lambda name, image, tail=b"", **kw: out.append((name, image, dict(dict(quality=90, subsampling=0), **kw), tail))
    for rgb in (False, True):
        t = "rgb" if rgb else "grey"
        sh = lambda r, c: (r, c, 3) if rgb else (r, c)
        add(f"{t}_1x1", jc.noise(1, sh(1, 1)), quality=75)
        add(f"{t}_8x8", jc.noise(2, sh(8, 8)), optimize=True)
        add(f"{t}_7x9", jc.noise(3, sh(7, 9)), restart_marker_blocks=1)
        add(f"{t}_9x7", jc.noise(4, sh(9, 7)), restart_marker_blocks=2, optimize=True)
        add(f"{t}_row75", jc.smooth(sh(8, 600)), quality=95, restart_marker_blocks=7)
        add(f"{t}_row75_noise", jc.noise(5, sh(5, 597)), quality=85)
        add(f"{t}_q100_noise", jc.noise(6, sh(64, 72)), quality=100)
        add(f"{t}_q100_noise_opt", jc.noise(7, sh(64, 72)), quality=100, optimize=True, restart_marker_blocks=9)
        add(f"{t}_smooth_rows", jc.smooth(sh(40, 56)), quality=60, restart_marker_blocks=7)
        add(f"{t}_beyond", jc.noise(8, sh(19, 21)), restart_marker_blocks=5000)
        add(f"{t}_own_tables", jc.noise(9, sh(17, 33)), qtables=own if rgb else own[:1], restart_marker_blocks=2, quality=None)
        add(f"{t}_ones", jc.checkerboard(16, 24) if not rgb else np.stack([jc.checkerboard(16, 24), jc.flat_blocks(16, 24), 255 - jc.checkerboard(16, 24)], -1),
            qtables=[[1] * 64] * (2 if rgb else 1), quality=None, optimize=True)
        add(f"{t}_q1", jc.smooth(sh(33, 17)), quality=1, restart_marker_blocks=1)
        add(f"{t}_com_app", jc.noise(10, sh(23, 5)), comment=b"a comment", icc_profile=b"profile " * 9, restart_marker_blocks=3)
        add(f"{t}_trailing", jc.noise(11, sh(9, 9)), tail=b"\x00\xff\xd8 behind EOI \xff\xd9\xff", optimize=True)
        add(f"{t}_checker", np.stack([jc.checkerboard(24, 40)] * 3, -1) if rgb else jc.checkerboard(24, 40), quality=100)
    return out


def unsupported_cases():
    """(name, image, mode, save arguments): what Pillow writes that the stage does not decode."""
    rgb = jc.smooth((24, 40, 3))
    return [("progressive", rgb, "RGB", dict(progressive=True, subsampling=0)), ("progressive_grey", jc.smooth((24, 40)), "L", dict(progressive=True)),
            ("s420", rgb, "RGB", dict(subsampling=2)), ("s422", rgb, "RGB", dict(subsampling=1)),
            ("cmyk", np.concatenate([rgb, rgb[..., :1]], -1), "CMYK", dict())]


def pillow_write(image, kw, tail=b"", mode=None):
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image, mode).save(buf, "JPEG", **{k: v for k, v in kw.items() if v is not None})
    return buf.getvalue() + tail


def pillow_read(data):
    import io

    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


class Golden:
    """tests/golden/jpegdec_pil.npz: names, the streams back to back, Pillow's pixels for the sound ones."""

    def __init__(self):
        z = np.load(os.path.join(GOLDEN, "jpegdec_pil.npz"))
        self.names = [str(n) for n in z["names"]]
        self.files = {n: z["data"][z["offsets"][i]:z["offsets"][i + 1]].tobytes() for i, n in enumerate(self.names)}
        self.pixels = {n: z["pixels_%02d" % i] for i, n in enumerate(self.names) if "pixels_%02d" % i in z.files}
        self.sound = [n for n in self.names if n in self.pixels]
        self.unsupported = [n for n in self.names if n not in self.pixels]


def encoder_files():
    """The older fixture: tests/golden/jpeg_pil_files.npz, files Pillow wrote for tests/jpeg_cases.py's inputs."""
    z = np.load(os.path.join(GOLDEN, "jpeg_pil_files.npz"))
    return [(str(n), z["data"][z["offsets"][i]:z["offsets"][i + 1]].tobytes()) for i, n in enumerate(z["names"])]


def find(data, marker, start=0):
    """The offset of the first FF `marker` of the header's chain (not a search through segment bodies)."""
    p = 2
    while p + 4 <= len(data):
        if data[p + 1] == marker and p >= start:
            return p
        p += 2 + (data[p + 2] << 8 | data[p + 3])
    raise KeyError(marker)


def patched(data, what):
    """Streams Pillow does not write, from one it does: the SOF's precision 12; SOF0 become SOF9 (arithmetic), SOF1
    (extended), SOF3 (lossless); a 16-bit quantiser table; two components; dimensions of 0; an SOS that names table 3."""
    d = bytearray(data)
    sof, dqt, sos = find(d, 0xC0), find(d, 0xDB), find(d, 0xDA)
    if what == "12bit":
        d[sof + 4] = 12
    elif what in ("arithmetic", "extended", "lossless"):
        d[sof + 1] = dict(arithmetic=0xC9, extended=0xC1, lossless=0xC3)[what]
    elif what == "q16":
        d[dqt + 4] |= 0x10
    elif what == "zero_rows":
        d[sof + 5] = d[sof + 6] = 0
    elif what == "zero_columns":
        d[sof + 7] = d[sof + 8] = 0
    elif what == "no_table":
        d[sos + 6] = 0x33
    elif what == "no_soi":
        d[1] = 0xD9
    elif what == "long_segment":
        d[sos + 2] = 0xFF
    elif what == "two_components":
        assert d[sof + 9] == 3                         # from a stream of three
        d[sof + 9], d[sof + 3] = 2, 8 + 6
        del d[sof + 16:sof + 19]
    return bytes(d)


PATCHES = {"12bit": ds.UNSUPPORTED, "arithmetic": ds.UNSUPPORTED, "extended": ds.UNSUPPORTED, "lossless": ds.UNSUPPORTED, "q16": ds.UNSUPPORTED,
           "two_components": ds.UNSUPPORTED, "zero_rows": ds.DAMAGED, "zero_columns": ds.DAMAGED, "no_table": ds.DAMAGED, "no_soi": ds.DAMAGED,
           "long_segment": ds.DAMAGED}


def scan_markers(data):
    """Offsets of the RSTm markers of a sound stream's scan."""
    h = ds.parse_header(data)
    a = np.frombuffer(data, np.uint8)
    at = np.nonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7))[0]
    return [int(i) for i in at if i >= h["scan"]]


def damaged_set(small, marked, seed=5):
    """(name, stream): `small` cut at every byte; single byte flips in its scan; from `marked` (a stream with at least three
    RSTm): one RSTm removed, two swapped, one become another marker, one more inserted, the EOI gone."""
    rng = np.random.default_rng(seed)
    out = [("cut_%d" % n, small[:n]) for n in range(len(small))]
    begin = ds.parse_header(small)["scan"]
    for i in range(60):
        at = int(rng.integers(begin, len(small) - 2))
        d = bytearray(small)
        d[at] ^= int(rng.integers(1, 256))
        out.append(("flip_%d" % at, bytes(d)))
    m = scan_markers(marked)
    assert len(m) >= 3
    d = bytearray(marked)
    out.append(("rst_removed", bytes(d[:m[1]] + d[m[1] + 2:])))
    d[m[0] + 1], d[m[1] + 1] = d[m[1] + 1], d[m[0] + 1]
    out.append(("rst_swapped", bytes(d)))
    d = bytearray(marked)
    d[m[1] + 1] = 0xC4
    out.append(("other_marker", bytes(d)))
    d = bytearray(marked)
    out.append(("rst_inserted", bytes(d[:-2] + bytes([0xFF, 0xD0 + (len(m) & 7)]) + d[-2:])))
    out.append(("no_eoi", bytes(marked[:-2])))
    out.append(("cut_in_scan", bytes(marked[:m[1] + 1])))
    return out


def rule_table_inputs(golden):
    """What tests/golden/jpegdec_rule_table.txt is recorded from: an optimised table (the first component's AC table of a
    stream written with optimize=True) and the streams whose headers are cut at every byte: sound, unsupported, damaged."""
    base, opt = golden.files["grey_7x9"], golden.files["rgb_9x7"]
    hf = ds.parse_header(opt)["huff"][0]
    assert hf[2] != js.AC_LUM_BITS
    flipped = [f for n, f in damaged_set(base, golden.files["grey_smooth_rows"]) if n.startswith("flip_")][:6]
    files = [base, patched(base, "12bit"), patched(base, "q16"), patched(base, "extended"), patched(base, "no_table")] + flipped + [opt]
    return (hf[2], hf[3]), files


def adversarial(blocks=200, seed=9):
    """A stream whose subsequence guesses stay wrong for as long as they can at S = 128.  One DC symbol of one code bit and one
    magnitude bit, the same for the only AC symbol (run 0, one bit), no EOB ever: every symbol is two bits and every block
    128, so a walk that starts on a symbol boundary with the wrong zigzag index stays on symbol boundaries and never finds
    the block boundary again.  The first DC symbol is four bits (code 10, two magnitude bits), which puts the true block
    boundaries at bit 130 + 128 k (block 0 is 4 + 63 * 2 bits), 2 bits off the guesses at 128 k - every guess `a block begins here` is wrong, and so is every exit state computed from
    one: the right states advance one lane per round, LANES rounds for a full tile.  -> (stream, coefficients (blocks, 64))."""
    rng = np.random.default_rng(seed)
    coef = rng.choice([-1, 1], (blocks, 64))
    dc = np.cumsum(coef[:, 0])                          # the differences are the +-1; the coefficients their sums
    dc[0:] += 2 - coef[0, 0]                            # the first difference: +2, category 2
    bits = []
    for b in range(blocks):
        for k in range(64):
            if b == 0 and k == 0:
                bits += [1, 0, 1, 0]                    # code 10, magnitude bits 10: +2
            else:
                bits += [0, 1 if coef[b, k] > 0 else 0]
    bits += [1] * (-len(bits) % 8)
    body = np.packbits(np.array(bits, np.uint8)).tobytes()
    assert b"\xff" not in body
    be16 = lambda v: [v >> 8, v & 255]
    head = [0xFF, 0xD8, 0xFF, 0xDB, 0, 67, 0] + [1] * 64
    head += [0xFF, 0xC0, 0, 11, 8] + be16(8) + be16(8 * blocks) + [1, 1, 0x11, 0]
    head += [0xFF, 0xC4, 0, 19 + 2, 0x00, 1, 1] + [0] * 14 + [1, 2]
    head += [0xFF, 0xC4, 0, 19 + 1, 0x10, 1] + [0] * 15 + [0x01]
    head += [0xFF, 0xDA, 0, 8, 1, 1, 0x00, 0, 63, 0]
    want = coef.copy()
    want[:, 0] = dc
    return bytes(head) + body + b"\xff\xd9", want
