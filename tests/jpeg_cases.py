"""Inputs of the JPEG stage's tests, shared by the CPU tier (tests/test_jpeg_spec.py: the specification against Pillow and
against the recorded fixture) and the GPU tier (tests/test_gpu_jpeg.py: the device against the specification).  A case is
(name, image, parameters): parameters has `restart` and either `quality` or `tables` ((2, 64), natural order)."""
import numpy as np

import jpeg_spec as js

ONES = np.ones((2, 64), np.int64)


def late_tables(*positions):
    """255 everywhere except the given zigzag positions, which are 1: whatever survives has a long run in front."""
    t = np.full((2, 64), 255, np.int64)
    for k in positions:
        t[:, js.ZIGZAG[k]] = 1
    return t


def noise(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape, dtype=np.uint8)


def smooth(shape):
    rows, columns = shape[:2]
    y, x = np.mgrid[0:rows, 0:columns]
    g = (127.5 + 80 * np.sin(x / 9.0) * np.cos(y / 7.0) + 40 * np.sin((x + 2 * y) / 23.0)).astype(np.uint8)
    return g if len(shape) == 2 else np.stack([g, np.roll(g, 3, 0), 255 - g], -1)


def checkerboard(rows, columns):
    y, x = np.mgrid[0:rows, 0:columns]
    return (((y + x) & 1) * 255).astype(np.uint8)


def flat_blocks(rows, columns):
    """Blocks of 0 and of 255 in turn: the largest DC differences."""
    y, x = np.mgrid[0:rows, 0:columns]
    return ((((y >> 3) + (x >> 3)) & 1) * 255).astype(np.uint8)


def event_cases():
    """Inputs chosen so that together they reach every event the specification counts (tests assert that they do).  Every
    one is Pillow-comparable: quality, or tables through Pillow's qtables=."""
    both = np.concatenate([checkerboard(32, 48), flat_blocks(32, 48)])
    return [
        # all-ones tables: category 11 DC differences, category 10 AC coefficients, blocks without EOB; 24 intervals: RSTm wraps twice
        ("ones_checker_flat", both, dict(tables=ONES, restart=2)),
        ("ones_checker_rgb", np.stack([checkerboard(16, 24), flat_blocks(16, 24), 255 - checkerboard(16, 24)], -1), dict(tables=ONES, restart=0)),
        # only zigzag 63 survives: three ZRL in front of it; 40 and 63: two ZRL, then one
        ("late_63", noise(11, (40, 40), 108, 149), dict(tables=late_tables(63), restart=0)),
        ("late_40_63_rgb", noise(12, (16, 24, 3), 108, 149), dict(tables=late_tables(40, 63), restart=4)),
        # found by a seeded search over noise at quality 100: two 0xFF in a row; a filled last byte of 0xFF
        ("ff_pair", noise(491, (32, 32)), dict(quality=100, restart=0)),
        ("pad_ff", noise(1, (16, 16)), dict(quality=100, restart=1)),
        # flat: DC category 0; 21 intervals of one MCU
        ("flat_r1", np.full((24, 56), 200, np.uint8), dict(quality=75, restart=1)),
        # 5 x 5 MCUs in intervals of 7: a last interval shorter than the others; of 6: a last interval of one MCU
        ("short_last", noise(13, (40, 40, 3)), dict(quality=50, restart=7)),
        ("last_of_one", smooth((40, 40)), dict(quality=90, restart=6)),
    ]


def golden_cases():
    """What tests/golden/make_jpeg_golden.py records Pillow's files for: the event-rich inputs and plain ones."""
    return event_cases() + [
        ("one_pixel", np.array([[77]], np.uint8), dict(quality=50, restart=0)),
        ("one_pixel_rgb", np.array([[[250, 3, 99]]], np.uint8), dict(quality=90, restart=2)),
        ("grey_noise", noise(21, (37, 45)), dict(quality=90, restart=0)),
        ("grey_smooth", smooth((64, 72)), dict(quality=75, restart=3)),
        ("grey_q10", noise(22, (33, 17)), dict(quality=10, restart=1)),
        ("grey_q1", smooth((17, 33)), dict(quality=1, restart=0)),
        ("grey_row_of_75", smooth((8, 600)), dict(quality=95, restart=75)),
        ("rgb_noise", noise(23, (19, 21, 3)), dict(quality=90, restart=0)),
        ("rgb_smooth", smooth((24, 40, 3)), dict(quality=60, restart=3)),
        ("rgb_q100", noise(24, (16, 16, 3)), dict(quality=100, restart=1)),
        ("rgb_own_tables", noise(25, (9, 7, 3)), dict(tables=np.stack([np.arange(1, 65), np.arange(64, 0, -1) * 3]), restart=5000)),
    ]


def spec_file(image, params):
    return js.encode(image, quality=params.get("quality"), tables=params.get("tables"), restart=params["restart"])


def pillow_file(image, params):
    """The same input through Pillow's libjpeg, baseline, 4:4:4, no optimisation."""
    import io

    from PIL import Image
    kw = dict(optimize=False, subsampling=0, restart_marker_blocks=params["restart"])
    if "quality" in params:
        kw["quality"] = params["quality"]
    else:
        t = np.asarray(params["tables"]).reshape(2, 64)
        kw["qtables"] = [[int(v) for v in row] for row in (t if image.ndim == 3 else t[:1])]
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "JPEG", **kw)
    return buf.getvalue()
