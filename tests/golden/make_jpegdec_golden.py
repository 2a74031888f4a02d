"""Writes tests/golden/jpegdec_rule_table.txt (the specification's table for make jpegdec-host-check) and
tests/golden/jpegdec_pil.npz: the streams Pillow's libjpeg writes for tests/jpegdec_cases.py's pillow_cases() and
unsupported_cases(), and Pillow's own pixels for the sound ones (libjpeg's slow-integer inverse DCT, its default).  Run
from the repository root where Pillow is installed: python tests/golden/make_jpegdec_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpegdec_cases as dc  # noqa: E402


def main():
    names, files, arrays = [], [], {}
    for name, image, kw, tail in dc.pillow_cases():
        data = dc.pillow_write(image, kw, tail)
        arrays["pixels_%02d" % len(names)] = dc.pillow_read(data)
        names.append(name)
        files.append(data)
    for name, image, mode, kw in dc.unsupported_cases():
        names.append(name)
        files.append(dc.pillow_write(image, kw, mode=mode))
    assert len(names) <= 64
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "jpegdec_pil.npz"), names=np.array(names), data=np.frombuffer(b"".join(files), np.uint8), offsets=offsets,
                        **arrays)
    print(len(names), "streams,", int(offsets[-1]), "bytes")
    # the table csrc/jpegdec_host_check.cpp replays, from the specification on those streams
    import jpegdec_spec as ds
    with open(os.path.join(HERE, "jpegdec_rule_table.txt"), "w") as f:
        f.write(ds.rule_table_text(*dc.rule_table_inputs(dc.Golden())))


if __name__ == "__main__":
    main()
