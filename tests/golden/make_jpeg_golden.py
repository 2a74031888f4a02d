"""Writes tests/golden/jpeg_pil_files.npz: the files Pillow's libjpeg writes (baseline, 4:4:4, optimize=False) for the
inputs of tests/jpeg_cases.py's golden_cases -- what holds the specification (tests/jpeg_spec.py), and through it the
device, to an outside implementation on machines without Pillow.  Needs Pillow; deterministic:
    python tests/golden/make_jpeg_golden.py

Recorded with Pillow 12.2.0, libjpeg-turbo (PIL.features.version("jpg")) 6.2.  The recorder refuses to write a file that
differs from the specification's, and prints the versions it ran with; the file keeps them under "versions".

The file holds, per case in golden_cases' order, the name, the image (uint8, as given to both encoders) and the file's
bytes, the files back to back with their offsets."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_cases as jc  # noqa: E402

PATH = os.path.join(HERE, "jpeg_pil_files.npz")
MAX_BYTES = 64 * 1024


def make():
    import PIL
    from PIL import features
    arrays, files, names = {}, [], []
    for i, (name, image, params) in enumerate(jc.golden_cases()):
        theirs = jc.pillow_file(image, params)
        ours, _ = jc.spec_file(image, params)
        assert theirs == ours, name
        names.append(name)
        files.append(theirs)
        arrays["image_%02d" % i] = image
    arrays["names"] = np.array(names)
    arrays["offsets"] = np.cumsum([0] + [len(f) for f in files]).astype(np.uint32)
    arrays["data"] = np.frombuffer(b"".join(files), np.uint8)
    arrays["versions"] = np.array(["Pillow " + PIL.__version__, "libjpeg " + str(features.version("jpg"))])
    return arrays


if __name__ == "__main__":
    arrays = make()
    print(list(arrays["versions"]), len(arrays["names"]), "files,", len(arrays["data"]), "bytes of them")
    np.savez_compressed(PATH, **arrays)
    size = os.path.getsize(PATH)
    print(PATH, size, "bytes")
    assert size <= MAX_BYTES, size
