"""GPU tier: xrit_demod_host --flywheel.  A capture whose 12 frames hold the planted sync word of tests/lock_cases.py,
behind four plain frames in which the demodulator settles; the symbols the program sends to its TCP sink are walked by
the specification, and the VCDUs it decodes with and without the flywheel must be the specification's."""
import os
import socket
import subprocess
import threading

import numpy as np
import pytest

import ccsds
import framer_cases as fc
import lock_cases as lc
import lock_spec as ls
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BIN = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")


def run_host(capture, extra, timeout=300):
    """The program on the capture with a listening socket as its sink: (the finished process, the symbols it sent)."""
    srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    srv.bind(("127.0.0.1", 0))
    srv.listen(1)
    port = srv.getsockname()[1]
    got = bytearray()

    def serve():
        conn, _ = srv.accept()
        while True:
            b = conn.recv(65536)
            if not b:
                break
            got.extend(b)
        conn.close()

    th = threading.Thread(target=serve)
    th.start()
    r = subprocess.run([HOST_BIN, "--input", str(capture), "--mode", "lrit", "--sample-rate", "1250000", "--block", "200000",
                        "--sink", f"tcp://127.0.0.1:{port}"] + extra, capture_output=True, text=True, timeout=timeout)
    th.join(timeout=30)
    srv.close()
    return r, np.frombuffer(bytes(got), np.int8)


def test_flywheel_keeps_the_frames_the_plain_stream_sync_loses(oracle_mod, tmp_path):
    import xritdemod_amd
    assert xritdemod_amd.device_count() >= 1 and os.path.exists(HOST_BIN)
    warm, _ = fc.coded_frames(4, np.random.default_rng(21))
    stream, _ = lc.stream_a(plants=(2,))
    sym = np.concatenate([warm.reshape(-1), stream]).astype(np.float64) / 100.0
    p = synth.SynthParams(fs_in=1.25e6, seed=21)
    synth.generate(p, int((len(sym) + 64) * p.sps_in), symbols=sym).tofile(tmp_path / "iq.cf32")
    out, sent_symbols = {}, None
    for tag, extra in (("fly", ["--flywheel"]), ("plain", ["--stream-sync"])):
        r, symbols = run_host(tmp_path / "iq.cf32", ["--decode", str(tmp_path / (tag + ".bin"))] + extra)
        assert r.returncode == 0, (tag, r.stderr)
        out[tag] = (np.fromfile(tmp_path / (tag + ".bin"), np.uint8).reshape(-1, 892), r.stderr)
        assert sent_symbols is None or np.array_equal(symbols, sent_symbols)         # the same symbols both times
        sent_symbols = symbols
    assert "lock:" in out["fly"][1] and "lock:" not in out["plain"][1]
    # what the specification decodes from the symbols the program had (however it cut them into calls)
    cache = {}
    for tag, recheck in (("fly", 4), ("plain", 1)):
        rows, _, _ = ls.walk(sent_symbols, recheck=recheck, cache=cache)
        good = rows.block[(rows.info["ok"] != 0)][:, :892]
        assert np.array_equal(out[tag][0], good), tag
    # the 12 frames behind the settling: all of them with the flywheel, frames 2 and 3 lost without it
    sent = {v.tobytes(): i for i, v in enumerate(lc.sent_vcdus())}
    found = {tag: [sent[v.tobytes()] for v in out[tag][0] if v.tobytes() in sent] for tag in out}
    print(out["fly"][1], out["plain"][1], found)
    assert found["fly"] == list(range(12))
    assert found["plain"] == [0, 1] + list(range(4, 12))
