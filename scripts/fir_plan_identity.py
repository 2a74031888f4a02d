#!/usr/bin/env python3
"""Two builds of libxritdemod_amd.so on the same inputs: do the FIR stage and the chains around it compute the same words?

    python scripts/fir_plan_identity.py PARENT_LIB TREE_LIB [--out FILE]

Needs a HIP device.  Every part runs PARENT_LIB, TREE_LIB and PARENT_LIB a second time (what varies without any change),
each in a child process of its own, one at a time under `timeout -k 10`; the first child that does not end with status 0
(a signal, 124, 134, 137 or 139 among them) ends the script, nothing is tried again.  A child records a SHA-256 per output,
the parent compares.

stages: xrit_fir_work at decimations 1 2 3 4 5 6 7 8 12 16 18 32 64 with the taps of the stage tests, fast and exact order,
        calls of 30000, 1, 777, 0, 12345 and 3 outputs.
chains: C1, C2, C3, C5; bursts of 300 k symbols as cf32 and, where there is a decimator, s16 and s8, with front_exact 0, 2
        and -1; bursts of 1.1 M symbols as cf32 with front_exact 0 and 2.  The soft symbols bit for bit and every field of the
        statistics.  Behind a decimator the burst is the 1.25 Msps (C3: 2.5 Msps) burst with every sample repeated D times.
No case has an odd decimation from 17 up: the exact order's launch there read out of bounds before fir_plan.h.
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGE_D = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 18, 32, 64)
CASES = {"C1": ("lrit", 1.25e6, 1, {}), "C2": ("lrit", 6.25e6, 5, {}),
         "C3": ("hrit", 2.5e6, 1, {"symbol_rate": 927000.0, "alpha": 0.3}), "C5": ("lrit", 40e6, 32, {})}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def burst(case, symbols):
    import synth
    mode, fs, D, kw = CASES[case]
    rate = kw.get("symbol_rate", 293883.0)
    kept = os.path.join(os.environ.get("FIR_IDENTITY_BURSTS", ""), "%s_%d.npy" % (case, symbols))      # shared by the children
    if os.path.exists(kept):
        x = np.load(kept)
    else:
        x = synth.generate(synth.SynthParams(fs_in=fs / D, **kw), int(symbols * fs / D / rate))
        if os.path.isdir(os.path.dirname(kept)):
            np.save(kept, x)
    return np.repeat(x, D) if D > 1 else x


def as_type(x, sample_type):
    """cf32 -> (array, sample type) as s16 (1) or s8 (2) interleaved IQ."""
    if sample_type == 0:
        return x
    v = np.ascontiguousarray(x).view(np.float32) / max(1e-9, float(np.abs(x).max()))
    return np.round(v * 20000).astype(np.int16) if sample_type == 1 else np.round(v * 100).astype(np.int8)


def child_stages(xa, o, out):
    taps = {"rrc": o.rrc_taps(1, 1.25e6, 293883, 0.5, 63), "lp5": o.lowpass_taps(1, 6.25e6, 625e3, 100e3),
            "lp32": o.lowpass_taps(1, 40e6, 625e3, 100e3), "short": np.array([0.5, -0.25, 0.125], np.float32),
            "lp16": o.lowpass_taps(1, 20e6, 625e3, 100e3), "one": np.array([0.75], np.float32)}
    n_out = [30000, 1, 777, 0, 12345, 3]
    for D in STAGE_D:
        rng = np.random.default_rng(100 + D)
        x = (rng.standard_normal(sum(n_out) * D) + 1j * rng.standard_normal(sum(n_out) * D)).astype(np.complex64)
        for kind in taps:
            for exact in (False, True):
                f, pos, h = xa.FirFilter(D, taps[kind], exact=exact), 0, hashlib.sha256()
                for n in n_out:
                    h.update(f.Work(x[pos:pos + n * D], n).tobytes())
                    pos += n * D
                out["fir D=%d %s %s" % (D, kind, "exact" if exact else "fast")] = h.hexdigest()[:24]


def chain_run(xa, case, x, sample_type, front_exact):
    mode, fs, D, _ = CASES[case]
    dem = xa.Demodulator(xa.Demodulator.config(mode, fs, D, front_exact=front_exact))
    soft = dem.process(as_type(x, sample_type), sample_type)
    st = dem.stats()
    return {"soft": sha(soft), "symbols": len(soft), "stats": {nm: getattr(st, nm) for nm, _ in st._fields_}}


def child_chains(xa, o, out):
    for case, (mode, fs, D, _) in CASES.items():
        print("    %s" % case, flush=True)
        x = burst(case, 300_000)
        for sample_type in ((0, 1, 2) if D > 1 else (0,)):
            for fe in (0, 2, -1):
                out["%s 300k type %d front_exact %d" % (case, sample_type, fe)] = chain_run(xa, case, x, sample_type, fe)
        x = burst(case, 1_100_000)
        for fe in (0, 2):
            out["%s 1.1M type 0 front_exact %d" % (case, fe)] = chain_run(xa, case, x, 0, fe)


def child(lib, part, dump):
    import xritdemod_amd as xa
    from xritdemod_amd import _capi
    _capi._LIB = os.path.abspath(lib)
    xa.lib()
    if xa.device_count() < 1:
        sys.exit("needs a HIP device")
    import oracle
    out = {}
    {"stages": child_stages, "chains": child_chains}[part](xa, oracle, out)
    with open(dump, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True, default=float)


class Fatal(Exception):
    pass


def run_child(lib, part, work, tag, seconds):
    dump = os.path.join(work, "%s_%s.json" % (part, tag))
    argv = [sys.executable, os.path.abspath(__file__), "--child", lib, "--part", part, "--dump", dump]
    print("  %s of %s ..." % (part, lib), flush=True)      # (the child's own output goes straight through)
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + argv, env=dict(os.environ, FIR_IDENTITY_BURSTS=work))
    if r.returncode != 0:
        raise Fatal("status %d from %s part %s" % (r.returncode, lib, part))
    with open(dump) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?")
    ap.add_argument("tree", nargs="?")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--part", default=None)
    ap.add_argument("--dump", default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child, o.part, o.dump)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    work = tempfile.mkdtemp(prefix="fir_identity_")
    ok = True
    try:
        say("# libxritdemod_amd.so: parent (%s) against tree (%s), one MI355X, one child process at a time" % (o.parent, o.tree))
        for part, seconds in (("stages", 300), ("chains", 900)):
            a, b, c = (run_child(lib, part, work, tag, seconds) for lib, tag in ((o.parent, "p1"), (o.tree, "t"), (o.parent, "p2")))
            different = [k for k in sorted(a) if a[k] != b.get(k)] + [k for k in sorted(b) if k not in a]
            varying = [k for k in sorted(a) if a[k] != c.get(k)]
            for k in sorted(a):
                note = ", %d symbols" % a[k]["symbols"] if isinstance(a[k], dict) else ""
                say("%s | %s%s: %s%s" % (part, k, note, "IDENTICAL" if k not in different else "DIFFERENT",
                                       " (parent against itself: DIFFERENT)" if k in varying else ""))
            say("%s: cases %d, different %d; parent run 1 against parent run 2: different %d" % (part, len(a), len(different), len(varying)))
            ok = ok and not different
    except Fatal as e:
        say("STOPPED: %s" % e)
        ok = False
    finally:
        shutil.rmtree(work, ignore_errors=True)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
