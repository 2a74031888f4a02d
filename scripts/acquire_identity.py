"""The carrier acquisition's device form on every case of tests/acquire_cases.py, from the library of the tree given as the
argument: one line per case with the bytes of xrit_acquire_estimate_record that estimate(apply=True) wrote in device memory
and the bytes of xrit_acquire_state after it, in hex.  Run it once per tree, each in a process of its own, and compare the
lines (profiles/wave_ops_identity.txt):

    python scripts/acquire_identity.py <tree> > a.txt;  python scripts/acquire_identity.py <other tree> > b.txt;  diff a.txt b.txt
"""
import os
import sys

ROOT = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import xritdemod_amd as xa
import acquire_cases as ac

assert os.path.abspath(xa.__file__).startswith(ROOT + os.sep), xa.__file__
for name in sorted(ac.CASES):
    c = ac.CASES[name]
    x = ac.samples(name)
    sample_type = ac.sample_type(name)
    n = len(x) // 2 if c.get("s16") else len(x)
    d_x = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    d_rec = torch.zeros(xa.ACQUIRE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    aq = xa.CarrierAcquirer(c["fs"], pre_sum=c["pre_sum"])
    aq.estimate_device(d_x.data_ptr(), n, sample_type, True, d_rec.data_ptr())
    state = aq.state()                      # waits for the call
    torch.cuda.synchronize()
    rec = d_rec.cpu().numpy()
    r = rec.view(xa.ACQUIRE_RECORD_DTYPE)[0]
    print(f"{name}: record {rec.tobytes().hex()} state {state.tobytes().hex()} (status {int(r['status'])} k0 {int(r['k0'])} hz {float(r['hz'])!r})")
    aq.close()
