"""The FIR stage's launch plan (csrc/fir_plan.h): no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fir_plan_host_check_under_sanitizers(tmp_path):
    """make fir-host-check: 15 tap counts x 69 decimations x both summation orders (and the chain's two static filters with
    their switches set) through fir_plan(), each row equal in every field to the table recorded from FirStage::init and
    FirStage::run before the plan left them (tests/golden/fir_plan_table.txt), and each plan held to what its launch needs:
    the key an existing kernel instance with the plan's per-lane count and skew, the tile as long as the furthest read, the
    tap image of the size the form walks, LDS within the limits -- in a stand-alone g++ program with
    -fsanitize=address,undefined.  The 390 exact rows at odd decimations from 17 up are not the table's (the recorded launch
    read past its taps and its tile): the program requires the generic exact kernel there.  The counts per form are those of
    an independent walk of the same grid (fast: 15 + 479 + 471 window walks, 34 polyphase, 36 too large for LDS; exact: 15 + 105
    + 45 + 225 shared walks, 255 + 390 generic), plus the twelve rows with the switches."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "fir-host-check",
                        f"FIR_CHECK={tmp_path / 'fir_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("fir_host_check: 2082 rows (window walk 971, exact walk 396, generic exact 645 of which 390 at odd decimations from 17 "
            "up, polyphase 34, 36 do not fit LDS), every plan's key an instance sized like its tile and taps: ok") in r.stdout, r.stdout
