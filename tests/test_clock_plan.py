"""The clock recovery's plain host parts (csrc/clock_plan.h, csrc/clock_ctl.h): no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clock_plan_host_check_under_sanitizers(tmp_path):
    """make clock-host-check: the plan of a call (chain geometry, relay segments, overlap ranges) over a grid of configurations and
    call sizes against the table recorded before the arithmetic left ClockStage::begin(), the looks at the control block row by
    row, and the numbers DESIGN.md quotes -- in a stand-alone g++ program with -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "clock-host-check",
                        f"CLOCK_CHECK={tmp_path / 'clock_host_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clock_host_check: 202 cases spelled out, 48 configurations summed, the looks and the documented numbers: ok" in r.stdout, r.stdout
