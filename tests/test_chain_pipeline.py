"""The chain handle's in-flight pipeline and the clock stage's bookkeeping as plain host code (csrc/chain_pipeline.h,
csrc/clock_jobs.h): no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xritdemod_amd", "csrc")


def test_chain_pipeline_host_check_under_sanitizers(tmp_path):
    """make chain-host-check: scripts of registrations, process calls and resets -- the plans of the streamed GPU tests, the chains
    path with the relay on and off, queues that mix the two paths, a Costas loop that goes on from the host, every misuse the ABI
    rejects -- through chain_pipeline.h, call for call against tests/golden/chain_pipeline_table.txt (recorded from the control flow
    the header was taken out of), the pipeline's invariants over every step, and one row per branch of chain_next; the clock
    stage's bookkeeping under the same scripts and its own (csrc/clock_jobs.h), step for step against
    tests/golden/clock_jobs_table.txt (recorded from the ClockStage methods it was taken out of), one row per branch of its
    decisions, and the count of accesses to a sample buffer, a curve, the carried state or a job's records that neither a
    stream, an event nor the host orders behind the access before -- in a stand-alone g++ program with
    -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", CSRC, "chain-host-check", f"CHAIN_CHECK={tmp_path / 'chain_host_check'}"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("chain_host_check: 34 scripts, 2191 logged calls against the recorded table, 1 known invariant breaks, "
            "0 walker waits behind another input's event, 32 rule rows; clock jobs: 47 scripts, 1412 rows against the recorded table, "
            "0 known differences, 31 rule rows, 0 accesses ordered by nothing: ok") in r.stdout, r.stdout


def test_chain_pipeline_header_is_plain_cpp(tmp_path):
    """chain_pipeline.h compiles alone with g++ -Wall -Wextra and pulls in no HIP header."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "only.cpp"
    src.write_text('#include "chain_pipeline.h"\nint main() { xrit::ChainQueue q; return q.count; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-H", "-fsyntax-only", str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hip_runtime" not in r.stderr and "/hip/" not in r.stderr, r.stderr


def test_clock_jobs_header_is_plain_cpp(tmp_path):
    """clock_jobs.h compiles alone with g++ -Wall -Wextra -Werror and pulls in no HIP header."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "only.cpp"
    src.write_text('#include "clock_jobs.h"\nint main() { xrit::ClockJobs c; return c.pick_buffer().b == 1 ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-H", "-fsyntax-only", str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hip_runtime" not in r.stderr and "/hip/" not in r.stderr, r.stderr
