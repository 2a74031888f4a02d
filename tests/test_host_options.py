"""CPU tier: the host program's command line, replayed from tests/golden/host_options_table.txt (recorded by
tests/golden/make_host_options_golden.py from the program as it was before it was split in pieces): every line parse()
refuses ends with status 2 and the recorded reason in front of the usage text, every line it accepts gets as far as the
chain's creation, which fails without a device: status 1, no usage text."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BIN = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
TABLE = os.path.join(ROOT, "tests", "golden", "host_options_table.txt")


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    if not os.path.exists(xritdemod_amd.lib_path()):
        xritdemod_amd.build()
    xritdemod_amd.lib()
    return xritdemod_amd


def table():
    with open(TABLE) as f:
        return [tuple(line.rstrip("\n").split("\t")) for line in f if line.strip()]


def test_table_holds_every_flag_and_refusal():
    rows = table()
    assert len(rows) >= 80 and {r[0] for r in rows} == {"accepted", "refused"}
    needs = [r for r in rows if r[0] == "refused" and r[2].endswith(" needs a value")]
    assert len(needs) == 30 and all(r[2] == r[1] + " needs a value" for r in needs)
    said = {r[2] for r in rows if r[0] == "refused"}
    for rule in ("--fifo:", "--decode:", "--channels / --decoder-stats:", "--packets:", "--files:", "--stream-sync needs", "--files-decompress needs",
                 "--canvas needs", "--products needs", "--jpeg needs", "--project needs", "--tune / --acquire:", "--monitor:", "unknown option",
                 "--jpeg 0: 1..100", "--jpeg 101: 1..100", "--flywheel 256: 1..255", "--product-factor x: 1..64", "--project-mode cubic:",
                 "--product-tone cubic:", "--project-grid 1:2:3:", "usage: xrit_demod_host"):
        assert any(s.startswith(rule) for s in said), rule


def test_host_program_check_under_sanitizers(tmp_path):
    """make host-program-check: the program's plain parts (host/source.h, sinks.h, outputs.h) in a stand-alone g++ program
    with -fsanitize=address,undefined, in a temporary directory."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "host-program-check",
                        f"HOST_PROGRAM_CHECK={tmp_path / 'host_program_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_program_check: ok" in r.stdout, r.stdout


@pytest.mark.parametrize("row", table(), ids=lambda r: (r[0] + " " + r[1]).replace(" ", "_"))
def test_host_program_command_line(xa, tmp_path, row):
    if xa.device_count() > 0:
        pytest.skip("with a device an accepted line would run; the CPU tier checks the command line")
    assert os.path.exists(HOST_BIN), "make -C xritdemod_amd/csrc builds it"
    verdict, args, said = row
    r = subprocess.run([HOST_BIN, "--input", str(tmp_path / "missing.cf32")] + args.split(), capture_output=True, text=True, timeout=60)
    if verdict == "refused":
        assert r.returncode == 2 and r.stderr.splitlines()[0] == said, r.stderr[:300]
        assert "usage: xrit_demod_host" in r.stderr
    else:
        assert r.returncode == 1 and "usage:" not in r.stderr, r.stderr[:300]
