"""CPU tier: the host program's --files-jpeg on the command line, replayed from tests/golden/host_files_jpeg_table.txt (the
older table, tests/golden/host_options_table.txt, stays as it is and is replayed by tests/test_host_options.py): a line
parse() refuses ends with status 2 and the recorded reason in front of the usage text; a line it accepts gets as far as
the chain's creation, which fails without a device: status 1, no usage text.  DIR in a line is a temporary directory.
The option's plain parts (host/jpeg_files.h) are held by make host-program-check, which tests/test_host_options.py runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BIN = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
TABLE = os.path.join(ROOT, "tests", "golden", "host_files_jpeg_table.txt")


def table():
    with open(TABLE) as f:
        return [tuple(line.rstrip("\n").split("\t")) + ("",) * (3 - len(line.rstrip("\n").split("\t"))) for line in f if line.strip()]


def test_table_holds_the_flag_s_rules():
    rows = table()
    assert sum(r[0] == "accepted" for r in rows) >= 6 and all("--files-jpeg" in r[1] for r in rows[:-1]) and "--files-jpeg" not in rows[-1][1]
    said = {r[2] for r in rows if r[0] == "refused"}
    assert {"--files-jpeg needs --files DIR", "unknown option 90", "--files: one GPU, without --drop"} <= said
    usage = subprocess.run([HOST_BIN], capture_output=True, text=True, timeout=60).stderr
    assert "[--files-jpeg]" in usage and "compression 2" in usage


@pytest.mark.parametrize("row", table(), ids=lambda r: (r[0] + " " + r[1]).replace(" ", "_"))
def test_host_program_files_jpeg_command_line(tmp_path, row):
    import xritdemod_amd as xa
    xa.lib()
    if xa.device_count() > 0:
        pytest.skip("with a device an accepted line would run; the CPU tier checks the command line")
    verdict, args, said = row
    argv = [str(tmp_path / "out") if a == "DIR" else a for a in args.split()]
    r = subprocess.run([HOST_BIN, "--input", str(tmp_path / "missing.cf32")] + argv, capture_output=True, text=True, timeout=60)
    if verdict == "refused":
        assert r.returncode == 2 and r.stderr.splitlines()[0] == said, r.stderr[:300]
        assert "usage: xrit_demod_host" in r.stderr
    else:
        assert r.returncode == 1 and "usage:" not in r.stderr, r.stderr[:300]
