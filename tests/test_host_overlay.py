"""CPU tier: the host program's --overlay, --graticule and --overlay-width on the command line, replayed from
tests/golden/host_overlay_table.txt the way tests/test_host_files_jpeg.py replays its table (the older tables stay as they
are): a line parse() refuses ends with status 2 and the recorded reason in front of the usage text; a line it accepts gets
as far as the chain's creation, which fails without a device: status 1, no usage text.  DIR in a line is a temporary
directory.  The options' plain parts and the polyline text (host/overlay_files.h) are held by make host-program-check; here
the specification's reading of such text is held to the same cases."""
import math
import os
import shutil
import subprocess

import pytest

import overlay_spec as ovs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_BIN = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
TABLE = os.path.join(ROOT, "tests", "golden", "host_overlay_table.txt")


def table():
    with open(TABLE) as f:
        return [tuple(line.rstrip("\n").split("\t")) + ("",) * (3 - len(line.rstrip("\n").split("\t"))) for line in f if line.strip()]


def test_table_holds_the_options_rules():
    rows = table()
    assert sum(r[0] == "accepted" for r in rows) >= 5 and sum(r[0] == "refused" for r in rows) >= 10
    said = {r[2] for r in rows if r[0] == "refused"}
    assert {"--overlay / --graticule need --products", "--overlay-width needs --overlay or --graticule", "--overlay needs a value",
            "--graticule 91: 0.1..90 degrees", "--overlay-width 9: 1..8"} <= said
    usage = subprocess.run([HOST_BIN], capture_output=True, text=True, timeout=60).stderr
    assert "[--overlay FILE] [--graticule DEG] [--overlay-width W]" in usage and "(255, 255, 0)" in usage and "(0, 255, 255) at 160 / 255" in usage
    assert ".view.map.ppm" in usage and ".geo.view.map.ppm" in usage


@pytest.mark.parametrize("row", table(), ids=lambda r: (r[0] + " " + r[1]).replace(" ", "_"))
def test_host_program_overlay_command_line(tmp_path, row):
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


def test_polyline_text_of_the_specification():
    """The cases csrc/host_program_check.cpp holds host/overlay_files.h to."""
    lon, lat = ovs.parse_polylines("> first\n-75.5 10\n  -74\t11.25  \r\n\n# note\n1e1 -2.5e0\n>\n3 4")
    nan = math.nan
    assert [(a, b) if not math.isnan(a) else None for a, b in zip(lon, lat)] == [None, (-75.5, 10.0), (-74.0, 11.25), None, None, (10.0, -2.5), None, (3.0, 4.0)]
    assert math.isnan(nan) and len(ovs.parse_polylines("")[0]) == 0 and len(ovs.parse_polylines("1 2\n")[0]) == 1 and len(ovs.parse_polylines("1 2\n\n")[0]) == 2
    for text, line in (("1 2\n3\n", 2), ("1 2 3", 1), ("1,2", 1), ("1 2\n>\nlon lat\n", 3), ("1 nan", 1), ("inf 2", 1), ("1 2x", 1), ("\n\n\n4 5 # east", 4)):
        assert ovs.parse_polylines(text) == ("error", line), text


def test_host_program_check_holds_the_overlay_s_plain_parts(tmp_path):
    """make host-program-check (under -fsanitize=address,undefined) covers host/overlay_files.h."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = open(os.path.join(ROOT, "xritdemod_amd", "csrc", "host_program_check.cpp")).read()
    assert '#include "../host/overlay_files.h"' in src and "check_overlay_files()" in src
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "xritdemod_amd", "csrc"), "host-program-check",
                        f"HOST_PROGRAM_CHECK={tmp_path / 'host_program_check'}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "host_program_check: ok" in r.stdout, r.stdout + r.stderr
