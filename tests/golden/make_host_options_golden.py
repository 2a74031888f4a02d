"""Records tests/golden/host_options_table.txt from a built xrit_demod_host:

    python tests/golden/make_host_options_golden.py PATH/TO/xrit_demod_host

Every command line below is run on a machine WITHOUT a HIP device, behind `--input` naming a file that does not exist.
A line that parse() refuses ends with status 2 and says why in its first stderr line (the usage text follows); a line it
accepts gets as far as the chain's creation, which fails without a device: status 1, no usage text.  The table holds,
tab separated, `refused` or `accepted`, the arguments (none of them holds a blank) and, for a refused line, that first
stderr line.  tests/test_host_options.py replays it against the program as it is built now.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "host_options_table.txt")
MISSING = "/nonexistent/host_options.cf32"

FILES = "--files D --files-decompress"
CANVAS = FILES + " --canvas"
PRODUCTS = CANVAS + " --products"
PROJECT = CANVAS + " --project"

# the flags that take a value: each refused when the command line ends behind it
VALUE_FLAGS = """--input --format --mode --sink --sample-rate --decimation --block --device --connect-tries --diag --queue-symbols
--sndbuf --gpus --fifo-block --fifo-lag --decode --channels --decoder-stats --packets --files --canvas-slots --canvas-mib
--product-tone --product-factor --project-grid --project-mode --tune --acquire-presum --monitor --monitor-block""".split()

ACCEPTED = [
    "--format s16", "--format s8", "--format u8", "--mode hrit", "--sink null", "--sink file:/dev/null", "--sample-rate 1250000",
    "--decimation 5", "--block 200000", "--device 0", "--connect-tries 1", "--diag udp://127.0.0.1:9000", "--drop --queue-symbols 4096",
    "--sndbuf 65536", "--gpus 2", "--fifo", "--fifo --fifo-block 524288 --fifo-lag 3", "--decode P", "--decode P --stream-sync",
    "--decode P --flywheel", "--flywheel 255 --decode P", "--channels D", "--decoder-stats P", "--packets D", "--files D", FILES,
    CANVAS, CANVAS + " --canvas-slots 64 --canvas-mib 4096", PRODUCTS, PRODUCTS + " --product-tone linear",
    PRODUCTS + " --product-tone stretch:100:9900 --product-factor 64", PRODUCTS + " --jpeg", PRODUCTS + " --jpeg 100", PRODUCTS + " --jpeg 1 --stats",
    PROJECT, PROJECT + " --project-grid -135:60:0.1:1200:900", PROJECT + " --project-mode nearest", PRODUCTS + " --project --project-mode bilinear",
    "--tune -12500.5", "--acquire", "--acquire --acquire-presum 64", "--monitor F", "--monitor F --monitor-block 32768", "--front-exact",
    "--front-exact 2", "--front-exact -1", "--paced", "--stats",
]

REFUSED = [flag for flag in VALUE_FLAGS] + [
    "--bogus", "--format f64", "--block 0", "--decimation 0", "--gpus 0",
    "--product-tone cubic", "--product-tone stretch:5", "--product-tone stretch:9000:100", "--product-tone stretch:0:10001",
    "--product-factor x", "--product-factor 0", "--product-factor 65", "--product-factor 8x",
    "--jpeg 0", "--jpeg 101", "--jpeg 9x", "--flywheel 0", "--flywheel 256", "--flywheel 4x",
    "--project-grid 1:2:3", "--project-grid 0:0:0:10:10", "--project-grid 0:0:0.1:0:10", "--project-grid 0:0:0.1:10:16385",
    "--project-grid 0:91:0.1:10:10", "--project-grid 0:0:0.1:10:10x", "--project-mode cubic",
    "--fifo --fifo-block 0", "--fifo --fifo-block 524289", "--fifo --fifo-lag 0", "--fifo --gpus 2",
    "--decode P --drop", "--decode P --gpus 2", "--channels D --drop", "--decoder-stats P --gpus 2", "--packets D --drop",
    "--packets D --gpus 2", "--files D --drop", "--files D --gpus 2", "--stream-sync", "--flywheel", "--files-decompress",
    "--canvas", "--files D --canvas", CANVAS + " --canvas-slots 0", CANVAS + " --canvas-slots 65", CANVAS + " --canvas-mib 0",
    CANVAS + " --canvas-mib 4097", FILES + " --products", CANVAS + " --product-tone linear", CANVAS + " --product-factor 4",
    CANVAS + " --jpeg", FILES + " --project", CANVAS + " --project-mode nearest", CANVAS + " --project-grid -135:60:0.1:1200:900",
    "--tune 100 --gpus 2", "--tune 100 --format u8", "--acquire --format u8", "--acquire --acquire-presum 0", "--acquire --acquire-presum 65",
    "--monitor F --gpus 2", "--monitor F --monitor-block 0", "--monitor F --monitor-block 32832", "--monitor F --monitor-block 100",
]


def run(host_bin, args):
    r = subprocess.run([host_bin, "--input", MISSING] + args.split(), capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


def main():
    host_bin = sys.argv[1]
    lines = []
    for args in ACCEPTED:
        status, err = run(host_bin, args)
        assert status == 1 and "usage:" not in err, (args, status, err[:200])
        lines.append("accepted\t%s\t" % args)
    for args in REFUSED:
        status, err = run(host_bin, args)
        assert status == 2 and "usage:" in err, (args, status, err[:200])
        lines.append("refused\t%s\t%s" % (args, err.splitlines()[0]))
    with open(TABLE, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d lines -> %s" % (len(lines), TABLE))


if __name__ == "__main__":
    main()
