"""Writes tests/golden/overlay_rule_table.txt: the specification's table (tests/overlay_spec.py, rule_table_text) that
make overlay-host-check replays through csrc/overlay_rule.h.  Run from the repository root:
python tests/golden/make_overlay_golden.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import overlay_spec as ovs  # noqa: E402


def main():
    text = ovs.rule_table_text()
    with open(os.path.join(HERE, "overlay_rule_table.txt"), "w") as f:
        f.write(text)
    print(text.count("\n"), "rows")


if __name__ == "__main__":
    main()
