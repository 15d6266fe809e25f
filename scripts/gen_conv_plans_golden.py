"""Writes tests/golden/conv_plans.json: what the loaded library (MDCTGAN_HIP_LIB, else the tree's) answers about every geometry
of tests/test_conv_plan_golden_host.py.  Needs no GPU.

    python scripts/gen_conv_plans_golden.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import pytest  # noqa: E402
import test_conv_plan_golden_host as T  # noqa: E402


def main():
    mp = pytest.MonkeyPatch()
    try:
        cases = T.collect(mp)
    finally:
        mp.undo()
    with open(T.GOLDEN, "w") as f:
        json.dump({"fields": [list(T.FIELDS), list(T.LAYER_FIELDS)], "cases": cases}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(len(cases), "cases,", os.path.getsize(T.GOLDEN), "bytes ->", T.GOLDEN)


if __name__ == "__main__":
    main()
