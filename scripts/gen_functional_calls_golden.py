"""Writes tests/golden/functional_calls.json: the launcher calls, grad-ready notifications and per-parameter gradient flags of the
five scenarios of tests/functional_calls.py (float32, fp16, fp16_checked, bare, fused_tail), as the tree under the script makes them.  Run it on the commit whose behaviour is to be
kept, commit the file unchanged.  Needs a GPU.

    python scripts/gen_functional_calls_golden.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import functional_calls as R  # noqa: E402


def main(path=R.GOLDEN):
    traces = {name: R.normal(run()) for name, run in R.SCENARIOS.items()}
    doc = R.pack(traces)
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in traces.items()}, "records,", len(doc["records"]), "distinct,", os.path.getsize(path), "bytes ->", path)


if __name__ == "__main__":
    main(*sys.argv[1:])
