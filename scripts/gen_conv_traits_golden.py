"""Writes tests/golden/conv_traits.json: what the ten layer predicates of mdctgan_amd/ops.py (tiles_are_casts, precast_ok,
weights_are_casts, wino_images_half, wino_vnext_ok, wino_vnext_positions, wino_md_from_norm_ok, wgrad_checks_finite, wgrad_h16_ok,
wgrad_adam_ok) answer for every case of tests/test_conv_traits_host.py, each under the case's own environment and with a cold memo.
A predicate that raises (a gradient pass asked about on a forward-only route, before ops.traits) is recorded as null.  Needs no GPU.

    python scripts/gen_conv_traits_golden.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import pytest  # noqa: E402
import test_conv_traits_host as T  # noqa: E402


def main():
    from mdctgan_amd import ops
    mp = pytest.MonkeyPatch()
    cases, raised = {}, 0
    try:
        for key, shape, prec, env in T.traits_cases():
            T.apply_env(mp, env)
            for memo in ("_CASTS", "_TRAITS"):          # fresh answers, whichever memo the tree under the script keeps
                getattr(ops, memo, {}).clear()
            cases[key] = T.views(T.P.geom_of(shape, prec), raised=(NotImplementedError,))
            raised += sum(v is None for v in cases[key])
    finally:
        mp.undo()
    with open(T.GOLDEN, "w") as f:
        json.dump({"views": list(T.VIEWS), "cases": cases}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(len(cases), "cases,", raised, "answers raised,", os.path.getsize(T.GOLDEN), "bytes ->", T.GOLDEN)


if __name__ == "__main__":
    main()
