"""Every answer the C ABI gives about a convolution from its geometry alone -- kernel instance, K splits, launch order, FLOPs,
workspace and image sizes, the four capability queries -- pinned to tests/golden/conv_plans.json for every case of
test_conv_plan_coverage_host.walk_cases() (with the case's planner hooks applied as that test applies them) and for the full-size
layers of BASELINE configs[1], [2] and [4] (test_fullsize_gpu's tables) in both precisions.  On the host, no GPU.
scripts/gen_conv_plans_golden.py writes the file; a change of host code that is meant to leave every plan alone leaves it alone."""
import ctypes
import json
import os

import test_conv_plan_coverage_host as cov
import test_conv_plans_gpu as P
import test_fullsize_gpu as full

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.json")
FIELDS = ("name", "splits", "order", "flops", "workspace")        # per pass
LAYER_FIELDS = ("fwd_instnorm_workspace", "wino_weights_bytes", "wino_tiles_bytes", "wgrad_adam_ok", "wgrad_checks_finite",
                "wino_md_from_norm_ok", "wino_vnext_ok")


def golden_cases():
    """(key, shape (B, Ci, H, W, Co, k, stride, pad, reflect), precision, planner hooks), each distinct combination once."""
    seen = set()
    cases = [(shape, prec, env) for shape, prec, env, _ in cov.walk_cases()]
    for table in (full.SHAPES, full.SHAPES_CFG2, full.SHAPES_CFG4):
        for name, B, H, W, Ci, Co, k, s, p, reflect in table:
            cases += [((B, Ci, H, W, Co, k, s, p, reflect), prec, {}) for prec in (cov.F32, cov.F16)]
    for shape, prec, env in cases:
        key = "%s|f%d|%s" % (",".join(str(int(v)) for v in shape), 16 if prec else 32,
                             ";".join("%s=%s" % kv for kv in sorted(env.items())))
        if key not in seen:
            seen.add(key)
            yield key, tuple(shape), prec, env


def answers(g):
    """What the library says about geometry g under the current environment."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(96)
    passes = []
    for ps, ws in enumerate((lib.mg_conv_fwd_workspace, lib.mg_conv_dgrad_workspace, lib.mg_conv_wgrad_workspace)):
        assert lib.mg_conv_plan_name(ps, g, buf, 96) == 0
        passes.append([buf.value.decode(), int(lib.mg_conv_plan_splits(ps, g)), list(P.plan_order(ps, g)),
                       float(lib.mg_conv_plan_flops(ps, g)), int(ws(g))])
    return {"passes": passes,
            "layer": [int(lib.mg_conv_fwd_instnorm_workspace(g)), int(lib.mg_conv_wino_weights_bytes(g)),
                      [int(lib.mg_conv_wino_tiles_bytes(g, 0)), int(lib.mg_conv_wino_tiles_bytes(g, 1))],
                      int(lib.mg_conv_wgrad_adam_ok(g)), int(lib.mg_conv_wgrad_checks_finite(g)),
                      int(lib.mg_conv_wino_md_from_norm_ok(g)), int(lib.mg_conv_wino_vnext_ok(g))]}


def collect(monkeypatch):
    out = {}
    for key, shape, prec, env in golden_cases():
        P.apply_env(monkeypatch, env)
        out[key] = answers(P.geom_of(shape, prec))
    return out


def test_conv_plans_are_the_recorded_ones(monkeypatch):
    # (MG_HALF_NBUF, MG_NO_BK32 and the MG_NO_WINOGRAD* switches are read once per process, the other two are no planner hooks
    # that apply_env clears: the file is that of the default build)
    for key in ("MG_HALF_NBUF", "MG_NO_BK32", "MG_NO_WINOGRAD", "MG_NO_WINOGRAD4", "MG_NO_WINOGRAD42", "MG_NO_HGEMM_SA",
                "MG_HGEMM_AS_GROUPS"):
        assert key not in os.environ, key
    with open(GOLDEN) as f:
        want = json.load(f)
    got = collect(monkeypatch)
    assert sorted(got) == sorted(want["cases"])
    assert want["fields"] == [list(FIELDS), list(LAYER_FIELDS)]
    wrong = [(key, got[key], want["cases"][key]) for key in sorted(got) if got[key] != want["cases"][key]]
    assert not wrong, (len(wrong), wrong[:3])
