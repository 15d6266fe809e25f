"""What the Python side asks the library about a convolution layer's images and fused side paths -- ops.traits(g), one
mg_conv_traits call -- against tests/golden/conv_traits.json, which scripts/gen_conv_traits_golden.py recorded from the ten
predicate functions of ops.py as they were before the struct existed (kernel-name parsing and byte-count comparisons).  On the
host, no GPU.

The cases: every case of test_conv_plan_golden_host.golden_cases() under its planner hooks; every hook-free one again under
MG_PRECISION_F32_WINO43 and MG_PRECISION_F16_INFER; the rows of test_wino43_host.py and test_infer_f16_host.py under their lowered
thresholds; two weight-streaming layers with and without MG_NO_HGEMM_SA."""
import ctypes
import inspect
import json
import os

import test_conv_plan_golden_host as G
import test_conv_plans_gpu as P
import test_wino43_host as W43T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "conv_traits.json")
F32, F16, W43, HINF = 0, 1, 2, 3
# what a case may set beside the planner hooks of test_conv_plans_gpu.ENV_KEYS; cleared before every case
CASE_ENV = P.ENV_KEYS + ("MG_WINO43_MIN_C", "MG_INFER_F16_MIN_C", "MG_INFER_F16_MIN_TILES", "MG_NO_HGEMM_SA")
# the recorded answers, in file order: the ten predicate functions of ops.py (precast_ok for pass 0 and pass 1)
VIEWS = ("tiles_are_casts", "precast_ok_0", "precast_ok_1", "weights_are_casts", "wino_images_half", "wino_vnext_ok",
         "wino_vnext_positions", "wino_md_from_norm_ok", "wgrad_checks_finite", "wgrad_h16_ok", "wgrad_adam_ok")
# test_infer_f16_host.test_route_with_lowered_thresholds: (B, Ci, Co, H, W) -> MG_INFER_F16_MIN_TILES values it runs the row under
LOWERED = {"MG_INFER_F16_MIN_C": "64"}
INFER_ROWS = (((2, 64, 64, 2, 2), ("1",)), ((3, 64, 128, 4, 32), ("1", None, "97", "96")), ((2, 128, 64, 8, 16), ("1",)),
              ((1, 64, 64, 4, 164), ("1",)), ((1, 64, 64, 20, 32), ("1",)), ((1, 64, 64, 14, 46), ("1",)),
              ((1, 64, 96, 8, 16), ("1",)), ((1, 96, 64, 8, 16), ("1",)))
# test_amp_gpu.test_weight_streaming_gemm_equals_the_im2col_gemm: (B, Ci, H, W, Co, k, stride, pad, reflect)
SA_ROWS = ((8, 256, 4, 8, 256, 3, 1, 1, True), (8, 2048, 4, 8, 512, 1, 1, 0, False))


def traits_cases():
    """[(key, shape (B, Ci, H, W, Co, k, stride, pad, reflect), precision, environment)], each distinct combination once."""
    raw = []
    for _, shape, prec, env in G.golden_cases():
        raw.append((shape, prec, env))
        if not env:
            raw += [(shape, W43, {}), (shape, HINF, {})]
    for (B, Ci, Co, H, W, min_c) in W43T.TABLE:
        for reflect in (True, False):
            raw.append(((B, Ci, H, W, Co, 3, 1, 1, reflect), W43, {} if min_c is None else {"MG_WINO43_MIN_C": min_c}))
    for (B, Ci, Co, H, W), tiles in INFER_ROWS:
        for mt in tiles:
            raw.append(((B, Ci, H, W, Co, 3, 1, 1, True), HINF, dict(LOWERED, **({} if mt is None else {"MG_INFER_F16_MIN_TILES": mt}))))
    for shape in SA_ROWS:
        raw += [(shape, F16, {}), (shape, F16, {"MG_NO_HGEMM_SA": "1"})]
    seen, out = set(), []
    for shape, prec, env in raw:
        key = "%s|p%d|%s" % (",".join(str(int(v)) for v in shape), prec, ";".join("%s=%s" % kv for kv in sorted(env.items())))
        if key not in seen:
            seen.add(key)
            out.append((key, tuple(shape), prec, env))
    return out


def apply_env(monkeypatch, env):
    for key in CASE_ENV:
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)


def views(g, raised=()):
    """The answers of the ten predicate functions, as ints; None for one that raises an exception of `raised`."""
    from mdctgan_amd import ops

    def ask(fn, *args):
        try:
            return int(fn(*args))
        except raised:
            return None
    return [ask(ops.tiles_are_casts, g), ask(ops.precast_ok, 0, g), ask(ops.precast_ok, 1, g), ask(ops.weights_are_casts, g),
            ask(ops.wino_images_half, g), ask(ops.wino_vnext_ok, g), ask(ops.wino_vnext_positions, g),
            ask(ops.wino_md_from_norm_ok, g), ask(ops.wgrad_checks_finite, g), ask(ops.wgrad_h16_ok, g), ask(ops.wgrad_adam_ok, g)]


def recorded():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["views"] == list(VIEWS)
    return doc["cases"]


def fresh_traits(g):
    """One mg_conv_traits call, past ops.traits' memo."""
    from mdctgan_amd import _lib
    c = _lib.ConvTraits()
    assert _lib.load().mg_conv_traits(g, ctypes.byref(c)) == 0
    return c.astuple()


def test_traits_and_views_are_the_recorded_answers(monkeypatch):
    from mdctgan_amd import _lib, ops
    want = recorded()
    cases = traits_cases()
    assert sorted(key for key, *_ in cases) == sorted(want)
    for key, shape, prec, env in cases:
        apply_env(monkeypatch, env)
        g = P.geom_of(shape, prec)
        old = [0 if v is None else v for v in want[key]]         # (null: the old function raised -- a forward-only route)
        assert views(g) == old, key
        t = ops.traits(g)
        assert tuple(t) == fresh_traits(g), key
        # functional.py used to take tiles_are_casts apart again: "... and is_half(precision) and Co != 1"
        casts_of_x_dy = bool(old[0]) and _lib.is_half(prec) and g.Co != 1
        assert t.tiles == (1 if casts_of_x_dy else 2 if old[0] else 0), key
        assert t.precast == (old[1], old[2]) and (t.weight_image == _lib.IMAGE_CAST) == bool(old[3]), key
        assert (t.images_half, int(t.vnext_positions != 0), t.vnext_positions) == tuple(old[4:7]), key
        assert (t.md_from_norm, t.wgrad_checks_finite, t.wgrad_h16, t.wgrad_adam) == tuple(old[7:]), key


def test_memo_follows_the_environment(monkeypatch):
    """Forward through the cases, then back in reverse order, hooks and thresholds changing between cases and the memo never
    cleared: every answer equals a fresh library call under the environment of the moment."""
    from mdctgan_amd import ops
    cases = traits_cases()
    for key, shape, prec, env in cases + cases[::-1]:
        apply_env(monkeypatch, env)
        g = P.geom_of(shape, prec)
        assert tuple(ops.traits(g)) == fresh_traits(g), key
    # the thresholds of the two opt-in precisions, flipped on one geometry each
    for prec, name, shape in ((W43, "MG_WINO43_MIN_C", (2, 64, 8, 16, 64, 3, 1, 1, True)),
                              (HINF, "MG_INFER_F16_MIN_C", (8, 64, 8, 16, 64, 3, 1, 1, True))):
        apply_env(monkeypatch, {})
        g, g0 = P.geom_of(shape, prec), P.geom_of(shape, F16 if prec == HINF else F32)
        home = ops.traits(g)
        assert tuple(home) == tuple(ops.traits(g0))                  # below the threshold: the route of the plain precision
        monkeypatch.setenv(name, "64")
        if prec == HINF:
            monkeypatch.setenv("MG_INFER_F16_MIN_TILES", "1")
        low = ops.traits(g)
        assert low.weight_positions == (36 if prec == W43 else 16) and not low.wgrad_adam and low.tiles == 0, (prec, low)
        assert low.images_half == (prec == HINF)
        apply_env(monkeypatch, {})
        assert ops.traits(g) == home


def al256(n):
    return (n + 255) // 256 * 256


def image_bytes(g, t):
    """(u, v, md) byte sizes restated from the struct's fields and include/mdctgan_hip.h's description of the images."""
    from mdctgan_amd import _lib
    if t.weight_image == _lib.IMAGE_NONE:
        return 0, 0, 0
    if t.weight_image == _lib.IMAGE_CO1:          # 64 tap rows; v: the rounded x of an autocast layer, md: the scattered dy
        px = g.B * g.H * g.W
        return 64 * g.Ci * 4, al256(px * g.Ci * 4) if _lib.is_half(g.precision) else 0, al256(64 * ((px + 31) // 32 * 32) * 4)
    if t.weight_image == _lib.IMAGE_CAST:         # float16 copies, each kept only where the pass that writes it honours one
        on = t.tiles == 1
        return (g.Co * g.KH * g.KW * g.Ci * 2, al256(g.B * g.H * g.W * g.Ci * 2) if on and t.precast[0] else 0,
                al256(g.B * g.OH * g.OW * g.Co * 2) if on and t.precast[1] else 0)
    P_, e, Kc = t.weight_positions, t.weight_elem, g.Ci
    if P_ == 16:
        T = g.B * (g.H // 2) * (g.W // 2)
    elif P_ == 36:
        T = g.B * (g.H // 4) * (g.W // 4)
    elif g.stride == 1:
        T = g.B * ((g.H + 1) // 2) * ((g.W + 1) // 2)
    else:
        T, Kc = g.B * ((g.OH + 3) // 4) * ((g.OW + 3) // 4), 4 * g.Ci
    forward_only = P_ == 36 or t.images_half
    return P_ * g.Co * Kc * e, P_ * T * Kc * e, 0 if forward_only else P_ * T * g.Co * e


def test_kept_entry_points_agree_with_the_struct(monkeypatch):
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    kinds = set()
    for key, shape, prec, env in traits_cases():
        apply_env(monkeypatch, env)
        g = P.geom_of(shape, prec)
        t = ops.traits(g)
        kinds.add(t.weight_image)
        assert (lib.mg_conv_wino_md_from_norm_ok(g), lib.mg_conv_wgrad_adam_ok(g), lib.mg_conv_wgrad_checks_finite(g),
                lib.mg_conv_wgrad_h16_ok(g)) == (t.md_from_norm, t.wgrad_adam, t.wgrad_checks_finite, t.wgrad_h16), key
        assert lib.mg_conv_wino_vnext_ok(g) == int(t.vnext_positions != 0), key
        assert t.vnext_positions in (0, t.weight_positions) and t.weight_positions in (0, 16, 25, 36), key
        assert (t.weight_elem, t.images_half) == {_lib.IMAGE_NONE: (0, 0), _lib.IMAGE_WINO_F32: (4, 0), _lib.IMAGE_WINO_F16: (2, 1),
                                                 _lib.IMAGE_CAST: (2, 0), _lib.IMAGE_CO1: (4, 0)}[t.weight_image], key
        got = (lib.mg_conv_wino_weights_bytes(g), lib.mg_conv_wino_tiles_bytes(g, 0), lib.mg_conv_wino_tiles_bytes(g, 1))
        assert got == image_bytes(g, t), (key, t)
        assert lib.mg_conv_wino_tiles_bytes(g, 2) == 0
    assert kinds == {_lib.IMAGE_NONE, _lib.IMAGE_WINO_F32, _lib.IMAGE_WINO_F16, _lib.IMAGE_CAST, _lib.IMAGE_CO1}


def test_nothing_in_the_package_reads_plan_names():
    """ops.plan_name serves the profiler, bench.py and the tests that pin names; no module of the package calls it or the entry
    point behind it."""
    from mdctgan_amd import ops
    pkg = os.path.join(REPO, "mdctgan_amd")
    own = inspect.getsource(ops.plan_name)
    for name in sorted(os.listdir(pkg)):
        if not name.endswith(".py"):
            continue
        text = open(os.path.join(pkg, name)).read()
        if name == "ops.py":
            assert text.count(own) == 1
            text = text.replace(own, "")
        assert "plan_name(" not in text, name         # (a call of either; _lib.SIGNATURES declares the symbol, which is no call)
