"""Per-element float64 parity of the convolution kernels on EVERY tile shape, K split, launch order and fallback path, at small
shapes: the planner's hooks (MG_FORCE_PLAN, MG_FORCE_WGRAD, MG_FORCE_CONV_DMA, MG_FORCE_DENSE, MG_DGRAD_CLASS_ORDER; all read per
call) put a 128-wide tile, a split or a launch order on a geometry of a few hundred pixels, the case asserts through
mg_conv_plan_name / mg_conv_plan_splits / mg_conv_plan_order / the workspace queries that the library will launch exactly the
instance it names (a forced plan the shape does not admit is dropped silently), and all three passes are compared element by
element with the float64 CPU convolution -- test_conv_gpu.py's reference and bound for float32 (3e-5 of max|ref|),
test_amp_gpu.py's autocast reference and close_f16 for MG_PRECISION_F16.  A split or another tile does not move a bound.
Every output and the workspace carry guard elements behind them; an output starts from a sentinel, so an unwritten element fails.
tests/test_conv_plan_coverage_host.py keeps the case tables complete against the dispatch macros."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_amp_gpu import close_f16, h

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = 0, 1                  # mg_conv_geom.precision
FWD, DGRAD, WGRAD = 0, 1, 2
GUARD, FILL = 1024, 3.25         # floats behind every output / bytes behind the workspace; an output starts as SENTINEL
SENTINEL = 7.0
ENV_KEYS = ("MG_FORCE_PLAN", "MG_FORCE_WGRAD", "MG_FORCE_CONV_DMA", "MG_FORCE_DENSE", "MG_DGRAD_CLASS_ORDER", "MG_NO_WGRAD_RR",
            "MG_WINO42_MIN_WORK", "MG_F32_SPLIT")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def geom_of(shape, prec):
    from mdctgan_amd import ops
    B, Ci, H, W, Co, k, s, p, reflect = shape
    return ops.conv_geom(B, H, W, Ci, Co, k, k, s, p, reflect, prec)


def apply_env(monkeypatch, env):
    """The case's planner hooks and nothing else: a hook left over from the shell would change the plan under test."""
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)


def plan_order(pass_id, g):
    from mdctgan_amd import _lib
    gm, cls = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().mg_conv_plan_order(pass_id, g, ctypes.byref(gm), ctypes.byref(cls)) == 0
    return gm.value, cls.value


def workspace_bytes(pass_id, g):
    from mdctgan_amd import _lib
    lib = _lib.load()
    return int((lib.mg_conv_fwd_workspace, lib.mg_conv_dgrad_workspace, lib.mg_conv_wgrad_workspace)[pass_id](g))


def plans(shape, prec):
    """(kernel instance, DMA split count, gm, cls_order) of the three passes under the current environment."""
    from mdctgan_amd import _lib, ops
    g = geom_of(shape, prec)
    return tuple((ops.plan_name(ps, g), int(_lib.load().mg_conv_plan_splits(ps, g))) + plan_order(ps, g) for ps in range(3))


def igemm_splits(pass_id, shape, prec):
    """K splits of a forward pass / data gradient on the register-staged implicit GEMM (mg_conv_plan_splits speaks of the
    LDS-DMA kernels and the Winograd-domain GEMMs only): its workspace is exactly `splits` output-sized float32 slabs + 256
    bytes (256 bytes alone when unsplit)."""
    B, Ci, H, W, Co, k, s, p, _ = shape
    g = geom_of(shape, prec)
    n_out = B * g.OH * g.OW * Co if pass_id == FWD else B * H * W * Ci
    extra = workspace_bytes(pass_id, g) - 256
    assert extra % (4 * n_out) == 0, (extra, n_out)
    return max(1, extra // (4 * n_out))


@functools.lru_cache(maxsize=None)
def reference(shape, prec):
    """float64 CPU convolution, its data and weight gradients and the inputs (NHWC), built once per (shape, precision) and shared by
    every plan of that shape.  float32: test_conv_fwd_dgrad_wgrad's; MG_PRECISION_F16: test_conv_f16_precision's (operands rounded
    to float16, exact products, wide accumulation).  Checks that the reference itself is well-conditioned (outputs of order 1, a
    weight gradient of order sqrt(pixels)) with the 1 / sqrt(Ci k k) weight scaling: no bound below leans on cancellation."""
    B, Ci, H, W, Co, k, s, p, reflect = shape
    gen = torch.Generator().manual_seed(1000 * prec + (B * 7 + Ci * 5 + H * 3 + W + Co * 11 + k * 13 + s) % 997)
    x = torch.randn(B, Ci, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(Co, Ci, k, k, generator=gen, dtype=torch.float64) / np.sqrt(Ci * k * k)
    b = torch.randn(Co, generator=gen, dtype=torch.float64)
    xr, wr = (h(x), h(w)) if prec == F16 else (x, w)
    xr, wr = xr.requires_grad_(), wr.requires_grad_()
    xp = F.pad(xr, (p, p, p, p), mode="reflect") if (reflect and p) else xr
    y = F.conv2d(xp, wr, b, stride=s, padding=0 if (reflect and p) else p)
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(h(gy) if prec == F16 else gy)
    ref = dict(x=nhwc(x).float(), w=nhwc(w).float(), b=b.float(), gy=nhwc(gy).float(), y=nhwc(y.detach()), dx=nhwc(xr.grad),
               dw=nhwc(wr.grad), db=nhwc(gy).float().double().sum((0, 1, 2)),      # (the bias gradient is the column sum of the float32 dy in either precision)
                w64=wr.detach(), gy64=(h(gy) if prec == F16 else gy), b64=b)
    pixels = B * y.shape[2] * y.shape[3]
    # (unit-variance x, dy and bias: y has variance 2, dx variance Co / (Ci stride^2) -- its largest element a few deviations)
    assert 0.5 < ref["y"].abs().max().item() < 50 and 0.5 < ref["dx"].abs().max().item() / np.sqrt(Co / (Ci * s * s)) < 50
    assert 0.5 < ref["dw"].abs().max().item() / np.sqrt(pixels) < 50
    return ref


def guarded(n, fill=SENTINEL):
    """n floats to be written by a kernel (starting as `fill`) with GUARD floats of FILL right behind them in the same allocation."""
    buf = torch.full((n + GUARD,), FILL, dtype=torch.float32, device=DEV)
    buf[:n] = fill
    return buf


def guards_intact(*bufs):
    for buf, n in bufs:
        tail = buf[n:]
        if tail.dtype == torch.uint8:
            assert bool((tail == 0x5A).all()), "workspace overrun"
        else:
            assert bool((tail == FILL).all()), "output overrun"


class GuardedWorkspace:
    """Stands in for ops._ws: exactly the queried bytes (so that the query is also shown to suffice), 0x5A bytes behind them."""

    def __init__(self):
        self.bufs = []

    def __call__(self, nbytes, dev):
        buf = torch.full((int(nbytes) + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        self.bufs.append((buf, int(nbytes)))
        return buf[:int(nbytes)]


def rel_err(got, want):
    return (got.double().cpu() - want).abs().max().item() / want.abs().max().item()


def run_passes(shape, prec, monkeypatch, wino_f16=False, passes=(FWD, DGRAD, WGRAD)):
    """All three passes through ops.conv_fwd (with bias), ops.conv_dgrad and ops.conv_wgrad (with db, then accumulate=True) on
    guarded buffers, every element against the float64 reference."""
    from mdctgan_amd import ops
    B, Ci, H, W, Co, k, s, p, reflect = shape
    g = geom_of(shape, prec)
    ref = reference(shape, prec)
    assert (g.OH, g.OW) == tuple(ref["y"].shape[1:3])
    ws = GuardedWorkspace()
    monkeypatch.setattr(ops, "_ws", ws)
    xd, wd, bd, gyd = (ref[n].to(DEV) for n in ("x", "w", "b", "gy"))
    tol = dict(ulps=4.0, floor=2.0 ** -9) if wino_f16 else {}
    if FWD in passes:
        n = B * g.OH * g.OW * Co
        ybuf = guarded(n)
        y = ops.conv_fwd(g, xd, wd, bd, out=ybuf[:n].view(B, g.OH, g.OW, Co))
        err = rel_err(y, ref["y"])
        print("fwd", err)
        if prec == F16:
            close_f16(y, ref["y"], **tol)
        else:
            assert err < 3e-5, ("fwd", err)
        guards_intact((ybuf, n))
    if DGRAD in passes:
        n = B * H * W * Ci
        dxbuf = guarded(n)
        dx = ops.conv_dgrad(g, gyd, wd, out=dxbuf[:n].view(B, H, W, Ci))
        err = rel_err(dx, ref["dx"])
        print("dgrad", err)
        if prec == F16:
            close_f16(dx, ref["dx"], **tol)
        else:
            assert err < 3e-5, ("dgrad", err)
        guards_intact((dxbuf, n))
    if WGRAD in passes:
        n = Co * k * k * Ci
        dwbuf, dbbuf = guarded(n), guarded(Co)
        dw, db = dwbuf[:n].view(Co, k, k, Ci), dbbuf[:Co]
        ops.conv_wgrad(g, xd, gyd, dw, db)
        wtol = 2e-3 if wino_f16 else 3e-5
        e1, e2 = rel_err(dw, ref["dw"]), rel_err(db, ref["db"])
        ops.conv_wgrad(g, xd, gyd, dw, db, accumulate=True)
        e3, e4 = rel_err(dw, 2 * ref["dw"]), rel_err(db, 2 * ref["db"])
        print("wgrad", e1, e2, e3, e4)
        assert e1 < wtol and e2 < 3e-5 and e3 < wtol and e4 < 3e-5, ("wgrad", e1, e2, e3, e4)
        guards_intact((dwbuf, n), (dbbuf, Co))
    torch.cuda.synchronize()
    guards_intact(*ws.bufs)


def check_case(shape, prec, env, want, monkeypatch, **kw):
    """want: per pass (kernel instance, K splits or None, gm or None, cls_order or None) -- asserted BEFORE anything runs."""
    apply_env(monkeypatch, env)
    got = plans(shape, prec)
    for ps, (name, splits, gm, cls) in enumerate(want):
        if name is None:
            continue
        assert got[ps][0] == name, (ps, got[ps][0], name)
        if splits is not None:
            # (mg_conv_plan_splits speaks of the LDS-DMA kernels and of the Winograd-domain GEMMs; 0 elsewhere)
            have = got[ps][1] if got[ps][1] > 0 else other_splits(ps, shape, prec, env, monkeypatch)
            assert have == splits, (ps, name, have, splits)
        if gm is not None:
            assert got[ps][2] == gm, (ps, name, got[ps][2], gm)
        if cls is not None:
            assert got[ps][3] == cls, (ps, name, got[ps][3], cls)
    run_passes(shape, prec, monkeypatch, **kw)


def other_splits(pass_id, shape, prec, env, monkeypatch):
    """K splits of a pass on the register-staged implicit GEMM, read off the workspace query.  Forward / data gradient: exactly
    `splits` output-sized slabs + 256 bytes.  Weight gradient: max(`splits` dw-sized slabs when split, the bias gradient's
    column-sum scratch) + 256 bytes -- every case here is sized so that the slabs are the larger of the two."""
    B, Ci, H, W, Co, k, s, p, _ = shape
    g = geom_of(shape, prec)
    if pass_id == WGRAD:
        from mdctgan_amd import _lib
        slab = Co * k * k * Ci * 4
        colsum = int(_lib.load().mg_colsum_workspace(B * g.OH * g.OW, Co))
        extra = workspace_bytes(WGRAD, g) - 256
        if extra == colsum and colsum < 2 * slab:
            return 1
        assert extra % slab == 0 and extra > colsum, (extra, slab, colsum)
        return extra // slab
    return igemm_splits(pass_id, shape, prec)


# ---------------------------------------------------------------------------------------------------------------------------
# a. register-staged implicit GEMM (channels not multiples of 64): MG_FORCE_PLAN x MG_FORCE_WGRAD, both precisions
# (name, shape (B, Ci, H, W, Co, k, stride, pad, reflect), forward kernel per forced split count: "32" = conv_fwd32_kernel
# (Ci % 32 == 0 and one split or an even number of 16-deep chunks per split), "16" = conv_fwd_kernel; splits the shape admits)
IGEMM_SHAPES = {
    # 18 x 34 outputs (1224 pixels: no multiple of 64 or of 16), 27 forward chunks, parity classes of 18x34 / 18x33 / 17x34 / 17x33
    "s2_3x3_odd_co80": ((2, 48, 35, 67, 80, 3, 2, 1, False), {1: "16", 2: "16", 3: "16"}),
    # 4x4 stride 2 on an odd map: 9 x 17 outputs (306 pixels), 32 forward chunks (3 splits: 11 + 11 + 10, an odd count per split)
    "s2_4x4_odd_co96": ((2, 32, 17, 33, 96, 4, 2, 2, False), {1: "32", 2: "32", 3: "16"}),
    # ReflectionPad2d(1) + 3x3 on an odd map (no Winograd): 234 pixels, 18 chunks (2 splits: 9 each, odd -> the 16-deep kernel)
    "reflect_s1_odd_co80": ((2, 32, 9, 13, 80, 3, 1, 1, True), {1: "32", 2: "16", 3: "32"}),
    "reflect_s1_ci16_co96": ((3, 16, 9, 13, 96, 3, 1, 1, True), {1: "16", 2: "16", 3: "16"}),
}
IGEMM_TILES = ((128, 128), (128, 64), (64, 64))
WGRAD_FORCE = {1: "1,1", 2: "1,3", 3: "0,5"}          # MG_FORCE_WGRAD: 128x128 unsplit, 128x128 in three, 64x64 in five
IGEMM_CASES = [(name, prec, bm, bn, sp) for name in IGEMM_SHAPES for prec in (F32, F16) for bm, bn in IGEMM_TILES for sp in (1, 2, 3)
               # the weight gradient's forced split needs chunks / 8 >= splits: only the 1224-pixel shape admits 3 and 5
               if name == "s2_3x3_odd_co80" or sp == 1]
IGEMM_CASES += [(name, prec, bm, bn, -sp) for name in IGEMM_SHAPES if name != "s2_3x3_odd_co80" for prec in (F32, F16)
                for bm, bn in IGEMM_TILES for sp in (2, 3)]          # negative: forward / data gradient only


def igemm_want(name, prec, bm, bn, sp):
    shape, fwd_kind = IGEMM_SHAPES[name]
    tag = 2 if prec == F16 else 0
    t = 64 if abs(sp) == 3 else 128
    fwd = ("conv_fwd32_kernel<%d, %d, %d>" % (bm, bn, tag) if fwd_kind[abs(sp)] == "32"
           else "conv_fwd_kernel<%d, %d, true, %d>" % (bm, bn, tag))
    return ((fwd, abs(sp), 0, 0), ("conv_dgrad_kernel<%d, %d, true, true, %d>" % (bm, bn, tag), abs(sp), 0, 0),
            ("conv_wgrad_kernel<%d, %d, true, true, %d>" % (t, t, tag), (1, 3, 5)[abs(sp) - 1] if sp > 0 else None, 0, 0))


def igemm_env(bm, bn, sp):
    env = {"MG_FORCE_PLAN": "%d,%d,%d" % (bm, bn, abs(sp))}
    if sp > 0:
        env["MG_FORCE_WGRAD"] = WGRAD_FORCE[sp]
    return env


@pytest.mark.parametrize("case", IGEMM_CASES, ids=lambda c: "%s-f%d-%dx%d-sp%d" % (c[0], 16 if c[1] else 32, c[2], c[3], c[4]))
def test_implicit_gemm_tiles_and_splits(case, monkeypatch):
    name, prec, bm, bn, sp = case
    passes = (FWD, DGRAD, WGRAD) if sp > 0 else (FWD, DGRAD)
    want = igemm_want(name, prec, bm, bn, sp)
    check_case(IGEMM_SHAPES[name][0], prec, igemm_env(bm, bn, sp), want[:len(passes)], monkeypatch, passes=passes)


# channels that are no multiple of 4: the scalar-load instances (VEC = false) of the same tiles; Co % 4 != 0 admits no forward
# split and Ci % 4 != 0 no data-gradient split, the weight gradient splits regardless (378 pixels: 24 chunks, at most 3 splits)
NOVEC_SHAPE = (2, 22, 9, 21, 70, 3, 1, 1, False)
NOVEC_CASES = [(prec, bm, bn, wg) for prec in (F32, F16) for (bm, bn), wg in zip(IGEMM_TILES, ("1,1", "1,3", "0,3"))]


@pytest.mark.parametrize("case", NOVEC_CASES, ids=lambda c: "f%d-%dx%d-wgrad%s" % (16 if c[0] else 32, c[1], c[2], c[3]))
def test_implicit_gemm_scalar_load_instances(case, monkeypatch):
    prec, bm, bn, wg = case
    tag = 2 if prec == F16 else 0
    t = 128 if wg[0] == "1" else 64
    want = (("conv_fwd_kernel<%d, %d, false, %d>" % (bm, bn, tag), 1, 0, 0),
            ("conv_dgrad_kernel<%d, %d, false, false, %d>" % (bm, bn, tag), 1, 0, 0),
            ("conv_wgrad_kernel<%d, %d, false, false, %d>" % (t, t, tag), int(wg.split(",")[1]), 0, 0))
    check_case(NOVEC_SHAPE, prec, {"MG_FORCE_PLAN": "%d,%d,3" % (bm, bn), "MG_FORCE_WGRAD": wg}, want, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# b. LDS-DMA kernels (channels multiples of 64): MG_FORCE_CONV_DMA, all three passes, both precisions
# (shape, row-regular weight-gradient gather?, largest split count the DATA GRADIENT admits per precision: its planner keeps
# chunks / splits >= 8 with chunks = taps of the heaviest parity class x Co / 32 (float32) or Co / 64 (float16))
DMA_SHAPES = {
    "s2_3x3_odd": ((2, 128, 17, 33, 256, 3, 2, 1, False), False, {F32: 3, F16: 2}),       # 306 pixels: no multiple of 128, 64 or 32
    "s2_4x4_odd": ((2, 128, 17, 33, 256, 4, 2, 2, False), False, {F32: 3, F16: 2}),
    "s2_5x5_odd": ((2, 128, 17, 33, 256, 5, 2, 2, False), False, {F32: 3, F16: 3}),       # 9 / 6 / 6 / 4 taps per class
    "s1_3x3_zero_odd": ((2, 128, 19, 27, 256, 3, 1, 1, False), False, {F32: 3, F16: 3}),  # 1026 pixels
    "s1_3x3_reflect_odd": ((2, 128, 19, 27, 256, 3, 1, 1, True), False, {F32: 3, F16: 3}),    # data gradient: padded domain + fold
    "s2_3x3_row_regular": ((2, 128, 16, 64, 256, 3, 2, 1, False), True, {F32: 3, F16: 2}),    # 8 x 32 outputs: whole rows per chunk
}
DMA_TILES = ((64, 128), (128, 64), (128, 128))
DMA_CASES = [(name, prec, bm, bn, sp) for name in DMA_SHAPES for prec in (F32, F16) for bm, bn in DMA_TILES for sp in (1, 2, 3)]


def dma_want(name, prec, bm, bn, sp, cls=None):
    shape, rr, dgrad_max = DMA_SHAPES[name]
    half = "true" if prec == F16 else "false"
    return (("conv_fwd_dma_kernel<%d, %d, %s, 2>" % (bm, bn, half), sp, None, 0),
            ("conv_dgrad_dma_kernel<%d, %d, %s, 2>" % (bm, bn, half), sp, None, cls),
            ("conv_wgrad_dma_kernel<%d, %d, %s, 2, %s>" % (bm, bn, half, "true" if rr else "false"), sp, 0, 0))


@pytest.mark.parametrize("case", DMA_CASES, ids=lambda c: "%s-f%d-%dx%d-sp%d" % (c[0], 16 if c[1] else 32, c[2], c[3], c[4]))
def test_lds_dma_tiles_and_splits(case, monkeypatch):
    name, prec, bm, bn, sp = case
    shape, rr, dgrad_max = DMA_SHAPES[name]
    want = dma_want(name, prec, bm, bn, sp)
    passes = (FWD, DGRAD, WGRAD)
    if sp > dgrad_max[prec]:          # the data gradient's planner drops this split count here (and with it the forced tile)
        passes, want = (FWD, WGRAD), (want[0], ("conv_dgrad_dma_kernel<64, 64, %s, 2>" % ("true" if prec else "false"), 1, None, None), want[2])
    check_case(shape, prec, {"MG_FORCE_CONV_DMA": "%d,%d,%d" % (bm, bn, sp)}, want, monkeypatch, passes=passes)


@pytest.mark.parametrize("prec", [F32, F16], ids=["f32", "f16"])
def test_lds_dma_wgrad_general_gather_on_a_row_regular_shape(prec, monkeypatch):
    """MG_NO_WGRAD_RR=1: the per-lane coordinate walk of the 128-wide weight-gradient instances on the row-regular shape."""
    shape = DMA_SHAPES["s2_3x3_row_regular"][0]
    for bm, bn in DMA_TILES:
        want = dma_want("s2_3x3_row_regular", prec, bm, bn, 2)[2]
        want = (want[0].replace("true>", "false>"),) + want[1:]
        check_case(shape, prec, {"MG_FORCE_CONV_DMA": "%d,%d,2" % (bm, bn), "MG_NO_WGRAD_RR": "1"},
                   ((None,) * 4, (None,) * 4, want), monkeypatch, passes=(WGRAD,))


# ---------------------------------------------------------------------------------------------------------------------------
# c. launch order of the LDS-DMA forward pass and data gradient (mg_conv_plan_order): the tile order regrouped per XCD
# (cd_pick_gm: many row tiles, several column tiles, more input than weight bytes per tile) and the parity-class order of the
# stride-2 data gradient.  An order is a permutation of the same tiles: a wrong one leaves tiles unwritten or written twice.
# (name, shape, MG_FORCE_CONV_DMA, pass, gm)
GM_CASES = [
    ("fwd_groups_of_8_ragged_last_group", (3, 64, 41, 71, 256, 3, 1, 1, False), "128,64,2", FWD, 8),     # 69 row tiles = 8 x 8 + 5
    ("fwd_groups_of_2", (2, 64, 41, 71, 256, 3, 1, 1, False), "64,128,2", FWD, 2),                       # 91 row tiles = 45 x 2 + 1
    ("fwd_groups_of_1_1x1", (2, 128, 40, 71, 128, 1, 1, 0, False), "128,64,1", FWD, 1),
    ("dgrad_groups_of_1_1x1", (2, 128, 40, 71, 128, 1, 1, 0, False), "128,64,1", DGRAD, 1),
    ("dgrad_groups_of_1_1x1_64x64", (2, 128, 40, 71, 128, 1, 1, 0, False), "64,64,1", DGRAD, 1),
    # the data-gradient kernel keeps its own copy of the grouped map: 137 row tiles = 68 x 2 + 1 (a ragged last group) ...
    ("dgrad_groups_of_2_ragged_last_group", (3, 256, 41, 71, 64, 3, 1, 1, False), "64,64,1", DGRAD, 2),
    # ... the reflect-padded domain (42 x 73 per sample: 144 row tiles in groups of 4) ...
    ("dgrad_groups_of_4_reflect_padded_domain", (3, 256, 40, 71, 64, 3, 1, 1, True), "64,64,1", DGRAD, 4),
    # ... and a stride-2 launch on an odd map: the host sizes the groups for the largest class (9 row tiles), the kernel maps
    # each parity class with its own count (17x33, 17x32, 16x33 -> 9 tiles, a ragged group of 1; 16x32 -> 8 tiles)
    ("dgrad_groups_of_2_stride2_odd_classes", (2, 256, 33, 65, 64, 3, 2, 1, False), "128,64,1", DGRAD, 2),
]


@pytest.mark.parametrize("prec", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", GM_CASES, ids=lambda c: c[0])
def test_lds_dma_grouped_tile_order(case, prec, monkeypatch):
    name, shape, force, ps, gm = case
    bm, bn, sp = (int(v) for v in force.split(","))
    half = "true" if prec == F16 else "false"
    kern = ("conv_fwd_dma_kernel<%d, %d, %s, 2>", "conv_dgrad_dma_kernel<%d, %d, %s, 2>")[ps] % (bm, bn, half)
    want = [(None,) * 4] * 3
    want[ps] = (kern, sp, gm, None)
    check_case(shape, prec, {"MG_FORCE_CONV_DMA": force}, want, monkeypatch, passes=(ps,))


CLASS_ORDER_CASES = [(name, prec, cls, sp) for name in ("s2_3x3_odd", "s2_4x4_odd") for prec in (F32, F16) for cls in (0, 1) for sp in (1, 2)]


@pytest.mark.parametrize("case", CLASS_ORDER_CASES, ids=lambda c: "%s-f%d-order%d-sp%d" % (c[0], 16 if c[1] else 32, c[2], c[3]))
def test_lds_dma_dgrad_class_order(case, monkeypatch):
    """MG_DGRAD_CLASS_ORDER=0|1 on odd maps (four parity classes of different size, each splitting its own K range): the small
    grids of these shapes take order 1 by themselves, order 0 is what the bench's large grids run."""
    name, prec, cls, sp = case
    shape = DMA_SHAPES[name][0]
    apply_env(monkeypatch, {"MG_FORCE_CONV_DMA": "128,128,%d" % sp})
    assert plans(shape, prec)[DGRAD][3] == 1                  # the grid fits the resident slots: order 1 unless forced
    want = dma_want(name, prec, 128, 128, sp, cls=cls)
    check_case(shape, prec, {"MG_FORCE_CONV_DMA": "128,128,%d" % sp, "MG_DGRAD_CLASS_ORDER": str(cls)},
               ((None,) * 4, want[DGRAD], (None,) * 4), monkeypatch, passes=(DGRAD,))


# ---------------------------------------------------------------------------------------------------------------------------
# d. Winograd-domain GEMMs, float32: MG_FORCE_DENSE on dense_gemm.h (LDS-DMA dgemm32g_kernel; the register-staged dgemm32_kernel
# where the GEMM's K is no multiple of 32), MG_FORCE_PLAN where dense_plan declines (N % 64 != 0) and the GEMM runs on the
# convolution kernels' dense instances (tags 1 and 5).  Tile counts T: 544 (F(2x2,3x3)), 540 (F(2x2,4x4)), 40 (F(4x4,2x2)), 90 -- no multiples of 64.
# A forced tile / split that a pass does not admit is dropped for that pass (N % bn != 0; chunks / splits < 8): the rows say
# what each pass runs.  (MG_FORCE_PLAN=64,64,1 beside MG_FORCE_DENSE only pins the unused second plan of the workspace query.)
WINO_SHAPES = {
    "f23": (2, 128, 32, 34, 128, 3, 1, 1, False), "f23_reflect_small": (2, 64, 10, 18, 128, 3, 1, 1, True),
    "f24": (2, 128, 29, 35, 128, 4, 1, 2, False), "f42": (2, 128, 25, 33, 128, 4, 2, 2, False),
    "f23_kc48": (2, 48, 10, 18, 128, 3, 1, 1, True), "f24_kc80": (2, 80, 9, 17, 128, 4, 1, 2, False),
    "f23_co80": (2, 128, 10, 18, 80, 3, 1, 1, False), "f42_co48": (2, 32, 17, 33, 48, 4, 2, 2, False),
    "f23_decline": (2, 48, 10, 18, 80, 3, 1, 1, True), "f24_decline": (2, 48, 9, 17, 80, 4, 1, 2, False),
    "f42_decline": (2, 48, 17, 33, 80, 4, 2, 2, False), "f23_decline_big": (2, 144, 36, 72, 144, 3, 1, 1, True),
    "f23_decline_kc64": (2, 64, 10, 18, 80, 3, 1, 1, True),
    # more than 4096 tiles (4200) with >= 128 channels on both sides: the 25-position weight gradient on 128 x 128 tiles
    "f24_decline_big": (6, 144, 39, 69, 144, 4, 1, 2, False),
}
# (shape, hooks, kernel instance per pass, K splits per pass)
WINO_CASES = [
    ("f23", {"MG_FORCE_DENSE": "64,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 128, 2, 2, 0, 0, 2, 16, 0>", "dgemm32g_kernel<64, 128, 2, 2, 0, 1, 2, 16, 0>", "dgemm32g_kernel<64, 128, 2, 2, 1, 1, 2, 16, 0>"), (1, 1, 1)),
    ("f23", {"MG_FORCE_DENSE": "64,128,2", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 128, 2, 2, 0, 0, 2, 16, 0>", "dgemm32g_kernel<64, 128, 2, 2, 0, 1, 2, 16, 0>", "dgemm32g_kernel<64, 128, 2, 2, 1, 1, 2, 16, 0>"), (1, 1, 2)),
    ("f23", {"MG_FORCE_DENSE": "128,64,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<128, 64, 2, 2, 0, 0, 2, 16, 0>", "dgemm32g_kernel<128, 64, 2, 2, 0, 1, 2, 16, 0>", "dgemm32g_kernel<128, 64, 2, 2, 1, 1, 2, 16, 0>"), (1, 1, 1)),
    ("f23", {"MG_FORCE_DENSE": "128,64,2", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 128, 2, 2, 0, 0, 2, 16, 0>", "dgemm32g_kernel<64, 128, 2, 2, 0, 1, 2, 16, 0>", "dgemm32g_kernel<128, 64, 2, 2, 1, 1, 2, 16, 0>"), (1, 1, 2)),
    ("f23", {"MG_FORCE_DENSE": "128,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<128, 128, 2, 2, 0, 0, 2, 16, 0>", "dgemm32g_kernel<128, 128, 2, 2, 0, 1, 2, 16, 0>", "dgemm32g_kernel<128, 128, 2, 2, 1, 1, 2, 16, 0>"), (1, 1, 1)),
    ("f23", {"MG_FORCE_DENSE": "128,128,2", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 128, 2, 2, 0, 0, 2, 16, 0>", "dgemm32g_kernel<64, 128, 2, 2, 0, 1, 2, 16, 0>", "dgemm32g_kernel<128, 128, 2, 2, 1, 1, 2, 16, 0>"), (1, 1, 2)),
    ("f24", {"MG_FORCE_DENSE": "64,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 128, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<64, 128, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<64, 128, 2, 2, 1, 1, 2, 25, 0>"), (1, 1, 1)),
    ("f24", {"MG_FORCE_DENSE": "64,128,2", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 64, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<64, 64, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<64, 128, 2, 2, 1, 1, 2, 25, 0>"), (1, 1, 2)),
    ("f24", {"MG_FORCE_DENSE": "128,64,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<128, 64, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<128, 64, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<128, 64, 2, 2, 1, 1, 2, 25, 0>"), (1, 1, 1)),
    ("f24", {"MG_FORCE_DENSE": "128,64,2", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 64, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<64, 64, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<128, 64, 2, 2, 1, 1, 2, 25, 0>"), (1, 1, 2)),
    ("f24", {"MG_FORCE_DENSE": "128,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<128, 128, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<128, 128, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<128, 128, 2, 2, 1, 1, 2, 25, 0>"), (1, 1, 1)),
    ("f24", {"MG_FORCE_DENSE": "128,128,2", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 64, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<64, 64, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<128, 128, 2, 2, 1, 1, 2, 25, 0>"), (1, 1, 2)),
    ("f42", {"MG_FORCE_DENSE": "64,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 128, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<64, 128, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<64, 128, 2, 2, 1, 1, 2, 25, 0>"), (1, 1, 1)),
    ("f42", {"MG_FORCE_DENSE": "64,128,2", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<64, 128, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<64, 64, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<64, 128, 2, 2, 1, 1, 2, 25, 0>"), (2, 1, 1)),
    ("f42", {"MG_FORCE_DENSE": "128,64,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<128, 64, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<128, 64, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<128, 64, 2, 2, 1, 1, 2, 25, 0>"), (1, 1, 1)),
    ("f42", {"MG_FORCE_DENSE": "128,64,2", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<128, 64, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<64, 64, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<64, 128, 2, 2, 1, 1, 2, 25, 0>"), (2, 1, 1)),
    ("f42", {"MG_FORCE_DENSE": "128,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<128, 128, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<128, 128, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<128, 128, 2, 2, 1, 1, 2, 25, 0>"), (1, 1, 1)),
    ("f42", {"MG_FORCE_DENSE": "128,128,2", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<128, 128, 2, 2, 0, 0, 2, 25, 0>", "dgemm32g_kernel<64, 64, 2, 2, 0, 1, 2, 25, 0>", "dgemm32g_kernel<64, 128, 2, 2, 1, 1, 2, 25, 0>"), (2, 1, 1)),
    ("f23_reflect_small", {"MG_FORCE_DENSE": "128,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32g_kernel<128, 128, 2, 2, 0, 0, 2, 16, 0>", "dgemm32g_kernel<64, 64, 2, 2, 0, 1, 2, 16, 0>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (1, 1, 1)),
    ("f23_kc48", {"MG_FORCE_DENSE": "64,64,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32_kernel<64, 64, 2, 2, 0, 0, 0>", "conv_dgrad_kernel<64, 64, true, true, 1>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (1, 1, 1)),
    ("f23_kc48", {"MG_FORCE_DENSE": "128,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32_kernel<128, 128, 4, 2, 0, 0, 0>", "conv_dgrad_kernel<64, 64, true, true, 1>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (1, 1, 1)),
    ("f24_kc80", {"MG_FORCE_DENSE": "64,64,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32_kernel<64, 64, 2, 2, 0, 0, 0>", "conv_dgrad_kernel<64, 64, true, true, 5>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (1, 1, 1)),
    ("f24_kc80", {"MG_FORCE_DENSE": "128,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("dgemm32_kernel<128, 128, 4, 2, 0, 0, 0>", "conv_dgrad_kernel<64, 64, true, true, 5>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (1, 1, 1)),
    ("f23_co80", {"MG_FORCE_DENSE": "64,64,1", "MG_FORCE_PLAN": "64,64,1"},
     ("conv_fwd32_kernel<64, 64, 1>", "dgemm32_kernel<64, 64, 2, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (1, 1, 1)),
    ("f23_co80", {"MG_FORCE_DENSE": "128,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("conv_fwd32_kernel<64, 64, 1>", "dgemm32_kernel<128, 128, 4, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (1, 1, 1)),
    ("f42_co48", {"MG_FORCE_DENSE": "64,64,1", "MG_FORCE_PLAN": "64,64,1"},
     ("conv_fwd32_kernel<64, 64, 5>", "dgemm32_kernel<64, 64, 2, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (1, 1, 1)),
    ("f42_co48", {"MG_FORCE_DENSE": "128,128,1", "MG_FORCE_PLAN": "64,64,1"},
     ("conv_fwd32_kernel<64, 64, 5>", "dgemm32_kernel<128, 128, 4, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (1, 1, 1)),
    ("f23_decline", {"MG_FORCE_PLAN": "128,128,1"},
     ("conv_fwd_kernel<128, 128, true, 1>", "conv_dgrad_kernel<128, 128, true, true, 1>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (1, 1, 1)),
    ("f23_decline", {"MG_FORCE_PLAN": "128,128,2"},
     ("conv_fwd_kernel<128, 128, true, 1>", "conv_dgrad_kernel<128, 128, true, true, 1>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (2, 2, 1)),
    ("f23_decline", {"MG_FORCE_PLAN": "128,64,1"},
     ("conv_fwd_kernel<128, 64, true, 1>", "conv_dgrad_kernel<128, 64, true, true, 1>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (1, 1, 1)),
    ("f23_decline", {"MG_FORCE_PLAN": "128,64,2"},
     ("conv_fwd_kernel<128, 64, true, 1>", "conv_dgrad_kernel<128, 64, true, true, 1>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (2, 2, 1)),
    ("f23_decline", {"MG_FORCE_PLAN": "64,64,2"},
     ("conv_fwd_kernel<64, 64, true, 1>", "conv_dgrad_kernel<64, 64, true, true, 1>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (2, 2, 1)),
    ("f24_decline", {"MG_FORCE_PLAN": "128,128,1"},
     ("conv_fwd_kernel<128, 128, true, 5>", "conv_dgrad_kernel<128, 128, true, true, 5>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (1, 1, 1)),
    ("f24_decline", {"MG_FORCE_PLAN": "128,128,2"},
     ("conv_fwd_kernel<128, 128, true, 5>", "conv_dgrad_kernel<128, 128, true, true, 5>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (2, 2, 1)),
    ("f24_decline", {"MG_FORCE_PLAN": "128,64,1"},
     ("conv_fwd_kernel<128, 64, true, 5>", "conv_dgrad_kernel<128, 64, true, true, 5>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (1, 1, 1)),
    ("f24_decline", {"MG_FORCE_PLAN": "128,64,2"},
     ("conv_fwd_kernel<128, 64, true, 5>", "conv_dgrad_kernel<128, 64, true, true, 5>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (2, 2, 1)),
    ("f24_decline", {"MG_FORCE_PLAN": "64,64,2"},
     ("conv_fwd_kernel<64, 64, true, 5>", "conv_dgrad_kernel<64, 64, true, true, 5>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (2, 2, 1)),
    ("f42_decline", {"MG_FORCE_PLAN": "128,128,1"},
     ("conv_fwd32_kernel<128, 128, 5>", "dgemm32_kernel<64, 64, 2, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (1, 1, 1)),
    ("f42_decline", {"MG_FORCE_PLAN": "128,128,2"},
     ("conv_fwd32_kernel<128, 128, 5>", "dgemm32_kernel<64, 64, 2, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (2, 1, 1)),
    ("f42_decline", {"MG_FORCE_PLAN": "128,64,1"},
     ("conv_fwd32_kernel<128, 64, 5>", "dgemm32_kernel<64, 64, 2, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (1, 1, 1)),
    ("f42_decline", {"MG_FORCE_PLAN": "128,64,2"},
     ("conv_fwd32_kernel<128, 64, 5>", "dgemm32_kernel<64, 64, 2, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (2, 1, 1)),
    ("f42_decline", {"MG_FORCE_PLAN": "64,64,2"},
     ("conv_fwd32_kernel<64, 64, 5>", "dgemm32_kernel<64, 64, 2, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 5>"), (2, 1, 1)),
    ("f23_decline_big", {"MG_FORCE_PLAN": "128,128,1"},
     ("conv_fwd_kernel<128, 128, true, 1>", "conv_dgrad_kernel<128, 128, true, true, 1>", "conv_wgrad_kernel<128, 128, true, true, 1>"), (1, 1, 9)),
    ("f23_decline_big", {"MG_FORCE_PLAN": "128,128,2"},
     ("conv_fwd_kernel<128, 128, true, 1>", "conv_dgrad_kernel<128, 128, true, true, 1>", "conv_wgrad_kernel<128, 128, true, true, 1>"), (2, 2, 9)),
    ("f23_decline_big", {"MG_FORCE_PLAN": "128,64,1"},
     ("conv_fwd_kernel<128, 64, true, 1>", "conv_dgrad_kernel<128, 64, true, true, 1>", "conv_wgrad_kernel<128, 128, true, true, 1>"), (1, 1, 9)),
    ("f23_decline_big", {"MG_FORCE_PLAN": "128,64,2"},
     ("conv_fwd_kernel<128, 64, true, 1>", "conv_dgrad_kernel<128, 64, true, true, 1>", "conv_wgrad_kernel<128, 128, true, true, 1>"), (2, 2, 9)),
    ("f23_decline_big", {"MG_FORCE_PLAN": "64,64,2"},
     ("conv_fwd_kernel<64, 64, true, 1>", "conv_dgrad_kernel<64, 64, true, true, 1>", "conv_wgrad_kernel<128, 128, true, true, 1>"), (2, 2, 9)),
    ("f23_decline_kc64", {"MG_FORCE_PLAN": "128,128,1"},
     ("conv_fwd32_kernel<128, 128, 1>", "dgemm32_kernel<64, 64, 2, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (1, 1, 1)),
    ("f23_decline_kc64", {"MG_FORCE_PLAN": "128,64,1"},
     ("conv_fwd32_kernel<128, 64, 1>", "dgemm32_kernel<64, 64, 2, 2, 0, 1, 0>", "conv_wgrad_kernel<64, 64, true, true, 1>"), (1, 1, 1)),
    ("f24_decline_big", {"MG_FORCE_PLAN": "128,128,1"},
     ("conv_fwd_kernel<128, 128, true, 5>", "conv_dgrad_kernel<128, 128, true, true, 5>", "conv_wgrad_kernel<128, 128, true, true, 5>"), (1, 1, 8)),
]


# MG_PRECISION_F16 Winograd layers (>= 256 channels, >= 256 tiles) keep float32 images and run their GEMMs on the convolution
# kernels' float16 dense instances (tag 3): the wider close_f16 arguments of test_conv_f16_precision, 2e-3 for the weight gradient
WINO_F16_SHAPES = {"t256": (4, 256, 16, 16, 256, 3, 1, 1, False),          # 256 tiles: the weight gradient on 64 x 64 tiles
                   "t1088": (4, 256, 32, 34, 256, 3, 1, 1, True)}          # more than 1024 tiles: ... on 128 x 128 tiles
# (shape, MG_FORCE_PLAN, forward instance, K splits of forward / data gradient: 16 chunks in 6 splits leave an odd 3 per split,
# which the 32-deep forward kernel does not take)
WINO_F16_CASES = [("t256", "128,128,1", "conv_fwd32_kernel<128, 128, 3>", 1), ("t256", "128,64,1", "conv_fwd32_kernel<128, 64, 3>", 1),
                  ("t256", "64,64,2", "conv_fwd32_kernel<64, 64, 3>", 2), ("t256", "128,128,2", "conv_fwd32_kernel<128, 128, 3>", 2),
                  ("t256", "128,64,6", "conv_fwd_kernel<128, 64, true, 3>", 6), ("t256", "128,128,6", "conv_fwd_kernel<128, 128, true, 3>", 6),
                  ("t256", "64,64,6", "conv_fwd_kernel<64, 64, true, 3>", 6), ("t1088", "128,128,1", "conv_fwd32_kernel<128, 128, 3>", 1)]


@pytest.mark.parametrize("case", WINO_F16_CASES, ids=lambda c: c[0] + "-" + c[1].replace(",", "x"))
def test_winograd_domain_gemm_float16_instances(case, monkeypatch):
    key, force, fwd, sp = case
    bm, bn = (int(v) for v in force.split(",")[:2])
    t, wsp = (128, 8) if key == "t1088" else (64, 2)          # (the weight gradient's own plan: MG_FORCE_PLAN does not reach it)
    want = ((fwd, sp, 0, 0), ("conv_dgrad_kernel<%d, %d, true, true, 3>" % (bm, bn), sp, 0, 0),
            ("conv_wgrad_kernel<%d, %d, true, true, 3>" % (t, t), wsp, 0, 0))
    check_case(WINO_F16_SHAPES[key], F16, {"MG_FORCE_PLAN": force}, want, monkeypatch, wino_f16=True)


@pytest.mark.parametrize("case", WINO_CASES, ids=lambda c: c[0] + "-" + "-".join(v.replace(",", "x") for v in c[1].values()))
def test_winograd_domain_gemm_tiles_and_splits(case, monkeypatch):
    key, env, names, splits = case
    want = tuple((n, s, 0, 0) for n, s in zip(names, splits))
    check_case(WINO_SHAPES[key], F32, dict(env, MG_WINO42_MIN_WORK="0"), want, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------
# e. the fallback ladder of the plain C entry points: every family leaves its own kernels for the generic tail (LDS-DMA where its
# buffers allow, else the register-staged implicit GEMM with scalar loads and without a K split) when the workspace is missing
# or short, a pointer is not 16-byte aligned, or a data gradient carries a bias / activation the family cannot fuse.
# ops.py always passes aligned tensors and a full workspace, so these go through _lib directly.
# (family conv_route names, precision, shape, hooks)
LADDER_CASES = [
    ("co1", F32, (2, 64, 10, 14, 1, 4, 2, 2, False), {}),
    ("rowdot", F32, (2, 16, 32, 64, 1, 7, 1, 3, True), {}),
    ("h16", F16, (2, 128, 4, 8, 128, 3, 1, 1, True), {}),
    ("wino", F32, (2, 64, 8, 16, 64, 3, 1, 1, True), {}),
    ("wino4", F32, (2, 64, 9, 17, 128, 4, 1, 2, False), {}),
    ("wino42", F32, (2, 32, 16, 24, 48, 4, 2, 2, False), {"MG_WINO42_MIN_WORK": "0"}),
    ("smallc", F32, (3, 2, 20, 36, 64, 7, 1, 3, True), {}),
    ("smallc_4x4_s2", F32, (1, 3, 17, 33, 80, 4, 2, 2, False), {}),
    ("dma", F32, (2, 64, 17, 33, 64, 3, 2, 1, False), {}),
    ("dma_f16", F16, (2, 64, 17, 33, 128, 3, 2, 1, False), {}),
    ("dma_reflect", F32, (2, 64, 9, 13, 64, 3, 1, 1, True), {}),
    ("igemm_split_k", F32, (2, 48, 35, 67, 80, 3, 2, 1, False), {"MG_FORCE_PLAN": "64,64,3", "MG_FORCE_WGRAD": "0,3"}),
]
# the kernel the FIRST pass of each family reports with everything in order (what the ladder is left from)
LADDER_HOME = {"co1": "dgemm32g_kernel<64, 128, 2, 2, 0, 0, 2, 0, 0>", "rowdot": "conv_rowdot_fwd_kernel", "h16": "hgemm", "wino": "dgemm32g_kernel",
               "wino4": "dgemm32g_kernel", "wino42": "conv_fwd", "smallc": "conv_smallc_fwd_kernel", "smallc_4x4_s2": "conv_smallc_dgrad_kernel",
               "dma": "conv_fwd_dma_kernel", "dma_f16": "conv_fwd_dma_kernel", "dma_reflect": "conv_dgrad_dma_kernel", "igemm_split_k": "conv_fwd_kernel"}
MG_OK, MG_ERR_ARG = 0, -1
WAYS = ("no_workspace", "short_workspace", "unaligned_pointers", "dgrad_bias_relu")


def offset_copy(t, unaligned, n_guard=GUARD, fill=None):
    """A flat device buffer holding t (or `fill`) followed by guard floats; unaligned: the payload starts one float into the
    allocation (a [1:] slice: 4-byte aligned, not 16)."""
    n = t.numel() if torch.is_tensor(t) else int(t)
    lead = 1 if unaligned else 0
    buf = torch.full((lead + n + n_guard,), FILL, dtype=torch.float32, device=DEV)
    view = buf[lead:lead + n]
    if torch.is_tensor(t):
        view.copy_(t.reshape(-1))
    else:
        view.fill_(SENTINEL if fill is None else fill)
    assert (view.data_ptr() % 16 == 4) == bool(unaligned) and view.data_ptr() % 4 == 0
    return buf, view, lead + n


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("case", LADDER_CASES, ids=lambda c: c[0])
def test_entry_point_fallback_ladder(case, way, monkeypatch):
    """mg_conv_fwd / mg_conv_dgrad / mg_conv_wgrad with (1) no workspace, (2) a workspace 16 bytes short of the query, (3) every
    tensor one float off 16-byte alignment, (4) a data gradient with bias + ReLU: MG_OK and the float64 bound of the ordinary call.
    The weight gradient's workspace is NOT optional (include/mdctgan_hip.h; its bias gradient and split-K slabs live there):
    without it the call must refuse with MG_ERR_ARG and leave dw alone.
    (3) lands on the scalar-load instances of conv_{fwd,dgrad,wgrad}_kernel (VEC / VECA / VECB = false, no split, no float4
    epilogue) for every family: each family's own branch and the LDS-DMA tail require 16-byte aligned operands."""
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    family, prec, shape, env = case
    apply_env(monkeypatch, env)
    B, Ci, H, W, Co, k, s, p, reflect = shape
    g = geom_of(shape, prec)
    home = [ops.plan_name(ps, g) for ps in range(3)]
    assert any(n.startswith(LADDER_HOME[family]) for n in home), home
    ref = reference(shape, prec)
    un = way == "unaligned_pointers"
    st = _lib.stream()

    def workspace(ps):
        need = workspace_bytes(ps, g)
        if way == "no_workspace":
            return None, None, 0
        size = need - 16 if way == "short_workspace" else need
        buf = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        return buf, buf.data_ptr(), size

    def ws_intact(buf, size):
        if buf is not None:
            assert bool((buf[size:] == 0x5A).all()), "workspace overrun"

    def close(got, want, f16_out):
        if prec == F16 and f16_out:
            close_f16(got.view(want.shape), want)
        else:
            err = rel_err(got.view(want.shape), want)
            print(family, way, err)
            assert err < 3e-5, err

    _, xd, _ = offset_copy(ref["x"], un)
    _, wd, _ = offset_copy(ref["w"], un)
    _, gyd, _ = offset_copy(ref["gy"], un)
    if way == "dgrad_bias_relu":
        gen = torch.Generator().manual_seed(3)
        bias64 = torch.randn(Ci, generator=gen, dtype=torch.float64)
        _, bd, _ = offset_copy(bias64.float(), un)
        dxbuf, dx, end = offset_copy(B * H * W * Ci, un)
        wsb, wsp, size = workspace(DGRAD)
        rc = lib.mg_conv_dgrad(g, gyd.data_ptr(), wd.data_ptr(), bd.data_ptr(), dx.data_ptr(),
                               _lib.ACT_RELU, wsp, size, st)
        assert rc == MG_OK, rc
        close(dx, torch.relu(ref["dx"] + bias64.float().double()), True)
        assert bool((dxbuf[end:] == FILL).all()) and bool((dxbuf[:end - dx.numel()] == FILL).all())
        ws_intact(wsb, size)
        return
    _, bd, _ = offset_copy(ref["b"], un)
    # forward
    ybuf, y, end = offset_copy(B * g.OH * g.OW * Co, un)
    wsb, wsp, size = workspace(FWD)
    rc = lib.mg_conv_fwd(g, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), _lib.ACT_NONE, wsp, size, st)
    assert rc == MG_OK, rc
    close(y, ref["y"], True)
    assert bool((ybuf[end:] == FILL).all()) and bool((ybuf[:end - y.numel()] == FILL).all())
    ws_intact(wsb, size)
    # data gradient
    dxbuf, dx, end = offset_copy(B * H * W * Ci, un)
    wsb, wsp, size = workspace(DGRAD)
    rc = lib.mg_conv_dgrad(g, gyd.data_ptr(), wd.data_ptr(), None, dx.data_ptr(), _lib.ACT_NONE, wsp, size, st)
    assert rc == MG_OK, rc
    close(dx, ref["dx"], True)
    assert bool((dxbuf[end:] == FILL).all()) and bool((dxbuf[:end - dx.numel()] == FILL).all())
    ws_intact(wsb, size)
    # weight gradient (+ bias gradient, then accumulate)
    dwbuf, dw, end = offset_copy(Co * k * k * Ci, un)
    dbbuf, db, dbend = offset_copy(Co, un)
    wsb, wsp, size = workspace(WGRAD)
    rc = lib.mg_conv_wgrad(g, xd.data_ptr(), gyd.data_ptr(), dw.data_ptr(), db.data_ptr(), 0, wsp, size, st)
    if way in ("no_workspace", "short_workspace"):
        assert rc == MG_ERR_ARG, rc
        assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())
    else:
        assert rc == MG_OK, rc
        close(dw, ref["dw"], False)
        close(db, ref["db"], False)
        rc = lib.mg_conv_wgrad(g, xd.data_ptr(), gyd.data_ptr(), dw.data_ptr(), db.data_ptr(), 1, wsp, size, st)
        assert rc == MG_OK, rc
        close(dw, 2 * ref["dw"], False)
        close(db, 2 * ref["db"], False)
    assert bool((dwbuf[end:] == FILL).all()) and bool((dbbuf[dbend:] == FILL).all())
    ws_intact(wsb, size)


def all_cases():
    """(shape, precision, hooks, passes that the case RUNS and compares) of every parametrised case above: what
    tests/test_conv_plan_coverage_host.py walks.  The fallback-ladder cases are left out: they run what their family is left for."""
    every = (FWD, DGRAD, WGRAD)
    for name, prec, bm, bn, sp in IGEMM_CASES:
        yield IGEMM_SHAPES[name][0], prec, igemm_env(bm, bn, sp), every if sp > 0 else (FWD, DGRAD)
    for prec, bm, bn, wg in NOVEC_CASES:
        yield NOVEC_SHAPE, prec, {"MG_FORCE_PLAN": "%d,%d,3" % (bm, bn), "MG_FORCE_WGRAD": wg}, every
    for name, prec, bm, bn, sp in DMA_CASES:
        passes = every if sp <= DMA_SHAPES[name][2][prec] else (FWD, WGRAD)
        yield DMA_SHAPES[name][0], prec, {"MG_FORCE_CONV_DMA": "%d,%d,%d" % (bm, bn, sp)}, passes
    for prec in (F32, F16):
        for bm, bn in DMA_TILES:
            yield DMA_SHAPES["s2_3x3_row_regular"][0], prec, {"MG_FORCE_CONV_DMA": "%d,%d,2" % (bm, bn), "MG_NO_WGRAD_RR": "1"}, (WGRAD,)
        for name, shape, force, ps, gm in GM_CASES:
            yield shape, prec, {"MG_FORCE_CONV_DMA": force}, (ps,)
    for name, prec, cls, sp in CLASS_ORDER_CASES:
        yield DMA_SHAPES[name][0], prec, {"MG_FORCE_CONV_DMA": "128,128,%d" % sp, "MG_DGRAD_CLASS_ORDER": str(cls)}, (DGRAD,)
    for key, env, names, splits in WINO_CASES:
        yield WINO_SHAPES[key], F32, dict(env, MG_WINO42_MIN_WORK="0"), every
    for key, force, fwd, sp in WINO_F16_CASES:
        yield WINO_F16_SHAPES[key], F16, {"MG_FORCE_PLAN": force}, every


# One pointer at a time: with every pointer off alignment at once, a single aligned16() test in a family's branch would hide
# a missing test on another pointer (how the float2 weight loads of conv_smallc_fwd_kernel and the float2 dy loads of
# conv_smallc_wgrad_mfma_kernel went unnoticed).  The tap-GEMM and row-dot families (Co == 1) are left out: their branches do
# not test y / bias / dy / dw, and their kernels were not read for this test.
SINGLE_POINTER_CASES = [c for c in LADDER_CASES if c[0] not in ("co1", "rowdot")]


@pytest.mark.parametrize("which", ["x", "w", "dy", "bias", "out"])
@pytest.mark.parametrize("case", SINGLE_POINTER_CASES, ids=lambda c: c[0])
def test_entry_point_single_unaligned_pointer(case, which, monkeypatch):
    """Exactly one operand one float off 16-byte alignment (x, w, dy, the forward bias, or the pass's output), full aligned
    workspace: MG_OK and the ordinary bound, on whichever kernel the entry point then picks."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    family, prec, shape, env = case
    apply_env(monkeypatch, env)
    B, Ci, H, W, Co, k, s, p, reflect = shape
    g = geom_of(shape, prec)
    ref = reference(shape, prec)
    st = _lib.stream()
    _, xd, _ = offset_copy(ref["x"], which == "x")
    _, wd, _ = offset_copy(ref["w"], which == "w")
    _, gyd, _ = offset_copy(ref["gy"], which == "dy")
    _, bd, _ = offset_copy(ref["b"], which == "bias")
    out_un = which == "out"

    def close(got, want, f16_out):
        if prec == F16 and f16_out:
            close_f16(got.view(want.shape), want)
        else:
            err = rel_err(got.view(want.shape), want)
            print(family, which, err)
            assert err < 3e-5, err

    def run(ps, call, n, want, f16_out):
        need = workspace_bytes(ps, g)
        wsb = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        buf, out, end = offset_copy(n, out_un)
        rc = call(out, wsb.data_ptr(), need)
        assert rc == MG_OK, rc
        close(out, want, f16_out)
        assert bool((buf[end:] == FILL).all()) and bool((buf[:end - n] == FILL).all()) and bool((wsb[need:] == 0x5A).all())

    if which in ("x", "w", "bias", "out"):
        run(FWD, lambda y, ws, nb: lib.mg_conv_fwd(g, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), _lib.ACT_NONE, ws, nb, st),
            B * g.OH * g.OW * Co, ref["y"], True)
    if which in ("dy", "w", "out"):
        run(DGRAD, lambda dx, ws, nb: lib.mg_conv_dgrad(g, gyd.data_ptr(), wd.data_ptr(), None, dx.data_ptr(), _lib.ACT_NONE, ws, nb, st),
            B * H * W * Ci, ref["dx"], True)
    if which in ("x", "dy", "out"):
        run(WGRAD, lambda dw, ws, nb: lib.mg_conv_wgrad(g, xd.data_ptr(), gyd.data_ptr(), dw.data_ptr(), None, 0, ws, nb, st),
            Co * k * k * Ci, ref["dw"], False)
