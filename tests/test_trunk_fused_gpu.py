"""The fused one-workgroup-per-slab kernels of the ResnetBlock trunk (csrc/wino.h, csrc/instnorm.hip) against plain float64
evaluations of the same operations, at every register depth NT they are instantiated for and at the tile counts next to each
depth's and each eligibility limit:

  wino_out_norm_kernel<NT>            inverse transform + InstanceNorm (+ act, + residual)      ops.conv_fwd_instnorm
  wino_out_norm_kernel<NT, true>      ... + the next layer's B^T y B image                       ops.conv_fwd_instnorm(v_next=)
  wino_norm_bwd_dy_kernel<NT>         InstanceNorm backward + A dy A^T                           ops.instnorm_bwd_wino_md
  wino_dd_gather_kernel<NT>           B dV B^T + gather (+ bias, act, + skip gradient)           ops.conv_dgrad
  wino_adam_kernel                    G^T dU G + Adam + G w' G^T                                 ops.conv_wgrad_adam
  norm_slab_fwd_kernel<NP, true>      InstanceNorm over a forward pass's split-K slabs           ops.conv_fwd_instnorm on LDS-DMA layers

Inputs are float64 values that float32 holds exactly (test_elementwise_gpu.f32_exact), so the device sees the numbers the
reference evaluates.  Bounds: a convolution 3e-5 of max|ref| (test_conv_gpu.py); a normalised output 1e-5 of max|ref| and an
InstanceNorm backward 2e-5 of max|ref| (test_elementwise_gpu.test_instnorm_fwd_bwd); mean / rstd the relative bars of
test_conv_gpu.test_conv_fwd_instnorm_matches_separate_calls; the single-addition transforms B^T . B and G . G^T 2^-21 of the
largest input (two passes, each output one rounded sum of inputs already carrying the first pass's rounding).  The statistics and
the normalised output are compared with a float64 InstanceNorm of the DEVICE's raw convolution output, which float64 holds
exactly: neither the convolution's rounding nor an activation decision enters those bounds.  Outputs lie in guard-filled arenas."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_amp_gpu import close_f16, h
from test_conv_plans_gpu import DMA_SHAPES
from test_elementwise_gpu import f32_exact

gpu = pytest.mark.gpu            # (per test, not per module: the table assertion needs the library's host-side queries only)
DEV = "cuda"
F32, F16 = 0, 1                  # mg_conv_geom.precision
GUARD, FILL = 1024, 3.25         # floats of FILL in front of and behind every output
EPS = 1e-5
ACTS = {"none": lambda t: t, "relu": torch.relu, "lrelu": lambda t: F.leaky_relu(t, 0.2), "tanh": torch.tanh}

# (B, Ci, Co, H, W) -> register depth NT of the two norm kernels (None: outside their range).  3x3, stride 1, pad 1.
TABLE = {
    (2, 32, 32, 2, 2): 1,          # one tile: a reflected row / column index lands on the opposite pixel
    (3, 64, 64, 2, 16): 1,
    (2, 32, 32, 8, 16): 1,         # 32 tiles: NT1 full
    (2, 32, 32, 6, 22): 2,         # 33
    (1, 96, 96, 8, 32): 2,         # 64: the hand-over and gather limit
    (2, 32, 32, 10, 26): 3,        # 65: first size past that limit
    (1, 64, 64, 12, 32): 3,        # 96
    (1, 32, 32, 14, 28): 4,        # 98
    (1, 32, 32, 18, 30): 5,        # 135
    (1, 64, 64, 20, 32): 5,        # 160: the fused norm's limit
    (1, 32, 32, 14, 46): None,     # 161 tiles; 644 pixels are also too many for the one-launch slab norm
    (2, 32, 48, 8, 16): None,      # Co % 32 != 0
    (2, 48, 32, 8, 16): 1,         # Ci is not a multiple of 32
}
ROWS = list(TABLE)
FUSED_ROWS = [r for r in ROWS if TABLE[r] is not None]
NEXT_ROWS = [r for r in FUSED_ROWS if (r[3] // 2) * (r[4] // 2) <= 64]
# data gradient: 1, 8, 32, 33, 64 and 65 tiles and the Ci == 48 row (wino_dd_gather_kernel<1>, <2>; past 64 tiles and with
# Ci % 32 != 0 the two-kernel path: wino_dd_xform_kernel + wino_dx_gather_kernel)
DGRAD_ROWS = [(2, 32, 32, 2, 2), (3, 64, 64, 2, 16), (2, 32, 32, 8, 16), (2, 32, 32, 6, 22), (1, 96, 96, 8, 32), (2, 32, 32, 10, 26),
              (2, 48, 32, 8, 16)]


def tiles_of(row):
    return (row[3] // 2) * (row[4] // 2)


def row_id(row):
    return "%dx%dto%dx%dx%d_%dtiles" % (row[0], row[1], row[2], row[3], row[4], tiles_of(row))


def geom(row, reflect, prec=F32):
    from mdctgan_amd import ops
    B, Ci, Co, H, W = row
    return ops.conv_geom(B, H, W, Ci, Co, 3, 3, 1, 1, reflect, prec)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def dev(t):
    """NCHW float64 (float32-exact) -> NHWC float32 on the device."""
    return nhwc(t).float().to(DEV)


def rel_err(got, want):
    return (got.double().cpu() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


def test_shape_table_reaches_every_depth_and_limit():
    """NT = 1..5 each occur for the two norm kernels; NT = 1 and 2 and their limits (32, 64 tiles; 65 beyond) for the hand-over
    instances and the gather; the library agrees about every row's eligibility in both padding modes."""
    from mdctgan_amd import ops
    for row, depth in TABLE.items():
        for reflect in (True, False):
            g = geom(row, reflect)
            assert ops.wino_weights_bytes(g) == 16 * row[1] * row[2] * 4, row          # every row is an F(2x2,3x3) layer
            assert ops.wino_md_from_norm_ok(g) == (depth is not None), row
            if depth is not None:
                assert depth == (tiles_of(row) + 31) // 32 and tiles_of(row) <= 160 and row[2] % 32 == 0, row
            assert ops.wino_vnext_ok(g) == (row in NEXT_ROWS), row
    assert sorted({TABLE[r] for r in FUSED_ROWS}) == [1, 2, 3, 4, 5]
    assert {tiles_of(r) for r in FUSED_ROWS} >= {1, 32, 33, 64, 65, 96, 98, 135, 160}
    assert sorted({TABLE[r] for r in NEXT_ROWS}) == [1, 2] and {32, 33, 64} <= {tiles_of(r) for r in NEXT_ROWS}
    assert max(tiles_of(r) for r in NEXT_ROWS) == 64 and (2, 32, 32, 10, 26) not in NEXT_ROWS
    gather = [r for r in DGRAD_ROWS if r[1] % 32 == 0 and tiles_of(r) <= 64]          # wino.h: wino_dd_gather_ok
    assert sorted({(tiles_of(r) + 31) // 32 for r in gather}) == [1, 2] and {1, 32, 33, 64} <= {tiles_of(r) for r in gather}
    assert {tiles_of(r) for r in DGRAD_ROWS if r not in gather} == {65, 32}
    out_of_range = [r for r in ROWS if TABLE[r] is None]
    assert len(out_of_range) == 2 and tiles_of(out_of_range[0]) == 161 and out_of_range[1][2] == 48


# ---- float64 references --------------------------------------------------------------------------------------------------
def conv64(x, w, b, reflect, stride=1, pad=1):
    if reflect and pad:
        x, pad = F.pad(x, (pad,) * 4, mode="reflect"), 0
    return F.conv2d(x, w, b, stride=stride, padding=pad)


def instnorm64(y_raw, act, res):
    """NHWC float64 -> (y, mean [B, C], rstd [B, C])."""
    mean = y_raw.mean((1, 2))
    rstd = 1.0 / torch.sqrt(y_raw.var((1, 2), unbiased=False) + EPS)
    y = ACTS[act]((y_raw - mean[:, None, None, :]) * rstd[:, None, None, :])
    return (y if res is None else y + res), mean, rstd


BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
AM = torch.tensor([[1, 0], [1, 1], [1, -1], [0, -1]], dtype=torch.float64)
GM = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)


def input_image64(y, reflect):
    """NHWC float64 -> V [16][T][C] = B^T d B over the 4x4 patches (origin 2t - 1) of the reflect- / zero-padded map."""
    B, H, W, C = y.shape
    yp = nhwc(F.pad(nchw(y), (1, 1, 1, 1), mode="reflect" if reflect else "constant"))
    d = yp.unfold(1, 4, 2).unfold(2, 4, 2)                                # [B, TH, TW, C, 4, 4]
    return torch.einsum("ir,btxcrs,js->ijbtxc", BT, d, BT).reshape(16, B * (H // 2) * (W // 2), C)


def dy_image64(dy):
    """NHWC float64 -> Md [16][T][C] = A dy A^T over the 2x2 tiles."""
    B, H, W, C = dy.shape
    d = dy.unfold(1, 2, 2).unfold(2, 2, 2)                                # [B, TH, TW, C, 2, 2]
    return torch.einsum("ir,btxcrs,js->ijbtxc", AM, d, AM).reshape(16, B * (H // 2) * (W // 2), C)


def weight_image64(w):
    """OHWI float64 -> U [16][Co][Ci] = G w G^T."""
    return torch.einsum("ir,orsc,js->ijoc", GM, w, GM).reshape(16, w.shape[0], w.shape[3])


@functools.lru_cache(maxsize=None)
def layer_case(row, reflect):
    """Inputs of a layer (NCHW float64, float32-exact) and its float64 convolution, data and weight gradients (NHWC / OHWI).
    Built once per (row, padding mode), shared and never written."""
    B, Ci, Co, H, W = row
    gen = torch.Generator().manual_seed(sum(p * q for p, q in zip(row, (3, 5, 7, 11, 13))) + int(reflect))
    x = f32_exact(torch.randn(B, Ci, H, W, generator=gen, dtype=torch.float64)).requires_grad_()
    w = f32_exact(torch.randn(Co, Ci, 3, 3, generator=gen, dtype=torch.float64) / np.sqrt(9 * Ci)).requires_grad_()
    b = f32_exact(torch.randn(Co, generator=gen, dtype=torch.float64))
    res = f32_exact(torch.randn(B, Co, H, W, generator=gen, dtype=torch.float64))
    gy = f32_exact(torch.randn(B, Co, H, W, generator=gen, dtype=torch.float64))
    bi = f32_exact(torch.randn(Ci, generator=gen, dtype=torch.float64))              # a data gradient's bias and skip gradient
    add = f32_exact(torch.randn(B, Ci, H, W, generator=gen, dtype=torch.float64))
    y = conv64(x, w, b, reflect)
    y.backward(gy)
    return dict(x=x.detach(), w=w.detach(), b=b, res=res, gy=gy, bi=bi, add=add, y=nhwc(y.detach()), dx=nhwc(x.grad),
                dw=nhwc(w.grad))


# ---- guarded launches ----------------------------------------------------------------------------------------------------
class Arena:
    """n floats for a kernel to write with GUARD floats of FILL on either side in the same allocation."""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), FILL, dtype=dtype, device=DEV)
        self.out = self.buf[GUARD:GUARD + n]

    def intact(self):
        return bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.n:] == FILL).all())


def fused_fwd(g, x, w, b, act, res, need_raw=True, u=None, v=None, v_filled=False, v_next=None, next_reflect=False):
    """ops.conv_fwd_instnorm's launch with y, y_raw, mean and rstd inside guard-filled arenas -> (rc, y, y_raw, mean, rstd)."""
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    n, nc = g.B * g.OH * g.OW * g.Co, g.B * g.Co
    ay, araw, am, ar = Arena(n), (Arena(n) if need_raw else None), Arena(nc), Arena(nc)
    ws = ops._ws(lib.mg_conv_fwd_instnorm_workspace(g), x.device)
    tiles = ops._tiles(u, v, None, None, ops.TILES_V_FILLED if v_filled else 0)
    head = (g, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(araw.out) if need_raw else None, EPS, act, _lib.ptr(res),
            _lib.ptr(ay.out), _lib.ptr(am.out), _lib.ptr(ar.out), _lib.ptr(ws), ws.numel(), _lib.stream(), tiles)
    if v_next is not None:
        rc = lib.mg_conv_fwd_instnorm_next(*head, _lib.ptr(v_next), int(bool(next_reflect)))
    else:
        rc = lib.mg_conv_fwd_instnorm_h(*head, None)
    torch.cuda.synchronize()
    for a in (ay, araw, am, ar):
        assert a is None or a.intact(), "a fused forward call wrote outside its outputs"
    shape = (g.B, g.OH, g.OW, g.Co)
    return rc, ay.out.view(shape), (araw.out.view(shape) if need_raw else None), am.out.view(g.B, g.Co), ar.out.view(g.B, g.Co)


def check_fwd_instnorm(g, xd, wd, bd, resd, y_conv64, res64, worst, raw_f16=False):
    """The checks of a conv + InstanceNorm forward call, over act x residual x need_raw.  y_conv64: the float64 convolution (NHWC)."""
    from mdctgan_amd import ops
    codes = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU02}
    for act, code in codes.items():
        for with_res in (False, True):
            rc, y, y_raw, mean, rstd = fused_fwd(g, xd, wd, bd, code, resd if with_res else None)
            assert rc == 0
            if raw_f16:
                close_f16(y_raw, y_conv64)
            else:
                e = rel_err(y_raw, y_conv64)
                worst["y_raw"] = max(worst.get("y_raw", 0.0), e)
                assert e < 3e-5, ("y_raw", act, with_res, e)
            y64, m64, r64 = instnorm64(y_raw.double().cpu(), act, res64 if with_res else None)
            em = (mean.double().cpu() - m64).abs().max().item() / (m64.abs().max().item() + 1.0)
            er = (rstd.double().cpu() - r64).abs().max().item() / r64.abs().max().item()
            ey = rel_err(y, y64)
            for k, e in (("mean", em), ("rstd", er), ("y", ey)):
                worst[k] = max(worst.get(k, 0.0), e)
            assert em <= 1e-6 and er <= 2e-6 and ey < 1e-5, (act, with_res, em, er, ey)
            rc, y2, raw2, mean2, rstd2 = fused_fwd(g, xd, wd, bd, code, resd if with_res else None, need_raw=False)
            assert rc == 0 and raw2 is None
            assert torch.equal(y2, y) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd), (act, with_res)


# ---- 1. conv + InstanceNorm forward ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_conv_instnorm_forward_against_float64(row, reflect):
    """wino_out_norm_kernel<1..5> (and, on the two out-of-range rows, the two-launch path with the same contract): y_raw against
    the float64 convolution at 3e-5; mean, rstd and y against a float64 InstanceNorm of the device's own y_raw at 1e-6 * (max|mean|
    + 1), 2e-6 * max|rstd| and 1e-5 * max|y|; need_raw=False gives the same y, mean and rstd bit for bit; guards intact.
    Worst observed over all rows (MI355X): y_raw 3.5e-7, mean 3.5e-8, rstd 5.4e-8, y 1.4e-7."""
    c = layer_case(row, reflect)
    g = geom(row, reflect)
    worst = {}
    check_fwd_instnorm(g, dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), dev(c["res"]), c["y"], nhwc(c["res"]), worst)
    print("fwd_instnorm %s reflect=%d: %s" % (row_id(row), reflect, " ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


# ---- 2. hand-over image ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("next_reflect", [True, False], ids=["next_reflect", "next_zero"])
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("row", NEXT_ROWS, ids=row_id)
def test_next_layer_image_against_float64(row, reflect, next_reflect):
    """wino_out_norm_kernel<1, true> / <2, true>: v_next against the float64 B^T y B of the device's y at 2^-21 * max|y| (each
    pass of the transform is one rounded sum of two inputs: 2^-24 * 2 max|y| after the first, twice that carried into the second
    plus 2^-24 * 4 max|y| of its own); bit-equal to the image a plain conv_fwd of the next layer keeps; the next layer's forward
    run from it against the float64 convolution of y at 3e-5.  y, y_raw, mean, rstd are those of the call without v_next.
    Worst observed (MI355X): v_next 2.1e-7 of max|y| (2^-21 = 4.8e-7), next layer 4.2e-7."""
    from mdctgan_amd import ops
    c = layer_case(row, reflect)
    g = geom(row, reflect)
    B, Ci, Co, H, W = row
    xd, wd, bd, resd = dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), dev(c["res"])
    g_next = ops.conv_geom(B, H, W, Co, Co, 3, 3, 1, 1, next_reflect)
    nv = 16 * B * tiles_of(row) * Co
    v_plain, _ = ops.wino_tile_buffers(g_next, DEV, want_md=False)
    assert v_plain is not None and v_plain.numel() == nv
    gen = torch.Generator().manual_seed(tiles_of(row))
    w2 = f32_exact(torch.randn(Co, Co, 3, 3, generator=gen, dtype=torch.float64) / np.sqrt(9 * Co))
    w2d = dev(w2)
    for act, with_res in ((ops.ACT_RELU, False), (ops.ACT_NONE, True)):          # the trunk's two layers: ReLU, then + skip
        res = resd if with_res else None
        av = Arena(nv)
        rc, y, y_raw, mean, rstd = fused_fwd(g, xd, wd, bd, act, res, v_next=av.out, next_reflect=next_reflect)
        assert rc == 0 and av.intact()
        rc0, y0, raw0, mean0, rstd0 = fused_fwd(g, xd, wd, bd, act, res)
        assert rc0 == 0 and torch.equal(y, y0) and torch.equal(y_raw, raw0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
        y64 = y.double().cpu()
        want = input_image64(y64, next_reflect)
        err = (av.out.double().cpu().view(16, -1, Co) - want).abs().max().item() / y64.abs().max().item()
        z_plain = ops.conv_fwd(g_next, y, w2d, v_out=v_plain)
        assert torch.equal(av.out, v_plain)
        z = ops.conv_fwd(g_next, y, w2d, v_out=av.out, v_filled=True)
        ez = rel_err(z, nhwc(conv64(nchw(y64), w2, None, next_reflect)))
        print("v_next %s reflect=%d next_reflect=%d act=%d: image %.3g of max|y|, next layer %.3g" % (row_id(row), reflect, next_reflect, act, err, ez))
        assert err <= 2.0 ** -21
        assert torch.equal(z, z_plain) and ez < 3e-5


@gpu
@pytest.mark.parametrize("row", [(2, 32, 32, 10, 26), (2, 32, 48, 8, 16)], ids=row_id)
def test_next_layer_image_is_refused_outside_its_range(row):
    """65 tiles (no NT3 instance keeps a plane in LDS) and Co % 32 != 0: MG_ERR_ARG, and the guard-filled v_next stays untouched."""
    from mdctgan_amd import ops
    c = layer_case(row, True)
    g = geom(row, True)
    assert not ops.wino_vnext_ok(g)
    v = torch.full((16 * row[0] * tiles_of(row) * row[2] + GUARD,), FILL, device=DEV)
    rc = fused_fwd(g, dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), ops.ACT_RELU, None, v_next=v, next_reflect=True)[0]
    assert rc == -1          # MG_ERR_ARG
    assert bool((v == FILL).all())
    with pytest.raises(ValueError):
        ops.conv_fwd_instnorm(g, dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), ops.ACT_RELU, None, EPS, v_next=v, next_reflect=True)
    torch.cuda.synchronize()
    assert bool((v == FILL).all())


# ---- 3. norm backward into md ---------------------------------------------------------------------------------------------
# row -> the generator seed of its synthetic y_raw and gy.  Chosen on the CPU so that the float64 normalised values keep clear of
# zero (asserted below): a ReLU / LeakyReLU mask decided in float32 from float32 statistics is then the float64 one.
NORM_BWD_SEEDS = {(2, 32, 32, 2, 2): 0, (3, 64, 64, 2, 16): 0, (2, 32, 32, 8, 16): 0, (2, 32, 32, 6, 22): 0, (1, 96, 96, 8, 32): 0,
                  (2, 32, 32, 10, 26): 0, (1, 64, 64, 12, 32): 1, (1, 32, 32, 14, 28): 1, (1, 32, 32, 18, 30): 0,
                  (1, 64, 64, 20, 32): 5, (2, 48, 32, 8, 16): 0}
# smallest |xhat|: 2.3e-4 2.6e-4 1.2e-4 3.3e-5 3.0e-5 4.8e-5 4.4e-5 2.0e-4 7.3e-5 6.8e-5 1.2e-4


def norm_bwd_inputs(row, seed):
    B, Ci, Co, H, W = row
    gen = torch.Generator().manual_seed(seed)
    y_raw = f32_exact(torch.randn(B, Co, H, W, generator=gen, dtype=torch.float64) * 3 + 1.5)
    gy = f32_exact(torch.randn(B, Co, H, W, generator=gen, dtype=torch.float64))
    return y_raw, gy


@functools.lru_cache(maxsize=None)
def norm_bwd_case(row):
    """y_raw, gy (NCHW float64), the float64 statistics, min|xhat| and, per activation, autograd's gradient at y_raw (NHWC)."""
    y_raw, gy = norm_bwd_inputs(row, NORM_BWD_SEEDS[row])
    want = {}
    for act in ("none", "relu", "lrelu"):
        yr = y_raw.clone().requires_grad_()
        ACTS[act](F.instance_norm(yr, eps=EPS)).backward(gy)
        want[act] = nhwc(yr.grad)
    mean = y_raw.mean((2, 3))
    rstd = 1.0 / torch.sqrt(y_raw.var((2, 3), unbiased=False) + EPS)
    return y_raw, gy, mean, rstd, F.instance_norm(y_raw, eps=EPS).abs().min().item(), want


@gpu
@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
@pytest.mark.parametrize("row", FUSED_ROWS, ids=row_id)
def test_norm_backward_image_against_float64(row, act):
    """wino_norm_bwd_dy_kernel<1..5> alone, from a synthetic y_raw and float64 statistics rounded to float32: md per element
    against A dy64 A^T, dy64 = float64 autograd through act(instance_norm(.)), at 4 * 2e-5 * max|dy64| (test_instnorm_fwd_bwd's
    backward bar times the at most four terms of an md element); then the data gradient (both padding modes) and the weight
    gradient started from the images against float64 at 3e-5.
    Worst observed (MI355X): md 2.7e-7 of max|dy64| (bound 8e-5), dx 4.3e-7, dw 8.3e-7."""
    from mdctgan_amd import ops
    code = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU02}[act]
    B, Ci, Co, H, W = row
    y_raw, gy, mean, rstd, min_xhat, want = norm_bwd_case(row)
    assert min_xhat > 1e-5, (row, min_xhat)          # the float32 mask is the float64 mask
    dy64 = want[act]
    g = geom(row, True)
    assert ops.wino_md_from_norm_ok(g)
    n = 16 * B * tiles_of(row) * Co
    amd = Arena(n)
    ops.instnorm_bwd_wino_md(g, dev(gy), dev(y_raw), mean.float().to(DEV), rstd.float().to(DEV), code, amd.out)
    torch.cuda.synchronize()
    assert amd.intact()
    err = (amd.out.double().cpu().view(16, -1, Co) - dy_image64(dy64)).abs().max().item() / dy64.abs().max().item()
    print("norm_bwd md %s %s: %.3g of max|dy64|, min|xhat| %.3g" % (row_id(row), act, err, min_xhat))
    assert err <= 4 * 2e-5
    # the two gradients from the images
    for reflect in (True, False):
        c = layer_case(row, reflect)
        gr = geom(row, reflect)
        x = c["x"].clone().requires_grad_()
        w = c["w"].clone().requires_grad_()
        conv64(x, w, None, reflect).backward(nchw(dy64))
        xd, wd = dev(c["x"]), dev(c["w"])
        adx = Arena(B * H * W * Ci)
        dx = ops.conv_dgrad(gr, None, wd, md_out=amd.out, out=adx.out.view(B, H, W, Ci))
        torch.cuda.synchronize()
        e_dx = rel_err(dx, nhwc(x.grad))
        v, _ = ops.wino_tile_buffers(gr, DEV, want_md=False)
        ops.conv_fwd(gr, xd, wd, v_out=v)
        adw = Arena(Co * 9 * Ci)
        dw = adw.out.view(Co, 3, 3, Ci)
        ops.conv_wgrad(gr, None, None, dw, None, v=v, md=amd.out)
        torch.cuda.synchronize()
        e_dw = rel_err(dw, nhwc(w.grad))
        print("  from the images, reflect=%d: dx %.3g dw %.3g" % (reflect, e_dx, e_dw))
        assert adx.intact() and adw.intact() and amd.intact()
        assert e_dx < 3e-5 and e_dw < 3e-5


# ---- 4. data gradient with bias, act and add -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("row", DGRAD_ROWS, ids=row_id)
def test_data_gradient_bias_act_add_against_float64(row, reflect):
    """wino_dd_gather_kernel<1>, <2> (and the two-kernel path at 65 tiles and with Ci == 48): dx against float64
    act(L(dy) + bias) + add, L autograd's data gradient of the padded convolution, at 3e-5 of the maximum; act over none, relu,
    lrelu, tanh; bias and add each present and absent; guards around dx.
    Worst observed (MI355X): 1.5e-6."""
    from mdctgan_amd import ops
    codes = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU02, "tanh": ops.ACT_TANH}
    B, Ci, Co, H, W = row
    c = layer_case(row, reflect)
    g = geom(row, reflect)
    gyd, wd, bid, addd = dev(c["gy"]), dev(c["w"]), c["bi"].float().to(DEV), dev(c["add"])
    worst = 0.0
    for act, code in codes.items():
        for with_bias in (False, True):
            for with_add in (False, True):
                pre = c["dx"] + c["bi"] if with_bias else c["dx"]
                want = ACTS[act](pre) + (nhwc(c["add"]) if with_add else 0.0)
                a = Arena(B * H * W * Ci)
                dx = ops.conv_dgrad(g, gyd, wd, bid if with_bias else None, code, out=a.out.view(B, H, W, Ci),
                                    add=addd if with_add else None)
                torch.cuda.synchronize()
                err = rel_err(dx, want)
                worst = max(worst, err)
                assert a.intact() and err < 3e-5, (act, with_bias, with_add, err)
    print("dgrad bias/act/add %s reflect=%d: worst %.3g" % (row_id(row), reflect, worst))


# ---- 5. weight side --------------------------------------------------------------------------------------------------------
B1, B2, ADAM_EPS, LR = 0.5, 0.999, 1e-8, 2e-4
B2_DEV = float(np.float32(B2))          # the C ABI takes the betas as floats: the value the device clock raises to the step
WEIGHT_GEOMS = [(32, 32), (48, 80), (96, 64)]          # (Co, Ci) on the 8 x 16 map, batch 2


def clock(steps):
    """The device-resident Adam clock {step, lr, lr / (1 - b1^step), sqrt(1 - b2^step), the next step's two terms} after `steps`
    ticks from a primed start."""
    from mdctgan_amd import ops
    state = torch.zeros(6, dtype=torch.float64, device=DEV)
    state[1] = LR
    ops.adam_prime(state, B1, B2)
    for _ in range(steps):
        ops.adam_tick(state, B1, B2)
    return state


@gpu
@pytest.mark.parametrize("steps", [0, 7])
def test_adam_clock_next_step_terms_against_float64(steps):
    """state[4] = 1 - b1^(step + 1) and state[5] = sqrt(1 - b2^(step + 1)) after mg_adam_prime and after each tick: 1e-12
    relative (double pow and sqrt are good to a few 2^-53; 1 - 0.999^n cancels up to three digits).  Worst observed (MI355X): 0, the host's doubles."""
    from mdctgan_amd import ops
    state = torch.zeros(6, dtype=torch.float64, device=DEV)
    state[0], state[1] = steps, LR
    ops.adam_prime(state, B1, B2)
    worst = 0.0
    for tick in range(3):
        s = state.cpu()
        step = steps + tick
        assert s[0].item() == step and s[1].item() == LR
        want = {4: 1.0 - B1 ** (step + 1), 5: math.sqrt(1.0 - B2_DEV ** (step + 1))}
        if tick:
            want.update({2: LR / (1.0 - B1 ** step), 3: math.sqrt(1.0 - B2_DEV ** step)})
        for i, wv in want.items():
            worst = max(worst, abs(s[i].item() - wv) / wv)
            assert abs(s[i].item() - wv) <= 1e-12 * wv, (step, i, s[i].item(), wv)
        ops.adam_tick(state, B1, B2)
    print("adam clock from step %d: worst %.3g" % (steps, worst))


@gpu
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("steps", [0, 7])
@pytest.mark.parametrize("co_ci", WEIGHT_GEOMS, ids=lambda c: "co%d_ci%d" % c)
def test_wgrad_adam_fusion_is_bit_identical(co_ci, steps, grad_scale):
    """wino_adam_kernel (ops.conv_wgrad_adam) from non-zero moments, a clock at step 0 and at step 7 and a gradient scale: w, m, v
    and u bit-equal to conv_wgrad, tick, adam_step_dev, wino_weights from the same start -- from x and dy and (where the layer's
    A dy A^T image may be handed over: Co % 32 == 0) from the images alone.  The chain is anchored: the separate dw against float64
    at 3e-5, u against the float64 G w' G^T of the updated weights at 2^-21 * max|w'|, and the step moves the weights by about lr.
    Worst observed (MI355X): dw 3.5e-7, u 7.1e-8 of max|w'| (2^-21 = 4.8e-7); largest step 1.0 to 1.5 lr."""
    from mdctgan_amd import ops
    Co, Ci = co_ci
    row = (2, Ci, Co, 8, 16)
    c = layer_case(row, True)
    g = geom(row, True)
    assert ops.wgrad_adam_ok(g)
    xd, gyd, w0 = dev(c["x"]), dev(c["gy"]), dev(c["w"])
    gen = torch.Generator().manual_seed(Co + Ci)
    m0 = (torch.randn(Co, 3, 3, Ci, generator=gen) * 0.05).to(DEV)
    v0 = (torch.rand(Co, 3, 3, Ci, generator=gen) * 1e-2 + 1e-4).to(DEV)
    state = clock(steps)
    images = [(xd, gyd, None, None)]
    if ops.wino_md_from_norm_ok(g):
        v_img, md_img = ops.wino_tile_buffers(g, DEV)
        ops.conv_fwd(g, xd, w0, v_out=v_img)
        ops.conv_dgrad(g, gyd, w0, md_out=md_img)
        images.append((None, None, v_img, md_img))
    else:
        assert Co % 32 != 0
    for x_, dy_, v_, md_ in images:
        # separate: gradient, tick, step, transform
        dw = torch.full((Co, 3, 3, Ci), FILL, device=DEV)
        ops.conv_wgrad(g, x_, dy_, dw, None, v=v_, md=md_)
        e_dw = rel_err(dw, c["dw"])
        w1, m1, v1, st1 = w0.clone(), m0.clone(), v0.clone(), state.clone()
        ops.adam_tick(st1, B1, B2)
        ops.adam_step_dev(w1, dw, m1, v1, st1, B1, B2, ADAM_EPS, grad_scale)
        u1 = ops.wino_weights(g, w1)
        # fused (the clock has not ticked yet)
        aw, am, av, au = Arena(Co * 9 * Ci), Arena(Co * 9 * Ci), Arena(Co * 9 * Ci), Arena(16 * Co * Ci)
        for a, t in ((aw, w0), (am, m0), (av, v0)):
            a.out.copy_(t.view(-1))
        st2 = state.clone()
        ops.conv_wgrad_adam(g, x_, dy_, aw.out, am.out, av.out, au.out, st2, B1, B2, ADAM_EPS, grad_scale, v=v_, md=md_)
        torch.cuda.synchronize()
        assert all(a.intact() for a in (aw, am, av, au)) and torch.equal(st2, state)
        for name, got, want in (("w", aw.out, w1), ("m", am.out, m1), ("v", av.out, v1), ("u", au.out, u1)):
            assert torch.equal(got, want.view(-1)), (name, (got - want.view(-1)).abs().max().item())
        w64 = w1.double().cpu()
        e_u = (u1.double().cpu().view(16, Co, Ci) - weight_image64(w64)).abs().max().item() / w64.abs().max().item()
        moved = (w1 - w0).abs().max().item()
        print("wgrad_adam co%d ci%d steps=%d scale=%g images=%d: dw %.3g, u %.3g of max|w'|, max step %.3g" % (Co, Ci, steps, grad_scale, x_ is None, e_dw, e_u, moved))
        assert e_dw < 3e-5 and e_u <= 2.0 ** -21
        assert 0.01 * LR < moved < 100 * LR          # a step of the order of lr: neither none nor one without bias correction


# ---- 6. slab-summing norm at small sizes -----------------------------------------------------------------------------------
# (B, Ci, H, W, Co, k, stride, pad, reflect) -> NP of norm_slab_fwd_kernel<NP, true> (pixels per sample <= 128 / 256 / 512 / 640)
SLAB_SHAPES = {"s2_3x3_45px": ((2, 128, 9, 17, 256, 3, 2, 1, False), 4),
               "s1_3x3_reflect_320px": ((2, 64, 5, 64, 64, 3, 1, 1, True), 16)}          # (an odd height: off the Winograd route)
SLAB_SHAPES.update({name: (shape, {153: 8, 256: 8, 513: 20}[((shape[2] + 2 * shape[7] - shape[5]) // shape[6] + 1) *
                                                           ((shape[3] + 2 * shape[7] - shape[5]) // shape[6] + 1)])
                    for name, (shape, _, _) in DMA_SHAPES.items()})


def test_slab_shapes_reach_every_depth():
    assert sorted({np_ for _, np_ in SLAB_SHAPES.values()}) == [4, 8, 16, 20]


@functools.lru_cache(maxsize=None)
def slab_case(name, prec):
    """Inputs (float32-exact) and the float64 convolution of the arithmetic the precision stands for (MG_PRECISION_F16:
    test_amp_gpu.py's autocast reference -- operands rounded to float16, exact products, wide accumulation)."""
    B, Ci, H, W, Co, k, s, p, reflect = SLAB_SHAPES[name][0]
    gen = torch.Generator().manual_seed(len(name) + 100 * prec)
    x = f32_exact(torch.randn(B, Ci, H, W, generator=gen, dtype=torch.float64))
    w = f32_exact(torch.randn(Co, Ci, k, k, generator=gen, dtype=torch.float64) / np.sqrt(Ci * k * k))
    b = f32_exact(torch.randn(Co, generator=gen, dtype=torch.float64))
    y = conv64(h(x) if prec == F16 else x, h(w) if prec == F16 else w, b, reflect, s, p)
    res = f32_exact(torch.randn(y.shape, generator=gen, dtype=torch.float64))
    return x, w, b, res, nhwc(y)


@gpu
@pytest.mark.parametrize("prec", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("name", list(SLAB_SHAPES))
def test_instnorm_over_split_k_slabs_against_float64(name, splits, prec, monkeypatch):
    """norm_slab_fwd_kernel<4 / 8 / 16 / 20, true> behind an LDS-DMA forward pass forced to 2 and 3 K splits: the route and the
    split are asserted first, then the checks of test_conv_instnorm_forward_against_float64 (MG_PRECISION_F16: y_raw against the
    autocast reference with close_f16), and y, y_raw, mean, rstd bit-equal to the epilogue + norm launches of MG_NO_FWD_DEFER=1.
    Worst observed (MI355X): y_raw 8.5e-7 (float32), mean 3.5e-8, rstd 5.3e-8, y 1.2e-7."""
    from mdctgan_amd import _lib, ops
    shape, np_ = SLAB_SHAPES[name]
    B, Ci, H, W, Co, k, s, p, reflect = shape
    monkeypatch.setenv("MG_FORCE_CONV_DMA", "64,64,%d" % splits)
    monkeypatch.delenv("MG_NO_FWD_DEFER", raising=False)
    g = ops.conv_geom(B, H, W, Ci, Co, k, k, s, p, reflect, prec)
    assert ops.plan_name(0, g) == "conv_fwd_dma_kernel<64, 64, %s, 2>" % ("true" if prec == F16 else "false")
    assert _lib.load().mg_conv_plan_splits(0, g) == splits
    hw = g.OH * g.OW
    assert Co % 32 == 0 and np_ == (4 if hw <= 128 else 8 if hw <= 256 else 16 if hw <= 512 else 20) and hw <= 640
    x, w, b, res, y64 = slab_case(name, prec)
    xd, wd, bd, resd = dev(x), dev(w), b.float().to(DEV), dev(res)
    worst = {}
    check_fwd_instnorm(g, xd, wd, bd, resd, y64, nhwc(res), worst, raw_f16=prec == F16)
    print("slab norm %s splits=%d prec=%d NP=%d: %s" % (name, splits, prec, np_, " ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU02):
        for r in (None, resd):
            monkeypatch.delenv("MG_NO_FWD_DEFER", raising=False)
            got = fused_fwd(g, xd, wd, bd, act, r)
            monkeypatch.setenv("MG_NO_FWD_DEFER", "1")
            two = fused_fwd(g, xd, wd, bd, act, r)
            assert got[0] == 0 and two[0] == 0
            for a, b_ in zip(got[1:], two[1:]):
                assert torch.equal(a, b_), (act, r is not None)
