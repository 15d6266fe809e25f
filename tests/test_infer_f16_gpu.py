"""The opt-in half-precision inference mode (MG_PRECISION_F16_INFER, csrc/wino_h16.h) on the GPU:

  winoh_{weight,input}_xform_kernel + winoh_gemm_kernel + wino_output_xform_kernel(round_f16)     ops.conv_fwd
  winoh_out_norm_kernel<NT>          inverse transform + float16 rounding + InstanceNorm (+ act, + residual)   ops.conv_fwd_instnorm
  winoh_out_norm_kernel<NT, true>    ... + the next layer's float16 image                            ops.conv_fwd_instnorm(v_next=)
  amp.infer_f16 / --infer_fp16 / MG_INFER_F16                                                         Pix2PixHDModel.inference

Inputs of the op-level cases are float16-representable, so "the float64 convolution" is one number whether the operands are
rounded first or not; outputs lie in guard-filled arenas.  The convolution bar is the one tests/test_amp_gpu.py holds the float16
Winograd forward to, close_f16(ulps=4.0, floor=2**-9), which also asserts float16-representable outputs; the InstanceNorm bars are
those of test_trunk_fused_gpu.check_fwd_instnorm, against a float64 InstanceNorm of the DEVICE's own raw output.
MG_INFER_F16_MIN_C=64 and MG_INFER_F16_MIN_TILES=1 bring the route's thresholds (256 channels, 256 tiles) down to the test shapes."""
import functools

import numpy as np
import pytest
import torch

import test_trunk_fused_gpu as TF
from test_amp_gpu import close_f16
from test_trunk_fused_gpu import ACTS, DEV, EPS, Arena, conv64, instnorm64, nchw, nhwc, rel_err

pytestmark = pytest.mark.gpu
F16, HINF = 1, 3
BAR = dict(ulps=4.0, floor=2.0 ** -9)

# (B, Ci, Co, H, W), 3x3 stride 1 pad 1
PLAIN_ROWS = [
    (2, 64, 64, 2, 2),          # T = 2: one ragged row tile; a reflected index lands on the opposite pixel
    (3, 64, 128, 4, 32),        # T = 96: not a multiple of 64
    (2, 128, 64, 8, 16),        # two K chunks
    (1, 64, 64, 4, 164),        # 2 x 82 tiles per sample
]
DEFAULT_ROW = (8, 256, 256, 8, 16)          # no overrides: the default thresholds
INELIGIBLE_ROW = (1, 64, 96, 8, 16)         # Co % 64 != 0
# tiles per sample 1, 32, 33, 64, 65, 96, 98, 160 (the fused tail's NT = 1..5 and its limits) and 161 (the unfused sequence)
NORM_ROWS = [(2, 64, 64, 2, 2), (2, 64, 64, 8, 16), (2, 64, 64, 6, 22), (1, 64, 64, 8, 32), (2, 64, 64, 10, 26), (1, 64, 64, 12, 32),
             (1, 64, 64, 14, 28), (1, 64, 64, 20, 32), (1, 64, 64, 14, 46)]
NEXT_ROWS = [r for r in NORM_ROWS if (r[3] // 2) * (r[4] // 2) <= 64]


def tiles_of(row):
    return (row[3] // 2) * (row[4] // 2)


def row_id(row):
    return "%dx%dto%dx%dx%d_%dtiles" % (row[0], row[1], row[2], row[3], row[4], tiles_of(row))


def geom(row, reflect, prec=HINF):
    from mdctgan_amd import ops
    B, Ci, Co, H, W = row
    return ops.conv_geom(B, H, W, Ci, Co, 3, 3, 1, 1, reflect, prec)


def h(t):
    return t.half().double()


def dev(t):
    return nhwc(t).float().to(DEV)


@pytest.fixture()
def small_shapes(monkeypatch):
    monkeypatch.setenv("MG_INFER_F16_MIN_C", "64")
    monkeypatch.setenv("MG_INFER_F16_MIN_TILES", "1")


@functools.lru_cache(maxsize=None)
def layer_case(row, reflect):
    """float16-representable inputs of a layer (NCHW float64) and its float64 convolution with and without the bias (NHWC).
    Built once per (row, padding mode), shared and never written."""
    B, Ci, Co, H, W = row
    gen = torch.Generator().manual_seed(sum(p * q for p, q in zip(row, (3, 5, 7, 11, 13))) + int(reflect))
    x = h(torch.randn(B, Ci, H, W, generator=gen, dtype=torch.float64))
    w = h(torch.randn(Co, Ci, 3, 3, generator=gen, dtype=torch.float64) / np.sqrt(9 * Ci))
    b = torch.randn(Co, generator=gen, dtype=torch.float64).float().double()
    res = torch.randn(B, Co, H, W, generator=gen, dtype=torch.float64).float().double()
    return dict(x=x, w=w, b=b, res=res, y=nhwc(conv64(x, w, b, reflect)), y_nobias=nhwc(conv64(x, w, None, reflect)))


def is_winoh(g):
    from mdctgan_amd import ops
    return ops.plan_name(0, g).startswith("winoh_gemm_kernel") and ops.wino_weights_bytes(g) == 16 * g.Co * g.Ci * 2


def guarded_conv(g, x, w, b, act, u=None, v=None, v_filled=False):
    """ops.conv_fwd with y inside a guard-filled arena."""
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    ay = Arena(g.B * g.OH * g.OW * g.Co)
    ws = ops._ws(lib.mg_conv_fwd_workspace(g), x.device)
    rc = lib.mg_conv_fwd_w(g, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(ay.out), act, _lib.ptr(ws), ws.numel(), _lib.stream(),
                           ops._tiles(u, v, None, None, ops.TILES_V_FILLED if v_filled else 0))
    torch.cuda.synchronize()
    assert rc == 0 and ay.intact()
    return ay.out.view(g.B, g.OH, g.OW, g.Co)


def fused_fwd(g, x, w, b, act, res, need_raw=True, u=None, v=None, v_filled=False, v_next=None, next_reflect=False, y16=None):
    """The conv + InstanceNorm launch with y, y_raw, mean and rstd inside guard-filled arenas -> (rc, y, y_raw, mean, rstd).
    v_next (float16): through mg_conv_fwd_instnorm_next_h."""
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    n, nc = g.B * g.OH * g.OW * g.Co, g.B * g.Co
    ay, araw, am, ar = Arena(n), (Arena(n) if need_raw else None), Arena(nc), Arena(nc)
    ws = ops._ws(lib.mg_conv_fwd_instnorm_workspace(g), x.device)
    tiles = ops._tiles(u, v, None, None, ops.TILES_V_FILLED if v_filled else 0)
    head = (g, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(araw.out) if need_raw else None, EPS, act, _lib.ptr(res),
            _lib.ptr(ay.out), _lib.ptr(am.out), _lib.ptr(ar.out), _lib.ptr(ws), ws.numel(), _lib.stream(), tiles)
    if v_next is not None:
        rc = lib.mg_conv_fwd_instnorm_next_h(*head, _lib.ptr(v_next), int(bool(next_reflect)), _lib.ptr(y16))
    else:
        rc = lib.mg_conv_fwd_instnorm_h(*head, _lib.ptr(y16))
    torch.cuda.synchronize()
    for a in (ay, araw, am, ar):
        assert a is None or a.intact(), "a fused forward call wrote outside its outputs"
    shape = (g.B, g.OH, g.OW, g.Co)
    return rc, ay.out.view(shape), (araw.out.view(shape) if need_raw else None), am.out.view(g.B, g.Co), ar.out.view(g.B, g.Co)


# ---- 1. plain pipeline ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("row", PLAIN_ROWS, ids=row_id)
def test_plain_pipeline_against_float64(small_shapes, row, reflect):
    """float16(G w G^T), float16(B^T d B), the 16-position float16 GEMM, act(A^T M A + bias) rounded through float16, against the
    float64 convolution at close_f16(4 ulps, 2^-9 of the largest element), with a bias under each activation and without one; a
    prepared U16 and a second call give the same bits.
    Worst observed over all rows (MI355X): 6.3e-4 of max|ref|, 2.0e-3 under tanh."""
    from mdctgan_amd import ops
    c = layer_case(row, reflect)
    g = geom(row, reflect)
    assert is_winoh(g), ops.plan_name(0, g)
    xd, wd, bd = dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV)
    codes = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU02, "tanh": ops.ACT_TANH}
    for act, code in codes.items():
        got = guarded_conv(g, xd, wd, bd, code)
        want = ACTS[act](c["y"])
        print("infer_f16 plain %s reflect=%d act=%s: %.3g of max|ref|" % (row_id(row), reflect, act, rel_err(got, want)))
        close_f16(got, want, **BAR)
    got = guarded_conv(g, xd, wd, None, ops.ACT_NONE)
    print("infer_f16 plain %s reflect=%d no bias: %.3g of max|ref| (%s)" % (row_id(row), reflect, rel_err(got, c["y_nobias"]),
                                                                           ops.plan_name(0, g)))
    close_f16(got, c["y_nobias"], **BAR)
    u = ops.wino_weights(g, wd)
    assert u is not None and u.numel() * 4 == 16 * row[1] * row[2] * 2
    assert torch.equal(guarded_conv(g, xd, wd, None, ops.ACT_NONE, u=u), got)
    assert torch.equal(guarded_conv(g, xd, wd, None, ops.ACT_NONE), got)


def test_default_thresholds_row_against_float64():
    """(8, 256 -> 256, 8 x 16) with nothing in the environment: the route, the bar, a prepared U16 and repeatability."""
    import os
    from mdctgan_amd import ops
    assert "MG_INFER_F16_MIN_C" not in os.environ and "MG_INFER_F16_MIN_TILES" not in os.environ
    for reflect in (True, False):
        c = layer_case(DEFAULT_ROW, reflect)
        g = geom(DEFAULT_ROW, reflect)
        assert is_winoh(g), ops.plan_name(0, g)
        xd, wd, bd = dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV)
        got = guarded_conv(g, xd, wd, bd, ops.ACT_NONE)
        print("infer_f16 plain %s reflect=%d: %.3g of max|ref|" % (row_id(DEFAULT_ROW), reflect, rel_err(got, c["y"])))
        close_f16(got, c["y"], **BAR)
        assert torch.equal(guarded_conv(g, xd, wd, bd, ops.ACT_NONE, u=ops.wino_weights(g, wd)), got)
        assert torch.equal(guarded_conv(g, xd, wd, bd, ops.ACT_NONE), got)


@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
def test_ineligible_geometry_runs_as_float16(small_shapes, reflect):
    """Co % 64 != 0: the plan names and the output bits of MG_PRECISION_F16, through the plain call and the conv + InstanceNorm call."""
    from mdctgan_amd import ops
    row = INELIGIBLE_ROW
    c = layer_case(row, reflect)
    xd, wd, bd, resd = dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), dev(c["res"])
    g, g16 = geom(row, reflect), geom(row, reflect, F16)
    assert not is_winoh(g)
    assert [ops.plan_name(p, g) for p in range(3)] == [ops.plan_name(p, g16) for p in range(3)]
    for act in (ops.ACT_NONE, ops.ACT_RELU):
        assert torch.equal(guarded_conv(g, xd, wd, bd, act), guarded_conv(g16, xd, wd, bd, act))
    a = fused_fwd(g, xd, wd, bd, ops.ACT_RELU, resd)
    b = fused_fwd(g16, xd, wd, bd, ops.ACT_RELU, resd)
    assert a[0] == 0 and b[0] == 0 and all(torch.equal(p, q) for p, q in zip(a[1:], b[1:]))


# ---- 2. fused output transform + InstanceNorm ------------------------------------------------------------------------------
def test_norm_rows_reach_every_depth():
    assert [tiles_of(r) for r in NORM_ROWS] == [1, 32, 33, 64, 65, 96, 98, 160, 161]
    assert sorted({(tiles_of(r) + 31) // 32 for r in NORM_ROWS[:-1]}) == [1, 2, 3, 4, 5]
    assert [tiles_of(r) for r in NEXT_ROWS] == [1, 32, 33, 64]


@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("row", NORM_ROWS, ids=row_id)
def test_conv_instnorm_forward_against_float64(small_shapes, row, reflect):
    """winoh_out_norm_kernel<1..5> (161 tiles: wino_output_xform_kernel(round_f16) + the InstanceNorm call, same contract): y_raw
    against the float64 convolution at the bar above; mean, rstd and y against a float64 InstanceNorm of the device's own y_raw at
    1e-6 * (max|mean| + 1), 2e-6 * max|rstd| and 1e-5 * max|y| over act x residual; need_raw=False gives the same y, mean and rstd
    bit for bit; the optional float16 copy of y is float16(y); guards intact.
    Worst observed over all rows (MI355X): y_raw 6.1e-4 of max|ref|, mean 3.6e-8, rstd 5.4e-8, y 1.0e-7."""
    from mdctgan_amd import ops
    c = layer_case(row, reflect)
    g = geom(row, reflect)
    assert is_winoh(g), ops.plan_name(0, g)
    assert ops.wino_vnext_ok(g) == (tiles_of(row) <= 64)
    xd, wd, bd, resd = dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), dev(c["res"])
    res64 = nhwc(c["res"])
    worst = {}
    for act, code in {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU02}.items():
        for with_res in (False, True):
            res = resd if with_res else None
            rc, y, y_raw, mean, rstd = fused_fwd(g, xd, wd, bd, code, res)
            assert rc == 0
            worst["y_raw"] = max(worst.get("y_raw", 0.0), rel_err(y_raw, c["y"]))
            y64, m64, r64 = instnorm64(y_raw.double().cpu(), act, res64 if with_res else None)
            em = (mean.double().cpu() - m64).abs().max().item() / (m64.abs().max().item() + 1.0)
            er = (rstd.double().cpu() - r64).abs().max().item() / r64.abs().max().item()
            ey = rel_err(y, y64)
            for k, e in (("mean", em), ("rstd", er), ("y", ey)):
                worst[k] = max(worst.get(k, 0.0), e)
            print("infer_f16 fwd_instnorm %s reflect=%d act=%s res=%d: y_raw %.3g mean %.3g rstd %.3g y %.3g"
                  % (row_id(row), reflect, act, with_res, rel_err(y_raw, c["y"]), em, er, ey))
            close_f16(y_raw, c["y"], **BAR)
            assert em <= 1e-6 and er <= 2e-6 and ey < 1e-5, (act, with_res, em, er, ey)
            rc, y2, raw2, mean2, rstd2 = fused_fwd(g, xd, wd, bd, code, res, need_raw=False)
            assert rc == 0 and raw2 is None
            assert torch.equal(y2, y) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd), (act, with_res)
    a16 = Arena(y.numel(), dtype=torch.float16)
    rc, y3, _, _, _ = fused_fwd(g, xd, wd, bd, ops.ACT_LRELU02, resd, need_raw=False, y16=a16.out)
    assert rc == 0 and a16.intact() and torch.equal(y3, y) and torch.equal(a16.out.view(y.shape), y.half())


# ---- 3. hand-over image ----------------------------------------------------------------------------------------------------
def f16_ulp(v):
    """Spacing of float16 at |v| (float64 tensor): 2^(floor(log2 |v|) - 10), 2^-24 below the smallest normal."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -30))
    return torch.pow(2.0, (e - 1).clamp_min(-14).double() - 10.0)


@pytest.mark.parametrize("next_reflect", [True, False], ids=["next_reflect", "next_zero"])
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("row", NEXT_ROWS, ids=row_id)
def test_next_layer_image(small_shapes, row, reflect, next_reflect):
    """winoh_out_norm_kernel<1, true> / <2, true>: every element of v_next within one float16 ulp of float16(B^T y B) computed in
    float64 from the device's y (the kernel sums in double, exactly, and rounds once); bit-equal to the image a plain conv_fwd of
    the next layer keeps; the next layer gives the same bits from it as when it transforms y itself, and meets the convolution bar.
    y, y_raw, mean, rstd are those of the call without v_next.
    Observed (MI355X): at most 4 of 65 536 elements differ from the float64 image, each by one ulp."""
    from mdctgan_amd import ops
    c = layer_case(row, reflect)
    g = geom(row, reflect)
    B, Ci, Co, H, W = row
    assert is_winoh(g) and ops.wino_vnext_ok(g) and ops.wino_vnext_positions(g) == 16 and ops.wino_images_half(g)
    xd, wd, bd, resd = dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), dev(c["res"])
    g_next = ops.conv_geom(B, H, W, Co, Co, 3, 3, 1, 1, next_reflect, HINF)
    assert is_winoh(g_next)
    nv = 16 * B * tiles_of(row) * Co
    v_plain, _ = ops.wino_tile_buffers(g_next, DEV, want_md=False)
    assert v_plain is not None and v_plain.numel() * 4 == nv * 2
    v_plain = v_plain.view(torch.float16)
    gen = torch.Generator().manual_seed(tiles_of(row))
    w2 = h(torch.randn(Co, Co, 3, 3, generator=gen, dtype=torch.float64) / np.sqrt(9 * Co))
    w2d = dev(w2)
    for act, with_res in ((ops.ACT_RELU, False), (ops.ACT_NONE, True)):          # the trunk's two layers: ReLU, then + skip
        res = resd if with_res else None
        av = Arena(nv, dtype=torch.float16)
        rc, y, y_raw, mean, rstd = fused_fwd(g, xd, wd, bd, act, res, v_next=av.out, next_reflect=next_reflect)
        assert rc == 0 and av.intact()
        rc0, y0, raw0, mean0, rstd0 = fused_fwd(g, xd, wd, bd, act, res)
        assert rc0 == 0 and torch.equal(y, y0) and torch.equal(y_raw, raw0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
        y64 = y.double().cpu()
        want = h(TF.input_image64(y64, next_reflect))
        got = av.out.double().cpu().view(16, -1, Co)
        off = ((got - want).abs() / f16_ulp(want)).max().item()
        z_plain = guarded_conv(g_next, y, w2d, None, ops.ACT_NONE, v=v_plain)
        assert torch.equal(av.out, v_plain)
        z = guarded_conv(g_next, y, w2d, None, ops.ACT_NONE, v=av.out, v_filled=True)
        print("infer_f16 v_next %s reflect=%d next_reflect=%d act=%d: image off by at most %.3g float16 ulp, %d of %d elements differ"
              % (row_id(row), reflect, next_reflect, act, off, int((got != want).sum()), got.numel()))
        assert off <= 1.0
        assert torch.equal(z, z_plain)
        # (y is not float16-representable: the bar's reference is the convolution of y itself, whose image the layer rounds)
        close_f16(z, nhwc(conv64(nchw(y64), w2, None, next_reflect)), **BAR)


def test_next_layer_image_is_refused_outside_its_range(small_shapes):
    """65 tiles: MG_ERR_ARG from the float16 entry point, and the guard-filled v_next stays untouched; the float32 entry point
    refuses a layer whose image is float16."""
    from mdctgan_amd import _lib, ops
    row = (2, 64, 64, 10, 26)
    c = layer_case(row, True)
    g = geom(row, True)
    assert is_winoh(g) and not ops.wino_vnext_ok(g)
    v = torch.full((16 * row[0] * tiles_of(row) * row[2] + TF.GUARD,), TF.FILL, device=DEV, dtype=torch.float16)
    rc = fused_fwd(g, dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), ops.ACT_RELU, None, v_next=v, next_reflect=True)[0]
    assert rc == -1 and bool((v == TF.FILL).all())
    row = (2, 64, 64, 8, 16)
    c = layer_case(row, True)
    vf = torch.full((16 * 2 * 32 * 64 + TF.GUARD,), TF.FILL, device=DEV)
    rc = TF.fused_fwd(geom(row, True), dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), ops.ACT_RELU, None, v_next=vf, next_reflect=True)[0]
    assert rc == -1 and bool((vf == TF.FILL).all())


def test_functional_layers_hand_the_image_over(small_shapes):
    """functional.conv_instnorm under no_grad inside amp.infer_f16: the first layer attaches a float16 image, the second consumes it
    (WINO_NEXT_STATS) and gives the bits it gives without one; with gradients enabled the context changes nothing."""
    from mdctgan_amd import amp, ops
    from mdctgan_amd import functional as Fh
    row = (2, 64, 64, 8, 16)
    c = layer_case(row, True)
    x = c["x"].float().to(DEV).contiguous(memory_format=torch.channels_last)
    w = torch.nn.Parameter(c["w"].float().to(DEV).contiguous(memory_format=torch.channels_last))
    b = torch.nn.Parameter(c["b"].float().to(DEV))
    with torch.no_grad(), amp.infer_f16():
        assert amp.current_precision() == HINF
        made, used = Fh.WINO_NEXT_STATS["made"], Fh.WINO_NEXT_STATS["used"]
        y1 = Fh.conv_instnorm(x, w, b, padding=1, reflect=True, act=ops.ACT_RELU, next_reflect=True)
        assert Fh.WINO_NEXT_STATS["made"] == made + 1
        v = y1._mg_wino_v[0]
        assert v.dtype == torch.float16 and v.numel() == 16 * 2 * 32 * 64 and getattr(y1, "_mg_h16", None) is None
        y2 = Fh.conv_instnorm(y1, w, b, padding=1, reflect=True, residual=x)
        assert Fh.WINO_NEXT_STATS["used"] == used + 1
        y2_own = Fh.conv_instnorm(y1.clone(), w, b, padding=1, reflect=True, residual=x)         # a copy carries no image
        assert Fh.WINO_NEXT_STATS["used"] == used + 1 and torch.equal(y2, y2_own)
        plain = Fh.conv2d(x, w, b, padding=1, reflect=True)
        with amp.infer_f16(False), amp.autocast(True):
            train_path = Fh.conv2d(x, w, b, padding=1, reflect=True)
        close_f16(nhwc(plain), c["y"], **BAR)
        close_f16(nhwc(train_path), c["y"], **BAR)
    want = Fh.conv_instnorm(x, w, b, padding=1, reflect=True, act=ops.ACT_RELU)
    with amp.infer_f16():
        again = Fh.conv_instnorm(x, w, b, padding=1, reflect=True, act=ops.ACT_RELU)
    assert torch.equal(again.detach(), want.detach()) and not torch.equal(nhwc(want.detach()), nhwc(y1))


# ---- 4. whole model ----------------------------------------------------------------------------------------------------------
T_SEG, NSEG = 32512, 8


@functools.lru_cache(maxsize=None)
def toy_inputs():
    from oracle import nets as onets
    gen = torch.Generator().manual_seed(16)
    netG = onets.init_weights(onets.build_generator("global", 2, 1, 16, 4, 3, input_size=(128, 256)), gen)
    hr = 0.05 * torch.randn(NSEG, T_SEG, generator=gen)
    spec = torch.fft.rfft(hr)
    spec[:, spec.shape[-1] // 6:] = 0                    # 8 kHz content of a 48 kHz clip
    return netG, torch.fft.irfft(spec, n=T_SEG), hr


def toy_model(*extra):
    """--netG global --ngf 16, 4 downsamplings, 3 blocks: a 128x256 spectrogram becomes an 8x16 map of 256 channels in the trunk --
    at 8 segments the (8, 256 -> 256, 8 x 16) layer, eligible at the default thresholds."""
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    from oracle import nets as onets
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "8000", "--netG", "global", "--ngf", "16",
                           "--n_downsample_global", "4", "--n_blocks_global", "3", "--n_blocks_attn_g", "0", "--num_D", "2",
                           "--ndf", "8", "--batchSize", str(NSEG), "--gpu_ids", "0", *extra)
    model = create_model(opt)
    model.netG.load_state_dict(toy_inputs()[0].state_dict())
    onets.fill_deterministic(model.netD)
    return model


def infer(model, lr):
    model.eval()
    try:
        out = model.inference(lr)
    finally:
        model.train()
    return out[0], out[1], out[4]


def rel_l2(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return (torch.linalg.norm(a - b) / torch.linalg.norm(b)).item()


def test_whole_model_inference_and_graph(monkeypatch):
    """sr_spectro under --infer_fp16 against the float64 oracle generator on the same weights and the same generator input: relative
    L2 error at most twice that of the same model under amp.autocast(True) + no_grad on the training-path kernels (same operands and
    roundings; only the float32 accumulation order differs, 2^-24 beside roundings of 2^-11; the factor 2 covers the spread of the
    statistic), and at most 2e-2 against the float32 oracle, the project's bar for autocast forwards.  MG_INFER_F16=1 on a model
    without the flag gives the flag's bits; leaving the mode gives the default bits back; the graphed generate replays the eager
    call's bits.  Observed (MI355X): the mode 3.23e-3, autocast by hand 3.33e-3, float32 2.8e-6."""
    import os
    from mdctgan_amd import amp, ops
    from mdctgan_amd import functional as Fh
    from mdctgan_amd.generate_audio import generate, make_graphed_generate
    assert "MG_INFER_F16" not in os.environ and "MG_INFER_F16_MIN_C" not in os.environ
    netG, lr, hr = toy_inputs()
    lr_d = lr.to(DEV)
    trunk = ops.conv_geom(NSEG, 8, 16, 256, 256, 3, 3, 1, 1, True, HINF)
    assert is_winoh(trunk) and ops.wino_vnext_ok(trunk)
    entered = []
    real = amp.infer_f16
    monkeypatch.setattr(amp, "infer_f16", lambda enabled=True: (entered.append(bool(enabled)), real(enabled))[1])
    mode, plain = toy_model("--infer_fp16"), toy_model()
    assert mode.opt.infer_fp16 and not plain.opt.infer_fp16 and not mode.opt.fp16
    made0, used0 = Fh.WINO_NEXT_STATS["made"], Fh.WINO_NEXT_STATS["used"]
    spec_m, audio_m, lr_spec = infer(mode, lr_d)
    assert entered == [True]
    assert Fh.WINO_NEXT_STATS["made"] > made0 and Fh.WINO_NEXT_STATS["used"] > used0      # the trunk hands its images over
    spec_p, audio_p, lr_spec_p = infer(plain, lr_d)
    assert entered == [True, False] and torch.equal(lr_spec, lr_spec_p)                  # K1 stays float32
    assert not torch.equal(spec_m, spec_p), "the mode did not change the arithmetic: it did not run"
    monkeypatch.setenv("MG_INFER_F16", "1")
    spec_e, audio_e, _ = infer(plain, lr_d)
    monkeypatch.delenv("MG_INFER_F16")
    assert entered == [True, False, True] and torch.equal(spec_e, spec_m) and torch.equal(audio_e, audio_m)
    spec_p2, audio_p2, _ = infer(plain, lr_d)                # back in the default mode: the mode's cached images are not read
    assert torch.equal(spec_p2, spec_p) and torch.equal(audio_p2, audio_p)
    with amp.autocast(True):
        spec_a, _, _ = infer(plain, lr_d)                    # what a user can do by hand: the training-path float16 kernels
    assert not torch.equal(spec_a, spec_m)
    with torch.no_grad():
        x_in = plain._two_channel(lr_spec).cpu()
        o32 = netG(x_in)
        o64 = netG.double()(x_in.double())
        netG.float()
    e_mode, e_auto, e_def = rel_l2(spec_m, o64), rel_l2(spec_a, o64), rel_l2(spec_p, o64)
    e_mode32 = rel_l2(spec_m, o32)
    print("whole model, relative L2 of sr_spectro against the float64 oracle: --infer_fp16 %.4g | autocast by hand %.4g | float32 %.3g;"
          " --infer_fp16 against the float32 oracle %.4g (bar 2e-2)" % (e_mode, e_auto, e_def, e_mode32))
    assert e_mode <= 2.0 * e_auto
    assert e_mode32 <= 2e-2
    # graphed generate in the mode == eager generate in the mode
    eager = generate(mode, lr_d, batch_size=NSEG, gen_overlap=0)
    assert torch.equal(eager.reshape(-1), audio_m.reshape(-1))
    run = make_graphed_generate(mode, lr_d, batch_size=NSEG, gen_overlap=0)
    for _ in range(2):
        assert torch.equal(run(lr_d).view(1, -1), eager)
    del run


def test_generate_many_in_the_mode():
    """Three utterances of different lengths (a batch of 8 segments on the route, a last batch of 2 on the MG_PRECISION_F16 kernels):
    finite output, within relative L2 2e-2 of the float32 result.  Observed (MI355X): 4.4e-3 to 4.9e-3."""
    from mdctgan_amd.generate_audio import generate_many
    _, lr, _ = toy_inputs()
    flat = lr.reshape(-1).to(DEV)
    lengths = [3 * T_SEG, 2 * T_SEG + 1000, 4 * T_SEG - 7]
    waves, at = [], 0
    for n in lengths:
        waves.append(flat[at:at + n].clone())
        at += n // 2
    mode, plain = toy_model("--infer_fp16"), toy_model()
    mode.eval(), plain.eval()
    got = generate_many(mode, waves, batch_size=NSEG, gen_overlap=0, segment_length=T_SEG)
    want = generate_many(plain, waves, batch_size=NSEG, gen_overlap=0, segment_length=T_SEG)
    assert len(got) == len(want) == 3
    for u, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and bool(torch.isfinite(a).all())
        e = rel_l2(a, b)
        print("generate_many utterance %d (%d samples): relative L2 %.4g against float32 (bar 2e-2)" % (u, a.numel(), e))
        assert not torch.equal(a, b) and e <= 2e-2


def test_training_step_inside_the_context_is_unchanged():
    """With gradients enabled amp.infer_f16() changes nothing: a training step inside it is bit-identical to one outside it."""
    from mdctgan_amd import amp
    _, lr, hr = toy_inputs()
    lr_d, hr_d = lr[:2].to(DEV), hr[:2].to(DEV)
    inside, outside = toy_model(), toy_model()
    with amp.infer_f16():
        li = inside.optimize_parameters(lr_d, hr_d)
    lo = outside.optimize_parameters(lr_d, hr_d)
    assert sorted(li) == sorted(lo)
    for k in li:
        assert torch.equal(torch.as_tensor(li[k]), torch.as_tensor(lo[k])), k
    for net in ("netG", "netD"):
        for (ka, pa), (kb, pb) in zip(getattr(inside, net).state_dict().items(), getattr(outside, net).state_dict().items()):
            assert ka == kb and torch.equal(pa, pb), (net, ka)
