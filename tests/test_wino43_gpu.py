"""The opt-in Winograd F(4x4,3x3) family of inference passes (csrc/wino43.h, MG_PRECISION_F32_WINO43) on the GPU, against plain
float64 evaluations of the same operations:

  wino43_{weight,input,output}_xform_kernel + the 36-position batched GEMM          ops.conv_fwd
  wino43_out_norm_kernel<NT>          inverse transform + InstanceNorm (+ act, + residual)      ops.conv_fwd_instnorm
  wino43_out_norm_kernel<NT, true>    ... + the next layer's B^T y B image                       ops.conv_fwd_instnorm(v_next=)
  amp.wino43 / --wino43 / MG_WINO43   the whole generator                                        Pix2PixHDModel.inference

Inputs are float64 values that float32 holds exactly, outputs lie in guard-filled arenas, the references and the bars are those of
tests/test_trunk_fused_gpu.py (its helpers are imported): a convolution 3e-5 of max|ref|; a normalised output 1e-5 of max|ref| and
the relative mean / rstd bars, against a float64 InstanceNorm of the DEVICE's raw output.  MG_WINO43_MIN_C=32 brings the family's
channel threshold (256 by default) down to the test shapes."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_trunk_fused_gpu as TF
from test_elementwise_gpu import f32_exact
from test_trunk_fused_gpu import ACTS, DEV, EPS, Arena, conv64, dev, layer_case, nchw, nhwc, rel_err

pytestmark = pytest.mark.gpu
F32, W43 = 0, 2

# (B, Ci, Co, H, W), 3x3 stride 1 pad 1
PLAIN_ROWS = [
    (2, 32, 32, 4, 4),          # one tile: a reflected row / column index lands on the opposite pixel
    (3, 64, 64, 4, 32),         # Co % 64 == 0: the LDS-DMA dense GEMM's 36-position instance
    (2, 32, 32, 8, 16),
    (2, 48, 32, 8, 16),         # Ci is not a multiple of 32
    (2, 32, 48, 8, 16),         # Co % 32 != 0: the unfused route
    (1, 32, 32, 4, 164),        # 41 tiles: past the fused kernel's limit
]
FUSED_ROWS = [r for r in PLAIN_ROWS if r[2] % 32 == 0 and (r[3] // 4) * (r[4] // 4) <= 40] + [
    (1, 32, 32, 20, 32),        # 40 tiles: the limit, NT = 3
    (1, 96, 96, 16, 8),         # 8 tiles, three channel slabs
    (1, 32, 32, 8, 36),         # 18 tiles: NT = 2
]
BT43 = torch.tensor([[1, -1.5, -2, 1.5, 1, 0], [0, -1, 0.5, 2.5, 1, 0], [0, 1, -2.5, 0.5, 1, 0], [0, -2, -1, 2, 1, 0],
                     [0, 0.5, -1, -0.5, 1, 0], [0, 1, -1.5, -2, 1.5, 1]], dtype=torch.float64)


def tiles_of(row):
    return (row[3] // 4) * (row[4] // 4)


def row_id(row):
    return "%dx%dto%dx%dx%d_%dtiles" % (row[0], row[1], row[2], row[3], row[4], tiles_of(row))


def geom(row, reflect, prec=W43):
    from mdctgan_amd import ops
    B, Ci, Co, H, W = row
    return ops.conv_geom(B, H, W, Ci, Co, 3, 3, 1, 1, reflect, prec)


@pytest.fixture(autouse=True)
def small_channels(monkeypatch):
    monkeypatch.setenv("MG_WINO43_MIN_C", "32")


def is_wino43(g):
    """The forward pass of g is the 36-position batched launch: weights image of 36 * Co * Ci floats, the dense GEMM's 36-position
    instance or the implicit-GEMM kernels' tag 5."""
    from mdctgan_amd import ops
    name = ops.plan_name(0, g)
    return ops.wino_weights_bytes(g) == 36 * g.Co * g.Ci * 4 and (name.endswith(", 36, 0>") or name.endswith(", 5>")
                                                                 or name.startswith("dgemm32_kernel"))


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


# ---- 1. plain pipeline ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("row", PLAIN_ROWS, ids=row_id)
def test_plain_pipeline_against_float64(row, reflect):
    """U = G w G^T, V = B^T d B, 36 GEMMs, act(A^T M A + bias) against the float64 convolution at 3e-5 of max|ref| (the bound of
    tests/test_conv_gpu.py), with a bias and each activation and without a bias; a prepared U gives the same bits.
    Worst observed over all rows and activations (MI355X): 1.13e-5 of max|ref|; the raw output 2.3e-6."""
    from mdctgan_amd import ops
    c = layer_case(row, reflect)
    g = geom(row, reflect)
    assert is_wino43(g), ops.plan_name(0, g)
    xd, wd, bd = dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV)
    y64_nobias = nhwc(conv64(c["x"], c["w"], None, reflect))
    codes = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU02, "tanh": ops.ACT_TANH}
    worst = 0.0
    for act, code in codes.items():
        got = guarded_conv(g, xd, wd, bd, code)
        e = rel_err(got, ACTS[act](c["y"]))
        worst = max(worst, e)
        assert e < 3e-5, (act, e)
    got = guarded_conv(g, xd, wd, None, ops.ACT_NONE)
    e = rel_err(got, y64_nobias)
    assert e < 3e-5, ("no bias", e)
    u = ops.wino_weights(g, wd)
    assert u is not None and u.numel() == 36 * row[1] * row[2]
    assert torch.equal(guarded_conv(g, xd, wd, None, ops.ACT_NONE, u=u), got)
    print("wino43 plain %s reflect=%d: worst %.3g of max|ref| (%s)" % (row_id(row), reflect, max(worst, e), ops.plan_name(0, g)))


# ---- 2. fused output transform + InstanceNorm ------------------------------------------------------------------------------
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("row", FUSED_ROWS + [(2, 32, 48, 8, 16), (1, 32, 32, 4, 164)], ids=row_id)
def test_conv_instnorm_forward_against_float64(row, reflect):
    """wino43_out_norm_kernel<1..3> (and, on the two rows outside its range, the unfused sequence with the same contract): y_raw
    against the float64 convolution at 3e-5; mean, rstd and y against a float64 InstanceNorm of the device's own y_raw at the
    bars of test_trunk_fused_gpu.check_fwd_instnorm (1e-6 * (max|mean| + 1), 2e-6 * max|rstd|, 1e-5 * max|y|), over act x residual;
    need_raw=False gives the same y, mean and rstd bit for bit; guards intact.
    Worst observed over all rows (MI355X): y_raw 2.3e-6, mean 3.5e-8, rstd 5.2e-8, y 1.2e-7."""
    from mdctgan_amd import ops
    c = layer_case(row, reflect)
    g = geom(row, reflect)
    assert is_wino43(g), ops.plan_name(0, g)
    fused = row[2] % 32 == 0 and tiles_of(row) <= 40
    assert ops.wino_vnext_ok(g) == fused
    worst = {}
    TF.check_fwd_instnorm(g, dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), dev(c["res"]), c["y"], nhwc(c["res"]), worst)
    print("wino43 fwd_instnorm %s reflect=%d fused=%d: %s" % (row_id(row), reflect, fused,
                                                              " ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def test_fused_rows_reach_every_depth():
    depths = sorted({(tiles_of(r) + 15) // 16 for r in FUSED_ROWS})
    assert depths == [1, 2, 3] and max(tiles_of(r) for r in FUSED_ROWS) == 40


# ---- 3. hand-over image ----------------------------------------------------------------------------------------------------
def input_image64(y, reflect):
    """NHWC float64 -> V [36][T][C] = B^T d B over the 6x6 patches (origin 4t - 1) of the reflect- / zero-padded map."""
    B, H, W, C = y.shape
    yp = nhwc(F.pad(nchw(y), (1, 1, 1, 1), mode="reflect" if reflect else "constant"))
    d = yp.unfold(1, 6, 4).unfold(2, 6, 4)                                # [B, TH, TW, C, 6, 6]
    return torch.einsum("ir,btxcrs,js->ijbtxc", BT43, d, BT43).reshape(36, B * (H // 4) * (W // 4), C)


@pytest.mark.parametrize("next_reflect", [True, False], ids=["next_reflect", "next_zero"])
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
@pytest.mark.parametrize("row", FUSED_ROWS, ids=row_id)
def test_next_layer_image_against_float64(row, reflect, next_reflect):
    """wino43_out_norm_kernel<NT, true>: v_next against the float64 B^T y B of the device's y.  The bound comes from the matrix:
    two passes, each output a sum of at most 5 products (6 roundings: 5 products -- exact where the entry is a power of two -- and
    the additions), every pass growing a value by at most s = 7, the largest absolute row sum of B^T: 2 * 6 * 2^-24 * s^2 * max|y|
    = 3.5e-5 * max|y|.  The image is bit-equal to the one a plain conv_fwd of the next layer keeps, and the next layer run from it
    gives the bits it gives when it transforms y itself (and meets the convolution bound, 3e-5).  y, y_raw, mean, rstd are those
    of the call without v_next.  Worst observed (MI355X): v_next 1.6e-6 of max|y|, next layer 3.0e-6."""
    from mdctgan_amd import ops
    c = layer_case(row, reflect)
    g = geom(row, reflect)
    B, Ci, Co, H, W = row
    assert ops.wino_vnext_ok(g) and ops.wino_vnext_positions(g) == 36
    xd, wd, bd, resd = dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), dev(c["res"])
    g_next = ops.conv_geom(B, H, W, Co, Co, 3, 3, 1, 1, next_reflect, W43)
    assert is_wino43(g_next)
    nv = 36 * B * tiles_of(row) * Co
    v_plain, _ = ops.wino_tile_buffers(g_next, DEV, want_md=False)
    assert v_plain is not None and v_plain.numel() == nv
    gen = torch.Generator().manual_seed(tiles_of(row))
    w2 = f32_exact(torch.randn(Co, Co, 3, 3, generator=gen, dtype=torch.float64) / np.sqrt(9 * Co))
    w2d = dev(w2)
    bound = 2 * 6 * 2.0 ** -24 * 7 ** 2
    for act, with_res in ((ops.ACT_RELU, False), (ops.ACT_NONE, True)):          # the trunk's two layers: ReLU, then + skip
        res = resd if with_res else None
        av = Arena(nv)
        rc, y, y_raw, mean, rstd = TF.fused_fwd(g, xd, wd, bd, act, res, v_next=av.out, next_reflect=next_reflect)
        assert rc == 0 and av.intact()
        rc0, y0, raw0, mean0, rstd0 = TF.fused_fwd(g, xd, wd, bd, act, res)
        assert rc0 == 0 and torch.equal(y, y0) and torch.equal(y_raw, raw0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
        y64 = y.double().cpu()
        want = input_image64(y64, next_reflect)
        err = (av.out.double().cpu().view(36, -1, Co) - want).abs().max().item() / y64.abs().max().item()
        z_plain = ops.conv_fwd(g_next, y, w2d, v_out=v_plain)
        assert torch.equal(av.out, v_plain)
        z = ops.conv_fwd(g_next, y, w2d, v_out=av.out, v_filled=True)
        ez = rel_err(z, nhwc(conv64(nchw(y64), w2, None, next_reflect)))
        print("wino43 v_next %s reflect=%d next_reflect=%d act=%d: image %.3g of max|y| (bound %.3g), next layer %.3g"
              % (row_id(row), reflect, next_reflect, act, err, bound, ez))
        assert err <= bound
        assert torch.equal(z, z_plain) and ez < 3e-5


@pytest.mark.parametrize("row", [(1, 32, 32, 4, 164), (2, 32, 48, 8, 16)], ids=row_id)
def test_next_layer_image_is_refused_outside_its_range(row):
    """41 tiles and Co % 32 != 0: MG_ERR_ARG, and the guard-filled v_next stays untouched."""
    from mdctgan_amd import ops
    c = layer_case(row, True)
    g = geom(row, True)
    assert is_wino43(g) and not ops.wino_vnext_ok(g)
    v = torch.full((36 * row[0] * tiles_of(row) * row[2] + TF.GUARD,), TF.FILL, device=DEV)
    rc = TF.fused_fwd(g, dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), ops.ACT_RELU, None, v_next=v, next_reflect=True)[0]
    assert rc == -1          # MG_ERR_ARG
    assert bool((v == TF.FILL).all())


# ---- 4. fallback -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,min_c", [((2, 32, 32, 6, 16), "32"), ((2, 32, 32, 8, 16), None)], ids=["H_not_4n", "below_min_c"])
def test_ineligible_geometry_runs_as_float32(monkeypatch, row, min_c):
    """H % 4 != 0, and a layer below the default min_c of 256 without the override: the plan names and the output bits of
    MG_PRECISION_F32, through the plain call and the conv + InstanceNorm call."""
    from mdctgan_amd import ops
    if min_c is None:
        monkeypatch.delenv("MG_WINO43_MIN_C")
    c = layer_case(row, True)
    xd, wd, bd, resd = dev(c["x"]), dev(c["w"]), c["b"].float().to(DEV), dev(c["res"])
    g, g32 = geom(row, True), geom(row, True, F32)
    assert not is_wino43(g)
    assert [ops.plan_name(p, g) for p in range(3)] == [ops.plan_name(p, g32) for p in range(3)]
    assert torch.equal(guarded_conv(g, xd, wd, bd, ops.ACT_RELU), guarded_conv(g32, xd, wd, bd, ops.ACT_RELU))
    a = TF.fused_fwd(g, xd, wd, bd, ops.ACT_RELU, resd)
    b = TF.fused_fwd(g32, xd, wd, bd, ops.ACT_RELU, resd)
    assert a[0] == 0 and b[0] == 0 and all(torch.equal(p, q) for p, q in zip(a[1:], b[1:]))


# ---- 5. whole model ----------------------------------------------------------------------------------------------------------
T_SEG = 32512


@functools.lru_cache(maxsize=None)
def toy_inputs():
    from oracle import nets as onets
    gen = torch.Generator().manual_seed(43)
    netG = onets.init_weights(onets.build_generator("global", 2, 1, 4, 4, 3, input_size=(128, 256)), gen)
    hr = 0.05 * torch.randn(2, T_SEG, generator=gen)
    spec = torch.fft.rfft(hr)
    spec[:, spec.shape[-1] // 6:] = 0                    # 8 kHz content of a 48 kHz clip
    return netG, torch.fft.irfft(spec, n=T_SEG), hr


def toy_model(*extra):
    """--netG global --ngf 4, 4 downsamplings, 3 blocks: a 128x256 spectrogram becomes an 8x16 map of 64 channels in the trunk."""
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    from oracle import nets as onets
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "8000", "--netG", "global", "--ngf", "4",
                           "--n_downsample_global", "4", "--n_blocks_global", "3", "--n_blocks_attn_g", "0", "--num_D", "2",
                           "--ndf", "8", "--batchSize", "2", "--gpu_ids", "0", *extra)
    model = create_model(opt)
    model.netG.load_state_dict(toy_inputs()[0].state_dict())
    onets.fill_deterministic(model.netD)
    return model


def infer(model, lr):
    model.eval()
    try:
        sr_spectro, sr_audio = model.inference(lr)[:2]
    finally:
        model.train()
    return sr_spectro, sr_audio


def test_whole_model_inference_train_and_graph(monkeypatch):
    """inference with --wino43 against oracle.step.HotPathRef.inference on the same weights at the project's own bar (sr_spectro
    within 1e-3 of its range, sr_audio within 1e-3 of its peak, as test_fullsize_gpu.test_batch64_generate_against_oracle), the
    default path's error printed beside it; MG_WINO43=1 on a model without the flag gives the flag's bits; a training step
    afterwards is bit-identical to one of a model that never entered the mode; the graphed generate equals the eager one."""
    from mdctgan_amd import amp, ops
    from mdctgan_amd.generate_audio import generate, make_graphed_generate
    from oracle import step as ostep
    netG, lr, hr = toy_inputs()
    lr_d, hr_d = lr.to(DEV), hr.to(DEV)
    trunk = ops.conv_geom(2, 8, 16, 64, 64, 3, 3, 1, 1, True, W43)
    assert is_wino43(trunk) and ops.wino_vnext_ok(trunk)
    entered = []
    real = amp.wino43
    monkeypatch.setattr(amp, "wino43", lambda enabled=True: (entered.append(bool(enabled)), real(enabled))[1])
    mode, plain = toy_model("--wino43"), toy_model()
    assert mode.opt.wino43 and not plain.opt.wino43
    from mdctgan_amd import functional as Fh
    made0, used0 = Fh.WINO_NEXT_STATS["made"], Fh.WINO_NEXT_STATS["used"]
    spec_m, audio_m = infer(mode, lr_d)
    assert entered == [True]
    assert Fh.WINO_NEXT_STATS["made"] > made0 and Fh.WINO_NEXT_STATS["used"] > used0      # the trunk hands its images over
    spec_p, audio_p = infer(plain, lr_d)
    assert entered == [True, False]
    assert not torch.equal(spec_m, spec_p), "the mode did not change the arithmetic: it did not run"
    monkeypatch.setenv("MG_WINO43", "1")
    spec_e, audio_e = infer(plain, lr_d)
    monkeypatch.delenv("MG_WINO43")
    assert entered == [True, False, True] and torch.equal(spec_e, spec_m) and torch.equal(audio_e, audio_m)
    spec_p2, audio_p2 = infer(plain, lr_d)                  # back in the default mode: the other family's cached images are not read
    assert torch.equal(spec_p2, spec_p) and torch.equal(audio_p2, audio_p)
    ref = ostep.HotPathRef(netG, None, ostep.CodecCfg(lr_rate=8000), num_D=2)
    o_spec, o_audio, _, _ = ref.inference(lr.numpy())
    o_spec, o_audio = o_spec.numpy(), np.asarray(o_audio).reshape(2, -1)
    errs = {}
    for name, spec, audio in (("wino43", spec_m, audio_m), ("default", spec_p, audio_p)):
        es = np.abs(spec.cpu().numpy() - o_spec).max() / max(np.abs(o_spec).max(), 1e-3)
        ea = np.abs(audio.cpu().numpy().reshape(2, -1) - o_audio).max() / np.abs(o_audio).max()
        errs[name] = (es, ea)
    print("whole model against the oracle: wino43 sr_spectro %.3g sr_audio %.3g | default sr_spectro %.3g sr_audio %.3g (bar 1e-3)"
          % (errs["wino43"] + errs["default"]))
    assert errs["wino43"][0] <= 1e-3 and errs["wino43"][1] <= 1e-3
    assert errs["default"][0] <= 1e-3 and errs["default"][1] <= 1e-3
    # graphed generate in the mode == eager generate in the mode
    eager = generate(mode, lr_d, batch_size=2, gen_overlap=0)
    assert torch.equal(eager.reshape(-1), audio_m.reshape(-1))
    run = make_graphed_generate(mode, lr_d, batch_size=2, gen_overlap=0)
    assert torch.equal(run(lr_d).view(1, -1), eager)
    del run
    # a training step afterwards: the mode leaves nothing behind
    never = toy_model()
    lm, ln = mode.optimize_parameters(lr_d, hr_d), never.optimize_parameters(lr_d, hr_d)
    assert sorted(lm) == sorted(ln)
    for k in lm:
        assert torch.equal(torch.as_tensor(lm[k]), torch.as_tensor(ln[k])), k
    for (ka, pa), (kb, pb) in zip(mode.netG.state_dict().items(), never.netG.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb), ka
    for (ka, pa), (kb, pb) in zip(mode.netD.state_dict().items(), never.netD.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb), ka


# ---- 6. off by default -------------------------------------------------------------------------------------------------------
def test_off_by_default():
    """Without the flag, the context and the environment a forward pass under no_grad carries MG_PRECISION_F32: the trunk row runs the
    F(2x2,3x3) route it ran before the mode existed -- the tag-1 GEMM and wino_out_norm_kernel with its 16-position hand-over --
    and gives that route's bits."""
    import os
    from mdctgan_amd import amp, ops
    from mdctgan_amd import functional as Fh
    assert "MG_WINO43" not in os.environ
    row = (2, 32, 32, 8, 16)
    c = layer_case(row, True)
    g32 = geom(row, True, F32)
    assert ops.plan_name(0, g32) == "conv_fwd_kernel<64, 64, true, 1>" and ops.wino_weights_bytes(g32) == 16 * 32 * 32 * 4
    assert ops.wino_vnext_ok(g32) and ops.wino_vnext_positions(g32) == 16
    x = c["x"].float().to(DEV).contiguous(memory_format=torch.channels_last)
    w = torch.nn.Parameter(c["w"].float().to(DEV).contiguous(memory_format=torch.channels_last))
    b = torch.nn.Parameter(c["b"].float().to(DEV))
    want = ops.conv_fwd_instnorm(g32, dev(c["x"]), dev(c["w"]), b.detach(), ops.ACT_RELU, None, EPS, need_raw=False)[0]
    with torch.no_grad():
        assert amp.current_precision() == F32
        made = Fh.WINO_NEXT_STATS["made"]
        got = Fh.conv_instnorm(x, w, b, padding=1, reflect=True, act=ops.ACT_RELU, next_reflect=True)
        assert Fh.WINO_NEXT_STATS["made"] == made + 1 and got._mg_wino_v[0].numel() == 16 * 2 * 4 * 8 * 32
        assert torch.equal(nhwc(got), want)
        with amp.wino43():
            mode = Fh.conv_instnorm(x, w, b, padding=1, reflect=True, act=ops.ACT_RELU, next_reflect=True)
        assert mode._mg_wino_v[0].numel() == 36 * 2 * 2 * 4 * 32 and not torch.equal(mode, got)
    with amp.wino43():          # grad mode: the context changes nothing
        again = Fh.conv_instnorm(x, w, b, padding=1, reflect=True, act=ops.ACT_RELU)
    assert torch.equal(nhwc(again.detach()), want)
