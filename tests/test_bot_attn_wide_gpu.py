"""K10 attention on feature maps of 129 to 256 tokens: the attn_wide_* kernels of csrc/bot_attn.hip (one workgroup per block
of 32 queries, every contraction on the exact-float32 MFMA) op by op under the bar of tests/test_bot_attn_gpu.py, then through
networks.BottleStack and through whole models whose generator carries a 256-token map (n_fft 1024 and n_fft 512).

The cases and what each is for: WIDE_CASES of tests/test_bot_attn_wide_host.py, which also shows on the CPU that the bar
rejects wrong restatements at these sizes.
"""
import numpy as np
import pytest
import torch

import test_bot_attn_gpu as T
from test_bot_attn_wide_host import WIDE_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------------------------
# 1. - 3. the kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WIDE_CASES, ids=T.attn_id)
def test_wide_attention_fwd_bwd(case):
    """The whole body of test_attention_fwd_bwd: out, P, its row sums, dqkv, demb_h, demb_w under
    e(HIP) <= 4 e(float32 CPU) + 4 * 2^-23, accumulate = 1, no tables, and a bit-identical second call on NaN-filled buffers."""
    assert 128 < case[1] * case[2] <= 256
    T.test_attention_fwd_bwd(case)


def test_wide_attention_sample_alone_has_the_bits_it_has_in_the_batch():
    """The grid of the wide kernels is (B * heads, blocks of 32 queries): a block's instructions do not depend on B."""
    case = (40, 8, 24, 8, 8, 1.0)
    _, _, _, heads, d, _ = case
    qkv, eh, ew, dout = (t.to(DEV) for t in T.attn_inputs(case))
    nan = float("nan")
    outs = []
    for sl in (slice(None), slice(0, 1)):
        dh, dw = torch.full_like(eh, nan), torch.full_like(ew, nan)
        outs.append(T.raw_attention(qkv[sl].contiguous(), eh, ew, dout[sl].contiguous(), heads, d, dh, dw, 0))
    for name, whole, alone in zip(("out", "P", "dqkv"), *outs):
        assert alone.shape[0] == 1 and torch.equal(whole[:1], alone), name


def test_wide_attention_outputs_stay_inside_their_buffers():
    """n = 203 (a ragged last block of 32 queries, a ragged last key tile), d = 5 (27 idle columns of a feature tile): out, P,
    dqkv, demb_h, demb_w and the workspace as views into buffers that carry 64 sentinel floats after them."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    case = (1, 7, 29, 1, 5, 1.0)
    B, fh, fw, heads, d, _ = case
    n = fh * fw
    qkv, eh, ew, dout = (t.to(DEV) for t in T.attn_inputs(case))
    SENT, nan = 7.25, float("nan")
    ws_floats = lib.mg_attention_bwd_workspace(B, fh, fw, heads, d) // 4
    assert ws_floats * 4 == lib.mg_attention_bwd_workspace(B, fh, fw, heads, d)
    sizes = dict(out=B * n * heads * d, P=B * heads * n * n, dqkv=B * n * 3 * heads * d, demb_h=fh * d, demb_w=fw * d, ws=ws_floats)
    buf = {k: torch.full((s + 64,), SENT, device=DEV) for k, s in sizes.items()}
    v = {k: b[:sizes[k]] for k, b in buf.items()}
    for k in v:
        v[k].fill_(nan)
    _lib.check(lib.mg_attention_fwd(_lib.ptr(qkv), _lib.ptr(eh), _lib.ptr(ew), B, fh, fw, heads, d, _lib.ptr(v["out"]),
                                    _lib.ptr(v["P"]), _lib.stream()), "mg_attention_fwd")
    _lib.check(lib.mg_attention_bwd(_lib.ptr(qkv), _lib.ptr(eh), _lib.ptr(ew), _lib.ptr(dout), _lib.ptr(v["P"]), B, fh, fw, heads,
                                    d, _lib.ptr(v["dqkv"]), _lib.ptr(v["demb_h"]), _lib.ptr(v["demb_w"]), 0, _lib.ptr(v["ws"]),
                                    sizes["ws"] * 4, _lib.stream()), "mg_attention_bwd")
    torch.cuda.synchronize()
    for k in ("out", "P", "dqkv", "demb_h", "demb_w"):
        assert torch.isfinite(v[k]).all(), k
    for k, b in buf.items():
        assert (b[sizes[k]:] == SENT).all(), k


# ------------------------------------------------------------------------------------------------------------------
# 4. BottleStack at 256 tokens against oracle.nets.BotStackRef (the method of test_nets_gpu.py::test_bottleneck_transformer_stack)
# ------------------------------------------------------------------------------------------------------------------
def judged(got, f32, f64, what, k=4.0):
    """The bars of tests/test_nets_gpu.py::judged: relative L2 against float64 with float32-CPU's own error as the yardstick
    (floor 5e-4: one ReLU-mask flip in either float32 run costs ~1e-4), and a max-abs guard against localised garbage."""
    got, f32, f64 = (np.asarray(t, dtype=np.float64) for t in (got, f32, f64))
    nrm = max(np.linalg.norm(f64), 1e-30)
    e_hip, e_32 = np.linalg.norm(got - f64) / nrm, np.linalg.norm(f32 - f64) / nrm
    print("K10 wide stack | %s | e_hip %.3e | e_f32 %.3e" % (what, e_hip, e_32))
    assert e_hip <= max(k * e_32, 5e-4) + 2e-6, "%s: HIP rel-L2 err %.3e vs fp32-CPU %.3e" % (what, e_hip, e_32)
    worst, worst32 = np.abs(got - f64).max(), np.abs(f32 - f64).max()
    assert worst <= max(2e-2 * max(np.abs(f64).max(), 1e-30), 1.5 * k * worst32), "%s: max-abs %.3e (fp32-CPU %.3e)" % (what, worst, worst32)


@pytest.mark.parametrize("cfg", [dict(dim=64, fmap=(8, 32), heads=2, dim_head=16, layers=2, B=2),
                                 dict(dim=128, fmap=(16, 16), heads=2, dim_head=128, layers=1, B=2)],
                         ids=["tokens256_8x32", "tokens256_16x16_d128"])
def test_bottleneck_transformer_stack_at_256_tokens(cfg):
    """Forward, input / parameter gradients and the running statistics; the oracle's ReLUs take the decisions HIP's forward
    took, each differing decision at a tie (|pre-activation| <= 1e-5 of its tensor's scale)."""
    from mdctgan_amd import functional as Fh
    from mdctgan_amd import networks
    from oracle import nets as onets
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(cfg["B"], cfg["dim"], *cfg["fmap"], generator=gen)
    gy = torch.randn(cfg["B"], cfg["dim"], *cfg["fmap"], generator=gen)
    res = {}

    def oracle():
        return onets.BotStackRef(cfg["dim"], cfg["fmap"], cfg["dim"], cfg["layers"], 4, cfg["heads"], cfg["dim_head"])

    hip = onets.fill_deterministic(networks.BottleStack(dim=cfg["dim"], fmap_size=cfg["fmap"], dim_out=cfg["dim"],
                                                        num_layers=cfg["layers"], proj_factor=4, heads=cfg["heads"],
                                                        dim_head=cfg["dim_head"], downsample=False)).to(DEV).train()
    assert list(hip.state_dict().keys()) == list(oracle().state_dict().keys())
    xd = x.clone().to(DEV).requires_grad_()
    Fh.TAP = []
    try:
        y = hip(xd)
        masks = [m.cpu() for _, m in Fh.TAP]      # every ReLU of the stack, in call order
    finally:
        Fh.TAP = None
    (y * gy.to(DEV)).sum().backward()

    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        net = onets.fill_deterministic(oracle()).to(dt).train()
        calls = []

        def pinned(mod, inp, out, calls=calls, name=name):
            pre, m = inp[0], masks[len(calls)]
            assert m.shape == pre.shape, (len(calls), tuple(m.shape), tuple(pre.shape))
            own = pre.detach() > 0
            tie = pre.detach().abs() <= 1e-5 * pre.detach().abs().max()
            assert not ((m != own) & ~tie).any(), "%s ReLU %d: HIP's decision differs away from a tie" % (name, len(calls))
            calls.append(int((m != own).sum()))
            return pre * m.to(pre.dtype)
        relus = {id(m): m for m in net.modules() if isinstance(m, torch.nn.ReLU)}
        for m in relus.values():
            m.register_forward_hook(pinned)
        xx = x.clone().to(dt).requires_grad_()
        y_ref = net(xx)
        assert len(calls) == len(masks), (len(calls), len(masks))
        assert sum(calls) <= 4, "%s: %d pinned ReLU decisions differ from the oracle's own" % (name, sum(calls))
        (y_ref * gy.to(dt)).sum().backward()
        res[name] = dict(y=y_ref.detach().numpy(), dx=xx.grad.numpy(), grads={k: p.grad.numpy() for k, p in net.named_parameters()},
                         bufs={k: b.numpy() for k, b in net.named_buffers()})
    judged(y.detach().cpu().numpy(), res["f32"]["y"], res["f64"]["y"], "BoT forward")
    judged(xd.grad.cpu().numpy(), res["f32"]["dx"], res["f64"]["dx"], "BoT dx", k=6.0)
    for k, p in hip.named_parameters():
        assert p.grad is not None, k
        judged(p.grad.cpu().numpy(), res["f32"]["grads"][k], res["f64"]["grads"][k], "BoT grad " + k, k=6.0)
    for k, b in hip.named_buffers():
        if "num_batches" in k:
            assert int(b) == 1
        else:
            np.testing.assert_allclose(b.cpu().numpy(), res["f64"]["bufs"][k], rtol=1e-4, atol=1e-6, err_msg=k)


# ------------------------------------------------------------------------------------------------------------------
# 5. whole model, n_fft 1024: a 128 x 512 spectrogram, 4 downsamplings, an 8 x 32 = 256-token map
# ------------------------------------------------------------------------------------------------------------------
SEG_1024 = 65024


def model_1024():
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    from oracle import nets as onets
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--n_fft", "1024", "--hop_length", "512",
                           "--win_length", "1024", "--bins", "128", "--segment_length", SEG_1024, "--netG", "global", "--ngf", "4",
                           "--n_downsample_global", "4", "--n_blocks_global", "2", "--n_blocks_attn_g", "1", "--heads_g", "2",
                           "--dim_head_g", "8", "--num_D", "2", "--ndf", "8", "--batchSize", "2", "--gpu_ids", "0")
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    onets.fill_deterministic(model.netD)
    return model


@pytest.fixture(scope="module")
def clips_1024():
    g = torch.Generator().manual_seed(3)
    hr = 0.05 * torch.randn(2, SEG_1024, generator=g)
    lr = 0.05 * torch.randn(2, SEG_1024, generator=g)
    return lr, hr


def test_n_fft_1024_model_with_attention_step(clips_1024):
    """_forward losses against the oracle's step (the tolerance of test_local_enhancer_with_attention_step), one optimisation
    step, and inference."""
    from oracle import nets as onets
    from oracle import step as ostep
    lr, hr = clips_1024
    model = model_1024()
    assert sorted(v.shape[0] for k, v in model.netG.state_dict().items() if "pos_emb" in k) == [8, 32]
    netG = onets.fill_deterministic(onets.build_generator("global", 2, 1, 4, 4, 2, input_size=(128, 512), n_attn_g=1,
                                                          heads_g=2, dim_head_g=8))
    netD = onets.fill_deterministic(onets.MultiscaleDRef(3, ndf=8, n_layers=3, num_D=2))
    assert list(netG.state_dict().keys()) == list(model.netG.state_dict().keys())
    ref = ostep.HotPathRef(netG, netD, ostep.CodecCfg(n_fft=1024, hop=512, win=1024), num_D=2)
    lo, _ = ref.forward_losses(lr.numpy(), hr.numpy())
    lh, _ = model._forward(lr.to(DEV), hr.to(DEV))
    for k, v in zip(model.loss_names, lh):
        print("K10 wide n_fft 1024 | %s | hip %.6e | oracle %.6e" % (k, v.item(), float(lo[k])))
        assert abs(v.item() - float(lo[k])) <= 0.05 * abs(float(lo[k])) + 1e-3, (k, v.item(), float(lo[k]))
    ld = model.optimize_parameters(lr.to(DEV), hr.to(DEV))
    assert all(np.isfinite(v.item()) for v in ld.values())
    for k, p in model.netG.named_parameters():
        assert p.grad is not None, k
    sr_spectro, sr_audio, *_ = model.inference(lr.to(DEV))
    assert sr_audio.shape == (2, 1, 1, SEG_1024) and torch.isfinite(sr_audio).all()


def test_n_fft_1024_graphed_step_equals_eager_steps(clips_1024):
    """2 warm-up + 3 replays == 5 eager steps, bit for bit: the wide kernels use static LDS, nothing is configured at launch
    time, so they capture like any other launch."""
    lr, hr = (t.to(DEV) for t in clips_1024)
    eager, graphed = model_1024(), model_1024()
    for _ in range(5):
        le = eager.optimize_parameters(lr, hr)
    run = graphed.make_graphed_step(lr, hr, warmup=2)
    for _ in range(3):
        lg = run(lr, hr)
    torch.cuda.synchronize()
    for k in le:
        assert le[k].item() == lg[k].item(), k
    for (k, a), (_, b) in zip(eager.netG.state_dict().items(), graphed.netG.state_dict().items()):
        assert torch.equal(a, b), k
    for (k, a), (_, b) in zip(eager.netD.state_dict().items(), graphed.netD.state_dict().items()):
        assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------------------------
# 6. whole model, n_fft 512: 64 frames at 3 downsamplings, an 8 x 32 map
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--fp16"]], ids=["f32", "fp16"])
def test_n_fft_512_model_with_256_token_attention_step(extra):
    """The flags of test_local_enhancer_with_attention_step with netG global at 3 downsamplings; attention stays float32 under
    --fp16."""
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    from oracle import nets as onets
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                           "--n_downsample_global", "3", "--n_blocks_global", "2", "--n_blocks_local", "1",
                           "--n_blocks_attn_g", "2", "--heads_g", "2", "--dim_head_g", "8", "--num_D", "3", "--ndf", "8",
                           "--batchSize", "2", "--bins", "64", "--segment_length", "16128", "--gpu_ids", "0", *extra)
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    onets.fill_deterministic(model.netD)
    shapes = sorted(v.shape[0] for k, v in model.netG.state_dict().items() if "pos_emb" in k)
    assert shapes == [8, 8, 32, 32], shapes
    g = torch.Generator().manual_seed(3)
    hr = 0.05 * torch.randn(2, 16128, generator=g)
    lr = 0.05 * torch.randn(2, 16128, generator=g)
    ld = model.optimize_parameters(lr.to(DEV), hr.to(DEV))
    assert all(np.isfinite(v.item()) for v in ld.values()), {k: v.item() for k, v in ld.items()}
