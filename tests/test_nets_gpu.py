"""HIP-backed generator / discriminator / losses / optimisation step against the CPU oracle (torch float64 and
float32) and against the golden vectors captured from the reference.

Tolerance policy (stated): these InstanceNorm stacks amplify a 1e-7 input perturbation ~1e3x (measured in
tests/test_oracle_golden.py), so agreement is judged against float64 truth relative to float32's own error:
    err(HIP vs fp64)  <=  4 * err(torch-fp32-CPU vs fp64) + 2e-6 * scale.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import nets as onets
from oracle import step as ostep
from oracle import transform

pytestmark = pytest.mark.gpu
DEV = "cuda"

CFGS = {
    "global": dict(netG="global", ngf=8, n_downsample_global=4, n_blocks_global=2),
    "local": dict(netG="local", ngf=4, n_downsample_global=3, n_blocks_global=2, n_blocks_local=1),
    "global_resconv_interp": dict(netG="global", ngf=4, n_downsample_global=3, n_blocks_global=1,
                                  upsample_type="interpolate", downsample_type="resconv"),
}
OCFGS = {
    "global": dict(netG="global", ngf=8, n_down_global=4, n_blocks_global=2),
    "local": dict(netG="local", ngf=4, n_down_global=3, n_blocks_global=2, n_blocks_local=1),
    "global_resconv_interp": dict(netG="global", ngf=4, n_down_global=3, n_blocks_global=1, up="interpolate",
                                  down="resconv"),
}


def hip_g(tag):
    from mdctgan_amd import networks
    c = dict(CFGS[tag])
    net = networks.define_G(2, 1, c.pop("ngf"), c.pop("netG"), input_size=(32, 256), n_attn_g=0, **c)
    return onets.fill_deterministic(net).to(DEV)


def oracle_g(tag, dtype):
    c = dict(OCFGS[tag])
    return onets.fill_deterministic(onets.build_generator(c.pop("netG"), 2, 1, input_size=(32, 256), **c)).to(dtype)


def judged(got, f32, f64, what, k=4.0):
    """Relative L2 error against float64 truth, with float32-CPU's own error as the yardstick.  (Max-abs is
    not usable: a single ReLU-mask flip |xhat| < 1e-6 -- legitimate float32 behaviour, it happens to the CPU
    float32 run as well, at other elements -- moves one gradient entry by O(1e-3) of the scale; measured with
    scripts/diag_bwd*.py.)  A loose max-abs bound still guards against localised garbage."""
    got, f32, f64 = (np.asarray(t, dtype=np.float64) for t in (got, f32, f64))
    nrm = max(np.linalg.norm(f64), 1e-30)
    e_hip, e_32 = np.linalg.norm(got - f64) / nrm, np.linalg.norm(f32 - f64) / nrm
    # floor 5e-4: one mask flip in either float32 run already costs ~1e-4 (the op-level tests in test_conv_gpu /
    # test_elementwise_gpu and, for the K10 BatchNorm / attention kernels, test_bot_attn_gpu hold the tight 3e-5 bars;
    # this test guards the wiring, where a bug costs O(1))
    assert e_hip <= max(k * e_32, 5e-4) + 2e-6, "%s: HIP rel-L2 err %.3e vs fp32-CPU %.3e" % (what, e_hip, e_32)
    # localised-garbage guard: 2 % of the tensor's scale, or 1.5 k x float32-CPU's own worst element where that is larger (a
    # ReLU-mask flip behind a 2048-channel reduction moves single elements by more than 2 % in ANY float32 run)
    worst, worst32 = np.abs(got - f64).max(), np.abs(f32 - f64).max()
    assert worst <= max(2e-2 * max(np.abs(f64).max(), 1e-30), 1.5 * k * worst32), "%s: max-abs %.3e (fp32-CPU %.3e)" % (what, worst, worst32)


@pytest.mark.parametrize("tag", list(CFGS))
def test_generator_forward(tag, golden):
    g = golden("g5_netG_" + tag)
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        y64 = oracle_g(tag, torch.float64)(x.double()).numpy()
        y32 = oracle_g(tag, torch.float32)(x).numpy()
        net = hip_g(tag)
        y = net(x.to(DEV))
    assert y.shape == (1, 1, 32, 256)
    judged(y.cpu().numpy(), y32, y64, "netG " + tag)
    judged(y.cpu().numpy(), g["y"], y64, "netG %s vs reference golden" % tag)   # golden == reference fp32 CPU


def _dead_bias(key, g64, grads64):
    """A conv bias whose output goes (possibly through an add with another conv) straight into InstanceNorm2d(affine=
    False) has a true gradient of exactly 0: float64 autograd returns ~1e-17 of the layer's weight-gradient scale there,
    every float32 implementation returns rounding noise.  Detected from the float64 run itself."""
    if not key.endswith(".bias"):
        return False
    wkey = key[:-4] + "weight"
    return np.abs(g64).max() <= 1e-9 * np.abs(grads64[wkey]).max()


@pytest.mark.parametrize("tag", list(CFGS))
def test_generator_backward(tag):
    """Every parameter gradient of the three generator variants (GlobalGenerator; LocalEnhancer: two-branch add +
    average-pool pyramid; resconv / interpolate sampling blocks: ConvResBlock, InterpolateUpsample) against the oracle's
    float64 autograd, with the oracle's float32 run as the yardstick (models/networks.py:173-267, 375-417)."""
    gen = torch.Generator().manual_seed(7)
    x = torch.rand(2, 2, 32, 256, generator=gen) * 2 - 1
    gy = torch.randn(2, 1, 32, 256, generator=gen)
    grads, dxs = {}, {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        net = oracle_g(tag, dt)
        xx = x.clone().to(dt).requires_grad_()      # clone: x.to(float32) is x itself
        (net(xx) * gy.to(dt)).sum().backward()
        grads[name] = {k: p.grad.numpy() for k, p in net.named_parameters()}
        dxs[name] = xx.grad.numpy()
    net = hip_g(tag)
    xd = x.to(DEV).requires_grad_()
    (net(xd) * gy.to(DEV)).sum().backward()
    judged(xd.grad.cpu().numpy(), dxs["f32"], dxs["f64"], "%s dL/dx" % tag, k=6.0)
    live = 0
    for k, p in net.named_parameters():
        if _dead_bias(k, grads["f64"][k], grads["f64"]):
            continue
        assert p.grad is not None, k
        judged(p.grad.cpu().numpy(), grads["f32"][k], grads["f64"][k], "%s grad %s" % (tag, k), k=6.0)
        live += 1
    assert live >= len(grads["f64"]) // 2


def test_local_attention_sandwich(golden):
    """LocalEnhancer with n_blocks_attn_l = 1 (networks.py:218-237): state-dict keys and the eval-mode forward against
    fixture G10 (the reference's module tree, shared modules included), and every parameter gradient in training mode --
    the shared down- / up-samplers accumulate two / three weight-gradient contributions per step -- against the oracle's
    float64 autograd."""
    from mdctgan_amd import networks
    g = golden("g10_netG_local_attn_l")
    kw = dict(input_size=(64, 256), n_attn_l=1, proj_factor_l=4, heads_l=2, dim_head_l=8)
    net = networks.define_G(2, 1, 4, "local", 2, 1, 1, 3, n_attn_g=0, **kw)
    assert list(net.state_dict().keys()) == list(g["keys"])
    onets.fill_deterministic(net)
    net = net.to(DEV).eval()
    x = torch.from_numpy(g["x"])
    o64 = onets.fill_deterministic(onets.build_generator("local", 2, 1, 4, 2, 1, 3, **kw)).double()
    o32 = onets.fill_deterministic(onets.build_generator("local", 2, 1, 4, 2, 1, 3, **kw))
    with torch.no_grad():
        y = net(x.to(DEV)).cpu().numpy()
        y64 = o64.eval()(x.double()).numpy()
    judged(y, g["y"], y64, "local + attn_l forward vs reference golden")
    # gradients (training mode: BatchNorm batch statistics)
    gen = torch.Generator().manual_seed(9)
    xb = torch.rand(2, 2, 64, 256, generator=gen) * 2 - 1
    gy = torch.randn(2, 1, 64, 256, generator=gen)
    grads = {}
    for name, o in (("f64", o64), ("f32", o32)):
        o.train()
        o.zero_grad()
        dt = torch.float64 if name == "f64" else torch.float32
        (o(xb.to(dt)) * gy.to(dt)).sum().backward()
        grads[name] = {k: p.grad.numpy().copy() for k, p in o.named_parameters()}
    net.train()
    (net(xb.to(DEV)) * gy.to(DEV)).sum().backward()
    checked = 0
    for k, p in net.named_parameters():
        if _dead_bias(k, grads["f64"][k], grads["f64"]):
            continue
        assert p.grad is not None, k
        judged(p.grad.cpu().numpy(), grads["f32"][k], grads["f64"][k], "attn_l grad " + k, k=6.0)
        checked += 1
    assert checked >= 20


def test_discriminator_forward_backward(golden):
    from mdctgan_amd import networks
    g = golden("g6_netD")
    x = torch.from_numpy(g["x"])
    netD = onets.fill_deterministic(networks.define_D(3, 8, 3, "instance", False, 2, True)).to(DEV)
    xd = x.to(DEV).requires_grad_()
    feats = netD(xd)
    o64 = onets.fill_deterministic(onets.MultiscaleDRef(3, 8, 3, 2)).double()
    o32 = onets.fill_deterministic(onets.MultiscaleDRef(3, 8, 3, 2))
    x64, x32 = x.double().requires_grad_(), x.clone().requires_grad_()
    f64, f32 = o64(x64), o32(x32)
    for i in range(2):
        for j in range(5):
            assert tuple(feats[i][j].shape) == g["f%d_%d" % (i, j)].shape
            judged(feats[i][j].detach().cpu().numpy(), f32[i][j].detach().numpy(), f64[i][j].detach().numpy(),
                   "D feat %d/%d" % (i, j))
            judged(feats[i][j].detach().cpu().numpy(), g["f%d_%d" % (i, j)], f64[i][j].detach().numpy(),
                   "D feat %d/%d vs reference golden" % (i, j))
    # LSGAN + feature losses and their gradients (wrt the input and every weight)
    def total(fe, mod):
        lg = mod.lsgan_loss(fe, True) if mod is onets else None
        return lg
    l64 = onets.lsgan_loss(f64, True) + sum(f.abs().mean() for sc in f64 for f in sc[:-1])
    l32 = onets.lsgan_loss(f32, True) + sum(f.abs().mean() for sc in f32 for f in sc[:-1])
    l64.backward(); l32.backward()
    from mdctgan_amd import functional as Fh
    crit = networks.GANLoss()
    lh = crit(feats, True)
    for sc in feats:
        for f in sc[:-1]:
            lh = lh + Fh.l1_loss(f, torch.zeros_like(f))
    lh.backward()
    assert abs(lh.item() - l64.item()) <= 4 * abs(l32.item() - l64.item()) + 1e-5 * abs(l64.item())
    judged(xd.grad.cpu().numpy(), x32.grad.numpy(), x64.grad.numpy(), "dL/dx", k=6.0)
    g32 = dict(o32.named_parameters()); g64 = dict(o64.named_parameters())
    for k, p in netD.named_parameters():
        if k.endswith(".bias") and any("layer%d" % j in k for j in (1, 2, 3)):
            continue
        judged(p.grad.cpu().numpy(), g32[k].grad.numpy(), g64[k].grad.numpy(), "grad " + k, k=6.0)


def make_model(golden_lr=None):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                           "--n_blocks_global", "2", "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8",
                           "--batchSize", "2", "--bins", "32", "--segment_length", "7936", "--gpu_ids", "0")
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    onets.fill_deterministic(model.netD)
    return model


def oracle_model(dtype):
    netG = onets.fill_deterministic(onets.build_generator("global", 2, 1, 4, 4, 2, input_size=(32, 256)))
    netD = onets.fill_deterministic(onets.MultiscaleDRef(3, ndf=8, n_layers=3, num_D=2))
    return ostep.HotPathRef(netG, netD, ostep.CodecCfg(), num_D=2, dtype=dtype)


def test_forward_losses_and_step(golden):
    g = golden("g6_step_global")
    hr = torch.from_numpy(g["hr"])          # full-band input for both legs: keeps the codec well conditioned
    lr = torch.from_numpy(g["lr"])
    model = make_model()
    assert model.loss_names == list(g["loss_names"])
    # 1) losses on the golden (lr, hr) pair vs the reference's captured values.  The float32 MDCT moves worst-case
    #    bins by <= 5e-4 and the toy net amplifies ~1e3x, hence the loose end-to-end tolerance; the per-stage tests
    #    above and in test_mdct_gpu.py are the tight ones.
    losses, sr = model._forward(lr.to(DEV), hr.to(DEV), infer=True)
    want = dict(zip(g["loss_names"], g["losses"]))
    for k, v in zip(model.loss_names, losses):
        assert abs(v.item() - want[k]) <= 0.05 * abs(want[k]) + 1e-3, (k, v.item(), want[k])
    # 2) same spectrograms into both legs: oracle spectro -> oracle nets, HIP K1 spectro -> HIP nets, compared
    #    stage by stage with the fp64 yardstick
    o64, o32 = oracle_model(torch.float64), oracle_model(torch.float32)
    l64, sr64 = o64.forward_losses(g["lr"], g["hr"])
    l32, sr32 = o32.forward_losses(g["lr"], g["hr"])
    for k, v in zip(model.loss_names, losses):
        e32 = abs(float(l32[k]) - float(l64[k]))
        assert abs(v.item() - float(l64[k])) <= 0.05 * abs(float(l64[k])) + 50 * e32, k
    # 3) the optimisation step: parameters move by +-lr on the first Adam step wherever the gradient sign is
    #    well defined; compare against the oracle step
    ld = model.optimize_parameters(lr.to(DEV), hr.to(DEV))
    assert set(ld) == set(model.loss_names)
    o32.train_step(g["lr"], g["hr"])
    o64.train_step(g["lr"], g["hr"])
    for net_h, net_o, net_y in ((model.netG, o32.netG, o64.netG), (model.netD, o32.netD, o64.netD)):
        po, py = dict(net_o.state_dict()), dict(net_y.state_dict())
        for k, p in net_h.state_dict().items():
            if k.endswith(".bias"):
                continue
            d = (p.detach().cpu() - po[k]).abs()
            assert d.max().item() <= 2 * 2e-4 + 2e-6, k
            # Which near-zero gradients change sign follows the spectrogram's float32 rounding (bins within 5e-4 of the float64
            # codec, amplified ~1e3x by this toy net): the two oracles, which share ONE float64 spectrogram, disagree on y < 0.1 %
            # of the entries; HIP's float32 K1 moves 0-5.1 % per layer (the worst layer read 4.x % with the dense-table K1 and
            # 5.1 % with the factored one).  A coarse net under the gradient tests proper (G6, test_step_gradients_*).
            y = ((po[k].double() - py[k]).abs() > 2e-6).float().mean().item()
            flips = (d > 2e-6).float().mean().item()
            assert y <= 0.01 and flips <= 0.08, (k, flips, y)
    # second step runs (moments in place, arena intact) and losses stay finite
    ld2 = model.optimize_parameters(lr.to(DEV), hr.to(DEV))
    assert all(np.isfinite(v.item()) for v in ld2.values())


def test_step_gradients_against_reference_golden(golden):
    """Fixture G6 holds the REFERENCE's own generator and discriminator gradients of one train.py:160-202 iteration
    (gG/*, gD/*: loss_G.backward() and loss_D.backward() of Pix2PixHDModel._forward on the deterministic weights).  The
    HIP step (one shared discriminator forward, two backward passes) is compared with them directly, parameter by
    parameter.  Both legs get the same float32 spectrograms (the oracle's, pinned to the reference at 1e-11 in
    tests/test_oracle_golden.py) so the comparison isolates networks + losses + backward wiring from K1's 5e-4
    worst-case bins.  Yardstick: the golden is a float32 run; its own distance to the oracle's float64 gradients is
    the scale of legitimate float32 disagreement on this ill-conditioned toy net."""
    g = golden("g6_step_global")
    model = make_model()
    o64 = oracle_model(torch.float64)
    lr_s, norm = o64.spectro(g["lr"])
    hr_s, _ = o64.spectro(g["hr"])
    lr_d, hr_d = lr_s.float().to(DEV), hr_s.float().to(DEV)
    model.preprocess.forward = lambda audio: (lr_d, None, None)
    model.preprocess.hr_forward = lambda audio: (hr_d, None, None)
    ld = model.optimize_parameters(torch.from_numpy(g["lr"]).to(DEV), torch.from_numpy(g["hr"]).to(DEV))
    want = dict(zip(g["loss_names"], g["losses"]))
    for k, v in ld.items():
        assert abs(v.item() - want[k]) <= 2e-3 * abs(want[k]) + 1e-6, (k, v.item(), want[k])
    # float64 truth for the yardstick
    l64, _ = o64.forward_losses(g["lr"], g["hr"])
    (l64["G_GAN"] + l64["G_GAN_Feat"]).backward()
    g64G = {k: p.grad.numpy().copy() for k, p in o64.netG.named_parameters()}
    # The discriminator gradients depend on the fake spectrogram, i.e. on the toy generator's conditioning-limited
    # output (1e-3 between any two float32 runs): isolate the discriminator-loss wiring by feeding the HIP discriminator
    # the REFERENCE's own fake (fixture `sr_spectro`) through the same batch-stacked pass the step uses.
    from mdctgan_amd import functional as Fh
    model_d = make_model()                  # fresh deterministic weights (the step above has already moved `model`'s)
    model_d.optimizer_D.zero_grad()
    sr_gold = torch.from_numpy(g["sr_spectro"]).to(DEV)
    pred = model_d.netD.forward(Fh.d_input_pair(lr_d, sr_gold, hr_d, float(model.norm_range[0])))
    loss_D = 0
    for scale_out in pred:
        l_fake, l_real = Fh.mse_const_pair_loss(scale_out[-1], 0.0, 1.0)
        loss_D = loss_D + (l_fake + l_real) * 0.5
    loss_D.backward()
    # ... and the float64 yardstick on the same fake
    o64.netD.zero_grad()
    two = o64.two_channel
    srg = torch.from_numpy(g["sr_spectro"]).double()
    l64D = 0.5 * (onets.lsgan_loss(o64.netD(torch.cat((lr_s, two(srg)), 1)), False)
                  + onets.lsgan_loss(o64.netD(torch.cat((lr_s, two(hr_s)), 1)), True))
    l64D.backward()
    g64D = {k: p.grad.numpy().copy() for k, p in o64.netD.named_parameters()}
    checked = 0
    for net, pre, g64 in ((model.netG, "gG/", g64G), (model_d.netD, "gD/", g64D)):
        for k, p in net.named_parameters():
            if _dead_bias(k, g64[k], g64):
                continue
            ref, got, truth = g[pre + k].astype(np.float64), p.grad.cpu().numpy().astype(np.float64), g64[k]
            nrm = max(np.linalg.norm(truth), 1e-30)
            e_ref = np.linalg.norm(ref - truth) / nrm          # the reference's own float32 error
            e_hip = np.linalg.norm(got - truth) / nrm
            d = np.linalg.norm(got - ref) / nrm
            assert e_hip <= max(6.0 * e_ref, 5e-4), (pre + k, e_hip, e_ref)
            assert d <= max(7.0 * e_ref, 1e-3), (pre + k, d, e_ref)
            checked += 1
    assert checked >= 20


def test_full_size_generator_forward_configs1():
    """The configs[1] generator at its real size (ngf 64, 4 stride-2 stages, nine 1024-channel ResNet blocks, 128 x 256
    input, networks.py weights_init N(0, 0.02) from a seeded generator) against the CPU oracle, batch 1: a
    well-conditioned counterpart of the toy-size net tests -- every tuned plan of the bench (Winograd, split-K,
    32-deep forward kernels, the tiled 7x7 kernels) in one chain.  float32 CPU and float64 CPU as yardstick / truth."""
    gen = torch.Generator().manual_seed(123)
    o32 = onets.init_weights(onets.build_generator("global", 2, 1, 64, 4, 9, input_size=(128, 256)), gen)
    x = torch.rand(1, 2, 128, 256, generator=gen) * 2 - 1
    from mdctgan_amd import networks
    net = networks.define_G(2, 1, 64, "global", 4, 9, input_size=(128, 256), n_attn_g=0)
    net.load_state_dict(o32.state_dict())
    net = net.to(DEV)
    with torch.no_grad():
        y = net(x.to(DEV)).cpu().numpy()
        y32 = o32(x).numpy()
        y64 = o32.double()(x.double()).numpy()
    assert y.shape == (1, 1, 128, 256)
    nrm = np.linalg.norm(y64)
    e_hip, e_32 = np.linalg.norm(y - y64) / nrm, np.linalg.norm(y32 - y64) / nrm
    assert e_hip <= max(4.0 * e_32, 2e-5), (e_hip, e_32)
    assert np.abs(y - y64).max() <= 1e-3 * np.abs(y64).max(), np.abs(y - y64).max()


def test_full_size_generator_forward_configs2():
    """configs[2]'s generator at its real size (netG=local, ngf 64 -> 2048-channel 4x8 trunk, two bottleneck-attention
    blocks of 8 x 64 heads on 32 tokens, three 128-channel local blocks; 2.95 GB of float32 weights) against the CPU
    oracle in float32, batch 1, in float32 and under autocast (--fp16; compared with the float32 oracle at float16
    resolution).  The bottleneck-transformer arithmetic inside is the oracle's restatement (parity unpinned)."""
    from mdctgan_amd import amp, networks
    gen = torch.Generator().manual_seed(321)
    o32 = onets.init_weights(onets.build_generator("local", 2, 1, 64, 4, 9, 3, input_size=(128, 256), n_attn_g=2,
                                                   heads_g=8, dim_head_g=64), gen)
    x = torch.rand(1, 2, 128, 256, generator=gen) * 2 - 1
    net = networks.define_G(2, 1, 64, "local", 4, 9, 1, 3, input_size=(128, 256), n_attn_g=2, heads_g=8, dim_head_g=64)
    assert list(net.state_dict().keys()) == list(o32.state_dict().keys())
    net.load_state_dict(o32.state_dict())
    net = net.to(DEV)
    with torch.no_grad():
        y32 = o32(x).numpy()
        y = net(x.to(DEV)).cpu().numpy()
        with amp.autocast(True):
            yh = net(x.to(DEV)).cpu().numpy()
    nrm = np.linalg.norm(y32)
    assert np.linalg.norm(y - y32) / nrm <= 2e-4, np.linalg.norm(y - y32) / nrm
    assert np.abs(y - y32).max() <= 2e-3 * np.abs(y32).max()
    assert np.linalg.norm(yh - y32) / nrm <= 2e-2, np.linalg.norm(yh - y32) / nrm


def test_inference_and_codec_round_trip(golden):
    g = golden("g6_step_global")
    model = make_model()
    lr = torch.from_numpy(g["lr"]).to(DEV)
    sr_spectro, sr_audio, lr_pha, norm_param, lr_spectro = model.inference(lr)
    assert sr_spectro.shape == (2, 1, 32, 256) and sr_audio.shape == (2, 1, 1, 7936) and lr_spectro.shape == (2, 1, 32, 256)
    # K1 against the oracle on the band-limited clip (empty-band bins are the sensitive ones)
    s_or, _ = transform.to_spectro(g["lr"], transform.kbd_window(512), 512, 256, **ostep.CodecCfg().codec)
    assert np.abs(lr_spectro.cpu().numpy() - s_or).max() <= 5e-4
    # K2 on the network's own output == oracle decoder on the same spectrogram
    want = transform.to_audio(sr_spectro.cpu().numpy(), {"min": np.float32([[[[-5.0]]]]), "max": np.float32([[[[5.0]]]])},
                              transform.kbd_window(512), 512, 256, **ostep.CodecCfg().codec)
    assert np.abs(sr_audio.cpu().numpy() - want).max() <= 3e-6 * max(np.abs(want).max(), 1e-3) + 1e-7
    # to_spectro / to_audio round trip through the facade
    hr = torch.from_numpy(g["hr"]).to(DEV)
    s, _, npar = model.preprocess.to_spectro(hr)
    back = model.preprocess.to_audio(s, npar, None)
    assert (back[:, 0, 0] - hr).abs().max().item() < 2e-6


def test_graphed_step_equals_eager_steps(golden):
    """A hipGraph replay of optimize_parameters() advances the model exactly like an eager call (device-resident Adam
    clock, no step-dependent kernel argument): 2 warm-up + 3 replays == 5 eager steps, bit for bit."""
    g = golden("g6_step_global")
    lr, hr = torch.from_numpy(g["lr"]).to(DEV), torch.from_numpy(g["hr"]).to(DEV)
    eager, graphed = make_model(), make_model()
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
    # new data through the captured input buffers
    lg2 = run(hr, hr)
    assert np.isfinite(lg2["G_GAN"].item())


@pytest.mark.parametrize("cfg", [dict(dim=64, fmap=(4, 8), heads=2, dim_head=16, layers=2, B=2),
                                 dict(dim=128, fmap=(8, 16), heads=2, dim_head=128, layers=1, B=2),
                                 dict(dim=2048, fmap=(4, 8), heads=8, dim_head=64, layers=2, B=8, init="normal")],
                         ids=["tokens32", "tokens128_d128", "configs2_dim2048_8x64_tokens32"])
def test_bottleneck_transformer_stack(cfg):
    """K10 (BatchNorm2d + MHSA kernels + 1x1 convs) against the oracle's restatement of BottleStack (parity of that
    third-party block is unpinned; this checks HIP == restatement), forward, input / parameter gradients and the
    running-statistics update.

    The oracle's ReLUs take the decisions HIP's forward took (mask-pinned, like oracle/step.py::MaskPins): at configs[2] size
    one pre-activation of the first block's output sits at 1e-6 of its scale, float32 rounding may put it either side of
    zero, and that one flip moves every gradient of the block by ~1e-3 (relative L2).  Each pinned decision that differs
    from the oracle's own must sit at such a tie (|pre-activation| <= 1e-5 of its tensor's scale)."""
    from mdctgan_amd import functional as Fh
    from mdctgan_amd import networks
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(cfg["B"], cfg["dim"], *cfg["fmap"], generator=gen)
    gy = torch.randn(cfg["B"], cfg["dim"], *cfg["fmap"], generator=gen)
    res = {}

    def fill(net):
        # configs[2] size: the closed-form sine fill drives the 2048-channel softmax logits to +-40 (float32 CPU itself is
        # then 5 % off float64: nothing to judge against), so this case uses weights_init's N(0, 0.02) from a fixed seed
        if cfg.get("init") == "normal":
            torch.manual_seed(5)
            ref = onets.BotStackRef(cfg["dim"], cfg["fmap"], cfg["dim"], cfg["layers"], 4, cfg["heads"], cfg["dim_head"])
            onets.init_weights(ref, torch.Generator().manual_seed(17))
            net.load_state_dict(ref.state_dict())
            return net
        return onets.fill_deterministic(net)

    hip = fill(networks.BottleStack(dim=cfg["dim"], fmap_size=cfg["fmap"], dim_out=cfg["dim"],
                                    num_layers=cfg["layers"], proj_factor=4, heads=cfg["heads"],
                                    dim_head=cfg["dim_head"], downsample=False)).to(DEV).train()
    assert list(hip.state_dict().keys()) == list(onets.BotStackRef(cfg["dim"], cfg["fmap"], cfg["dim"], cfg["layers"], 4,
                                                                   cfg["heads"], cfg["dim_head"]).state_dict().keys())
    xd = x.clone().to(DEV).requires_grad_()
    Fh.TAP = []
    try:
        y = hip(xd)
        masks = [m.cpu() for _, m in Fh.TAP]      # every ReLU of the stack, in call order
    finally:
        Fh.TAP = None
    (y * gy.to(DEV)).sum().backward()

    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        net = fill(onets.BotStackRef(cfg["dim"], cfg["fmap"], cfg["dim"], cfg["layers"], 4,
                                     cfg["heads"], cfg["dim_head"])).to(dt).train()
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
    # eval mode uses the running statistics
    hip.eval()
    ref = onets.BotStackRef(cfg["dim"], cfg["fmap"], cfg["dim"], cfg["layers"], 4, cfg["heads"], cfg["dim_head"]).double().eval()
    with torch.no_grad():
        ye = hip(x.to(DEV))
    sd = {k: v.double().cpu() for k, v in hip.state_dict().items()}
    ref.load_state_dict(sd)
    with torch.no_grad():
        want = ref(x.double())
    assert np.abs(ye.cpu().numpy() - want.numpy()).max() <= 2e-4 * np.abs(want.numpy()).max()


def test_inference_weight_image_cache_follows_updates(golden):
    """Under no_grad the Winograd layers keep their transformed weights between calls; an optimiser step (raw-pointer
    update, invisible to torch's version counter) or a state-dict load must invalidate them."""
    g = golden("g6_step_global")
    lr, hr = torch.from_numpy(g["lr"]).to(DEV), torch.from_numpy(g["hr"]).to(DEV)
    model = make_model()
    a1 = model.inference(lr)[0].clone()
    a2 = model.inference(lr)[0].clone()
    assert torch.equal(a1, a2)
    cached = [p for p in model.netG.parameters() if getattr(p, "_mg_u_cache", None) is not None]
    assert cached, "no Winograd layer took the cached path"
    model.optimize_parameters(lr, hr)
    b1 = model.inference(lr)[0].clone()
    assert not torch.equal(a1, b1)
    fresh = make_model()
    fresh.netG.load_state_dict(model.netG.state_dict())
    assert torch.equal(fresh.inference(lr)[0], b1)
    # ... and loading other weights into the same modules drops the images too
    model.netG.load_state_dict(make_model().netG.state_dict())
    assert torch.equal(model.inference(lr)[0], a1)


@pytest.mark.parametrize("num_D", [2, 3])
def test_shared_discriminator_pass_matches_separate_passes(num_D):
    """optimize_parameters() runs ONE discriminator forward over [fake, real] and backpropagates the G loss (fake half,
    data gradients only) and the D loss (whole stack, weight gradients) through it.  Same losses, same gradients and
    the same parameters after two Adam steps as the three-pass form of train.py:160-202 (share_d_fake_pass = False):
    float32 rounding of different GEMM plans only (2e-5 of each tensor's largest element)."""
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model

    def build(share):
        opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                               "--n_blocks_global", "2", "--n_blocks_attn_g", "0", "--num_D", str(num_D), "--ndf", "8",
                               "--batchSize", "3", "--bins", "64", "--segment_length", "16128", "--gpu_ids", "0")
        m = create_model(opt)
        onets.fill_deterministic(m.netG)
        onets.fill_deterministic(m.netD)
        m.share_d_fake_pass = share
        return m

    a, b = build(True), build(False)
    gen = torch.Generator().manual_seed(21)
    for it in range(2):
        hr = (0.05 * torch.randn(3, 16128, generator=gen)).to(DEV)
        lr = (0.05 * torch.randn(3, 16128, generator=gen)).to(DEV)
        la, lb = a.optimize_parameters(lr, hr), b.optimize_parameters(lr, hr)
        assert a._shared_rows == 3 and b._shared_rows == 0
        # iteration 0 starts from identical weights: tight.  Adam's first update is +-lr wherever the gradient sign is
        # defined, so elements with a rounding-level gradient may step apart and iteration 1 is compared loosely.
        tol = 2e-5 if it == 0 else 5e-2
        for k in la:
            assert abs(la[k].item() - lb[k].item()) <= tol * abs(lb[k].item()) + 1e-7, (it, k)
        for net in ("netG", "netD"):
            pa, pb = dict(getattr(a, net).named_parameters()), dict(getattr(b, net).named_parameters())
            for k in pa:
                ga, gb = pa[k].grad, pb[k].grad
                assert ga is not None and gb is not None, (net, k)
                scale = gb.abs().max().item()
                assert (ga - gb).abs().max().item() <= tol * scale + 1e-12, (it, net, k)
    for net in ("netG", "netD"):
        pa, pb = dict(getattr(a, net).named_parameters()), dict(getattr(b, net).named_parameters())
        for k in pa:
            assert (pa[k] - pb[k]).abs().max().item() <= 2 * 2e-4 * 2 + 1e-6, (net, k)


def test_local_enhancer_with_attention_step():
    """configs[2]-shaped model at toy width (netG=local, 2 bottleneck-attention blocks, num_D=3), float32: one full
    optimize_parameters() step against the oracle's step on the same deterministic weights."""
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "local", "--ngf", "4",
                           "--n_downsample_global", "3", "--n_blocks_global", "2", "--n_blocks_local", "1",
                           "--n_blocks_attn_g", "2", "--heads_g", "2", "--dim_head_g", "8", "--num_D", "3", "--ndf", "8",
                           "--batchSize", "2", "--bins", "64", "--segment_length", "16128", "--gpu_ids", "0")
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    onets.fill_deterministic(model.netD)
    netG = onets.fill_deterministic(onets.build_generator("local", 2, 1, 4, 3, 2, 1, input_size=(64, 256), n_attn_g=2,
                                                          heads_g=2, dim_head_g=8))
    netD = onets.fill_deterministic(onets.MultiscaleDRef(3, ndf=8, n_layers=3, num_D=3))
    assert list(netG.state_dict().keys()) == list(model.netG.state_dict().keys())
    ref = ostep.HotPathRef(netG, netD, ostep.CodecCfg(), num_D=3)
    g = torch.Generator().manual_seed(3)
    hr = 0.05 * torch.randn(2, 16128, generator=g)
    lr = 0.05 * torch.randn(2, 16128, generator=g)
    lo, _ = ref.forward_losses(lr.numpy(), hr.numpy())
    lh, _ = model._forward(lr.to(DEV), hr.to(DEV))
    for k, v in zip(model.loss_names, lh):
        assert abs(v.item() - float(lo[k])) <= 0.05 * abs(float(lo[k])) + 1e-3, (k, v.item(), float(lo[k]))
    ld = model.optimize_parameters(lr.to(DEV), hr.to(DEV))
    assert all(np.isfinite(v.item()) for v in ld.values())
    # every parameter, including BatchNorm affine and position embeddings, moved by one Adam step
    for k, p in model.netG.named_parameters():
        assert p.grad is not None, k


def test_published_checkpoint_architecture_runs():
    """The flags of the reference's train.sh / generate_audio.sh (the architecture of the published vctk checkpoints,
    SURVEY F3): netG local, ngf 56 (channel counts that are NOT multiples of 16 in the local branch), resconv / interpolate
    sampling, 3 bottleneck-attention blocks of 6 x 128 heads on 8 x 16 tokens, num_D 3, fit_residual, 16 kHz input.  One
    optimisation step in float32 and one under --fp16 stay finite, inference returns a waveform, and the state dict
    round-trips through save / load_network."""
    import os, tempfile
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    flags = ["--lr_sampling_rate", "16000", "--sr_sampling_rate", "48000", "--arcsinh_transform", "--abs_spectro",
             "--arcsinh_gain", "1000", "--center", "--norm_range", "-1", "1", "--smooth", "0.0", "--abs_norm", "--src_range", "-5", "5",
             "--netG", "local", "--ngf", "56", "--n_downsample_global", "3", "--n_blocks_global", "4", "--n_blocks_attn_g", "3",
             "--dim_head_g", "128", "--heads_g", "6", "--proj_factor_g", "4", "--n_blocks_attn_l", "0", "--n_blocks_local", "3",
             "--fit_residual", "--upsample_type", "interpolate", "--downsample_type", "resconv", "--num_D", "3"]
    gen = torch.Generator().manual_seed(2)
    hr = 0.05 * torch.randn(1, 32512, generator=gen)
    spec = torch.fft.rfft(hr)
    spec[:, spec.shape[-1] // 3:] = 0
    lr = torch.fft.irfft(spec, n=hr.shape[-1])
    for extra in ([], ["--fp16"]):
        with tempfile.TemporaryDirectory() as tmp:
            opt = options.make_opt(*flags, *extra, "--batchSize", "1", "--gpu_ids", "0", "--checkpoints_dir", tmp, "--name", "pub")
            model = create_model(opt)
            keys = list(model.netG.state_dict().keys())
            assert any(k.startswith("model1_1.") for k in keys) and any(".conv_res." in k for k in keys)
            assert any("to_qkv" in k for k in keys) and any("pos_emb.height" in k for k in keys)
            ld = model.optimize_parameters(lr.to(DEV), hr.to(DEV))
            assert all(np.isfinite(v.item()) for v in ld.values())
            sr_spectro, sr_audio, *_ = model.inference(lr.to(DEV))
            assert sr_audio.shape == (1, 1, 1, 32512) and torch.isfinite(sr_audio).all()
            os.makedirs(model.save_dir, exist_ok=True)
            model.save("latest")
            before = {k: v.detach().clone() for k, v in model.netG.state_dict().items()}
            with torch.no_grad():
                for p in model.netG.parameters():
                    p.add_(1.0)
            model.load_network(model.netG, "G", "latest")
            for k, v in model.netG.state_dict().items():
                assert torch.equal(v, before[k]), k


def test_published_checkpoint_architecture_against_oracle():
    """SURVEY F3 / VERDICT r2 item 8: the generator of the published vctk checkpoints (train.sh:11-15 -- netG local, ngf 56
    (channel counts 56 / 112 in the local branch, 112 ... 896 in the global one: not multiples of 64, several not of 16),
    resconv / interpolate sampling blocks, 3 bottleneck-attention blocks of 6 x 128 heads on 8 x 16 tokens) at its real size
    against the CPU oracle on the same N(0, 0.02) weights: forward, input gradient and EVERY parameter gradient, float64
    truth with the oracle's float32 run as the yardstick.  The attention block inside is the oracle's restatement of the
    third-party package (parity unpinned)."""
    from mdctgan_amd import networks
    kw = dict(input_size=(128, 256), n_attn_g=3, heads_g=6, dim_head_g=128, proj_factor_g=4)
    gen = torch.Generator().manual_seed(56)
    torch.manual_seed(56)
    o = onets.init_weights(onets.build_generator("local", 2, 1, 56, 3, 4, 3, up="interpolate", down="resconv", **kw), gen)
    sd = {k: v.clone() for k, v in o.state_dict().items()}
    net = networks.define_G(2, 1, 56, "local", 3, 4, 1, 3, upsample_type="interpolate", downsample_type="resconv", **kw)
    assert list(net.state_dict().keys()) == list(sd.keys())
    assert [tuple(v.shape) for v in net.state_dict().values()] == [tuple(v.shape) for v in sd.values()]
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    x = torch.rand(1, 2, 128, 256, generator=gen) * 2 - 1
    gy = torch.randn(1, 1, 128, 256, generator=gen)
    res = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    try:
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            o = o.to(dt).train()
            o.load_state_dict({k: v.to(dt) if v.dtype.is_floating_point else v for k, v in sd.items()})   # reset BN buffers
            o.zero_grad()
            xx = x.clone().to(dt).requires_grad_()
            y = o(xx)
            (y * gy.to(dt)).sum().backward()
            res[name] = dict(y=y.detach().numpy(), dx=xx.grad.numpy(),
                             grads={k: p.grad.numpy().copy() for k, p in o.named_parameters()})
    finally:
        torch.set_num_threads(threads)
    xd = x.to(DEV).requires_grad_()
    y = net(xd)
    (y * gy.to(DEV)).sum().backward()
    judged(y.detach().cpu().numpy(), res["f32"]["y"], res["f64"]["y"], "published arch forward")
    judged(xd.grad.cpu().numpy(), res["f32"]["dx"], res["f64"]["dx"], "published arch dL/dx", k=6.0)
    live = 0
    for k, p in net.named_parameters():
        if _dead_bias(k, res["f64"]["grads"][k], res["f64"]["grads"]):
            continue
        assert p.grad is not None, k
        judged(p.grad.cpu().numpy(), res["f32"]["grads"][k], res["f64"]["grads"][k], "published arch grad " + k, k=6.0)
        live += 1
    assert live >= 60, live


def test_step_without_abs_spectro_pair(golden):
    """pix2pixHD_model.py:404, 425-427, 440 (the else branches): without --abs_spectro --arcsinh_transform the generator sees
    the 1-channel spectrogram and the discriminators cat(lr, sr) -- here with --raw_mdct.  Forward losses against the oracle,
    one optimisation step (three discriminator passes: the stacked / shared passes are built on the 3-channel input
    kernel), every parameter of G and D receives a gradient, and the data gradient through the channel concat is checked
    against float64 directly."""
    from mdctgan_amd import functional as Fh
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    g = golden("g6_step_global")
    opt = options.make_opt("--raw_mdct", "--norm_range", "-1", "1", "--abs_norm", "--src_range", "-60", "60", "--input_nc", "1",
                           "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4", "--n_blocks_global", "2",
                           "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8", "--batchSize", "2", "--bins", "32",
                           "--segment_length", "7936", "--gpu_ids", "0")
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    onets.fill_deterministic(model.netD)
    assert next(iter(model.netD.parameters())).shape[1] == 2          # D input: lr + sr
    netG = onets.fill_deterministic(onets.build_generator("global", 1, 1, 4, 4, 2, input_size=(32, 256)))
    netD = onets.fill_deterministic(onets.MultiscaleDRef(2, ndf=8, n_layers=3, num_D=2))
    cfg = ostep.CodecCfg(arcsinh_transform=False, raw_mdct=True, src_range=(-60.0, 60.0), abs_spectro=False)
    ref = ostep.HotPathRef(netG, netD, cfg, num_D=2)
    lo, _ = ref.forward_losses(g["lr"], g["hr"])
    lr, hr = torch.from_numpy(g["lr"]).to(DEV), torch.from_numpy(g["hr"]).to(DEV)
    lh, _ = model._forward(lr, hr)
    for k, v in zip(model.loss_names, lh):
        assert abs(v.item() - float(lo[k])) <= 0.05 * abs(float(lo[k])) + 1e-3, (k, v.item(), float(lo[k]))
    ld = model.optimize_parameters(lr, hr)
    assert model._shared_rows == 0 and all(np.isfinite(v.item()) for v in ld.values())
    for net in (model.netG, model.netD):
        for k, p in net.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
    # the concat itself
    gen = torch.Generator().manual_seed(2)
    a = torch.randn(2, 1, 5, 7, generator=gen).to(DEV).requires_grad_()
    b = torch.randn(2, 3, 5, 7, generator=gen).to(DEV).requires_grad_()
    w = torch.randn(2, 4, 5, 7, generator=gen).to(DEV)
    y = Fh.cat_channels(a, b)
    assert torch.equal(y, torch.cat((a, b), dim=1))
    (y * w).sum().backward()
    assert torch.equal(a.grad, w[:, :1]) and torch.equal(b.grad, w[:, 1:])


def test_image_pool_step():
    """--pool_size 2 (pix2pixHD_model.py:294-298, 366-374): the D loss's fake pass reads the history pool.  While the pool
    fills up a query returns the images it was given, so the first iteration equals the pool-less three-pass step bit for bit;
    later iterations run on stored inputs (finite losses, every parameter still gets its gradient)."""
    import random
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model

    def build(*extra):
        opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                               "--n_blocks_global", "2", "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8", "--batchSize", "2",
                               "--bins", "32", "--segment_length", "7936", "--gpu_ids", "0", *extra)
        m = create_model(opt)
        onets.fill_deterministic(m.netG)
        onets.fill_deterministic(m.netD)
        return m
    random.seed(3)
    pooled, plain = build("--pool_size", "2"), build()
    plain.stack_d_loss_passes = False
    gen = torch.Generator().manual_seed(8)
    for it in range(4):
        hr = (0.05 * torch.randn(2, 7936, generator=gen)).to(DEV)
        lr = (0.05 * torch.randn(2, 7936, generator=gen)).to(DEV)
        lp = pooled.optimize_parameters(lr, hr)
        assert pooled._shared_rows == 0 and all(np.isfinite(v.item()) for v in lp.values())
        if it == 0:
            lq = plain.optimize_parameters(lr, hr)
            for k in lp:
                assert lp[k].item() == lq[k].item(), k
    assert pooled.fake_pool.num_imgs == 2 and len(pooled.fake_pool.images) == 2
    for k, p in pooled.netD.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_weight_side_fusion_is_bit_identical(golden, monkeypatch):
    """mg_conv_wgrad_adam_w (csrc/wino.h::wino_adam_kernel): for the Winograd trunk layers the weight gradient's inverse
    transform, the Adam update and the next iteration's weight transform are one kernel inside loss_G.backward(); the gradient
    never reaches the arena.  Five iterations (the persistent U images are used from the second on) must leave G and D bit
    for bit where the three separate kernels leave them (MG_NO_WINO_ADAM_FUSION=1), eagerly and as a hipGraph replay, and a
    learning-rate change must reach the fused kernels through the device clock."""
    g = golden("g6_step_global")
    lr, hr = torch.from_numpy(g["lr"]).to(DEV), torch.from_numpy(g["hr"]).to(DEV)

    def build():
        from mdctgan_amd import options
        from mdctgan_amd.pix2pixHD_model import create_model
        opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "8",
                               "--n_blocks_global", "2", "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8", "--batchSize", "2",
                               "--bins", "32", "--segment_length", "7936", "--gpu_ids", "0", "--niter_decay", "10")
        m = create_model(opt)
        onets.fill_deterministic(m.netG)
        onets.fill_deterministic(m.netD)
        return m

    snaps = {}

    def run(m, graphed):
        step = m.make_graphed_step(lr, hr, warmup=2) if graphed else (lambda: m.optimize_parameters(lr, hr))
        for it in range(2 if graphed else 0, 5):         # five iterations; the first two of the graphed model are its warm-up
            if it == 3:
                m.update_learning_rate()
                # (the optimiser's arena is built by the first zero_grad(): iteration 0 still ran the separate kernels)
                snaps[id(m)] = [p.grad.clone() for k, p in m.netG.named_parameters() if "conv_block" in k and k.endswith("weight")]
            step()
        torch.cuda.synchronize()
        return m

    monkeypatch.setenv("MG_NO_WINO_ADAM_FUSION", "1")
    plain = run(build(), False)
    trunk = [p for k, p in plain.netG.named_parameters() if "conv_block" in k and k.endswith("weight")]
    assert trunk and all(getattr(p, "_mg_u_persist", None) is None for p in trunk)
    monkeypatch.delenv("MG_NO_WINO_ADAM_FUSION")
    fused = run(build(), False)
    ftrunk = [p for k, p in fused.netG.named_parameters() if "conv_block" in k and k.endswith("weight")]
    assert all(getattr(p, "_mg_u_persist", None) is not None for p in ftrunk), "the trunk layers did not take the fused path"
    # a fused layer's gradient never reaches the arena: its buffer still holds iteration 0's values; the separate kernels rewrote it
    assert all(torch.equal(p.grad, s0) for p, s0 in zip(ftrunk, snaps[id(fused)]))
    assert not any(torch.equal(p.grad, s0) for p, s0 in zip(trunk, snaps[id(plain)]))
    for (k, a), (_, b) in zip(plain.netG.state_dict().items(), fused.netG.state_dict().items()):
        assert torch.equal(a, b), k
    for (k, a), (_, b) in zip(plain.netD.state_dict().items(), fused.netD.state_dict().items()):
        assert torch.equal(a, b), k
    assert torch.equal(plain.optimizer_G.flat_m, fused.optimizer_G.flat_m) and torch.equal(plain.optimizer_G.flat_v, fused.optimizer_G.flat_v)
    # the refreshed image is the transform of the updated weights
    from mdctgan_amd import ops
    p0 = ftrunk[0]
    gq = ops.conv_geom(2, 2, 16, p0.shape[1], p0.shape[0], 3, 3, 1, 1, True)
    assert torch.equal(p0._mg_u_persist, ops.wino_weights(gq, p0.detach()))
    # ... and the captured step carries the fused kernels
    graphed = run(build(), True)
    for (k, a), (_, b) in zip(plain.netG.state_dict().items(), graphed.netG.state_dict().items()):
        assert torch.equal(a, b), k
    assert torch.equal(fused.inference(lr)[0], plain.inference(lr)[0])


def test_next_layer_winograd_image_is_bit_identical(golden, monkeypatch):
    """mg_conv_fwd_instnorm_next (csrc/wino.h::wino_out_norm_kernel<NT, true>): inside a chain of ResnetBlocks the fused output
    transform + InstanceNorm kernel of a layer also writes the NEXT layer's Winograd input image, which then skips its own input
    transform.  Same float32 arithmetic on the same values: four training iterations (the image is also the consumer's saved
    operand for its weight gradient) and an inference pass must be bit for bit what MG_NO_WINO_NEXT=1 gives, eagerly and as a
    hipGraph replay, and the hand-over must really happen (3 blocks: 5 images made, 5 used per forward)."""
    from mdctgan_amd import functional as Fh
    g = golden("g6_step_global")
    lr, hr = torch.from_numpy(g["lr"]).to(DEV), torch.from_numpy(g["hr"]).to(DEV)

    def build():
        from mdctgan_amd import options
        from mdctgan_amd.pix2pixHD_model import create_model
        opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "8",
                               "--n_blocks_global", "3", "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8", "--batchSize", "2",
                               "--bins", "32", "--segment_length", "7936", "--gpu_ids", "0")
        m = create_model(opt)
        onets.fill_deterministic(m.netG)
        onets.fill_deterministic(m.netD)
        return m

    def run(m, graphed):
        step = m.make_graphed_step(lr, hr, warmup=2) if graphed else (lambda: m.optimize_parameters(lr, hr))
        for _ in range(2 if graphed else 0, 4):
            step()
        torch.cuda.synchronize()
        return m

    monkeypatch.setenv("MG_NO_WINO_NEXT", "1")
    Fh.WINO_NEXT_STATS.update(made=0, used=0)
    plain = run(build(), False)
    assert Fh.WINO_NEXT_STATS == {"made": 0, "used": 0}
    monkeypatch.delenv("MG_NO_WINO_NEXT")
    handed = run(build(), False)
    # per generator forward: conv 1 of every block hands over to conv 2 (3), conv 2 of blocks 0 / 1 to the next block (2)
    assert Fh.WINO_NEXT_STATS["made"] == Fh.WINO_NEXT_STATS["used"] == 4 * 5, Fh.WINO_NEXT_STATS
    graphed = run(build(), True)
    for other in (handed, graphed):
        for a_net, b_net in ((plain.netG, other.netG), (plain.netD, other.netD)):
            for (k, a), (_, b) in zip(a_net.state_dict().items(), b_net.state_dict().items()):
                assert torch.equal(a, b), k
        assert torch.equal(plain.optimizer_G.flat_m, other.optimizer_G.flat_m) and torch.equal(plain.optimizer_G.flat_v, other.optimizer_G.flat_v)
    n0 = dict(Fh.WINO_NEXT_STATS)
    out_h = handed.inference(lr)[0]
    assert Fh.WINO_NEXT_STATS["used"] - n0["used"] == 5
    monkeypatch.setenv("MG_NO_WINO_NEXT", "1")
    assert torch.equal(out_h, plain.inference(lr)[0])


def test_no_lsgan_step_against_oracle():
    """--no_lsgan --no_ganFeat_loss (networks.py:106-109 BCELoss, :676-677 Sigmoid; the only form in which the reference's
    BCE branch runs -- with feature matching on, its discriminator forward never applies the Sigmoid and BCELoss rejects the
    logits, which create_model reports as NotImplementedError): the sigmoid / BCE kernels op by op against float64, then the
    three losses of one iteration against the oracle and a finite optimisation step with every gradient in place."""
    from mdctgan_amd import functional as Fh
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    gen = torch.Generator().manual_seed(12)
    z = (3.0 * torch.randn(2, 1, 9, 17, generator=gen)).to(DEV).requires_grad_()
    for label in (0.0, 1.0):
        z.grad = None
        loss = Fh.bce_const_loss(Fh.sigmoid(z), label)
        loss.backward()
        z64 = z.detach().double().cpu().requires_grad_()
        l64 = torch.nn.functional.binary_cross_entropy(torch.sigmoid(z64), torch.full_like(z64, label))
        l64.backward()
        assert abs(loss.item() - l64.item()) <= 1e-6 * abs(l64.item())
        assert (z.grad.double().cpu() - z64.grad).abs().max().item() <= 1e-6 * z64.grad.abs().max().item()
    sat = torch.tensor([[[[40.0, -40.0, 120.0]]]], device=DEV)          # saturated probabilities: the -100 clamp of BCELoss
    want = torch.nn.functional.binary_cross_entropy(torch.sigmoid(sat.cpu()), torch.zeros(1, 1, 1, 3))
    assert abs(Fh.bce_const_loss(Fh.sigmoid(sat), 0.0).item() - want.item()) <= 1e-5 * want.item()
    flags = [*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4", "--n_blocks_global", "2",
             "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8", "--batchSize", "2", "--bins", "32", "--segment_length", "7936",
             "--gpu_ids", "0", "--no_lsgan"]
    with pytest.raises(NotImplementedError):
        create_model(options.make_opt(*flags))
    model = create_model(options.make_opt(*flags, "--no_ganFeat_loss"))
    onets.fill_deterministic(model.netG)
    onets.fill_deterministic(model.netD)
    assert model.loss_names == ["G_GAN", "D_real", "D_fake"]
    netG = onets.fill_deterministic(onets.build_generator("global", 2, 1, 4, 4, 2, input_size=(32, 256)))
    netD = onets.fill_deterministic(onets.MultiscaleDRef(3, ndf=8, n_layers=3, num_D=2, use_sigmoid=True, interm=False))
    assert list(netD.state_dict().keys()) == list(model.netD.state_dict().keys())
    ref = ostep.HotPathRef(netG, netD, ostep.CodecCfg(), num_D=2, use_lsgan=False, feat_loss=False)
    g = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "g6_step_global.npz"))
    lo, _ = ref.forward_losses(g["lr"], g["hr"])
    lr, hr = torch.from_numpy(g["lr"]).to(DEV), torch.from_numpy(g["hr"]).to(DEV)
    lh, _ = model._forward(lr, hr)
    for k, v in zip(model.loss_names, lh):
        assert abs(v.item() - float(lo[k])) <= 0.02 * abs(float(lo[k])) + 1e-4, (k, v.item(), float(lo[k]))
    ld = model.optimize_parameters(lr, hr)
    assert model._shared_rows == 0 and all(np.isfinite(v.item()) for v in ld.values())
    for net in (model.netG, model.netD):
        for k, p in net.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k


@pytest.mark.parametrize("gen_overlap", [0, 1024, 100])
def test_generate_with_stitching_k2_equals_decode_then_stitch(gen_overlap, monkeypatch):
    """generate_audio.py:28-53 end to end on a toy generator: 5 segments in batches of 2 -- K2 writing every batch straight into
    the stitched waveform (mg_imdct4_stitched) gives the bits of the reference's order of operations (decode every batch, concatenate,
    halve the edges / fold / crop: MG_NO_STITCHED_K2=1), for --gen_overlap 0, a multiple of 4 and one that is not; and
    segment_audio -> generate reproduces the input's length bookkeeping (the stitched waveform covers every input sample)."""
    from mdctgan_amd.generate_audio import generate, segment_audio
    model = make_model()
    T = 7936
    gen = torch.Generator().manual_seed(3)
    wave = 0.05 * torch.randn(4 * T + 123, generator=gen)
    segs = segment_audio(wave.to(DEV), T, gen_overlap)
    assert segs.shape[1] == T and segs.shape[0] >= 5
    monkeypatch.setenv("MG_NO_STITCHED_K2", "1")
    want = generate(model, segs, batch_size=2, gen_overlap=gen_overlap)
    monkeypatch.delenv("MG_NO_STITCHED_K2")
    got = generate(model, segs, batch_size=2, gen_overlap=gen_overlap)
    assert got.shape == want.shape and got.shape[-1] >= wave.numel()
    assert torch.equal(got, want), (gen_overlap, (got - want).abs().max().item())


@pytest.mark.parametrize("fp16,num_D", [(False, 2), (True, 3)], ids=["f32_numD2", "fp16_numD3"])
def test_feature_loss_gradient_joins_inside_the_layer_kernels(golden, monkeypatch, fp16, num_D):
    """Round 6 (functional.ExtraGrad): the feature-matching loss's gradient of a discriminator feature map is no longer added to the
    next layer's data gradient by an autograd accumulation launch -- the loss parks it and the map's producer (conv + LeakyReLU /
    InstanceNorm + LeakyReLU) reads dy + extra inside its own backward kernel (mg_act_bwd_add / mg_instnorm_bwd_add).  The same
    float32 addition: three iterations leave every parameter and both Adam moments bit for bit where MG_NO_EXTRA_GRAD=1 leaves
    them, and the parked gradients are really taken (no holder is left full)."""
    g = golden("g6_step_global")
    lr, hr = torch.from_numpy(g["lr"]).to(DEV), torch.from_numpy(g["hr"]).to(DEV)

    def run(off):
        if off:
            monkeypatch.setenv("MG_NO_EXTRA_GRAD", "1")
        else:
            monkeypatch.delenv("MG_NO_EXTRA_GRAD", raising=False)
        from mdctgan_amd import functional as Fh
        from mdctgan_amd import options
        from mdctgan_amd.pix2pixHD_model import create_model
        opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "8",
                               "--n_blocks_global", "2", "--n_blocks_attn_g", "0", "--num_D", str(num_D), "--ndf", "8", "--batchSize", "2",
                               "--bins", "32", "--segment_length", "7936", "--gpu_ids", "0", *(["--fp16"] if fp16 else []))
        m = create_model(opt)
        onets.fill_deterministic(m.netG)
        onets.fill_deterministic(m.netD)
        if fp16:
            m.scaler.state[0] = 64.0
        parked = []
        real = Fh._take_extra

        def spy(ctx, like):
            got = real(ctx, like)
            if got is not None:
                parked.append(tuple(got.shape))
            return got
        monkeypatch.setattr(Fh, "_take_extra", spy)
        for _ in range(3):
            ld = m.optimize_parameters(lr, hr)
        torch.cuda.synchronize()
        monkeypatch.setattr(Fh, "_take_extra", real)
        return m, {k: v.item() for k, v in ld.items()}, parked
    a, la, pa = run(False)
    b, lb, pb = run(True)
    assert len(pa) == 3 * 4 * num_D and pb == [], (len(pa), len(pb))      # four feature maps per scale, every iteration
    assert la == lb
    for net in ("netG", "netD"):
        for (k, x), (_, y) in zip(getattr(a, net).state_dict().items(), getattr(b, net).state_dict().items()):
            assert torch.equal(x, y), (net, k)
    for oa, ob in ((a.optimizer_G, b.optimizer_G), (a.optimizer_D, b.optimizer_D)):
        assert torch.equal(oa.flat_m, ob.flat_m) and torch.equal(oa.flat_v, ob.flat_v)
