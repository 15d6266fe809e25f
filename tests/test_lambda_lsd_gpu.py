"""--lambda_lsd on the device: the loss node's two new entry points on their own (mg_lsd_mean_loss, mg_lsd_rows_backward_seeded;
csrc/metrics_rows.hip, csrc/lsd_rows_grad.hip), metrics.lsd_loss_term against today's composition 0.5 * lsd_loss(...), and the
training step with the term (Pix2PixHDModel._forward / optimize_parameters / make_graphed_step, float32 and --fp16).

The accuracy of the LSD gradient is tests/test_lsd_loss_gpu.py's subject; here the seeded path must have that path's BITS (scale
0.5 is a power of two, so forming the rows' upstream gradient on the device changes no rounding), and the step must add the term's
gradient to the discriminator's at the generator's output with one float32 add and change nothing else."""
import os

import numpy as np
import pytest
import torch

import test_lsd_loss_host as H
from test_lsd_loss_gpu import opt_for
from test_metrics_many_gpu import GUARD, signal_pair

pytestmark = pytest.mark.gpu
REPO = H.REPO
UNWRITTEN = -7.0
LAMBDA = 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reduction
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.5, 3.0])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097])
def test_mean_loss_reduction(n, scale):
    """One workgroup walks tiles of 256 frames: 1 and 2 sit inside a wave of the first tile, 255 is one short of the tile, 256 fills
    it, 257 starts a second tile (the ascending add), 4097 is sixteen tiles and one frame.  A double sum rounded once lies within
    one float32 unit of the float64 numpy value rounded to float32: |got - want| <= 2^-23 |want|.  A rerun has the same bits; the
    input (inside a guard-filled array) is only read, and nothing but loss[0] is written."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    x = (0.5 + (np.arange(n) * 0.6180339887498949) % 1.0).astype(np.float32)
    want = np.float32(scale * x.astype(np.float64).sum() / n)
    buf = np.full(n + 16, GUARD, np.float32)
    buf[8:8 + n] = x
    d = torch.from_numpy(buf).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((3,), UNWRITTEN, dtype=torch.float32, device="cuda")
        _lib.check(lib.mg_lsd_mean_loss(_lib.ptr(d[8:]), n, scale, _lib.ptr(out[1:]), _lib.stream()), "mg_lsd_mean_loss")
        outs.append(out.cpu().numpy())
    got = outs[0][1]
    print("mg_lsd_mean_loss n=%d scale=%g: got %.9g want %.9g" % (n, scale, got, want))
    assert outs[0][0] == UNWRITTEN and outs[0][2] == UNWRITTEN
    assert abs(float(got) - float(want)) <= 2.0 ** -23 * abs(float(want))
    assert outs[0].tobytes() == outs[1].tobytes()
    assert np.array_equal(d.cpu().numpy(), buf)


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. the seeded backward and the value against today's path
# ---------------------------------------------------------------------------------------------------------------------
def dense_batch(T, seed, B=3, same=1):
    """B "noise" pairs of T samples, clip `same` with sr == hr -> (hr, sr) float32 [B, T]."""
    rng = np.random.default_rng(seed)
    pairs = [signal_pair("noise", T, rng) for _ in range(B)]
    hr, sr = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    sr[same] = hr[same]
    return hr, sr


def seeded_backward(hr, sr, n_fft, hop, center, go, scale):
    """mg_lsd_rows_backward_seeded on a dense [B, T] batch, as test_lsd_loss_gpu.lsd_backward calls the unseeded entry point: the
    gradient buffer and the workspace lie inside guard-filled arrays that are checked here; the buffer starts as UNWRITTEN."""
    from mdctgan_amd import _lib
    from mdctgan_amd.metrics import plan_metrics
    lib = _lib.load()
    B, T = sr.shape
    plan = plan_metrics([T] * B, n_fft, hop, center)
    total = plan.total_frames
    rows = torch.tensor([[b * T, 0, b * T, T] for b in range(B)], dtype=torch.int64).cuda()
    fsd = torch.tensor(plan.frame_start, dtype=torch.int64).cuda()
    hd, sd = torch.from_numpy(hr.reshape(-1)).cuda(), torch.from_numpy(sr.reshape(-1)).cuda()
    wd = torch.from_numpy(H.window32(n_fft)).cuda()
    god = torch.tensor([go], dtype=torch.float32).cuda()
    nbytes = lib.mg_lsd_rows_backward_workspace(total, n_fft)
    ws = torch.full((nbytes // 4 + 8,), GUARD, dtype=torch.float32, device="cuda")
    grad = torch.full((B * T + 24,), UNWRITTEN, dtype=torch.float32, device="cuda")
    _lib.check(lib.mg_lsd_rows_backward_seeded(_lib.ptr(hd), hd.numel(), _lib.ptr(sd), sd.numel(), _lib.ptr(rows), B, _lib.ptr(fsd),
                                               total, None, _lib.ptr(wd), n_fft, hop, int(center), _lib.ptr(god), scale,
                                               _lib.ptr(grad[12:]), _lib.ptr(ws[4:]), nbytes, _lib.stream()),
               "mg_lsd_rows_backward_seeded")
    assert bool((ws[:4] == GUARD).all()) and bool((ws[4 + nbytes // 4:] == GUARD).all())
    assert bool((grad[:12] == UNWRITTEN).all()) and bool((grad[12 + B * T:] == UNWRITTEN).all())
    return grad[12:12 + B * T].reshape(B, T)


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("hop_div", [2, 4])
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_seeded_backward_has_the_bits_of_the_composition(n_fft, hop_div, center):
    """B = 3 clips of 7936 and of 5000 samples (a ragged last frame when not centred), clip 1 with sr == hr; go = 1, scale = 0.5.
    d lsd_loss_term / d sr == d (0.5 * lsd_loss) / d sr == the C entry point, all with torch.equal; the sr == hr clip's gradient is
    exactly 0; every sample of the dense batch is written (no zero fill behind it) and nothing around the buffer is.  The value:
    |term - float32(0.5 * lsd_loss)| <= 2^-22 term (the mean over all frames against the mean of per-clip means, both in double
    and rounded once: one float32 unit, and one more for the cast of the reference)."""
    from mdctgan_amd.metrics import lsd_loss, lsd_loss_term
    hop = n_fft // hop_div
    opt = opt_for(n_fft, hop, center)
    for T in (7936, 5000):
        hr, sr = dense_batch(T, n_fft + hop + center + T)
        hd = torch.from_numpy(hr).cuda()
        x = torch.from_numpy(sr).cuda().requires_grad_()
        ref = 0.5 * lsd_loss(x, hd, opt)
        (g_ref,) = torch.autograd.grad(ref, x)
        term = lsd_loss_term(x, hd, opt, 0.5)
        assert term.dtype == torch.float32 and term.dim() == 0
        (g_term,) = torch.autograd.grad(term, x)
        raw = seeded_backward(hr, sr, n_fft, hop, center, 1.0, 0.5)
        assert not bool((raw == UNWRITTEN).any())
        assert g_term.shape == x.shape and torch.equal(g_term, g_ref) and torch.equal(raw, g_ref)
        assert bool((g_term[1] == 0).all()) and float(g_term[0].abs().max()) > 0 and float(g_term[2].abs().max()) > 0
        assert bool(torch.isfinite(g_term).all())
        want = ref.detach().float().item()
        print("lsd_loss_term N=%d hop=%d center=%d T=%d: term %.9g, float32(0.5 lsd_loss) %.9g" % (n_fft, hop, center, T, term.item(), want))
        assert term.item() > 0 and abs(term.item() - want) <= 2.0 ** -22 * term.item()


def test_term_against_float64_autograd_of_the_reference():
    """N = 1024, hop 512, centred, the three [.., T] operand forms: the term is within the project's 2e-4 relative LSD bound of the
    float64 CPU value of the reference's expression, with the same bits for every form; lsd_loss's checks hold."""
    from mdctgan_amd.metrics import lsd_loss_term
    n_fft, hop, B, T = 1024, 512, 3, 7936
    hr, sr = dense_batch(T, 9)
    want = 0.5 * float(np.mean([H.lsd_autograd(h, s, H.window32(n_fft), n_fft, hop, True, torch.float64)[0] for h, s in zip(hr, sr)]))
    opt = opt_for(n_fft, hop, True)
    vals = [lsd_loss_term(torch.from_numpy(sr).cuda().reshape(shape), torch.from_numpy(hr).cuda().reshape(shape), opt, 0.5)
            for shape in ((B, T), (B, 1, T), (B, 1, 1, T))]
    print("lsd_loss_term %.9g, float64 reference %.9g" % (vals[0].item(), want))
    assert abs(vals[0].item() - want) <= 2e-4 * want
    assert torch.equal(vals[0], vals[1]) and torch.equal(vals[0], vals[2]) and vals[0].grad_fn is None
    with pytest.raises(ValueError):
        lsd_loss_term(torch.zeros(B, 2, T, device="cuda"), torch.zeros(B, 2, T, device="cuda"), opt, 0.5)
    with pytest.raises(ValueError):
        lsd_loss_term(torch.zeros(B, T, device="cuda"), torch.zeros(B, T - 1, device="cuda"), opt, 0.5)
    with pytest.raises(NotImplementedError, match="hr"):
        lsd_loss_term(torch.zeros(B, T, device="cuda"), torch.zeros(B, T, device="cuda").requires_grad_(), opt, 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the seed is read at replay
# ---------------------------------------------------------------------------------------------------------------------
def test_the_upstream_gradient_is_read_when_the_graph_replays():
    """Forward plus backward of the node captured with the upstream gradient in a device tensor holding 1; with 4 in it the replay
    gives exactly four times the gradient (a power of two through linear float32 arithmetic) and the same loss: a captured --fp16
    step follows a loss scale that changes between replays.  Only detached results are kept ("Graph capture")."""
    from mdctgan_amd.metrics import lsd_loss_term
    hr, sr = dense_batch(7936, 21, B=4)
    hd = torch.from_numpy(hr).cuda()
    x = torch.from_numpy(sr).cuda().requires_grad_()
    go = torch.ones((), dtype=torch.float32, device="cuda")
    opt = opt_for(1024, 512, True)

    def run():
        loss = lsd_loss_term(x, hd, opt, 0.5)
        (g,) = torch.autograd.grad(loss, x, grad_outputs=go)
        return loss.detach(), g
    l0, g0 = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lc, gc = run()
    graph.replay()
    l1, g1 = lc.clone(), gc.clone()
    go.fill_(4.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(l1, l0) and torch.equal(g1, g0) and float(g1.abs().max()) > 0
    assert torch.equal(gc, 4.0 * g1) and torch.equal(lc, l1)


# ---------------------------------------------------------------------------------------------------------------------
# the step: the toy model of tests/test_codec_grad_gpu.py::_toy_model (ngf 4, 2 blocks, bins 32, segment 7936, batch 2)
# ---------------------------------------------------------------------------------------------------------------------
def toy_model(*extra):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    from oracle import nets as onets
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                           "--n_blocks_global", "2", "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8",
                           "--batchSize", "2", "--bins", "32", "--segment_length", "7936", "--gpu_ids", "0", *extra)
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    onets.fill_deterministic(model.netD)
    return model


@pytest.fixture(scope="module")
def batch():
    g = np.load(os.path.join(REPO, "tests", "golden", "g6_step_global.npz"))
    return torch.from_numpy(g["lr"]).cuda(), torch.from_numpy(g["hr"]).cuda()


def node_gradient(model, spectro, lr_norm, hr):
    """d lsd_loss_term(to_audio(leaf, lr_norm), hr, opt, LAMBDA) / d leaf at leaf = spectro.detach()"""
    from mdctgan_amd.metrics import lsd_loss_term
    leaf = spectro.detach().clone().requires_grad_()
    (g,) = torch.autograd.grad(lsd_loss_term(model.preprocess.to_audio(leaf, lr_norm), hr, model.opt, LAMBDA), leaf)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    return g


@pytest.mark.parametrize("arrangement", ["stacked", "separate", "stacked_fit_residual"])
def test_forward_adds_the_term_at_the_generators_output(batch, arrangement):
    """_forward(infer=True) and a plain .backward() of G_GAN + G_GAN_Feat + G_lsd, with the two discriminator arrangements that
    plain backward calls reach (the shared pass is optimize_parameters': next test) and with --fit_residual: the gradient at the
    returned sr_spectro is the lambda = 0 model's there plus the node's, and the generator's parameter gradients are those of
    sr_spectro.backward(total)."""
    from mdctgan_amd import functional as Fh
    lr, hr = batch
    extra = ["--fit_residual"] if arrangement.endswith("fit_residual") else []

    def run(model):
        model.stack_d_loss_passes = not arrangement.startswith("separate")
        params = [p for p in model.netG.parameters() if p.requires_grad]
        for p in params:
            p.grad = None
        losses, sr_spectro = model._forward(lr, hr, infer=True)
        got = []
        sr_spectro.register_hook(lambda g: got.append(g.clone()))
        d = dict(zip(model.loss_names, losses))
        sum(d[k] for k in model.loss_names if k.startswith("G_")).backward()
        assert len(got) == 1
        return d, sr_spectro.detach(), got[0], params, [Fh.grad_of(p).clone() for p in params]

    plain = toy_model(*extra)
    assert plain.loss_names == ["G_GAN", "G_GAN_Feat", "D_real", "D_fake"]
    d0, s0, g0, _, _ = run(plain)
    model = toy_model(*extra, "--lambda_lsd", str(LAMBDA))
    assert model.loss_names == ["G_GAN", "G_GAN_Feat", "G_lsd", "D_real", "D_fake"]
    d1, s1, total, params, grads = run(model)
    assert torch.equal(s0, s1) and all(torch.equal(d0[k], d1[k]) for k in d0)
    lsd = d1["G_lsd"]
    assert lsd.dtype == torch.float32 and lsd.dim() == 0 and bool(torch.isfinite(lsd)) and lsd.item() > 0
    lr_norm = model.preprocess.forward(lr)[2]
    assert torch.equal(total, g0 + node_gradient(model, s1, lr_norm, hr))
    assert not torch.equal(total, g0)
    # two stages: the same total gradient pushed into a fresh forward pass of the generator
    for p in params:
        p.grad = None
    model.forward(lr, hr)[0].backward(total)
    assert all(torch.equal(a, Fh.grad_of(p)) for a, p in zip(grads, params))
    assert any(float(a.abs().max()) > 0 for a in grads)


def step_with_output_hook(model, lr, hr):
    """one optimize_parameters(); -> (loss dict, the generator's output, the gradient that arrived there)"""
    seen = {"out": [], "grad": []}
    inner = model.netG.forward

    def forward(x):
        y = inner(x)
        seen["out"].append(y.detach().clone())
        y.register_hook(lambda g: seen["grad"].append(g.clone()))
        return y
    model.netG.forward = forward
    try:
        losses = model.optimize_parameters(lr, hr)
    finally:
        del model.netG.forward
    assert len(seen["out"]) == 1 and len(seen["grad"]) == 1
    return losses, seen["out"][0], seen["grad"][0]


def test_optimize_parameters_adds_the_term_in_the_shared_pass(batch):
    lr, hr = batch
    plain, model = toy_model(), toy_model("--lambda_lsd", str(LAMBDA))
    lr_norm = model.preprocess.forward(lr)[2]
    l0, y0, g0 = step_with_output_hook(plain, lr, hr)
    l1, y1, g1 = step_with_output_hook(model, lr, hr)
    assert plain._shared_rows == model._shared_rows == lr.shape[0], "the step did not take the shared discriminator pass"
    assert torch.equal(y0, y1)
    assert torch.equal(g1, g0 + node_gradient(model, y1, lr_norm, hr)) and not torch.equal(g1, g0)
    assert list(l1) == ["G_GAN", "G_GAN_Feat", "G_lsd", "D_real", "D_fake"] and list(l0) == ["G_GAN", "G_GAN_Feat", "D_real", "D_fake"]
    assert l1["G_lsd"].grad_fn is None and not l1["G_lsd"].requires_grad
    assert bool(torch.isfinite(l1["G_lsd"])) and l1["G_lsd"].item() > 0
    assert all(torch.equal(l0[k], l1[k]) for k in l0)
    torch.cuda.synchronize()
    g_same = [torch.equal(a, b) for a, b in zip(plain.netG.state_dict().values(), model.netG.state_dict().values())]
    assert not all(g_same)
    assert all(bool(torch.isfinite(v).all()) for v in model.netG.state_dict().values())
    # the term does not touch the discriminator's pass
    for (k, a), (_, b) in zip(plain.netD.state_dict().items(), model.netD.state_dict().items()):
        assert torch.equal(a, b), k


def eager_and_replayed(batch, *extra):
    """five eager steps against two warm-up steps and three replays of the captured step, a fresh model each"""
    lr, hr = batch
    eager, graphed = toy_model("--lambda_lsd", str(LAMBDA), *extra), toy_model("--lambda_lsd", str(LAMBDA), *extra)
    for _ in range(5):
        le = eager.optimize_parameters(lr, hr)
    run = graphed.make_graphed_step(lr, hr, warmup=2)
    for _ in range(3):
        lg = run(lr, hr)
    torch.cuda.synchronize()
    assert "G_lsd" in le and list(le) == list(lg)
    for k in le:
        assert le[k].grad_fn is None and lg[k].grad_fn is None
        assert np.isfinite(le[k].item()) and le[k].item() == lg[k].item(), k
    for a_net, b_net in ((eager.netG, graphed.netG), (eager.netD, graphed.netD)):
        for (k, a), (_, b) in zip(a_net.state_dict().items(), b_net.state_dict().items()):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), k
    assert torch.equal(eager.optimizer_G.flat_m, graphed.optimizer_G.flat_m) and torch.equal(eager.optimizer_G.flat_v, graphed.optimizer_G.flat_v)
    return eager, graphed


def test_graphed_step_with_the_term_equals_eager_steps(batch):
    eager, _ = eager_and_replayed(batch)
    # ... and the term moved the generator: five steps without it end elsewhere
    plain = toy_model()
    for _ in range(5):
        plain.optimize_parameters(*batch)
    assert not all(torch.equal(a, b) for a, b in zip(plain.netG.state_dict().values(), eager.netG.state_dict().values()))


def test_fp16_step_with_the_term(batch):
    """--fp16: to_audio and the term run in float32 on the generator's float32 output, the backward seed carries the loss scale
    (read on the device by the seeded kernel), and the captured step replays to the eager bits, GradScaler state included."""
    eager, graphed = eager_and_replayed(batch, "--fp16")
    assert eager.scaler is not None and bool(torch.isfinite(eager.scaler.state).all())
    assert torch.equal(eager.scaler.state, graphed.scaler.state) and eager.scaler.get_scale() > 0


def test_refusals(batch):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    lr, hr = batch
    base = ["--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4", "--n_blocks_global", "2", "--n_blocks_attn_g", "0",
            "--num_D", "2", "--ndf", "8", "--batchSize", "2", "--bins", "32", "--segment_length", "7936", "--gpu_ids", "0"]
    with pytest.raises(NotImplementedError, match="lambda_lsd"):
        create_model(options.make_opt("--explicit_encoding", "--lambda_lsd", "1", *base))
    with pytest.raises(NotImplementedError, match="lambda_lsd"):
        create_model(options.make_opt("--lambda_lsd", "1", *base))                       # no codec flag: the dB codec
    with pytest.raises(NotImplementedError, match="lambda_lsd"):
        create_model(options.make_opt(*options.SPECTRAL_FLAGS, "--n_fft", "2048", "--win_length", "2048", "--hop_length", "1024",
                                      "--lambda_lsd", "1", *base))
    with pytest.raises(NotImplementedError, match="lambda_lsd"):
        create_model(options.make_opt(*options.SPECTRAL_FLAGS, "--n_fft", "2048", "--lambda_lsd", "1", *base))
    with pytest.raises(NotImplementedError, match="lambda_lsd.*win_length"):
        create_model(options.make_opt(*options.SPECTRAL_FLAGS, "--win_length", "256", "--lambda_lsd", "1", *base))
    with pytest.raises(ValueError, match="lambda_lsd"):
        create_model(options.make_opt(*options.SPECTRAL_FLAGS, "--lambda_lsd", "-0.5", *base))
    model = toy_model("--lambda_lsd", "1")
    for call in (lambda h: model.optimize_parameters(lr, h), lambda h: model._forward(lr, h)):
        with pytest.raises(ValueError, match="hr_audio"):
            call(hr[:, :-256].contiguous())
    assert np.isfinite(model.optimize_parameters(lr, hr)["G_lsd"].item())
