"""K5/K7/K8/K9/K11/K12 kernels (csrc/instnorm.hip, elementwise.hip, loss.hip, optim.hip) against plain PyTorch float64 CPU references."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel_err(got, want):
    return (got.double().cpu() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


@pytest.mark.parametrize("shape", [(2, 16, 8, 16), (3, 5, 7, 9), (2, 64, 32, 64), (8, 256, 8, 16), (2, 1, 19, 35),
                                   # single-launch slab kernels (C % 32 == 0, HW <= 640): every register depth, ragged HW
                                   (2, 32, 9, 17), (1, 96, 16, 32), (2, 64, 17, 33), (2, 32, 18, 34), (1, 32, 20, 32),
                                   (1, 32, 2, 3), (2, 32, 21, 31)])
@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
def test_instnorm_fwd_bwd(shape, act):
    from mdctgan_amd import ops
    code = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU02}[act]
    fn = {"none": lambda t: t, "relu": torch.relu, "lrelu": lambda t: F.leaky_relu(t, 0.2)}[act]
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn(*shape, generator=gen, dtype=torch.float64) * 3 + 1.5).requires_grad_()
    res = torch.randn(*shape, generator=gen, dtype=torch.float64)
    y = fn(F.instance_norm(x, eps=1e-5)) + res
    gy = torch.randn(*shape, generator=gen, dtype=torch.float64)
    y.backward(gy)
    xd, rd, gyd = nhwc(x.detach()).float().to(DEV), nhwc(res).float().to(DEV), nhwc(gy).float().to(DEV)
    yd, mean, rstd = ops.instnorm_fwd(xd, code, rd)
    assert rel_err(yd, nhwc(y.detach())) < 1e-5
    dxd = ops.instnorm_bwd(gyd, xd, mean, rstd, code)
    assert rel_err(dxd, nhwc(x.grad)) < 2e-5
    y2, _, _ = ops.instnorm_fwd(xd, code, None)
    assert rel_err(y2, nhwc((y - res).detach())) < 1e-5


@pytest.mark.parametrize("shape", [(8, 64, 128, 256), (2, 64, 32, 64), (8, 128, 64, 128), (3, 12, 7, 9), (2, 4, 19, 35), (8, 256, 33, 65)])
@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
def test_instnorm_row_kernels_equal_the_flat_ones(shape, act, monkeypatch):
    """norm_apply_rows_kernel (statistics in registers, threads walk pixel rows) against norm_apply_{fwd,bwd}_kernel
    (MG_NO_NORM_ROWS=1): the same arithmetic per element, so the same bits -- outputs, the float16 copies, with and without the
    residual, ragged pixel counts and channel counts that do not fill a 64-channel block."""
    from mdctgan_amd import ops
    code = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU02}[act]
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(11)
    x = (torch.randn(B, H, W, C, generator=gen) * 2 + 0.5).to(DEV)
    res = torch.randn(B, H, W, C, generator=gen).to(DEV)
    gy = torch.randn(B, H, W, C, generator=gen).to(DEV)
    outs = []
    for rows in (False, True):
        if rows:
            monkeypatch.delenv("MG_NO_NORM_ROWS", raising=False)
        else:
            monkeypatch.setenv("MG_NO_NORM_ROWS", "1")
        y16 = torch.zeros(x.numel(), dtype=torch.float16, device=DEV)
        d16 = torch.zeros(x.numel(), dtype=torch.float16, device=DEV)
        y, mean, rstd = ops.instnorm_fwd(x, code, res, y16=y16)
        y2, _, _ = ops.instnorm_fwd(x, code, None)
        dx = ops.instnorm_bwd(gy, x, mean, rstd, code, dx16=d16)
        outs.append((y, y2, dx, y16, d16, mean, rstd))
    for a, b in zip(*outs):
        assert torch.equal(a, b), (shape, act)


def test_act_bwd_add_pool_upsample():
    from mdctgan_amd import ops
    gen = torch.Generator().manual_seed(2)
    for shape in [(2, 3, 32, 64), (1, 8, 17, 33), (2, 4, 5, 6)]:
        x = torch.randn(*shape, generator=gen, dtype=torch.float64, requires_grad=True)
        y = F.avg_pool2d(x, 3, stride=2, padding=1, count_include_pad=False)
        gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        y.backward(gy)
        xd = nhwc(x.detach()).float().to(DEV)
        yd = ops.avgpool_fwd(xd)
        assert yd.shape == nhwc(y).shape and rel_err(yd, nhwc(y.detach())) < 1e-6
        dxd = ops.avgpool_bwd(nhwc(gy).float().to(DEV), xd.shape)
        assert rel_err(dxd, nhwc(x.grad)) < 1e-6
        x.grad = None
        u = F.interpolate(x, scale_factor=2.0, mode="nearest")
        gu = torch.randn(u.shape, generator=gen, dtype=torch.float64)
        u.backward(gu)
        assert rel_err(ops.upsample_fwd(xd), nhwc(u.detach())) < 1e-6
        assert rel_err(ops.upsample_bwd(nhwc(gu).float().to(DEV)), nhwc(x.grad)) < 1e-6
    a = torch.randn(1000, generator=gen).to(DEV)
    b = torch.randn(1000, generator=gen).to(DEV)
    assert torch.equal(ops.add(a, b), a + b)
    for act, f in ((ops.ACT_TANH, torch.tanh), (ops.ACT_LRELU02, lambda t: F.leaky_relu(t, 0.2))):
        pre = torch.randn(1000, generator=gen, dtype=torch.float64, requires_grad=True)
        yy = f(pre)
        gg = torch.randn(1000, generator=gen, dtype=torch.float64)
        yy.backward(gg)
        got = ops.act_bwd(gg.float().to(DEV), yy.detach().float().to(DEV), act)
        assert rel_err(got, pre.grad) < 1e-5


def test_dinput_pair_losses_adam():
    from mdctgan_amd import ops
    gen = torch.Generator().manual_seed(3)
    lr = torch.randn(2, 8, 16, generator=gen, dtype=torch.float64)
    s = torch.randn(2, 8, 16, generator=gen, dtype=torch.float64, requires_grad=True)
    out = torch.stack((lr, s, s.abs() * 2 - 1), dim=-1)
    go = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    out.backward(go)
    od = ops.dinput_fwd(lr.float().to(DEV), s.detach().float().to(DEV), -1.0)
    assert rel_err(od, out.detach()) < 1e-6
    assert rel_err(ops.dinput_bwd(go.float().to(DEV), s.detach().float().to(DEV)), s.grad) < 1e-6
    pr = ops.pair_fwd(s.detach().float().to(DEV), -1.0)
    assert rel_err(pr, out.detach()[..., 1:]) < 1e-6
    # losses
    for n in (37, 5320, 300000):
        a = torch.randn(n, generator=gen, dtype=torch.float64, requires_grad=True)
        b = torch.randn(n, generator=gen, dtype=torch.float64)
        la = 0.7 * F.mse_loss(a, torch.ones_like(a)) + 1.3 * F.l1_loss(a, b)
        la.backward()
        ad, bd = a.detach().float().to(DEV), b.float().to(DEV)
        loss = torch.zeros(1, device=DEV)
        ops.mse_const_fwd(ad, 1.0, 0.7, loss, False)
        ops.l1_fwd(ad, bd, 1.3, loss, True)
        assert abs(loss.item() - la.item()) < 1e-5 * abs(la.item())
        go1 = torch.full((1,), 2.0, device=DEV)
        gsum = ops.mse_const_bwd(ad, 1.0, 0.7, go1) + ops.l1_bwd(ad, bd, 1.3, go1)
        assert rel_err(gsum, 2.0 * a.grad) < 1e-5
    # Adam == torch.optim.Adam (betas 0.5/0.999, lr 2e-4), three steps
    p0 = torch.randn(4097, generator=gen)
    pt = p0.clone().requires_grad_()
    opt = torch.optim.Adam([pt], lr=2e-4, betas=(0.5, 0.999))
    pd = p0.clone().to(DEV)
    m = torch.zeros_like(pd)
    v = torch.zeros_like(pd)
    for step in range(1, 4):
        g = torch.randn(4097, generator=gen) * 10 ** float(torch.randint(-6, 1, (1,), generator=gen))
        pt.grad = g.clone()
        opt.step()
        ops.adam_step(pd, g.to(DEV), m, v, 2e-4, 0.5, 0.999, 1e-8, step)
        assert (pd.cpu() - pt.detach()).abs().max().item() <= 2.4e-7   # 1 ulp at |p| < 4: lr * m/denom rounds once differently


def test_multi_tensor_losses_equal_the_single_tensor_calls():
    """mg_loss_multi_fwd / mg_loss_multi_bwd (the feature-matching sum over the discriminator layers as one launch per stage) ==
    the accumulate-in-place sequence of single-tensor calls, bit for bit; the backward also clears the requested tail."""
    from mdctgan_amd import _lib, ops
    lib = _lib.load()

    def bce_fwd(x, t, sc, loss, acc):
        ws = _lib.workspace(lib.mg_loss_workspace(), x.device)
        _lib.check(lib.mg_bce_const_fwd(_lib.ptr(x), x.numel(), t, sc, _lib.ptr(loss), int(acc), _lib.ptr(ws), _lib.stream()), "bce")

    def bce_bwd(x, t, sc, go, out):
        _lib.check(lib.mg_bce_const_bwd(_lib.ptr(x), x.numel(), t, sc, _lib.ptr(go), _lib.ptr(out), _lib.stream()), "bce")
    gen = torch.Generator().manual_seed(13)
    shapes = [(2, 65, 129, 64), (2, 33, 65, 128), (2, 17, 33, 256), (2, 18, 34, 512), (2, 3, 5, 1), (2, 700, 1100, 3)]
    for kind in (ops.LOSS_MSE_CONST, ops.LOSS_L1, ops.LOSS_BCE_CONST):
        a = [torch.rand(s, generator=gen).to("cuda") * 0.98 + 0.01 for s in shapes]
        b = [torch.rand(s, generator=gen).to("cuda") for s in shapes]
        target, scale = (0.0, 1.0) if kind == ops.LOSS_L1 else (1.0, 0.7)
        single_fwd = {ops.LOSS_MSE_CONST: lambda x, y, l, acc: ops.mse_const_fwd(x, target, scale, l, acc),
                      ops.LOSS_L1: lambda x, y, l, acc: ops.l1_fwd(x, y, scale, l, acc),
                      ops.LOSS_BCE_CONST: lambda x, y, l, acc: bce_fwd(x, target, scale, l, acc)}[kind]
        single_bwd = {ops.LOSS_MSE_CONST: lambda x, y, go, out: ops.mse_const_bwd(x, target, scale, go, out=out),
                      ops.LOSS_L1: lambda x, y, go, out: ops.l1_bwd(x, y, scale, go, out=out),
                      ops.LOSS_BCE_CONST: lambda x, y, go, out: bce_bwd(x, target, scale, go, out)}[kind]
        want = torch.full((1,), 3.25, device="cuda")
        got = want.clone()
        for i, (x, y) in enumerate(zip(a, b)):
            single_fwd(x, y, want, True)
        ops.loss_multi_fwd(kind, [(x, y if kind == ops.LOSS_L1 else None, None, 0) for x, y in zip(a, b)], target, scale, got, True)
        assert torch.equal(got, want), (kind, got.item(), want.item())
        fresh = torch.full((1,), float("nan"), device="cuda")
        ops.loss_multi_fwd(kind, [(x, y if kind == ops.LOSS_L1 else None, None, 0) for x, y in zip(a, b)], target, scale, fresh)
        assert torch.equal(fresh, want - 3.25) or abs(fresh.item() - (want.item() - 3.25)) <= 1e-6 * abs(want.item())
        go = torch.full((1,), 0.37, device="cuda")
        rows, wants, bufs = [], [], []
        for x, y in zip(a, b):
            tail = x.numel() // 2
            buf = torch.full((x.numel() + tail,), float("nan"), device="cuda")
            w_ = torch.empty_like(x)
            single_bwd(x, y, go, w_)
            rows.append((x, y if kind == ops.LOSS_L1 else None, buf, tail))
            wants.append(w_)
            bufs.append(buf)
        ops.loss_multi_bwd(kind, rows, target, scale, go)
        for buf, w_ in zip(bufs, wants):
            n = w_.numel()
            assert torch.equal(buf[:n], w_.reshape(-1)) and bool((buf[n:] == 0).all())


# ---- the list loss kernels against float64 (the single-tensor entry points are lists of one: the test above compares the list
# kernels with themselves, this one is their independent reference) ---------------------------------------------------------------
# An item has min(ceil(n / 1024), 1024) partial blocks: one block with one element, one block with a ragged last wave, exactly one
# full block, a second block with one element, and the first size past the cap (every block makes a second grid-stride trip).
LOSS_SIZES = [1, 1023, 1024, 1025, 1024 * 1024 + 5]
LOSS_LIST = (1025, 1, 1024 * 1024 + 5)            # one list of three unequal items
LOSS_CASES = {"mse": (0, 1.0, 0.7), "l1": (1, 0.0, 1.3), "bce_real": (2, 1.0, 0.7), "bce_fake": (2, 0.0, 0.7)}      # kind, target, scale
_loss_cache = {}


def loss_inputs(n):
    """(a, b) float32 on the CPU, in (0.01, 0.99) as the test above draws them (BCE's logarithms stay clear of the clamp), and no
    a - b is zero: |a - b| >= 0.01 by construction, so the float32 and the float64 sign agree."""
    if n not in _loss_cache:
        gen = torch.Generator().manual_seed(1000 + n % 997)
        a = torch.rand(n, generator=gen) * 0.98 + 0.01
        b = torch.rand(n, generator=gen) * 0.98 + 0.01
        b = torch.where((a - b).abs() < 0.01, 1.0 - a, b)           # |a - (1 - a)| < 0.01 only for a in (0.495, 0.505) ...
        b = torch.where((a - b).abs() < 0.01, a + 0.25, b)          # ... where a + 0.25 stays inside (0.01, 0.99)
        assert bool(((a.double() - b.double()).abs() >= 0.0099).all()) and 0.01 <= min(a.min(), b.min()) and max(a.max(), b.max()) <= 0.99
        _loss_cache[n] = (a, b)
    return _loss_cache[n]


def loss_ref(kind, a, b, target):
    """float64: (mean loss, its gradient with respect to a)."""
    n = a.numel()
    if kind == 0:
        return ((a - target) ** 2).mean().item(), 2.0 * (a - target) / n
    if kind == 1:
        return (a - b).abs().mean().item(), torch.sign(a - b) / n
    return (-(target * a.log() + (1.0 - target) * (1.0 - a).log())).mean().item(), (a - target) / ((1.0 - a) * a) / n


@pytest.mark.parametrize("sizes", [(n,) for n in LOSS_SIZES] + [LOSS_LIST], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", sorted(LOSS_CASES))
def test_list_losses_against_float64(case, sizes):
    """mg_loss_multi_fwd / mg_loss_multi_bwd against a CPU float64 evaluation: every block-count edge as a list of one, and one list
    of three; forward into a fresh scalar and accumulated onto one, backward under a grad_out tensor.  Bounds: those of
    test_dinput_pair_losses_adam (loss 1e-5 relative, gradients rel_err < 1e-5)."""
    from mdctgan_amd import ops
    kind, target, scale = LOSS_CASES[case]
    host = [loss_inputs(n) for n in sizes]
    refs = [loss_ref(kind, a.double(), b.double(), target) for a, b in host]
    want = scale * sum(r[0] for r in refs)
    dev = [(a.to(DEV), b.to(DEV) if kind == ops.LOSS_L1 else None) for a, b in host]
    fresh = torch.full((1,), float("nan"), device=DEV)
    ops.loss_multi_fwd(kind, [(a, b, None, 0) for a, b in dev], target, scale, fresh)
    onto = torch.full((1,), 3.25, device=DEV)
    ops.loss_multi_fwd(kind, [(a, b, None, 0) for a, b in dev], target, scale, onto, True)
    print("%s %s: loss %.9g / %.9g, accumulated %.9g / %.9g" % (case, sizes, fresh.item(), want, onto.item(), 3.25 + want))
    assert abs(fresh.item() - want) < 1e-5 * abs(want)
    assert abs(onto.item() - (3.25 + want)) < 1e-5 * abs(3.25 + want)
    go = torch.full((1,), 0.37, device=DEV)
    grads = [torch.full_like(a, float("nan")) for a, _ in dev]
    ops.loss_multi_bwd(kind, [(a, b, g, 0) for (a, b), g in zip(dev, grads)], target, scale, go)
    for n, g, r in zip(sizes, grads, refs):
        err = rel_err(g, 0.37 * scale * r[1])
        print("  n=%d gradient rel_err %.3g" % (n, err))
        assert err < 1e-5


# ---- joined gradients (mg_instnorm_bwd_add / mg_act_bwd_add), pooling edges, sign(0), mg_stats_finalize --------------------------
ACTS = {"none": lambda t: t, "relu": torch.relu, "lrelu": lambda t: F.leaky_relu(t, 0.2), "tanh": torch.tanh}
# (B, C, H, W) -> the generator seed of its inputs.  Chosen on the CPU so that the float64 normalised values keep clear of zero
# (joined_norm_case checks it): a ReLU / LeakyReLU mask decided in float32 is then the float64 one.
JOINED_NORM_SEEDS = {(1, 32, 2, 3): 0, (2, 32, 9, 17): 0, (1, 96, 16, 32): 4, (2, 64, 17, 33): 2, (2, 16, 8, 16): 0,
                     (2, 64, 32, 64): 5, (3, 5, 7, 9): 0}          # smallest |xhat|: 9.6e-4 7.6e-5 1.9e-4 4.8e-5 1.1e-4 2.4e-5 3.2e-3
_joined_cache = {}


def f32_exact(t):
    """float64 values that float32 holds exactly: the device sees the numbers the reference differentiates."""
    return t.float().double()


def joined_norm_inputs(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    x = f32_exact(torch.randn(*shape, generator=gen, dtype=torch.float64) * 3 + 1.5)
    gy = f32_exact(torch.randn(*shape, generator=gen, dtype=torch.float64))
    gy2 = f32_exact(torch.randn(*shape, generator=gen, dtype=torch.float64) * 0.5 + 0.25)
    return x, gy, gy2


def joined_norm_case(shape):
    """Inputs (NCHW float64), the smallest |xhat| of the float64 reference and, per activation, autograd's gradient of
    act(instance_norm(x)) seeded with gy + gy2.  Computed once per shape, shared and never written."""
    if shape not in _joined_cache:
        x, gy, gy2 = joined_norm_inputs(shape, JOINED_NORM_SEEDS[shape])
        want = {}
        for act in ("none", "relu", "lrelu"):
            xr = x.clone().requires_grad_()
            ACTS[act](F.instance_norm(xr, eps=1e-5)).backward(gy + gy2)
            want[act] = nhwc(xr.grad)
        _joined_cache[shape] = (x, gy, gy2, F.instance_norm(x, eps=1e-5).abs().min().item(), want)
    return _joined_cache[shape]


# (route of mg_instnorm_bwd_add, shape, MG_NO_NORM_ROWS, also request dx16)
JOINED_NORM_ROUTES = [
    ("slab_depth4", (1, 32, 2, 3), False, False), ("slab_depth8", (2, 32, 9, 17), False, True),
    ("slab_depth16", (1, 96, 16, 32), False, False), ("slab_depth20", (2, 64, 17, 33), False, False),
    ("rows_hw128", (2, 16, 8, 16), False, True), ("rows_hw2048", (2, 64, 32, 64), False, False),
    ("flat_vector_small", (2, 16, 8, 16), True, False), ("flat_vector_hw2048", (2, 64, 32, 64), True, False),
    ("flat_scalar", (3, 5, 7, 9), False, False)]


@pytest.mark.parametrize("route", JOINED_NORM_ROUTES, ids=lambda r: r[0])
@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
def test_instnorm_bwd_joined_gradient_against_float64(route, act, monkeypatch):
    """ops.instnorm_bwd(..., dy2=gy2) on every route that threads dy2 (slab kernels at the four register depths, the rows kernel,
    the flat vector and scalar kernels, both partial-sum kernels behind the last three) == float64 autograd seeded with gy + gy2:
    a route that dropped dy2, or added it behind the activation mask, misses by O(1).  2e-5 of max|ref| as test_instnorm_fwd_bwd."""
    from mdctgan_amd import ops
    name, shape, no_rows, want16 = route
    code = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU02}[act]
    x, gy, gy2, min_xhat, want = joined_norm_case(shape)
    assert min_xhat > 1e-5, (shape, min_xhat)          # the float32 mask is the float64 mask
    if no_rows:
        monkeypatch.setenv("MG_NO_NORM_ROWS", "1")
    else:
        monkeypatch.delenv("MG_NO_NORM_ROWS", raising=False)
    xd, gyd, gy2d = (nhwc(t).float().to(DEV) for t in (x, gy, gy2))
    _, mean, rstd = ops.instnorm_fwd(xd, code)
    d16 = torch.full((xd.numel(),), float("nan"), dtype=torch.float16, device=DEV) if want16 else None
    dx = ops.instnorm_bwd(gyd, xd, mean, rstd, code, dx16=d16, dy2=gy2d)
    err = rel_err(dx, want[act])
    print("instnorm_bwd dy2 %s %s: rel err %.3g, min|xhat| %.3g" % (name, act, err, min_xhat))
    assert err < 2e-5
    if want16:
        assert torch.equal(d16.view_as(dx), dx.half())
    # the joined call is not the unjoined one (dy2 is far from zero)
    assert rel_err(ops.instnorm_bwd(gyd, xd, mean, rstd, code), want[act]) > 1e-2


def test_instnorm_bwd_refuses_an_unaligned_second_gradient():
    """dy2 is read as float4: a view one element into its buffer is refused (MG_ERR_ARG), nothing is launched or written."""
    from mdctgan_amd import ops
    shape = (2, 32, 9, 17)
    x, gy, gy2, _, _ = joined_norm_case(shape)
    xd, gyd = nhwc(x).float().to(DEV), nhwc(gy).float().to(DEV)
    buf = torch.zeros(xd.numel() + 4, device=DEV)
    off = buf[1:1 + xd.numel()].view(xd.shape)
    off.copy_(nhwc(gy2).float())
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    _, mean, rstd = ops.instnorm_fwd(xd, ops.ACT_RELU)
    out = torch.full_like(xd, 3.25)
    with pytest.raises(ValueError):
        ops.instnorm_bwd(gyd, xd, mean, rstd, ops.ACT_RELU, out=out, dy2=off)
    assert bool((out == 3.25).all())


@pytest.mark.parametrize("n", [1, 255, 1000, 4096 * 256 + 3])          # the last: one element past a full grid, a second trip
@pytest.mark.parametrize("act", ["tanh", "lrelu", "relu"])
def test_act_bwd_joined_gradient_against_float64(n, act):
    """ops.act_bwd(gy, y, act, dy2=gy2) == float64 autograd of act(pre) seeded with gy + gy2 (1e-5 as the unjoined case)."""
    from mdctgan_amd import ops
    code = {"tanh": ops.ACT_TANH, "lrelu": ops.ACT_LRELU02, "relu": ops.ACT_RELU}[act]
    gen = torch.Generator().manual_seed(n % 1000 + len(act))
    pre = f32_exact(torch.randn(n, generator=gen, dtype=torch.float64)).requires_grad_()
    gy = f32_exact(torch.randn(n, generator=gen, dtype=torch.float64))
    gy2 = f32_exact(torch.randn(n, generator=gen, dtype=torch.float64) * 0.5 + 0.25)
    y = ACTS[act](pre)
    y.backward(gy + gy2)
    assert pre.detach().abs().min().item() > 0.0
    yd = y.detach().float().to(DEV)
    got = ops.act_bwd(gy.float().to(DEV), yd, code, dy2=gy2.float().to(DEV))
    err = rel_err(got, pre.grad)
    print("act_bwd dy2 %s n=%d: rel err %.3g" % (act, n, err))
    assert err < 1e-5
    assert rel_err(ops.act_bwd(gy.float().to(DEV), yd, code), pre.grad) > 1e-2 or n == 1


@pytest.mark.parametrize("shape", [(2, 64, 1, 7), (1, 3, 6, 1), (1, 1, 1, 1), (2, 130, 2, 3)])
def test_pool_upsample_edge_shapes(shape):
    """AvgPool2d(3, 2, 1, count_include_pad=False) and nearest 2x upsampling with H == 1 or W == 1 (both clamps of the 3x3 window
    active at once: divisors 1, 2, 4) and at the discriminator pyramid's channel counts, against float64."""
    from mdctgan_amd import ops
    gen = torch.Generator().manual_seed(sum(shape))
    x = f32_exact(torch.randn(*shape, generator=gen, dtype=torch.float64)).requires_grad_()
    y = F.avg_pool2d(x, 3, stride=2, padding=1, count_include_pad=False)
    gy = f32_exact(torch.randn(y.shape, generator=gen, dtype=torch.float64))
    y.backward(gy)
    xd = nhwc(x.detach()).float().to(DEV)
    yd = ops.avgpool_fwd(xd)
    assert yd.shape == nhwc(y).shape and rel_err(yd, nhwc(y.detach())) < 1e-6
    assert rel_err(ops.avgpool_bwd(nhwc(gy).float().to(DEV), xd.shape), nhwc(x.grad)) < 1e-6
    x.grad = None
    u = F.interpolate(x, scale_factor=2.0, mode="nearest")
    gu = f32_exact(torch.randn(u.shape, generator=gen, dtype=torch.float64))
    u.backward(gu)
    ud = ops.upsample_fwd(xd)
    assert ud.shape == nhwc(u).shape and rel_err(ud, nhwc(u.detach())) < 1e-6
    assert rel_err(ops.upsample_bwd(nhwc(gu).float().to(DEV)), nhwc(x.grad)) < 1e-6


def test_sign_of_zero_is_zero_in_dinput_and_l1_backward():
    """d|s|/ds at s == 0 and d|a - b|/da at a == b are exactly 0 (torch's sgn), also for a negative zero."""
    from mdctgan_amd import ops
    gen = torch.Generator().manual_seed(6)
    lr = torch.randn(2, 8, 16, generator=gen, dtype=torch.float64)
    s = f32_exact(torch.randn(2, 8, 16, generator=gen, dtype=torch.float64))
    s.view(-1)[[0, 5, 100, 255]] = 0.0
    s.view(-1)[[7, 254]] = -0.0
    s.requires_grad_()
    out = torch.stack((lr, s, s.abs() * 2 - 1), dim=-1)
    go = f32_exact(torch.randn(out.shape, generator=gen, dtype=torch.float64))
    out.backward(go)
    zero = s.detach() == 0
    assert int(zero.sum()) == 6
    got = ops.dinput_bwd(go.float().to(DEV), s.detach().float().to(DEV)).cpu()
    assert rel_err(got, s.grad) < 1e-6
    assert torch.equal(got[zero], go[..., 1].float()[zero])          # the |s| branch contributes exactly nothing there
    n = 1000
    a = f32_exact(torch.randn(n, generator=gen, dtype=torch.float64))
    b = f32_exact(torch.randn(n, generator=gen, dtype=torch.float64))
    tie = torch.zeros(n, dtype=torch.bool)
    tie[[0, 3, 255, 256, 999]] = True
    b[tie] = a[tie]
    a.requires_grad_()
    (1.3 * F.l1_loss(a, b)).backward()
    go1 = torch.full((1,), 2.0, device=DEV)
    got = ops.l1_bwd(a.detach().float().to(DEV), b.float().to(DEV), 1.3, go1).cpu()
    assert rel_err(got, 2.0 * a.grad) < 1e-6
    assert bool((got[tie] == 0).all()) and bool((got[~tie] != 0).all())


def test_stats_finalize_against_float64():
    """mg_stats_finalize: {sum, sum of squares} -> (s0 / n).float(), ((s1 - s0 * s0 / n) / (n - 1)).clamp_min(0).sqrt().float();
    a slightly negative variance gives 0, a NaN sum stays NaN.  One float32 rounding of the float64 value: 2^-23 relative."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(4)
    v = rng.standard_normal(1000) * 0.3 + 2.0
    three = 3.0
    cases = [((v.sum(), (v * v).sum()), 1000), ((v[:2].sum(), (v[:2] ** 2).sum()), 2),
             ((three, np.nextafter(three, 0.0)), 3),                  # s1 just below s0^2 / n: variance -7e-17
             ((float("nan"), 5.0), 10), ((1.0, float("nan")), 10)]
    for (s0, s1), n in cases:
        st = torch.tensor([s0, s1], dtype=torch.float64)
        want = torch.stack(((st[0] / n).float(), ((st[1] - st[0] * st[0] / n) / (n - 1)).clamp_min(0).sqrt().float())).double()
        out = torch.full((2,), 7.0, device=DEV)
        std = st.to(DEV)
        _lib.check(lib.mg_stats_finalize(_lib.ptr(std), n, _lib.ptr(out), _lib.stream()), "mg_stats_finalize")
        got = out.double().cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (s0, s1, n, got, want)
        ok = ~torch.isnan(want)
        assert bool(((got[ok] - want[ok]).abs() <= 2.0 ** -23 * want[ok].abs()).all()), (s0, s1, n, got, want)
    assert (cases[2][0][1] - three * three / 3) / 2 < 0                      # the clamp really is exercised ...
    st = torch.tensor(cases[2][0], dtype=torch.float64, device=DEV)
    out = torch.full((2,), 7.0, device=DEV)
    _lib.check(lib.mg_stats_finalize(_lib.ptr(st), 3, _lib.ptr(out), _lib.stream()), "mg_stats_finalize")
    assert out[1].item() == 0.0 and out[0].item() == 1.0                      # ... and gives exactly 0
    assert lib.mg_stats_finalize(_lib.ptr(st), 1, _lib.ptr(out), _lib.stream()) == -1          # n - 1 == 0 is refused
