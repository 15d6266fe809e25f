"""Gradients through MDCT4 / IMDCT4 and Audio2MDCT.to_spectro / to_audio (mdctgan_amd/mdct.py CodecGrad; the K1- / K2-shaped
backward kernels of csrc/mdct_ct.h on the fused geometry, the generic composition elsewhere) against the float64 oracle.
The adjoint identities used as references are checked on the CPU in tests/test_codec_grad_host.py.
Bars: raw transforms 4e-6 of max|ref|; codec backward 2e-5 of max|ref| per clip."""
import os

import numpy as np
import pytest
import torch

from oracle import transform as T

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_BAR, CODEC_BAR = 4e-6, 2e-5


def _rel(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def _jac_mdct(t, w, n_fft, hop, center=True):
    X, _ = T.mdct4(np.eye(t, dtype=np.float32), w, n_fft, hop, center)
    return X.reshape(t, -1).T                                   # [F * M, t]


def _jac_imdct(F, w, n_fft, hop, center=True, out_length=None):
    m = n_fft // 2
    y, _ = T.imdct4(np.eye(F * m).reshape(F * m, F, m), w, n_fft, hop, center, out_length)
    return y[:, 0, 0, :].T                                      # [T_out, F * M]


def _imdct_adjoint(gy, w, n_fft, hop, F, center=True):
    """IMDCT4^T: frames of gy with start padding win // 2, window, contract with C, 4/N (tests/test_codec_grad_host.py)."""
    win = len(w)
    gp = np.pad(gy, [(0, 0), (win // 2 if center else 0, (F - 1) * hop + win)])
    frames = gp[:, np.arange(win)[None, :] + hop * np.arange(F)[:, None]] * np.asarray(w, np.float64)
    return 4.0 / n_fft * frames @ T.mdct_matrix(n_fft)[:win]


def _mdct_adjoint(gX, w, n_fft, hop, t, center=True):
    """MDCT4^T: contract with C^T, window, overlap-add, crop the start padding, length t (tests/test_codec_grad_host.py)."""
    win = len(w)
    z = (gX @ T.mdct_matrix(n_fft)[:win].T) * np.asarray(w, np.float64)
    full = np.zeros((z.shape[0], (z.shape[1] - 1) * hop + win + t))
    for f in range(z.shape[1]):
        full[:, f * hop:f * hop + win] += z[:, f]
    start = hop if center else 0
    return full[:, start:start + t]


def _grad(y, x, g):
    (gx,) = torch.autograd.grad(y, x, g)
    return gx


def test_raw_transforms_fused_geometry():
    from mdctgan_amd.mdct import IMDCT4, MDCT4, kbdwin
    w = kbdwin(512)
    wn = w.numpy()
    rng = np.random.default_rng(1)
    mdct, imdct = MDCT4(512, 256, 512, w, device="cuda"), IMDCT4(512, 256, 512, w, device="cuda")
    assert mdct.fused and imdct.fused
    worst = {}
    # large batch against the shortcut identities
    t = 32512
    F = t // 256 + 1
    gy = rng.standard_normal((4, t)).astype(np.float32)
    spec = torch.from_numpy(rng.standard_normal((4, F, 256)).astype(np.float32)).cuda().requires_grad_()
    got = _grad(imdct(spec)[0], spec, torch.from_numpy(gy).cuda()[:, None, None]).cpu().numpy()
    want = 4.0 / 512 * T.mdct4(gy, wn, 512, 256)[0]
    worst["imdct_big"] = _rel(got, want)
    x = torch.from_numpy(rng.standard_normal((4, t)).astype(np.float32)).cuda().requires_grad_()
    gX = rng.standard_normal((4, F, 256)).astype(np.float32)
    got = _grad(mdct(x)[0], x, torch.from_numpy(gX).cuda()).cpu().numpy()
    want = 512 / 4.0 * T.imdct4(gX, wn, 512, 256)[0][:, 0, 0, :t]
    worst["mdct_big"] = _rel(got, want)
    # dense Jacobians at T = 2048
    t = 2048
    F = t // 256 + 1
    gy = rng.standard_normal((2, t)).astype(np.float32)
    spec = torch.from_numpy(rng.standard_normal((2, F, 256)).astype(np.float32)).cuda().requires_grad_()
    got = _grad(imdct(spec)[0], spec, torch.from_numpy(gy).cuda()[:, None, None]).cpu().numpy().reshape(2, -1)
    worst["imdct_jac"] = _rel(got, gy.astype(np.float64) @ _jac_imdct(F, wn, 512, 256))
    x = torch.from_numpy(rng.standard_normal((2, t)).astype(np.float32)).cuda().requires_grad_()
    gX = rng.standard_normal((2, F, 256)).astype(np.float32)
    got = _grad(mdct(x)[0], x, torch.from_numpy(gX).cuda()).cpu().numpy()
    worst["mdct_jac"] = _rel(got, gX.reshape(2, -1).astype(np.float64) @ _jac_mdct(t, wn, 512, 256))
    # out_length 7680 from T = 7936, float64 output, leading batch dimensions
    F = 7936 // 256 + 1
    im2 = IMDCT4(512, 256, 512, w, out_length=7680, device="cuda")
    gy = rng.standard_normal((3, 7680)).astype(np.float32)
    spec = torch.from_numpy(rng.standard_normal((3, F, 256)).astype(np.float32)).cuda().requires_grad_()
    got = _grad(im2(spec)[0], spec, torch.from_numpy(gy).cuda()[:, None, None]).cpu().numpy()
    want = 4.0 / 512 * T.mdct4(np.pad(gy, [(0, 0), (0, 256)]), wn, 512, 256)[0]
    worst["imdct_out_length"] = _rel(got, want)
    im64 = IMDCT4(512, 256, 512, w, device="cuda", dtype=torch.float64)
    g64 = _grad(im64(spec)[0], spec, torch.from_numpy(np.pad(gy, [(0, 0), (0, 256)])).double().cuda()[:, None, None])
    worst["imdct_f64"] = _rel(g64.cpu().numpy(), want)
    x = torch.from_numpy(rng.standard_normal((2, 3, 7936)).astype(np.float32)).cuda().requires_grad_()
    gX = rng.standard_normal((2, 3, F, 256)).astype(np.float32)
    got = _grad(mdct(x)[0], x, torch.from_numpy(gX).cuda()).cpu().numpy()
    want = 512 / 4.0 * T.imdct4(gX.reshape(6, F, 256), wn, 512, 256)[0][:, 0, 0, :7936].reshape(2, 3, 7936)
    worst["mdct_lead_dims"] = _rel(got, want)
    print("worst relative errors (bar %.0e):" % RAW_BAR, worst)
    assert max(worst.values()) <= RAW_BAR, worst


@pytest.mark.parametrize("n_fft,hop,win,center", [(1024, 256, 512, True), (2048, 512, 2048, True), (512, 128, 512, True),
                                                  (1024, 256, 512, False)])
def test_raw_transforms_generic_geometry(n_fft, hop, win, center):
    from mdctgan_amd.mdct import IMDCT4, MDCT4, kbdwin
    w = kbdwin(win)
    wn = w.numpy()
    rng = np.random.default_rng(n_fft + hop + center)
    t = 1536 if n_fft == 2048 else 1024
    mdct = MDCT4(n_fft, hop, win, w, center=center, device="cuda")
    imdct = IMDCT4(n_fft, hop, win, w, center=center, device="cuda")
    assert not mdct.fused and not imdct.fused
    F = T.frame_signal(np.zeros((1, t)), win, hop, center).shape[1]
    x = torch.from_numpy(rng.standard_normal((2, t)).astype(np.float32)).cuda().requires_grad_()
    gX = rng.standard_normal((2, F, n_fft // 2)).astype(np.float32)
    got = _grad(mdct(x)[0], x, torch.from_numpy(gX).cuda()).cpu().numpy()
    # the 2048-point dense Jacobians cost a minute of host time: there the explicit adjoints, which
    # tests/test_codec_grad_host.py checks against the dense Jacobians of the same geometry
    dense = n_fft < 2048
    want = (gX.reshape(2, -1).astype(np.float64) @ _jac_mdct(t, wn, n_fft, hop, center) if dense
            else _mdct_adjoint(gX.astype(np.float64), wn, n_fft, hop, t, center))
    e1 = _rel(got, want)
    spec = torch.from_numpy(rng.standard_normal((2, F, n_fft // 2)).astype(np.float32)).cuda().requires_grad_()
    t_out = imdct(spec.detach())[0].shape[-1]
    gy = rng.standard_normal((2, t_out)).astype(np.float32)
    got = _grad(imdct(spec)[0], spec, torch.from_numpy(gy).cuda()[:, None, None]).cpu().numpy().reshape(2, -1)
    want = (gy.astype(np.float64) @ _jac_imdct(F, wn, n_fft, hop, center) if dense
            else _imdct_adjoint(gy.astype(np.float64), wn, n_fft, hop, F, center).reshape(2, -1))
    e2 = _rel(got, want)
    print("mdct^T %.2e  imdct^T %.2e  (bar %.0e)" % (e1, e2, RAW_BAR))
    assert e1 <= RAW_BAR and e2 <= RAW_BAR


def _pre(raw=False, abs_norm=True, extra=()):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import Audio2MDCT
    flags = list(options.SPECTRAL_FLAGS)
    if raw:
        flags.remove("--arcsinh_transform")
        flags += ["--raw_mdct"]
    if not abs_norm:
        flags.remove("--abs_norm")
    return Audio2MDCT(options.make_opt(*flags, *extra, "--lr_sampling_rate", "12000", "--gpu_ids", "0"))


def _ocodec(pre):
    return dict(arcsinh_transform=bool(pre.arcsinh_transform), raw_mdct=bool(pre.raw_mdct), arcsinh_gain=float(pre.arcsinh_gain),
                norm_range=tuple(float(v) for v in pre.norm_range))


def _speech(B, t, seed):
    rng = np.random.default_rng(seed)
    n = np.arange(t)
    x = 0.05 * rng.standard_normal((B, t)) * (1 + np.sin(2 * np.pi * n / 4000.0)) + 0.1 * np.sin(2 * np.pi * 220 * n / 16000.0)
    return x.astype(np.float32)


def _dxds(s, mn, mx, pre):
    """float64 dX/ds at the normalised values s [B, F, M] with ranges mn / mx [B, 1, 1]."""
    nr0, nr1 = (float(v) for v in pre.norm_range)
    k = (mx - mn) / (nr1 - nr0)
    if not pre.arcsinh_transform:
        return np.broadcast_to(k, s.shape)
    ln10 = np.float64(np.float32(np.log(10.0)))
    return k * ln10 * np.cosh((s * k + mn - nr0 * k) * ln10) / float(pre.arcsinh_gain)


@pytest.mark.parametrize("mode", ["arcsinh", "arcsinh_per_sample", "range"])
def test_to_audio_backward(mode):
    pre = _pre(raw=mode == "range", abs_norm=mode != "arcsinh_per_sample")
    assert pre.fused
    t = 7936
    x = torch.from_numpy(_speech(3, t, 5)).cuda()
    with torch.no_grad():
        s, _, norm = pre.to_spectro(x)
    mn = norm["min"].reshape(-1, 1, 1).double().cpu().numpy()
    mx = norm["max"].reshape(-1, 1, 1).double().cpu().numpy()
    s_leaf = s.detach().clone().requires_grad_()
    gy = np.random.default_rng(6).standard_normal((3, t)).astype(np.float32)
    audio = pre.to_audio(s_leaf, norm)
    got = _grad(audio, s_leaf, torch.from_numpy(gy).cuda()[:, None, None]).cpu().numpy()[:, 0]
    sn = s.cpu().numpy()[:, 0].astype(np.float64)
    want = _dxds(sn, mn, mx, pre) * (4.0 / 512) * T.mdct4(gy, T.kbd_window(512), 512, 256)[0]
    # the expected value itself, by central float64 finite differences of the oracle's to_audio at 16 coordinates
    onorm = {"min": mn[:, :, :, None], "max": mx[:, :, :, None]}
    oc = _ocodec(pre)
    rng = np.random.default_rng(7)
    for _ in range(16):
        b, f, k = rng.integers(3), rng.integers(1, sn.shape[1] - 1), rng.integers(256)
        h = 1e-4
        sp, sm = sn[:, None].copy(), sn[:, None].copy()
        sp[b, 0, f, k] += h
        sm[b, 0, f, k] -= h
        fd = (gy[b].astype(np.float64) @ (T.to_audio(sp, onorm, T.kbd_window(512), 512, 256, **oc)[b, 0, 0]
                                          - T.to_audio(sm, onorm, T.kbd_window(512), 512, 256, **oc)[b, 0, 0])) / (2 * h)
        assert abs(fd - want[b, f, k]) <= 1e-6 * np.abs(want[b]).max() + 1e-9 * abs(fd), (fd, want[b, f, k])
    errs = [_rel(got[b], want[b]) for b in range(3)]
    print("to_audio %s: worst per-clip relative error %.2e (bar %.0e)" % (mode, max(errs), CODEC_BAR))
    assert max(errs) <= CODEC_BAR


@pytest.mark.parametrize("mode", ["arcsinh", "range"])
def test_to_spectro_backward(mode):
    pre = _pre(raw=mode == "range")
    t = 7936
    xn = _speech(3, t, 8)
    x = torch.from_numpy(xn).cuda().requires_grad_()
    s, _, norm = pre.to_spectro(x)
    assert s.requires_grad and not norm["min"].requires_grad and not norm["mean"].requires_grad
    gs = np.random.default_rng(9).standard_normal(tuple(s.shape)).astype(np.float32)
    got = _grad(s, x, torch.from_numpy(gs).cuda()).cpu().numpy()
    mn = np.full((3, 1, 1), float(pre.src_range[0]))
    mx = np.full((3, 1, 1), float(pre.src_range[1]))
    sn = s.detach().cpu().numpy()[:, 0].astype(np.float64)
    want = 512 / 4.0 * T.imdct4(gs[:, 0] / _dxds(sn, mn, mx, pre), T.kbd_window(512), 512, 256)[0][:, 0, 0, :t]
    # central finite differences of the oracle's codec at 16 samples check the expected value (the transform in float64:
    # it is linear, the float32 framing of oracle.mdct4 would swamp a small step)
    oc = dict(_ocodec(pre), abs_norm=True, src_range=tuple(float(v) for v in pre.src_range))
    w64 = T.kbd_window(512).astype(np.float64)
    C = T.mdct_matrix(512)

    def spectro(a):
        return T.normalize((T.frame_signal(a, 512, 256) * w64 @ C)[:, None], **oc)[0][0, 0]
    rng = np.random.default_rng(10)
    for _ in range(16):
        b, i = rng.integers(3), rng.integers(t)
        h = 1e-7
        xp, xm = xn[b:b + 1].astype(np.float64), xn[b:b + 1].astype(np.float64)
        xp[0, i] += h
        xm[0, i] -= h
        fd = np.sum(gs[b, 0] * (spectro(xp) - spectro(xm))) / (2 * h)
        assert abs(fd - want[b, i]) <= 1e-4 * np.abs(want[b]).max(), (fd, want[b, i])
    errs = [_rel(got[b], want[b]) for b in range(3)]
    print("to_spectro %s: worst per-clip relative error %.2e (bar %.0e)" % (mode, max(errs), CODEC_BAR))
    assert max(errs) <= CODEC_BAR
    # mask=True: the masked bins get no gradient, the rest the same
    s2, _, _ = pre.to_spectro(x, mask=True, mask_size=64)
    g2 = _grad(s2, x, torch.from_numpy(gs).cuda()).cpu().numpy()
    gs_m = gs.copy()
    gs_m[..., -64:] = 0
    g3 = _grad(pre.to_spectro(x)[0], x, torch.from_numpy(gs_m).cuda()).cpu().numpy()
    assert np.array_equal(g2, g3)


def test_out_of_scope_cases_raise_at_backward():
    x = torch.from_numpy(_speech(2, 7936, 11)).cuda().requires_grad_()
    s, _, _ = _pre(abs_norm=False).to_spectro(x)
    with pytest.raises(NotImplementedError, match="per-sample"):
        s.sum().backward()
    for extra in (("--src_range", "-160", "40"), ("--explicit_encoding", "--src_range", "-160", "40")):
        from mdctgan_amd import options
        from mdctgan_amd.pix2pixHD_model import Audio2MDCT
        flags = [f for f in options.SPECTRAL_FLAGS if f not in ("--arcsinh_transform",)]
        i = flags.index("--src_range")
        flags = flags[:i] + flags[i + 3:]
        pre = Audio2MDCT(options.make_opt(*flags, *extra, "--lr_sampling_rate", "12000", "--gpu_ids", "0"))
        assert pre.codec in (3, 4)
        s, pha, norm = pre.to_spectro(x)
        with pytest.raises(NotImplementedError, match="dB"):
            s.sum().backward()
        leaf = s.detach().requires_grad_()
        with pytest.raises(NotImplementedError, match="dB"):
            pre.to_audio(leaf, norm, pha).sum().backward()
    pre = _pre()
    with torch.no_grad():
        s, _, norm = pre.to_spectro(x)
    norm = dict(norm, min=norm["min"].clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="norm_param"):
        pre.to_audio(s, norm).sum().backward()


def test_forward_unchanged():
    from mdctgan_amd import _lib
    from mdctgan_amd.mdct import IMDCT4, MDCT4, kbdwin
    lib = _lib.load()
    pre = _pre()
    x = torch.from_numpy(_speech(2, 7936, 12)).cuda()
    with torch.no_grad():
        s0, _, n0 = pre.to_spectro(x)
        k0 = lib.mg_mdct_last_kernel(0)
        a0 = pre.to_audio(s0, n0)
        k1 = lib.mg_mdct_last_kernel(1)
    xg = x.clone().requires_grad_()
    s1, _, n1 = pre.to_spectro(xg)
    assert s1.grad_fn is not None and torch.equal(s1, s0) and not n1["mean"].requires_grad
    s1.sum().backward()
    assert lib.mg_mdct_last_kernel(0) == k0
    sg = s0.clone().requires_grad_()
    a1 = pre.to_audio(sg, n0)
    assert a1.grad_fn is not None and torch.equal(a1, a0)
    a1.sum().backward()
    assert lib.mg_mdct_last_kernel(1) == k1
    s2, _, _ = pre.to_spectro(x)
    assert s2.grad_fn is None and not s2.requires_grad
    with torch.no_grad():
        assert pre.to_audio(sg, n0).grad_fn is None and pre.to_spectro(xg)[0].grad_fn is None
    w = kbdwin(512)
    m, im = MDCT4(512, 256, 512, w, device="cuda"), IMDCT4(512, 256, 512, w, device="cuda")
    X0, _ = m(x)
    X1, _ = m(xg)
    assert X0.grad_fn is None and X1.grad_fn is not None and torch.equal(X0, X1)
    y0, _ = im(X0)
    y1, _ = im(X0.clone().requires_grad_())
    assert y0.grad_fn is None and y1.grad_fn is not None and torch.equal(y0, y1)


def _toy_model():
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    from oracle import nets as onets
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                           "--n_blocks_global", "2", "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8",
                           "--batchSize", "2", "--bins", "32", "--segment_length", "7936", "--gpu_ids", "0")
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    return model


def test_waveform_loss_reaches_the_generator():
    model = _toy_model()
    g = np.load(os.path.join(REPO, "tests", "golden", "g6_step_global.npz"))
    lr, hr = torch.from_numpy(g["lr"]).cuda(), torch.from_numpy(g["hr"]).cuda()
    params = [p for p in model.netG.parameters() if p.requires_grad]

    def grads(two_stage):
        # the weight-gradient kernels write p.grad themselves (mdctgan_amd/functional.py grad_buffer): start each pass fresh
        for p in params:
            p.grad = None
        sr_spectro, _, _, _, _, _, _, lr_norm = model.forward(lr, hr)
        if two_stage:
            leaf = sr_spectro.detach().requires_grad_()
            loss = (model.preprocess.to_audio(leaf, lr_norm)[:, 0, 0] - hr.reshape(hr.shape[0], -1)).abs().mean()
            (gs,) = torch.autograd.grad(loss, leaf)
            sr_spectro.backward(gs)
        else:
            loss = (model.preprocess.to_audio(sr_spectro, lr_norm)[:, 0, 0] - hr.reshape(hr.shape[0], -1)).abs().mean()
            loss.backward()
        return [Fh.grad_of(p).clone() for p in params]
    from mdctgan_amd import functional as Fh
    one, two = grads(False), grads(True)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    assert all(torch.isfinite(a).all() for a in one) and any(a.abs().max() > 0 for a in one)


def test_backward_is_deterministic_and_capturable():
    pre = _pre()
    x = torch.from_numpy(_speech(4, 7936, 13)).cuda()
    with torch.no_grad():
        s, _, norm = pre.to_spectro(x)
    gy = torch.from_numpy(np.random.default_rng(14).standard_normal((4, 1, 1, 7936)).astype(np.float32)).cuda()
    leaf = s.detach().clone().requires_grad_()
    g1 = _grad(pre.to_audio(leaf, norm), leaf, gy)
    g2 = _grad(pre.to_audio(leaf, norm), leaf, gy)
    assert torch.equal(g1, g2)
    xg = x.clone().requires_grad_()
    gs = torch.randn(s.shape, device="cuda")
    assert torch.equal(_grad(pre.to_spectro(xg)[0], xg, gs), _grad(pre.to_spectro(xg)[0], xg, gs))
    # single-stream capture of the to_audio forward + backward
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _grad(pre.to_audio(leaf, norm), leaf, gy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pre.to_audio(leaf, norm)
        gout = _grad(out, leaf, gy)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gout, g1) and torch.equal(out, pre.to_audio(s, norm))
