"""K1' / K2' (csrc/mdct_pow2.hip): the fused MDCT / IMDCT codec kernels of the power-of-two geometries other than 512
(n_fft 256 / 1024 / 2048, hop = n_fft / 2) against the float64 oracle, against the generic composition (MG_MDCT_POW2=0, the
route these geometries took before) and against themselves (stitched == decode + stitch, run-to-run bits, graph replay).
Bars are the project's: raw coefficients 3e-6 of max|X|, waveforms 3e-6 of max|y| + 1e-7, arcsinh spectrogram 5e-4 absolute,
round trip 1e-5 of max|x|, gradients 4e-6 (raw) / 2e-5 (codec) of max|ref| (tests/test_codec_generic.py, test_codec_grad_gpu.py)."""
import numpy as np
import pytest
import torch

from oracle import transform as T

pytestmark = pytest.mark.gpu

GEOMS = [(256, 128), (1024, 512), (2048, 1024)]
RAW_BAR, CODEC_BAR = 4e-6, 2e-5


def _lib():
    from mdctgan_amd import _lib as L
    return L.load()


def _kernel(which):
    return _lib().mg_mdct_last_kernel(which).decode()


def _pre(n_fft, hop, mode="arcsinh", abs_norm=True):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import Audio2MDCT
    flags = list(options.SPECTRAL_FLAGS)
    if mode == "range":
        flags.remove("--arcsinh_transform")
        flags += ["--raw_mdct"]
    elif mode == "db":
        flags.remove("--arcsinh_transform")
        i = flags.index("--src_range")
        flags = flags[:i] + flags[i + 3:] + ["--src_range", "-160", "40"]
    if not abs_norm:
        flags.remove("--abs_norm")
    return Audio2MDCT(options.make_opt(*flags, "--n_fft", n_fft, "--hop_length", hop, "--win_length", n_fft,
                                       "--lr_sampling_rate", "12000", "--gpu_ids", "0"))


def _ocodec(mode, abs_norm=True):
    oc = dict(norm_range=(-1.0, 1.0), abs_norm=abs_norm, src_range=(-5.0, 5.0))
    if mode == "arcsinh":
        oc.update(arcsinh_transform=True, arcsinh_gain=1000.0)
    elif mode == "range":
        oc.update(arcsinh_transform=False, raw_mdct=True)
    else:
        oc.update(arcsinh_transform=False, raw_mdct=False, src_range=(-160.0, 40.0))
    return oc


def _speech(B, t, seed):
    rng = np.random.default_rng(seed)
    n = np.arange(t)
    x = 0.05 * rng.standard_normal((B, t)) * (1 + np.sin(2 * np.pi * n / 4000.0)) + 0.1 * np.sin(2 * np.pi * 220 * n / 16000.0)
    return x.astype(np.float32)


def _rel(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------------
# 1. raw transforms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", GEOMS)
def test_raw_transforms_against_oracle(n_fft, hop, monkeypatch):
    from mdctgan_amd.mdct import IMDCT4, MDCT4, kbdwin
    w = kbdwin(n_fft)
    wn = w.numpy()
    m, im = MDCT4(n_fft, hop, n_fft, w, device="cuda"), IMDCT4(n_fft, hop, n_fft, w, device="cuda")
    assert not m.fused and not im.fused and m.fast and im.fast
    rng = np.random.default_rng(n_fft)
    for t, one_d in ((6 * n_fft + 3 * hop, False), (6 * n_fft + 37, False), (6 * n_fft + 37, True)):
        x = rng.standard_normal(t if one_d else (3, t)).astype(np.float32)
        X, _ = m(torch.from_numpy(x).cuda())
        assert "pow2" in _kernel(0), _kernel(0)
        want, _ = T.mdct4(x, wn, n_fft, hop)
        assert X.shape == want.shape and X.shape[-2] == _lib().mg_mdct4_num_frames(t, n_fft) == -(-t // hop) + 1
        e1 = _rel(X.cpu().numpy(), want)
        X3 = X.reshape(-1, *X.shape[-2:])
        y, _ = im(X3)
        assert "pow2" in _kernel(1), _kernel(1)
        wy, _ = T.imdct4(X3.cpu().numpy(), wn, n_fft, hop)
        assert y.shape == wy.shape and y.shape[-1] == (X.shape[-2] - 1) * hop >= t
        e2 = np.abs(y.cpu().numpy() - wy).max()
        x2 = x.reshape(-1, t)
        e3 = np.abs(y.cpu().numpy()[:, 0, 0, hop:t - hop] - x2[:, hop:t - hop]).max() / np.abs(x2).max()
        print("n_fft %d T %d: mdct %.2e of max|X|, imdct %.2e (max|y| %.2f), round trip %.2e" % (n_fft, t, e1, e2, np.abs(wy).max(), e3))
        assert e1 <= 3e-6
        assert e2 <= 3e-6 * np.abs(wy).max() + 1e-7
        assert e3 <= 1e-5
        # out_length crops inside the store
        y2, _ = IMDCT4(n_fft, hop, n_fft, w, device="cuda", out_length=t - 5)(X3)
        assert torch.equal(y2, y[..., :t - 5])
        # the switch restores the composition and its kernels' names
        monkeypatch.setenv("MG_MDCT_POW2", "0")
        assert not m.fast and not im.fast
        before = (_kernel(0), _kernel(1))
        Xc, _ = m(torch.from_numpy(x).cuda())
        yc, _ = im(X3)
        monkeypatch.delenv("MG_MDCT_POW2")
        assert _rel(Xc.cpu().numpy(), want) <= 3e-6 and np.abs(yc.cpu().numpy() - wy).max() <= 3e-6 * np.abs(wy).max() + 1e-7
        assert (_kernel(0), _kernel(1)) == before                       # the composition names what it named before: nothing new


def test_guarded_requests_do_not_reach_the_fused_kernels(monkeypatch):
    """Analysis frames and a float64 waveform are requests K1' / K2' do not serve (mdct.Transform.route_analysis / route_synthesis):
    they take the generic composition, which leaves mg_mdct_last_kernel alone -- after a 512 call it still names the 512 kernels --
    and give the bits of the same calls under MG_MDCT_POW2=0.  n_fft 256, B = 2, T = 1024: more than one tile row per clip."""
    from mdctgan_amd.mdct import IMDCT4, MDCT4, kbdwin
    rng = np.random.default_rng(256)
    w5 = kbdwin(512)
    X5, _ = MDCT4(512, 256, 512, w5, device="cuda")(torch.from_numpy(rng.standard_normal((2, 2048)).astype(np.float32)).cuda())
    IMDCT4(512, 256, 512, w5, device="cuda")(X5)
    names = (_kernel(0), _kernel(1))
    assert names[0].startswith("mdct4_") and names[1].startswith("imdct4_") and "pow2" not in names[0] + names[1], names
    w = kbdwin(256)
    m, im = MDCT4(256, 128, 256, w, device="cuda"), IMDCT4(256, 128, 256, w, device="cuda", dtype=torch.float64)
    assert m.fast and im.fast
    x = torch.from_numpy(rng.standard_normal((2, 1024)).astype(np.float32)).cuda()
    spec = torch.from_numpy(rng.standard_normal((2, 9, 128)).astype(np.float32)).cuda()

    def run():
        (X, frames), (y, _) = m(x, return_frames=True), im(spec)
        return X, frames, y
    got = run()
    assert (_kernel(0), _kernel(1)) == names
    assert got[0].shape == (2, 9, 128) and got[1].shape == (2, 9, 256) and got[2].shape == (2, 1, 1, 1024) and got[2].dtype == torch.float64
    monkeypatch.setenv("MG_MDCT_POW2", "0")
    assert not m.fast and not im.fast
    want = run()
    monkeypatch.delenv("MG_MDCT_POW2")
    for g, w_ in zip(got, want):
        assert torch.equal(g, w_)
    m(x)                                                                # (and the plain request does reach K1')
    assert "pow2" in _kernel(0), _kernel(0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. codec paths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["arcsinh", "range"])
@pytest.mark.parametrize("n_fft,hop", GEOMS)
def test_codec_paths_against_oracle(n_fft, hop, mode, monkeypatch):
    pre = _pre(n_fft, hop, mode)
    assert not pre.fused and pre.fast and pre.has_stitched_decoder
    t = 6 * n_fft + 3 * hop
    x = _speech(3, t, n_fft + 1)
    xd = torch.from_numpy(x).cuda()
    w = T.kbd_window(n_fft)
    oc = _ocodec(mode)
    ws, wnorm = T.to_spectro(x, w, n_fft, hop, **oc)
    s, _, norm = pre.to_spectro(xd)
    assert "pow2" in _kernel(0)
    monkeypatch.setenv("MG_MDCT_POW2", "0")
    sc, _, normc = pre.to_spectro(xd)
    monkeypatch.delenv("MG_MDCT_POW2")
    e_new, e_comp = np.abs(s.cpu().numpy() - ws).max(), np.abs(sc.cpu().numpy() - ws).max()
    print("%s n_fft %d: spectrogram error new %.3e, composition %.3e" % (mode, n_fft, e_new, e_comp))
    assert tuple(s.shape) == ws.shape
    assert e_new <= 5e-4
    assert e_new <= 3 * e_comp + 1e-6
    np.testing.assert_allclose(float(norm["mean"]), float(wnorm["mean"]), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(norm["std"]), float(wnorm["std"]), rtol=1e-4)
    # the generator's input pair (K1' in RAW mode + mg_codec_forward)
    r = pre.encode(xd, want_pair=True)
    pair = r["pair"]
    assert torch.equal(pair[..., 0], r["spec"]) and torch.equal(pair[..., 1], pair[..., 0].abs() * 2 + float(pre.norm_range[0]))
    assert np.abs(r["spec"].cpu().numpy() - ws[:, 0]).max() <= 5e-4
    # decoder on the oracle's spectrogram
    nparam = {k: (torch.from_numpy(np.asarray(v)).cuda() if k in ("min", "max") else v) for k, v in wnorm.items()}
    back = pre.to_audio(torch.from_numpy(ws).cuda(), nparam, None)
    assert "pow2" in _kernel(1)
    wback = T.to_audio(ws.astype(np.float64), wnorm, w, n_fft, hop, pha=None, **oc)
    assert back.shape == wback.shape
    e = np.abs(back.cpu().numpy() - wback).max()
    print("%s n_fft %d: decode error %.3e (max|y| %.3f)" % (mode, n_fft, e, np.abs(wback).max()))
    assert e <= 1e-5 * max(np.abs(wback).max(), 1e-3)


@pytest.mark.parametrize("n_fft,hop", GEOMS)
def test_per_clip_range_decode(n_fft, hop):
    """No --abs_norm: per-sample min / max -- K1' in RAW mode around mg_codec_forward, K2' with the per-clip constants."""
    pre = _pre(n_fft, hop, "arcsinh", abs_norm=False)
    t = 6 * n_fft + 3 * hop
    x = (np.array([[1.0], [4.0], [0.2]]) * _speech(3, t, n_fft + 2)).astype(np.float32)
    w = T.kbd_window(n_fft)
    oc = _ocodec("arcsinh", abs_norm=False)
    ws, wnorm = T.to_spectro(x, w, n_fft, hop, **oc)
    s, _, norm = pre.to_spectro(torch.from_numpy(x).cuda())
    assert "pow2" in _kernel(0)
    assert np.abs(s.cpu().numpy() - ws).max() <= 5e-4
    np.testing.assert_allclose(norm["min"].cpu().numpy().reshape(-1), wnorm["min"].reshape(-1), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(norm["max"].cpu().numpy().reshape(-1), wnorm["max"].reshape(-1), rtol=1e-5, atol=1e-5)
    nparam = {k: (torch.from_numpy(np.asarray(v)).cuda() if k in ("min", "max") else v) for k, v in wnorm.items()}
    back = pre.to_audio(torch.from_numpy(ws).cuda(), nparam, None)
    assert "pow2" in _kernel(1)
    wback = T.to_audio(ws.astype(np.float64), wnorm, w, n_fft, hop, pha=None, **oc)
    assert np.abs(back.cpu().numpy() - wback).max() <= 1e-5 * max(np.abs(wback).max(), 1e-3)


def test_db_codec_takes_the_raw_mode_route():
    """dB codec at n_fft 2048: K1' / K2' in RAW mode around mg_codec_forward / mg_codec_inverse, at the dB bars of
    tests/test_codec_generic.py (strong bins 3e-4 of the range, decoded coefficients 2e-5 of max|X|, waveform 1e-5)."""
    n_fft, hop = 2048, 1024
    pre = _pre(n_fft, hop, "db")
    assert pre.codec == 3 and pre.fast and not pre.has_stitched_decoder
    x = (0.05 * np.random.default_rng(11).standard_normal((2, 15 * hop))).astype(np.float32)
    w = T.kbd_window(n_fft)
    oc = _ocodec("db")
    s, pha, norm = pre.to_spectro(torch.from_numpy(x).cuda())
    assert "pow2" in _kernel(0)
    ws, wnorm = T.to_spectro(x, w, n_fft, hop, **oc)
    X, _ = T.mdct4(x, w, n_fft, hop)
    got = s.cpu().numpy()
    strong = (np.abs(X) >= 1e-3 * np.abs(X).max())[:, None]
    assert np.abs(got - ws)[strong].max() <= 3e-4
    dec = T.denormalize(got.astype(np.float64), wnorm["min"], wnorm["max"], arcsinh_transform=False, raw_mdct=False,
                        norm_range=(-1.0, 1.0))[:, 0] * np.sign(X)
    assert np.abs(dec - X).max() <= 2e-5 * np.abs(X).max()
    nparam = {k: (torch.from_numpy(np.asarray(v)).cuda() if k in ("min", "max") else v) for k, v in wnorm.items()}
    pre.up_ratio = 1
    back = pre.to_audio(torch.from_numpy(ws).cuda(), nparam, torch.sign(torch.from_numpy(X.astype(np.float32)))[:, None].cuda())
    assert "pow2" in _kernel(1)
    wback = T.to_audio(ws.astype(np.float64), wnorm, w, n_fft, hop, pha=None, **oc)
    assert np.abs(back.cpu().numpy() - wback).max() <= 1e-5 * max(np.abs(wback).max(), 1e-3)


# ---------------------------------------------------------------------------------------------------------------------
# 3. stitched decode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen_overlap", [0, 256])
def test_stitched_decode_equals_decode_then_stitch(gen_overlap, monkeypatch):
    from mdctgan_amd import mdct, ops
    n_fft, hop, L, n_seg = 1024, 512, 7168, 5
    pre = _pre(n_fft, hop)
    x = _speech(n_seg, L, 21)
    w = T.kbd_window(n_fft)
    with torch.no_grad():
        s, _, norm = pre.to_spectro(torch.from_numpy(x).cuda())
    total = _lib().mg_stitch_length(n_seg, L, gen_overlap)
    out = torch.full((total,), float("nan"), device="cuda")
    for i in range(0, n_seg, 2):
        got = pre.to_audio(s[i:i + 2], norm, stitch=(out, gen_overlap, i, L))
        assert got is out
    assert "stitched" in _kernel(1) and "pow2" in _kernel(1), _kernel(1)
    audio = pre.to_audio(s, norm)
    want = ops.stitch_segments(audio, L, gen_overlap)
    assert out.shape == want.reshape(-1).shape
    assert torch.equal(out, want.reshape(-1)), (out - want.reshape(-1)).abs().max().item()
    # batches in reverse order into a waveform the caller cleared
    out2 = torch.zeros(total, device="cuda")
    nr, sr = pre._ranges()
    for i in (4, 2, 0):
        mdct.imdct4_pow2(s[i:i + 2, 0], pre.window, n_fft, codec=pre.codec, gain=float(pre.arcsinh_gain), norm_range=nr, src_range=sr,
                         stitch=(out2, gen_overlap, i, L, 0))
    assert torch.equal(out2, out)
    oc = _ocodec("arcsinh")
    onorm = {"min": np.array([-5.0], np.float32)[None, None, None], "max": np.array([5.0], np.float32)[None, None, None]}
    oa = T.to_audio(s.cpu().numpy().astype(np.float64), onorm, w, n_fft, hop, **oc)
    ow = T.stitch_segments(oa, L, gen_overlap).reshape(-1)
    e = np.abs(out.cpu().numpy() - ow).max()
    print("stitched, overlap %d: %.2e against the oracle (max|y| %.3f)" % (gen_overlap, e, np.abs(ow).max()))
    assert e <= 3e-6 * np.abs(ow).max() + 1e-7
    # the switch restores today's behaviour
    monkeypatch.setenv("MG_MDCT_POW2", "0")
    with pytest.raises(NotImplementedError):
        pre.to_audio(s[:2], norm, stitch=(out, gen_overlap, 0, L))


# ---------------------------------------------------------------------------------------------------------------------
# 4. gradients
# ---------------------------------------------------------------------------------------------------------------------
def _dxds(s, mn, mx, pre):
    nr0, nr1 = (float(v) for v in pre.norm_range)
    k = (mx - mn) / (nr1 - nr0)
    ln10 = np.float64(np.float32(np.log(10.0)))
    return k * ln10 * np.cosh((s * k + mn - nr0 * k) * ln10) / float(pre.arcsinh_gain)


def _grad(y, x, g):
    (gx,) = torch.autograd.grad(y, x, g)
    return gx


@pytest.mark.parametrize("n_fft,hop", GEOMS[1:])
def test_codec_gradients(n_fft, hop, monkeypatch):
    pre = _pre(n_fft, hop)
    w = T.kbd_window(n_fft)
    t = 15 * hop
    xn = _speech(3, t, n_fft + 5)
    x = torch.from_numpy(xn).cuda()
    with torch.no_grad():
        s, _, norm = pre.to_spectro(x)
    mn, mx = np.full((3, 1, 1), -5.0), np.full((3, 1, 1), 5.0)
    sn = s.cpu().numpy()[:, 0].astype(np.float64)
    # to_audio
    gy = np.random.default_rng(6).standard_normal((3, t)).astype(np.float32)
    want = _dxds(sn, mn, mx, pre) * (4.0 / n_fft) * T.mdct4(gy, w, n_fft, hop)[0]

    def to_audio_grad():
        leaf = s.detach().clone().requires_grad_()
        return _grad(pre.to_audio(leaf, norm), leaf, torch.from_numpy(gy).cuda()[:, None, None]).cpu().numpy()[:, 0]
    got = to_audio_grad()
    monkeypatch.setenv("MG_MDCT_POW2", "0")
    comp = to_audio_grad()
    monkeypatch.delenv("MG_MDCT_POW2")
    errs = [max(_rel(got[b], want[b]), _rel(got[b], comp[b])) for b in range(3)]
    print("to_audio backward n_fft %d: worst per-clip error %.2e (oracle / composition; bar %.0e)" % (n_fft, max(errs), CODEC_BAR))
    assert max(errs) <= CODEC_BAR
    # to_spectro
    gs = np.random.default_rng(9).standard_normal(tuple(s.shape)).astype(np.float32)
    want = n_fft / 4.0 * T.imdct4(gs[:, 0] / _dxds(sn, mn, mx, pre), w, n_fft, hop)[0][:, 0, 0, :t]

    def to_spectro_grad():
        xg = x.clone().requires_grad_()
        sg = pre.to_spectro(xg)[0]
        return _grad(sg, xg, torch.from_numpy(gs).cuda()).cpu().numpy(), sg.detach()
    got, s_new = to_spectro_grad()
    assert torch.equal(s_new, s)
    # The composition at the SAME linearisation point: ds/dX is evaluated at the forward's stored spectrogram, and the two
    # routes' forwards differ by their transform rounding (up to 1e-4 of the arcsinh range in empty bins, where ds/dX is
    # steepest) -- an autograd run of each route would compare two linearisation points, not two backward passes.
    monkeypatch.setenv("MG_MDCT_POW2", "0")
    comp = pre._to_spectro_backward(torch.from_numpy(gs).cuda(), x, s).cpu().numpy()
    own, s_comp = to_spectro_grad()                    # ... and the composition end to end against the oracle at its own point
    monkeypatch.delenv("MG_MDCT_POW2")
    sc = s_comp.cpu().numpy()[:, 0].astype(np.float64)
    want_c = n_fft / 4.0 * T.imdct4(gs[:, 0] / _dxds(sc, mn, mx, pre), w, n_fft, hop)[0][:, 0, 0, :t]
    e_o, e_c, e_own = (max(_rel(a[b], r[b]) for b in range(3)) for a, r in ((got, want), (got, comp), (own, want_c)))
    print("to_spectro backward n_fft %d: %.2e against the oracle, %.2e against the composition at the same point, the "
          "composition end to end %.2e (bar %.0e)" % (n_fft, e_o, e_c, e_own, CODEC_BAR))
    assert max(e_o, e_c, e_own) <= CODEC_BAR
    # the raw modules, ragged length
    from mdctgan_amd.mdct import IMDCT4, MDCT4, kbdwin
    wk = kbdwin(n_fft)
    m, im = MDCT4(n_fft, hop, n_fft, wk, device="cuda"), IMDCT4(n_fft, hop, n_fft, wk, device="cuda")
    t2 = 6 * n_fft + 37
    F = -(-t2 // hop) + 1
    rng = np.random.default_rng(n_fft + 7)
    xr = torch.from_numpy(rng.standard_normal((2, t2)).astype(np.float32)).cuda().requires_grad_()
    gX = rng.standard_normal((2, F, hop)).astype(np.float32)
    got = _grad(m(xr)[0], xr, torch.from_numpy(gX).cuda()).cpu().numpy()
    e1 = _rel(got, n_fft / 4.0 * T.imdct4(gX, w, n_fft, hop)[0][:, 0, 0, :t2])
    spec = torch.from_numpy(rng.standard_normal((2, F, hop)).astype(np.float32)).cuda().requires_grad_()
    gy2 = rng.standard_normal((2, (F - 1) * hop)).astype(np.float32)
    got = _grad(im(spec)[0], spec, torch.from_numpy(gy2).cuda()[:, None, None]).cpu().numpy()
    e2 = _rel(got, 4.0 / n_fft * T.mdct4(gy2, w, n_fft, hop)[0][:, :F])
    print("raw backward n_fft %d: mdct^T %.2e  imdct^T %.2e (bar %.0e)" % (n_fft, e1, e2, RAW_BAR))
    assert e1 <= RAW_BAR and e2 <= RAW_BAR


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism and capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", GEOMS)
def test_determinism_and_graph_replay(n_fft, hop):
    pre = _pre(n_fft, hop)
    L = 14 * hop
    x = torch.from_numpy(_speech(5, L, n_fft + 9)).cuda()
    x2 = torch.from_numpy(_speech(5, L, n_fft + 10)).cuda()

    def run(a):
        r = pre.encode(a)
        y = pre.to_audio(r["spec4"], pre._norm_param(r, a.device))
        out = torch.zeros(_lib().mg_stitch_length(5, L, 2 * hop // 4), device="cuda")
        pre.to_audio(r["spec4"], pre._norm_param(r, a.device), stitch=(out, 2 * hop // 4, 0, L))
        return r["spec"], r["stats"], y, out
    with torch.no_grad():
        a, b = run(x), run(x)
        for i in (0, 2, 3):
            assert torch.equal(a[i], b[i])
        np.testing.assert_allclose(a[1].cpu().numpy(), b[1].cpu().numpy(), rtol=1e-12)
        want = run(x2)
        static = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = run(static)
        static.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        for i in (0, 2, 3):
            assert torch.equal(cap[i], want[i])
        np.testing.assert_allclose(cap[1].cpu().numpy(), want[1].cpu().numpy(), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# 6. whole path, toy model
# ---------------------------------------------------------------------------------------------------------------------
def _toy_model(n_fft, hop, seg):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    from oracle import nets as onets
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                           "--n_blocks_global", "2", "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8",
                           "--batchSize", "2", "--bins", "32", "--segment_length", seg, "--n_fft", n_fft, "--hop_length", hop,
                           "--win_length", n_fft, "--gpu_ids", "0")
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    onets.fill_deterministic(model.netD)
    return model


def test_generate_and_train_step_on_a_toy_model(monkeypatch):
    from mdctgan_amd.generate_audio import generate, make_graphed_generate, segment_audio
    n_fft, hop, seg, ov = 1024, 512, 15872, 128
    model = _toy_model(n_fft, hop, seg)
    assert model.preprocess.fast and model.preprocess.has_stitched_decoder
    gen = torch.Generator().manual_seed(3)
    wave = 0.05 * torch.randn(4 * seg + 123, generator=gen)
    segs = segment_audio(wave.cuda(), seg, ov)
    assert segs.shape == (5, seg)
    got = generate(model, segs, batch_size=2, gen_overlap=ov)
    assert "stitched" in _kernel(1) and "pow2" in _kernel(1), _kernel(1)
    assert "pow2" in _kernel(0)
    run = make_graphed_generate(model, segs, batch_size=2, gen_overlap=ov)
    assert torch.equal(run(segs).view(1, -1), got)
    # wiring check against the composition: its own response to a 3e-6 max|x| input perturbation is the yardstick
    monkeypatch.setenv("MG_MDCT_POW2", "0")
    comp = generate(model, segs, batch_size=2, gen_overlap=ov)
    noise = torch.randn(segs.shape, generator=torch.Generator().manual_seed(4)).cuda() * (3e-6 * segs.abs().max())
    comp_n = generate(model, segs + noise, batch_size=2, gen_overlap=ov)
    monkeypatch.delenv("MG_MDCT_POW2")
    yard = (comp_n - comp).abs().max().item()
    diff = (got - comp).abs().max().item()
    print("toy generate: |new - composition| %.3e, composition's response to 3e-6 input noise %.3e, max|y| %.3f"
          % (diff, yard, comp.abs().max().item()))
    assert got.shape == comp.shape
    assert diff <= 3 * yard
    # one training step on both routes
    lr = segs[:2].contiguous()
    hr = (segs[:2] + 0.01 * torch.randn(2, seg, generator=torch.Generator().manual_seed(5)).cuda()).contiguous()
    for off in (False, True):
        if off:
            monkeypatch.setenv("MG_MDCT_POW2", "0")
        ld = model.optimize_parameters(lr, hr)
        assert all(np.isfinite(v.item()) for v in ld.values()), ld
