"""The multi-scale mel-spectrogram L1 loss on the device (csrc/mel_loss_rows.hip; metrics.mel_many / mel_loss / mel_loss_term;
--lambda_mel in the step): the gradient per element against float64 autograd of the definition, the forward, the exact zeros,
pack invariance and containment, odd filterbanks, determinism and capture, the chain through Audio2MDCT.to_audio, and the step.

The gradient's bar has the project's form: per utterance e = max|got - g64| / max|g64| <= 4 e32, e32 the largest error of float32
CPU autograd (torch.stft) of the same expression among the utterances of the same launch, AND e <= CEILING = 1e-4, which does not
depend on the host.  Where the ceiling comes from, as in tests/test_mrstft_loss_gpu.py: the kernels' decisions (the two clamps and
the sign) are float64's, because the forward transform runs in double and the filterbank contraction, the logarithms and dL/dm are
formed in double -- the contraction adds no float32 rounding.  What is left is float32 rounding in the backward: H_k rounded once,
at most 11 butterfly stages of the inverse, the window product: 13 roundings of 2^-24 relative to the largest element of a frame,
summed over at most 12 taps per sample (4 overlapping frames, 3 positions) and 3 resolutions: 13 * 12 * 3 * 2^-24 = 2.8e-5 in the
worst case with every error aligned, rounded up to 1e-4.  The definition, the references, the inputs and the proof that the bars
have teeth live in tests/test_mel_loss_host.py, which also asserts that these inputs are tie-free."""
import functools
import os

import numpy as np
import pytest
import torch

import test_mel_loss_host as T
from test_lsd_loss_gpu import written_only_inside
from test_metrics_many_gpu import GUARD, pack
from test_mrstft_loss_gpu import capture, count_to_audio, device_tables, packed_case

H = T.H
pytestmark = pytest.mark.gpu
REPO = T.REPO
UNWRITTEN = -7.0
LAMBDA = 0.5
RATE = T.RATE
CEILING = T.CEILING              # per utterance, beside the 4 e32 bar: see the module's head


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points on packed numpy buffers, every output inside guard-filled arrays
# ---------------------------------------------------------------------------------------------------------------------
def bank_tensors(W):
    from mdctgan_amd.metrics import mel_band_tables
    band_k, band_j = mel_band_tables(W)
    return torch.from_numpy(W).cuda().contiguous(), torch.from_numpy(band_k).cuda(), torch.from_numpy(band_j).cuda()


def mel_forward(hr_buf, sr_buf, table, frames, n_fft, hop, W):
    """mg_mel_loss_rows -> row_out float64 [rows, 4] = {sum, 0, 0, loss} (device)"""
    from mdctgan_amd import _lib
    lib = _lib.load()
    rows, fsd, total = device_tables(table, frames)
    U = len(table)
    hd, sd, wd = torch.from_numpy(hr_buf).cuda(), torch.from_numpy(sr_buf).cuda(), torch.from_numpy(T.S.hann32(n_fft)).cuda()
    Wd, bk, bj = bank_tensors(W)
    nbytes = lib.mg_mel_loss_rows_workspace(total)
    assert nbytes == total * 8
    ws = torch.full((nbytes // 8 + 4,), GUARD, dtype=torch.float64, device="cuda")
    out = torch.full((U * 4 + 4,), UNWRITTEN, dtype=torch.float64, device="cuda")
    _lib.check(lib.mg_mel_loss_rows(_lib.ptr(hd), hd.numel(), _lib.ptr(sd), sd.numel(), _lib.ptr(rows), U, _lib.ptr(fsd), total,
                                    _lib.ptr(wd), n_fft, hop, 1, _lib.ptr(Wd), _lib.ptr(bk), _lib.ptr(bj), W.shape[0],
                                    _lib.ptr(out[2:]), _lib.ptr(ws[2:]), nbytes, _lib.stream()), "mg_mel_loss_rows")
    assert bool((ws[:2] == GUARD).all()) and bool((ws[2 + nbytes // 8:] == GUARD).all())
    assert bool((out[:2] == UNWRITTEN).all()) and bool((out[2 + 4 * U:] == UNWRITTEN).all())
    out = out[2:2 + 4 * U].reshape(U, 4).contiguous()
    assert bool(torch.isfinite(out).all()) and bool((out[:, 1:3] == 0).all())
    return out


def mel_backward(hr_buf, sr_buf, table, frames, n_fft, hop, W, upstream, grad=None):
    """mg_mel_loss_rows_backward.  grad None: into a buffer filled with UNWRITTEN (accumulate = 0); a tensor: added into it
    (accumulate = 1).  -> grad_sr [len(sr_buf)] on the device."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    rows, fsd, total = device_tables(table, frames)
    hd, sd, wd = torch.from_numpy(hr_buf).cuda(), torch.from_numpy(sr_buf).cuda(), torch.from_numpy(T.S.hann32(n_fft)).cuda()
    Wd, bk, bj = bank_tensors(W)
    up = torch.from_numpy(np.asarray(upstream, np.float32)).cuda()
    nbytes = lib.mg_mel_loss_rows_backward_workspace(total, n_fft)
    assert nbytes == total * n_fft * 4
    ws = torch.full((nbytes // 4 + 8,), GUARD, dtype=torch.float32, device="cuda")
    accumulate = grad is not None
    if grad is None:
        grad = torch.full((len(sr_buf),), UNWRITTEN, dtype=torch.float32, device="cuda")
    _lib.check(lib.mg_mel_loss_rows_backward(_lib.ptr(hd), hd.numel(), _lib.ptr(sd), sd.numel(), _lib.ptr(rows), len(table),
                                             _lib.ptr(fsd), total, _lib.ptr(wd), n_fft, hop, 1, _lib.ptr(Wd), _lib.ptr(bk),
                                             _lib.ptr(bj), W.shape[0], _lib.ptr(up), int(accumulate), _lib.ptr(grad),
                                             _lib.ptr(ws[4:]), nbytes, _lib.stream()), "mg_mel_loss_rows_backward")
    assert bool((ws[:4] == GUARD).all()) and bool((ws[4 + nbytes // 4:] == GUARD).all())
    assert bool(torch.isfinite(ws[4:4 + nbytes // 4]).all())
    return grad


@functools.lru_cache(maxsize=None)
def references(which, kind, res):
    """per utterance of gpu_pairs(which, kind): (loss64, g64, loss32, g32) of the resolutions `res`; computed once per session"""
    banks = T.banks_of(res)
    return [T.mel_autograd(hr, sr, banks, torch.float64)[:2] + T.mel_autograd(hr, sr, banks, torch.float32)[:2]
            for hr, sr in T.gpu_pairs(which, kind)]


def judge(tag, kind, got, refs, lengths):
    """the bar over the utterances of one launch; prints every e and the worst e / yardstick"""
    e32s = [H.rel_err(r[3], r[1]) for r in refs]
    yard = max(e32s)
    worst = 0.0
    for u, (g, r) in enumerate(zip(got, refs)):
        assert np.all(np.isfinite(g))
        e = H.rel_err(g, r[1])
        worst = max(worst, e / yard)
        print("%s %s T=%d: e %.3g, e32 %.3g (launch %.3g), e / yardstick %.3g" % (tag, kind, lengths[u], e, e32s[u], yard, e / yard))
    print("%s %s: worst e(HIP) / largest e32 of the launch = %.3f" % (tag, kind, worst))
    for u, (g, r) in enumerate(zip(got, refs)):
        e = H.rel_err(g, r[1])
        assert e <= 4 * yard, (tag, kind, u, lengths[u], e, yard)
        assert e <= CEILING, (tag, kind, u, lengths[u], e)


def launch_and_judge(tag, kind, pairs, refs, lengths, n_fft, hop, W):
    """one forward and one backward launch over the packed utterances: value, containment, gradient"""
    from mdctgan_amd.metrics import plan_metrics
    frames = plan_metrics(lengths, n_fft, hop, True).frames
    hb, hs, sb, ss = packed_case(pairs)
    table = list(zip(hs, ss, lengths))
    row_out = mel_forward(hb, sb, table, frames, n_fft, hop, W)
    for u, r in enumerate(refs):
        got = row_out[u, 3].item()
        print("%s %s T=%d: loss %.9g, float64 %.9g, error %.3g (float32 CPU %.3g)"
              % (tag, kind, lengths[u], got, r[0], abs(got - r[0]) / r[0], abs(r[2] - r[0]) / r[0]))
        assert abs(got - r[0]) <= 2e-4 * r[0], (kind, u)
    grad = mel_backward(hb, sb, table, frames, n_fft, hop, W, [1.0] * len(lengths))
    assert written_only_inside(grad, ss, lengths)
    g = grad.double().cpu().numpy()
    judge(tag, kind, [g[s:s + n] for s, n in zip(ss, lengths)], refs, lengths)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the gradient per element, 2. the forward per utterance
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("hop_div", [4, 2])
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_gradient_and_value_of_one_resolution(n_fft, hop_div, kind):
    """Five utterances per launch whose frames straddle the tiles; everything outside them is 1e3 (values) or UNWRITTEN (the
    gradient).  Value: |loss - loss64| <= 2e-4 loss64 per utterance.  Gradient: the bar of the module's head.
    Measured on the MI355X: value within 9.3e-9 on every utterance; e between 4.0e-8 and 2.1e-7 on all 155 utterances of this module (these
    launches, the three-resolution mean and the odd filterbanks), against e32 between 9.9e-8 and 1.1e-4; the worst e / yardstick of a
    launch is 0.68 (the odd bank with three filters per bin), on the default banks 0.58: the bar is 4."""
    res = ((n_fft, n_fft // hop_div, T.MELS[n_fft]),)
    launch_and_judge("mg_mel_loss_rows N=%d hop=%d" % res[0][:2], kind, T.gpu_pairs(n_fft, kind), references(n_fft, kind, res),
                     T.LENGTHS[n_fft], n_fft, res[0][1], T.fbank32(RATE, n_fft, T.MELS[n_fft]))


@pytest.mark.parametrize("kind", T.KINDS)
def test_gradient_and_value_of_the_three_resolution_mean(kind):
    """metrics.mel_many with the default resolutions on packed operands read in place"""
    from mdctgan_amd.metrics import MEL_RESOLUTIONS, mel_many
    lengths = T.MEAN_LENGTHS
    pairs = T.gpu_pairs("mean", kind)
    refs = references("mean", kind, MEL_RESOLUTIONS)
    hb, hs, sb, ss = packed_case(pairs)
    sbuf = torch.from_numpy(sb).cuda().requires_grad_()
    loss = mel_many((torch.from_numpy(hb).cuda(), hs, lengths), (sbuf, ss, lengths), RATE)
    assert loss.dtype == torch.float64 and loss.shape == (5,)
    for u, r in enumerate(refs):
        print("mel_many %s T=%d: loss %.9g, float64 %.9g" % (kind, lengths[u], loss[u].item(), r[0]))
        assert abs(loss[u].item() - r[0]) <= 2e-4 * r[0], (kind, u)
    (grad,) = torch.autograd.grad(loss.sum(), sbuf)
    g = grad.double().cpu().numpy()
    inside = np.zeros(len(sb), bool)
    for s, n in zip(ss, lengths):
        inside[s:s + n] = True
    assert np.all(g[~inside] == 0.0)
    judge("mel_many, three resolutions,", kind, [g[s:s + n] for s, n in zip(ss, lengths)], refs, lengths)


def test_operand_refusals_of_mel_many():
    from mdctgan_amd.metrics import mel_many
    with pytest.raises(NotImplementedError, match="hr"):
        mel_many([torch.zeros(3000, device="cuda").requires_grad_()], [torch.zeros(3000)], RATE)
    with pytest.raises(ValueError, match=r"resolution \(2048, 512, 160\): utterance 1"):
        mel_many([torch.zeros(3000), torch.zeros(1024)], [torch.zeros(3000), torch.zeros(1024)], RATE)
    with pytest.raises(ValueError, match=r"resolution \(512, 128, 40\).*filter \d+ is empty"):
        mel_many([torch.zeros(3000)], [torch.zeros(3000)], 200000)


def dense_batch(B, Tn, seed):
    pairs = [T.signal_pair(T.KINDS[b % 3], Tn, seed + b, 1024) for b in range(B)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def test_loss_and_term_on_a_dense_batch():
    """[B, T], [B, 1, T] and [B, 1, 1, T]: the mean over the clips within 2e-4 of the float64 value, the same bits for every shape,
    clip b's gradient the bits mel_many gives it alone, divided by B.  The step's node: float32(scale * mel_loss) within one float32
    rounding on each side, and with a power-of-two scale its gradient has the bits of scale * mel_loss's."""
    from mdctgan_amd.metrics import mel_loss, mel_loss_term, mel_many
    B, Tn = 3, 4160
    hr, sr = dense_batch(B, Tn, 40)
    banks = T.banks_of(T.DEFAULT)
    want = float(np.mean([T.mel_autograd(h, s, banks, torch.float64)[0] for h, s in zip(hr, sr)]))
    vals, terms = [], []
    for shape in ((B, Tn), (B, 1, Tn), (B, 1, 1, Tn)):
        x = torch.from_numpy(sr).cuda().reshape(shape).requires_grad_()
        hd = torch.from_numpy(hr).cuda().reshape(shape)
        loss = mel_loss(x, hd, RATE)
        assert loss.dim() == 0 and loss.dtype == torch.float64
        vals.append(loss.detach().clone())
        (g,) = torch.autograd.grad(loss, x)
        assert g.shape == x.shape
        g = g.reshape(B, Tn)
        for b in range(B):
            leaf = torch.from_numpy(sr[b]).cuda().requires_grad_()
            (alone,) = torch.autograd.grad(mel_many([torch.from_numpy(hr[b])], [leaf], RATE).sum() / B, leaf)
            assert torch.equal(g[b], alone), (shape, b)
        for scale in (0.5, 3.0):
            term = mel_loss_term(x, hd, RATE, scale)
            assert term.dtype == torch.float32 and term.dim() == 0
            b_ = float(np.float32(scale * loss.item()))
            print("mel_loss_term scale %g: %.9g, float32(scale * mel_loss) %.9g" % (scale, term.item(), b_))
            assert abs(term.item() - b_) <= 2.0 ** -23 * abs(b_)
            (gt,) = torch.autograd.grad(term, x)
            (gs,) = torch.autograd.grad(scale * mel_loss(x, hd, RATE), x)
            if scale == 0.5:
                assert torch.equal(gt, gs)
            ref = gs.double()
            assert float((gt.double() - ref).abs().max()) <= 4 * 2.0 ** -23 * float(ref.abs().max())
            terms.append(term.detach().clone())
    print("mel_loss %.9g, float64 reference %.9g" % (vals[0].item(), want))
    assert abs(vals[0].item() - want) <= 2e-4 * want
    assert torch.equal(vals[0], vals[1]) and torch.equal(vals[0], vals[2])
    assert torch.equal(terms[0], terms[2]) and torch.equal(terms[0], terms[4])
    with pytest.raises(ValueError):
        mel_loss(torch.zeros(B, 2, Tn, device="cuda"), torch.zeros(B, 2, Tn, device="cuda"), RATE)
    with pytest.raises(ValueError):
        mel_loss_term(torch.zeros(B, Tn, device="cuda"), torch.zeros(B, Tn - 1, device="cuda"), RATE, 1.0)
    with pytest.raises(ValueError, match="resolution"):
        mel_loss(torch.zeros(B, 1024, device="cuda"), torch.zeros(B, 1024, device="cuda"), RATE)
    with pytest.raises(NotImplementedError, match="hr"):
        mel_loss(torch.zeros(B, Tn, device="cuda"), torch.zeros(B, Tn, device="cuda").requires_grad_(), RATE)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the exact zeros
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_zeros_between_ordinary_utterances():
    """sr == hr, an all-zero pair and an all-zero sr against a live hr, each between two ordinary utterances, default resolutions:
    loss exactly 0 / exactly 0 / finite and positive, gradient exactly 0 for all three, everything finite; the neighbours have the
    bits they have without them."""
    from mdctgan_amd.metrics import mel_many
    lengths = [3000, 2600, 2100, 2049, 4100, 1025, 2500]
    a, b, c, d = (T.signal_pair(k, lengths[i], 90 + i, 1024) for k, i in (("below", 0), ("tone", 2), ("mixed", 4), ("above", 6)))
    live = T.signal_pair("above", lengths[1], 97, 1024)[0]
    same = (live, live.copy())
    zero = (np.zeros(lengths[3], np.float32), np.zeros(lengths[3], np.float32))
    zero_sr = (T.signal_pair("below", lengths[5], 98, 1024)[0], np.zeros(lengths[5], np.float32))

    def run(pairs):
        srs = [torch.from_numpy(p[1]).cuda().requires_grad_() for p in pairs]
        loss = mel_many([torch.from_numpy(p[0]) for p in pairs], srs, RATE)
        assert bool(torch.isfinite(loss).all())
        return loss, torch.autograd.grad(loss.sum(), srs)
    loss, g = run([a, same, b, zero, c, zero_sr, d])
    assert loss[1].item() == 0.0 and loss[3].item() == 0.0 and loss[5].item() > 0.0
    for u in (1, 3, 5):
        assert g[u].shape == (lengths[u],) and bool((g[u] == 0).all())
    loss_o, g_o = run([a, b, c, d])
    for u, v in ((0, 0), (2, 1), (4, 2), (6, 3)):
        assert loss[u].item() == loss_o[v].item() and loss[u].item() > 0 and torch.equal(g[u], g_o[v])
        assert float(g[u].abs().max()) > 0
    assert all(bool(torch.isfinite(x).all()) for x in g)


# ---------------------------------------------------------------------------------------------------------------------
# 4. pack invariance and containment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", [(512, 128), (1024, 512), (2048, 512)])
def test_a_row_has_the_same_bits_alone_and_nothing_else_is_written(n_fft, hop):
    """Tightly packed sr (the neighbour IS the next sample), a dead row (len 0, pointing at real samples) in the middle of the
    table: the dead row's sums are zeros, grad_sr keeps its fill everywhere outside the live rows, and every row's sums and
    gradient equal, bit for bit, the launches with that row alone in buffers of exactly its samples."""
    from mdctgan_amd.metrics import plan_metrics
    W = T.fbank32(RATE, n_fft, T.MELS[n_fft])
    lengths = T.LENGTHS[n_fft]
    frames = plan_metrics(lengths, n_fft, hop, True).frames
    pairs = T.gpu_pairs(n_fft, "mixed")
    rng = np.random.default_rng(n_fft + hop)
    up = rng.uniform(0.5, 2.0, len(lengths) + 1).astype(np.float32)
    hb, hs = pack([p[0] for p in pairs], 64, 64, GUARD, tail=64)
    sb, ss = pack([p[1] for p in pairs], 3, 1, GUARD, tail=5)
    table = [list(r) for r in zip(hs, ss, lengths)]
    table.insert(2, [hs[1], ss[1], 0])
    frames_d = frames[:2] + [0] + frames[2:]
    row_out = mel_forward(hb, sb, table, frames_d, n_fft, hop, W)
    assert bool((row_out[2] == 0).all())
    got = mel_backward(hb, sb, table, frames_d, n_fft, hop, W, up)
    assert written_only_inside(got, ss, lengths)
    for k, r in enumerate([0, 1, 3, 4, 5]):
        h, s = pairs[k]
        one = [[0, 0, lengths[k]]]
        ro = mel_forward(h, s, one, [frames[k]], n_fft, hop, W)
        assert torch.equal(ro[0], row_out[r]), (k, lengths[k])
        alone = mel_backward(h, s, one, [frames[k]], n_fft, hop, W, up[r:r + 1])
        assert torch.equal(got[ss[k]:ss[k] + lengths[k]], alone), (k, lengths[k])
    # only the dead row: zeros for it, nothing written at all
    dead = [table[2], table[2]]
    ro = mel_forward(hb, sb, dead, [0, 1], n_fft, hop, W)
    assert bool((ro == 0).all())
    assert bool((mel_backward(hb, sb, dead, [0, 1], n_fft, hop, W, up[:2]) == UNWRITTEN).all())


def test_three_resolution_gradient_is_the_float32_sum_in_resolution_order():
    """accumulate = 1 adds onto the gradient that is there, and mel_many chains its resolutions that way"""
    from mdctgan_amd.metrics import MEL_RESOLUTIONS, mel_many, plan_metrics
    lengths = T.MEAN_LENGTHS
    pairs = T.gpu_pairs("mean", "mixed")
    hb, hs, sb, ss = packed_case(pairs)
    table = list(zip(hs, ss, lengths))
    third = [np.float32(1.0 / 3.0)] * len(lengths)
    singles, chained = [], None
    for n_fft, hop, n_mels in MEL_RESOLUTIONS:
        W = T.fbank32(RATE, n_fft, n_mels)
        frames = plan_metrics(lengths, n_fft, hop, True).frames
        singles.append(mel_backward(hb, sb, table, frames, n_fft, hop, W, third))
        chained = mel_backward(hb, sb, table, frames, n_fft, hop, W, third, grad=chained)
    assert written_only_inside(chained, ss, lengths)
    inside = chained != UNWRITTEN
    want = (singles[0] + singles[1]) + singles[2]
    assert torch.equal(chained[inside], want[inside]) and not torch.equal(chained[inside], singles[0][inside])
    sbuf = torch.from_numpy(sb).cuda().requires_grad_()
    (g,) = torch.autograd.grad(mel_many((torch.from_numpy(hb).cuda(), hs, lengths), (sbuf, ss, lengths), RATE).sum(), sbuf)
    assert torch.equal(g[inside], chained[inside]) and bool((g[~inside] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. odd filterbanks: the band-table loops, the J tail, one-bin filters
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def odd_case(name):
    if name == "wide":
        n_fft, hop, W, pairs, lengths = 2048, 512, T.wide_fbank(), T.gpu_pairs(2048, "mixed"), T.LENGTHS[2048]
    else:
        n_fft, hop, W, pairs, lengths = 512, 128, T.odd_fbank(name), T.odd_pairs(name), T.ODD_LENGTHS
    banks = [(n_fft, hop, W)]
    refs = [T.mel_autograd(hr, sr, banks, torch.float64)[:2] + T.mel_autograd(hr, sr, banks, torch.float32)[:2] for hr, sr in pairs]
    return n_fft, hop, W, pairs, lengths, refs


@pytest.mark.parametrize("name", ["one", "wide", "three"])
def test_odd_filterbanks(name):
    """"one": J = 1, a filter over every bin (255 lanes of a frame own no filter).  "wide": J = 256 at N = 2048, the kernels' limit
    (filters of one and two bins at the low end).  "three": a bank handed in directly whose bins lie in three filters, with rows
    scaled so that a fifth of sr's energies lie under the 1e-5 floor and a seventh of its bins under the 1e-7 clamp."""
    from mdctgan_amd.metrics import mel_band_tables
    n_fft, hop, W, pairs, lengths, refs = odd_case(name)
    band_k, band_j = mel_band_tables(W)
    print("%s: J = %d, filters of %d to %d bins, bins in up to %d filters" % (name, W.shape[0], (band_k[:, 1] - band_k[:, 0]).min(),
                                                                              (band_k[:, 1] - band_k[:, 0]).max(),
                                                                              (band_j[:, 1] - band_j[:, 0]).max()))
    launch_and_judge("odd filterbank", name, pairs, refs, lengths, n_fft, hop, W)


# ---------------------------------------------------------------------------------------------------------------------
# 6. determinism and capture
# ---------------------------------------------------------------------------------------------------------------------
def test_loss_is_deterministic_and_capturable():
    """Two runs of forward plus backward are bit-identical, and a single-stream graph of both replays to the eager bits."""
    from mdctgan_amd.metrics import mel_loss
    hr, sr = dense_batch(4, 4160, 60)
    hd = torch.from_numpy(hr).cuda()
    x = torch.from_numpy(sr).cuda().requires_grad_()

    def run():
        loss = mel_loss(x, hd, RATE)
        (g,) = torch.autograd.grad(loss, x)
        return loss.detach(), g
    l1, g1 = run()
    l2, g2 = run()
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and float(g1.abs().max()) > 0
    graph, (lc, gc) = capture(run)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lc, l1) and torch.equal(gc, g1)


def test_the_upstream_gradient_is_read_when_the_graph_replays():
    """The step's node captured with the upstream gradient in a device tensor holding 1; with 4 in it the replay gives exactly four
    times the gradient and the same loss: a captured --fp16 step follows a loss scale that changes between replays."""
    from mdctgan_amd.metrics import mel_loss_term
    hr, sr = dense_batch(4, 4160, 61)
    hd = torch.from_numpy(hr).cuda()
    x = torch.from_numpy(sr).cuda().requires_grad_()
    go = torch.ones((), dtype=torch.float32, device="cuda")

    def run():
        loss = mel_loss_term(x, hd, RATE, 0.5)
        (g,) = torch.autograd.grad(loss, x, grad_outputs=go)
        return loss.detach(), g
    l0, g0 = run()
    graph, (lc, gc) = capture(run)
    graph.replay()
    l1, g1 = lc.clone(), gc.clone()
    go.fill_(4.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(l1, l0) and torch.equal(g1, g0) and float(g1.abs().max()) > 0
    assert torch.equal(gc, 4.0 * g1) and torch.equal(lc, l1)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the chain
# ---------------------------------------------------------------------------------------------------------------------
def test_loss_reaches_the_generator():
    from mdctgan_amd import functional as Fh
    from mdctgan_amd.metrics import mel_loss
    from test_codec_grad_gpu import _toy_model
    model = _toy_model()
    g = np.load(os.path.join(REPO, "tests", "golden", "g6_step_global.npz"))
    lr, hr = torch.from_numpy(g["lr"]).cuda(), torch.from_numpy(g["hr"]).cuda()
    params = [p for p in model.netG.parameters() if p.requires_grad]
    for p in params:
        p.grad = None
    sr_spectro, _, _, _, _, _, _, lr_norm = model.forward(lr, hr)
    loss = mel_loss(model.preprocess.to_audio(sr_spectro, lr_norm), hr.reshape(hr.shape[0], -1).contiguous(), model.opt.hr_sampling_rate)
    assert bool(torch.isfinite(loss)) and loss.item() > 0
    loss.backward()
    grads = [Fh.grad_of(p) for p in params]
    assert all(bool(torch.isfinite(a).all()) for a in grads) and any(float(a.abs().max()) > 0 for a in grads)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the step: the toy model of tests/test_lambda_lsd_gpu.py (segment 7936: longer than 1024 decoded samples)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    g = np.load(os.path.join(REPO, "tests", "golden", "g6_step_global.npz"))
    return torch.from_numpy(g["lr"]).cuda(), torch.from_numpy(g["hr"]).cuda()


def toy_model(*extra):
    from test_lambda_lsd_gpu import toy_model as make
    return make(*extra)


def hand_gradient(model, spectro, lr_norm, hr, others=False):
    """d (0.5 * mel_loss [+ the lsd and mrstft terms])(to_audio(leaf, lr_norm), hr) / d leaf at leaf = spectro.detach(): the mel term
    added BY HAND, as the float64 composition times lambda.  With the other two terms the nodes are made in the step's order, so
    that autograd adds the three float32 gradients at the decoded waveform in the step's order, (mel + mrstft) + lsd: the codec's
    backward amplifies a last-bit difference there some fifty-fold."""
    from mdctgan_amd.metrics import lsd_loss_term, mel_loss, mrstft_loss_term
    leaf = spectro.detach().clone().requires_grad_()
    audio = model.preprocess.to_audio(leaf, lr_norm)
    first = lsd_loss_term(audio, hr, model.opt, LAMBDA) + mrstft_loss_term(audio, hr, LAMBDA) if others else None
    loss = LAMBDA * mel_loss(audio, hr, model.opt.hr_sampling_rate)
    if others:
        loss = first + loss
    (g,) = torch.autograd.grad(loss, leaf)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    return g


@pytest.mark.parametrize("arrangement", ["mel", "all_three"])
def test_forward_adds_the_term_at_the_generators_output(batch, arrangement):
    """_forward(infer=True) and a plain .backward() of the generator's losses: loss_names, the value against the float64
    restatement of the decoded output, and the gradient at the returned sr_spectro = the model's without the flag there plus that
    of 0.5 * mel_loss(...) added by hand (one float32 add; 0.5 is a power of two, so the seeded kernels give the bits of the float64
    composition), bit for bit.  With --lambda_lsd and --lambda_mrstft as well, to_audio runs once and all three read the one decoded waveform."""
    from mdctgan_amd import functional as Fh
    lr, hr = batch
    three = arrangement == "all_three"

    def run(model):
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

    plain = toy_model()
    assert plain.loss_names == ["G_GAN", "G_GAN_Feat", "D_real", "D_fake"]
    d0, s0, g0, _, _ = run(plain)
    model = toy_model("--lambda_mel", str(LAMBDA), *(["--lambda_lsd", str(LAMBDA), "--lambda_mrstft", str(LAMBDA)] if three else []))
    assert model.loss_names == ["G_GAN", "G_GAN_Feat"] + (["G_lsd", "G_mrstft"] if three else []) + ["G_mel", "D_real", "D_fake"]
    calls = count_to_audio(model)
    d1, s1, total, params, grads = run(model)
    assert len(calls) == 1
    assert torch.equal(s0, s1) and all(torch.equal(d0[k], d1[k]) for k in d0)
    term = d1["G_mel"]
    assert term.dtype == torch.float32 and term.dim() == 0 and bool(torch.isfinite(term)) and term.item() > 0
    lr_norm = model.preprocess.forward(lr)[2]
    with torch.no_grad():
        audio = model.preprocess.to_audio(s1, lr_norm).reshape(hr.shape[0], -1).cpu().numpy()
    banks = T.banks_of(T.DEFAULT, model.opt.hr_sampling_rate)
    want = LAMBDA * float(np.mean([T.mel_autograd(h, a, banks, torch.float64)[0]
                                   for h, a in zip(hr.reshape(hr.shape[0], -1).cpu().numpy(), audio)]))
    print("G_mel %.9g, lambda * float64 restatement %.9g" % (term.item(), want))
    assert abs(term.item() - want) <= 2e-4 * want
    assert torch.equal(total, g0 + hand_gradient(model, s1, lr_norm, hr, others=three))
    assert not torch.equal(total, g0)
    for p in params:
        p.grad = None
    model.forward(lr, hr)[0].backward(total)
    assert all(torch.equal(a, Fh.grad_of(p)) for a, p in zip(grads, params))
    assert any(float(a.abs().max()) > 0 for a in grads)


def test_the_step_decodes_once_with_all_three_terms(batch):
    """optimize_parameters with --lambda_lsd, --lambda_mrstft and --lambda_mel: one to_audio call per step, and the codec's decode
    kernels (forward and backward) are launched as often as in the step of a model with --lambda_lsd alone (device activities of
    one eager step under torch.profiler)."""
    lr, hr = batch

    def decodes(*flags):
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        model = toy_model(*flags)
        model.optimize_parameters(lr, hr)
        calls = count_to_audio(model)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            model.optimize_parameters(lr, hr)
            torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            if e.device_type == DeviceType.CUDA:
                names[e.name] = names.get(e.name, 0) + 1
        return len(calls), names
    n_lsd, k_lsd = decodes("--lambda_lsd", str(LAMBDA))
    n_all, k_all = decodes("--lambda_lsd", str(LAMBDA), "--lambda_mrstft", str(LAMBDA), "--lambda_mel", str(LAMBDA))
    assert n_lsd == 1 and n_all == 1
    codec = [k for k in k_lsd if "imdct" in k.lower()]
    assert codec, sorted(k_lsd)
    for k in codec:                       # the decode kernels (forward and backward) run as often as with one term
        assert k_all.get(k) == k_lsd[k], (k, k_all.get(k), k_lsd[k])
    assert any("mel_loss" in k for k in k_all) and not any("mel_loss" in k for k in k_lsd)
    mel = {k: v for k, v in k_all.items() if "mel_loss" in k}
    print("mel kernels of one step: %s" % mel)
    assert sum(mel.values()) == 9            # per resolution: the frame kernel and the finish forward, the frame kernel backward


def test_lambda_mel_zero_leaves_the_step_as_it_is(batch):
    """--lambda_mel 0 against no flag: the same loss names, and after three steps the same loss values and weights bit for bit"""
    lr, hr = batch
    plain, off = toy_model(), toy_model("--lambda_mel", "0")
    assert off.loss_names == plain.loss_names == ["G_GAN", "G_GAN_Feat", "D_real", "D_fake"] and off.lambda_mel == 0.0
    calls = count_to_audio(off)
    for _ in range(3):
        l0, l1 = plain.optimize_parameters(lr, hr), off.optimize_parameters(lr, hr)
    assert not calls
    assert list(l0) == list(l1) and all(torch.equal(l0[k], l1[k]) for k in l0)
    for a_net, b_net in ((plain.netG, off.netG), (plain.netD, off.netD)):
        for (k, a), (_, b) in zip(a_net.state_dict().items(), b_net.state_dict().items()):
            assert torch.equal(a, b), k


def test_optimize_parameters_adds_the_term_in_the_shared_pass(batch):
    from test_lambda_lsd_gpu import step_with_output_hook
    lr, hr = batch
    plain, model = toy_model(), toy_model("--lambda_mel", str(LAMBDA))
    lr_norm = model.preprocess.forward(lr)[2]
    l0, y0, g0 = step_with_output_hook(plain, lr, hr)
    l1, y1, g1 = step_with_output_hook(model, lr, hr)
    assert plain._shared_rows == model._shared_rows == lr.shape[0], "the step did not take the shared discriminator pass"
    assert torch.equal(y0, y1)
    assert torch.equal(g1, g0 + hand_gradient(model, y1, lr_norm, hr)) and not torch.equal(g1, g0)
    assert list(l1) == ["G_GAN", "G_GAN_Feat", "G_mel", "D_real", "D_fake"] and list(l0) == ["G_GAN", "G_GAN_Feat", "D_real", "D_fake"]
    assert l1["G_mel"].grad_fn is None and bool(torch.isfinite(l1["G_mel"])) and l1["G_mel"].item() > 0
    assert all(torch.equal(l0[k], l1[k]) for k in l0)
    torch.cuda.synchronize()
    assert not all(torch.equal(a, b) for a, b in zip(plain.netG.state_dict().values(), model.netG.state_dict().values()))
    assert all(bool(torch.isfinite(v).all()) for v in model.netG.state_dict().values())
    for (k, a), (_, b) in zip(plain.netD.state_dict().items(), model.netD.state_dict().items()):
        assert torch.equal(a, b), k


def eager_and_replayed(batch, *extra, steps=5):
    """`steps` eager steps against two warm-up steps and steps - 2 replays of the captured step, a fresh model each
    -> (eager model, graphed model, the eager model's initial generator weights, its loss scale after every step or None)"""
    lr, hr = batch
    flags = ("--lambda_mel", str(LAMBDA)) + extra
    eager, graphed = toy_model(*flags), toy_model(*flags)
    initial = [v.clone() for v in eager.netG.state_dict().values()]
    scales = []
    for _ in range(steps):
        le = eager.optimize_parameters(lr, hr)
        if eager.scaler is not None:
            scales.append(eager.scaler.get_scale())
    run = graphed.make_graphed_step(lr, hr, warmup=2)
    for _ in range(steps - 2):
        lg = run(lr, hr)
    torch.cuda.synchronize()
    assert "G_mel" in le and list(le) == list(lg)
    for k in le:
        assert le[k].grad_fn is None and lg[k].grad_fn is None
        assert np.isfinite(le[k].item()) and le[k].item() == lg[k].item(), k
    for a_net, b_net in ((eager.netG, graphed.netG), (eager.netD, graphed.netD)):
        for (k, a), (_, b) in zip(a_net.state_dict().items(), b_net.state_dict().items()):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), k
    return eager, graphed, initial, scales or None


def test_graphed_step_with_the_term_equals_eager_steps(batch):
    eager, _, initial, _ = eager_and_replayed(batch)
    assert not all(torch.equal(a, b) for a, b in zip(initial, eager.netG.state_dict().values()))
    plain = toy_model()
    for _ in range(5):
        plain.optimize_parameters(*batch)
    assert not all(torch.equal(a, b) for a, b in zip(plain.netG.state_dict().values(), eager.netG.state_dict().values()))


def test_graphed_step_with_all_three_terms_equals_eager_steps(batch):
    eager, _, _, _ = eager_and_replayed(batch, "--lambda_lsd", str(LAMBDA), "--lambda_mrstft", str(LAMBDA))
    assert eager.loss_names == ["G_GAN", "G_GAN_Feat", "G_lsd", "G_mrstft", "G_mel", "D_real", "D_fake"]


FP16_STEPS = 12


def test_fp16_step_with_the_term(batch):
    """--fp16 from GradScaler's default scale of 65536, twelve steps.  On this toy model the first steps overflow in float16 and are
    skipped while the scale backs off (by data, not by a fault); then the steps are real ones.  Asserted: a back-off happened and
    reaches into the replays; the scale held from one step to the next at least once and sits above 65536 / 2^steps (so not every
    step was skipped); the generator moved from its initial weights and ends elsewhere than the --fp16 run without the term (the
    term's gradient arrived, finite, through the seeded kernels that read the loss scale on the device); and the captured step --
    two warm-up steps, then ten replays -- ends on the eager bits, GradScaler state included: the scaler's trajectory is the same."""
    eager, graphed, initial, scales = eager_and_replayed(batch, "--fp16", steps=FP16_STEPS)
    print("loss scale after each of the %d steps: %s" % (FP16_STEPS, scales))
    assert eager.scaler is not None and bool(torch.isfinite(eager.scaler.state).all())
    assert torch.equal(eager.scaler.state, graphed.scaler.state)
    assert scales[-1] < 65536.0 and scales[2] > scales[-1]
    assert any(a == b for a, b in zip(scales[2:], scales[3:])) and scales[-1] > 65536.0 / 2 ** FP16_STEPS
    assert any(not torch.equal(a, b) for a, b in zip(initial, eager.netG.state_dict().values()))
    assert all(bool(torch.isfinite(v).all()) for v in eager.netG.state_dict().values())
    plain = toy_model("--fp16")
    for _ in range(FP16_STEPS):
        plain.optimize_parameters(*batch)
    assert not all(torch.equal(a, b) for a, b in zip(plain.netG.state_dict().values(), eager.netG.state_dict().values()))


def test_refusals(batch):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    lr, hr = batch
    base = ["--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4", "--n_blocks_global", "2", "--n_blocks_attn_g", "0",
            "--num_D", "2", "--ndf", "8", "--batchSize", "2", "--bins", "32", "--gpu_ids", "0"]
    seg = ["--segment_length", "7936"]
    with pytest.raises(NotImplementedError, match="lambda_mel"):
        create_model(options.make_opt("--explicit_encoding", "--lambda_mel", "1", *base, *seg))
    with pytest.raises(NotImplementedError, match="lambda_mel"):
        create_model(options.make_opt("--lambda_mel", "1", *base, *seg))              # no codec flag: the dB codec
    with pytest.raises(ValueError, match="lambda_mel"):
        create_model(options.make_opt(*options.SPECTRAL_FLAGS, "--lambda_mel", "-0.5", *base, *seg))
    with pytest.raises(ValueError, match="lambda_mel.*segment_length"):
        create_model(options.make_opt(*options.SPECTRAL_FLAGS, "--lambda_mel", "1", *base, "--segment_length", "1024"))
    model = toy_model("--lambda_mel", "1")
    for call in (lambda h: model.optimize_parameters(lr, h), lambda h: model._forward(lr, h)):
        with pytest.raises(ValueError, match="hr_audio"):
            call(hr[:, :-256].contiguous())
    assert np.isfinite(model.optimize_parameters(lr, hr)["G_mel"].item())
