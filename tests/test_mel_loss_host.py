"""The multi-scale mel-spectrogram L1 loss without a GPU (metrics.mel_fbank / mel_many / mel_loss / mel_loss_term, --lambda_mel;
csrc/mel_loss_rows.hip).

For one resolution (N, hop, J): periodic Hann window of N samples (float64, rounded to float32 once), centred frames reflected at
the utterance's own ends, K = N/2 + 1 bins, F frames, p = re^2 + im^2, m = sqrt(max(p, 1e-7)), W the float32 filterbank [J, K],
    E_j = sum_k W[j][k] m_k,   l_j = ln max(E_j, 1e-5),   loss = sum_{f,j} |l_hr - l_sr| / (F J),
and the multi-scale loss is the mean over the resolutions.  Gradient in sr only.  At the non-smooth points, by definition: a filter
with l_hr == l_sr contributes 0, a filter with E_sr <= 1e-5 contributes 0, a bin with p_sr < 1e-7 contributes 0.

1. mel_fbank against an independent float64 restatement (scalar loops), its band tables, and the refusals of mel_band_tables.
2. The yardstick: the definition under torch.stft + autograd in float64 and float32 (mel_autograd), and the kernels' two-stage
   algorithm restated in float64 numpy (one window-weighted gradient frame per frame, then test_lsd_loss_host.gather); the two
   agree to 1e-11 of the largest element.
3. The bars of tests/test_mel_loss_gpu.py have teeth on that test's own inputs: six broken restatements each miss them by more
   than 10x.
4. Those inputs are tie-free on the float64 reference.  5. The exact zeros.  6. --lambda_mel, the model's refusals, header,
   bindings, exports, argument errors.
"""
import json
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import test_mrstft_loss_host as S

H = S.H
REPO = S.REPO
P_CLAMP, E_FLOOR = 1e-7, 1e-5
DEFAULT = ((512, 128, 40), (1024, 256, 80), (2048, 512, 160))
RATE = 16000
CEILING = 1e-4                   # the absolute ceiling of the GPU test's gradient bar (derived in its module head)
NEW = ("mg_mel_loss_rows_workspace", "mg_mel_loss_rows", "mg_mel_loss_rows_backward_workspace", "mg_mel_loss_rows_backward",
       "mg_mel_loss_rows_backward_seeded")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the filterbank
# ---------------------------------------------------------------------------------------------------------------------
def fbank64(rate, n_fft, n_mels, f_min=0.0, f_max=None):
    """the definition with scalar arithmetic: HTK mel points, triangles without area normalisation, float64"""
    f_max = rate / 2.0 if f_max is None else f_max
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    lo, hi = mel(f_min), mel(f_max)
    h = [700.0 * (10.0 ** ((lo + (hi - lo) * i / (n_mels + 1)) / 2595.0) - 1.0) for i in range(n_mels + 2)]
    W = np.zeros((n_mels, n_fft // 2 + 1))
    for j in range(n_mels):
        for k in range(n_fft // 2 + 1):
            f = k * rate / n_fft
            W[j, k] = max(0.0, min((f - h[j]) / (h[j + 1] - h[j]), (h[j + 2] - f) / (h[j + 2] - h[j + 1])))
    return W


def fbank32(rate, n_fft, n_mels):
    from mdctgan_amd.metrics import mel_fbank
    return mel_fbank(rate, n_fft, n_mels).numpy()


@pytest.mark.parametrize("rate,f_min,f_max", [(16000, 0.0, None), (44100, 0.0, None), (48000, 0.0, None), (22050, 80.0, 7600.0)])
def test_mel_fbank_against_the_float64_restatement(rate, f_min, f_max):
    """Within 1e-6 absolute of the scalar restatement (float32 rounding of values in [0, 1] is 6e-8; the two evaluate the mel points
    in different orders, which moves a point by 1e-12 of itself), no empty row for the defaults, at most two filters per bin, and the
    band tables reproduce the supports."""
    from mdctgan_amd.metrics import mel_band_tables, mel_fbank
    for n_fft, _, n_mels in DEFAULT:
        W = mel_fbank(rate, n_fft, n_mels, f_min, f_max)
        assert W.dtype == torch.float32 and tuple(W.shape) == (n_mels, n_fft // 2 + 1)
        want = fbank64(rate, n_fft, n_mels, f_min, f_max)
        assert float(np.abs(W.numpy().astype(np.float64) - want).max()) <= 1e-6
        nz = W.numpy() != 0
        assert nz.any(axis=1).all() and nz.sum(axis=0).max() <= 2
        band_k, band_j = mel_band_tables(W)
        assert band_k.dtype == np.int32 and band_j.dtype == np.int32 and band_k.shape == (n_mels, 2) and band_j.shape == (nz.shape[1], 2)
        for j in range(n_mels):
            assert np.array_equal(np.flatnonzero(nz[j]), np.arange(band_k[j, 0], band_k[j, 1]))
        for k in range(nz.shape[1]):
            assert np.array_equal(np.flatnonzero(nz[:, k]), np.arange(band_j[k, 0], band_j[k, 1]))


def test_band_tables_refuse_what_the_kernels_cannot_walk():
    from mdctgan_amd.metrics import mel_band_tables, mel_fbank
    W = fbank32(RATE, 512, 40)
    gap = W.copy()
    j = int(np.argmax((W != 0).sum(axis=1)))                 # a filter of at least three bins: a hole in its support
    k = np.flatnonzero(W[j])
    gap[j, k[1]] = 0.0
    with pytest.raises(ValueError, match="filter %d.*contiguous" % j):
        mel_band_tables(gap)
    empty = W.copy()
    empty[7] = 0.0
    with pytest.raises(ValueError, match="filter 7 is empty"):
        mel_band_tables(empty)
    swapped = W[::-1].copy()                                 # supports that run backwards
    with pytest.raises(ValueError, match="monotone"):
        mel_band_tables(swapped)
    split = np.zeros((3, 8), np.float32)                     # bin 2 lies in filters 0 and 2 but not in 1
    split[0, 1:3], split[1, 3:5], split[2, 2:7] = 1.0, 1.0, 1.0
    with pytest.raises(ValueError):
        mel_band_tables(split)
    for bad in (W.astype(np.float64), W[0], np.zeros((257, 4), np.float32), np.full((2, 4), np.nan, np.float32)):
        with pytest.raises(ValueError):
            mel_band_tables(bad)
    # too many filters for a transform: the lowest ones fall between two bins
    with pytest.raises(ValueError, match="empty"):
        mel_band_tables(mel_fbank(RATE, 512, 256))
    for bad in (dict(f_min=-1.0), dict(f_max=9000.0), dict(f_min=4000.0, f_max=4000.0)):
        with pytest.raises(ValueError):
            mel_fbank(RATE, 512, 40, **bad)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def banks_of(resolutions, rate=RATE):
    """[(n_fft, hop, W float32 numpy)] of (n_fft, hop, n_mels) triples"""
    return [(n, h, fbank32(rate, n, j)) for n, h, j in resolutions]


def mel_autograd(hr, sr, banks, dtype, center=True):
    """The definition for one utterance in `dtype` on the CPU -> (loss, d loss / d sr, [loss per resolution]), float64 numpy.
    hr, sr: float32 numpy; banks: [(n_fft, hop, W)].  (torch's clamp passes no gradient below the bound, its abs has sign(0) = 0.)"""
    x = torch.from_numpy(sr).to(dtype).requires_grad_()
    h = torch.from_numpy(hr).to(dtype)
    per = []
    for n_fft, hop, W in banks:
        Wt = torch.from_numpy(W).to(dtype)

        def logmel(a):
            s = S._spectrum(a, n_fft, hop, dtype, center)
            m = torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=P_CLAMP))
            return torch.log(torch.clamp(Wt @ m, min=E_FLOOR))
        lh, ls = logmel(h), logmel(x)
        per.append((lh - ls).abs().sum() / lh.numel())
    loss = sum(per) / len(per)
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), g.double().numpy(), [float(p.detach()) for p in per]


def frame_spectra(x, n_fft, hop):
    w = S.hann32(n_fft).astype(np.float64)
    M = n_fft // 2
    x = np.pad(x.astype(np.float64), (M, M), mode="reflect")
    F = 1 + (len(x) - n_fft) // hop
    return np.fft.rfft(x[hop * np.arange(F)[:, None] + np.arange(n_fft)[None, :]] * w, axis=-1)


def frame_gradients(hr, sr, n_fft, hop, W, upstream=1.0, second_window=True, e_clamp=True, p_clamp=True, sign=True, short_walk=False):
    """Stage one of the kernels in float64: [frames, n_fft], frame f = y_f[n] window[n], y_f the gradient of upstream * loss with
    respect to the windowed frame f of sr.  The keyword arguments are the faults of test 3."""
    w = S.hann32(n_fft).astype(np.float64)
    M = n_fft // 2
    Wd = W.astype(np.float64)
    if short_walk:                                           # every filter's walk stops one bin early
        Wd = Wd.copy()
        for j in range(Wd.shape[0]):
            Wd[j, np.flatnonzero(Wd[j])[-1]] = 0.0
    Xh, Xs = frame_spectra(hr, n_fft, hop), frame_spectra(sr, n_fft, hop)
    ph, ps = np.abs(Xh) ** 2, np.abs(Xs) ** 2
    p_floor, e_floor = (P_CLAMP if p_clamp else 1e-300), (E_FLOOR if e_clamp else 1e-300)
    mh, ms = np.sqrt(np.maximum(ph, p_floor)), np.sqrt(np.maximum(ps, p_floor))
    Eh, Es = mh @ Wd.T, ms @ Wd.T                            # [F, J]
    dl = np.log(np.maximum(Eh, e_floor)) - np.log(np.maximum(Es, e_floor))
    sg = np.sign(dl) if sign else np.ones_like(dl)
    dE = -(upstream / dl.size) * sg / Es
    dE[Es <= e_floor] = 0.0
    c = (dE @ Wd) / ms
    c[ps < p_floor] = 0.0
    G = c * Xs
    Hs = G / 2
    Hs[:, 0], Hs[:, M] = G[:, 0].real, G[:, M].real
    y = n_fft * np.fft.irfft(Hs, n=n_fft, axis=-1)
    return y * w if second_window else y


def mel_grad_two_stage(hr, sr, banks, **broken):
    reflected = broken.pop("reflected", True)
    out = np.zeros(len(sr))
    for n_fft, hop, W in banks:
        frames = frame_gradients(hr, sr, n_fft, hop, W, upstream=1.0 / len(banks), **broken)
        out += H.gather(frames, len(sr), n_fft, hop, True, reflected=reflected)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the inputs (shared with tests/test_mel_loss_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
KINDS = S.KINDS                                              # "below", "above", "mixed" (noise mixes), "tone"
FLOOR = 1e-3                                                 # the noise floor under the tone pair
LENGTHS, MEAN_LENGTHS = S.LENGTHS, S.MEAN_LENGTHS
MELS = {512: 40, 1024: 80, 2048: 160}
SEED0 = {512: 6120, 1024: 11240, 2048: 21480, "mean": 177}   # utterance u of kind k: SEED0 + 16 k + u


def signal_pair(kind, n, seed, n_fft):
    """float32 (hr, sr): the MR-STFT test's noise mixes, and its tone pair with an independent noise floor of amplitude 1e-3 under
    each signal, so that no filter's two energies come from the same handful of skirt bins."""
    hr, sr = S.signal_pair(kind, n, seed, n_fft)
    if kind == "tone":
        rng = np.random.default_rng(seed)
        hr = (hr.astype(np.float64) + FLOOR * rng.standard_normal(n)).astype(np.float32)
        sr = (sr.astype(np.float64) + FLOOR * rng.standard_normal(n)).astype(np.float32)
    return hr, sr


def gpu_pairs(which, kind):
    """The five utterances of one launch of the GPU test: which = 512 / 1024 / 2048 (one resolution) or "mean" (the three defaults)"""
    lengths = MEAN_LENGTHS if which == "mean" else LENGTHS[which]
    n_fft = 1024 if which == "mean" else which
    return [signal_pair(kind, n, SEED0[which] + 16 * KINDS.index(kind) + u, n_fft) for u, n in enumerate(lengths)]


def gpu_resolutions(which):
    return [DEFAULT] if which == "mean" else [((which, which // 4, MELS[which]),), ((which, which // 2, MELS[which]),)]


# the odd filterbanks of the GPU test, handed in directly: N = 512
def odd_fbank(name):
    """"one": J = 1, a ramp over every bin.  "three": 30 triangles of half-width 12 bins every 8 bins, so that most bins lie in
    three filters; every third row is scaled by 2e-4, which puts its energies on both sides of the 1e-5 floor on the quiet input."""
    K = 257
    k = np.arange(K, dtype=np.float64)
    if name == "one":
        return ((k + 1.0) / K)[None, :].astype(np.float32)
    W = np.stack([np.maximum(0.0, 1.0 - np.abs(k - 8.0 * (j + 1)) / 12.0) for j in range(30)])
    W[::3] *= 2e-4
    return W.astype(np.float32)


def wide_fbank():
    """J = 256 at N = 2048: the HTK bank of 48 kHz between 2 and 24 kHz (from 0 Hz the lowest filters would fall between two bins)"""
    from mdctgan_amd.metrics import mel_fbank
    return mel_fbank(48000, 2048, 256, f_min=2000.0).numpy()


ODD_LENGTHS = LENGTHS[512]
ODD_SEEDS = [901, 1000, 1125, 1200, 1350]        # (chosen: test 4 holds -- a level ramp walks many values past both bounds)


def odd_pairs(name):
    """"three": a quiet pair whose level rises along the utterance from 2e-5 to 2e-3 of the noise mixes' (frames from below the p
    clamp to above the E floor)."""
    out = []
    for u, n in enumerate(ODD_LENGTHS):
        hr, sr = signal_pair("mixed", n, ODD_SEEDS[u] if name == "three" else 900 + u, 512)
        if name == "three":
            ramp = 2e-4 * 10.0 ** (2.0 * np.arange(n) / n)
            hr, sr = (hr * ramp).astype(np.float32), (sr * ramp).astype(np.float32)
        out.append((hr, sr))
    return out


def tie_margins(hr, sr, n_fft, hop, W):
    """float64 -> (smallest non-zero |l_hr - l_sr|, smallest relative distance of an E to the floor, of a p to the clamp, fraction of
    E_sr under the floor, fraction of p_sr under the clamp)"""
    Wd = W.astype(np.float64)
    ph, ps = np.abs(frame_spectra(hr, n_fft, hop)) ** 2, np.abs(frame_spectra(sr, n_fft, hop)) ** 2
    Eh, Es = np.sqrt(np.maximum(ph, P_CLAMP)) @ Wd.T, np.sqrt(np.maximum(ps, P_CLAMP)) @ Wd.T
    dl = np.log(np.maximum(Eh, E_FLOOR)) - np.log(np.maximum(Es, E_FLOOR))
    nz = np.abs(dl[dl != 0.0])
    return (float(nz.min()) if nz.size else math.inf, float(min(np.abs(Eh / E_FLOOR - 1.0).min(), np.abs(Es / E_FLOOR - 1.0).min())),
            float(min(np.abs(ph / P_CLAMP - 1.0).min(), np.abs(ps / P_CLAMP - 1.0).min())), float((Es <= E_FLOOR).mean()),
            float((ps < P_CLAMP).mean()))


HOST_CASES = [(n_fft, n) for n_fft in (512, 1024, 2048) for n in (n_fft // 2 + 1, n_fft + 300)]


@pytest.mark.parametrize("n_fft,n", HOST_CASES)
def test_two_stage_restatement_equals_float64_autograd(n_fft, n):
    banks = banks_of(((n_fft, n_fft // 4, MELS[n_fft]),))
    for kind in KINDS:
        hr, sr = signal_pair(kind, n, n_fft + n, n_fft)
        loss, want, _ = mel_autograd(hr, sr, banks, torch.float64)
        got = mel_grad_two_stage(hr, sr, banks)
        err = H.rel_err(got, want)
        print("restatement N=%d T=%d %s: loss %.4f, error %.2e of the largest element" % (n_fft, n, kind, loss, err))
        assert np.all(np.isfinite(got)) and float(np.abs(want).max()) > 0 and err <= 1e-11, (kind, err)


def test_two_stage_restatement_of_the_three_resolution_mean():
    banks = banks_of(DEFAULT)
    hr, sr = signal_pair("mixed", 1500, 3, 1024)
    _, want, per = mel_autograd(hr, sr, banks, torch.float64)
    assert len(per) == 3 and H.rel_err(mel_grad_two_stage(hr, sr, banks), want) <= 1e-11
    hr, sr = odd_pairs("three")[2]
    odd = [(512, 128, odd_fbank("three"))]
    assert H.rel_err(mel_grad_two_stage(hr, sr, odd), mel_autograd(hr, sr, odd, torch.float64)[1]) <= 1e-11


# ---------------------------------------------------------------------------------------------------------------------
# 3. the GPU bars have teeth on the GPU test's own inputs
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = [{"reflected": False}, {"second_window": False}, {"e_clamp": False}, {"p_clamp": False}, {"sign": False}, {"short_walk": True}]


def launches(n_fft):
    """the launches of the GPU test at one transform size: (tag, pairs, banks)"""
    out = [(kind, gpu_pairs(n_fft, kind), banks_of(gpu_resolutions(n_fft)[0])) for kind in KINDS]
    if n_fft == 512:
        out.append(("odd three", odd_pairs("three"), [(512, 128, odd_fbank("three"))]))
    return out


@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_gpu_bars_reject_every_fault(n_fft):
    """Per launch of five utterances the gradient bar is min(4 max e32, 1e-4), e32 the error of float32 CPU autograd against
    float64.  The right restatement passes it on every utterance.  Each broken restatement misses it by more than 10x on every
    utterance of at least one launch at this transform size -- any such launch fails the GPU suite.  (A fault is invisible where it
    changes nothing: a dropped sign where every filter of sr is weaker than hr's, a missing clamp where nothing lies under it.  The
    E floor lies under every filter of an HTK bank -- a row's weights sum to more than one and m >= 3.2e-4 -- so it is the "odd
    three" launch, a bank with rows scaled by 2e-4 on a quiet input, that has energies under it and catches a missing E clamp; the same quiet input has a third of
    its bins under the p clamp, where the noise mixes have none and the floored tones a handful, so both clamp faults are asserted at
    N = 512 only.)"""
    caught = {json.dumps(f): 0.0 for f in FAULTS}
    for tag, pairs, banks in launches(n_fft):
        refs = [(mel_autograd(hr, sr, banks, torch.float64)[1], mel_autograd(hr, sr, banks, torch.float32)[1]) for hr, sr in pairs]
        yard = max(H.rel_err(g32, g64) for g64, g32 in refs)
        bar = min(4 * yard, CEILING)
        assert 0 < yard < 0.25
        for (hr, sr), (g64, _) in zip(pairs, refs):
            assert H.rel_err(mel_grad_two_stage(hr, sr, banks), g64) <= 1e-11
        for broken in FAULTS:
            miss = min(H.rel_err(mel_grad_two_stage(hr, sr, banks, **broken), g64) / bar for (hr, sr), (g64, _) in zip(pairs, refs))
            print("N=%d %s: yardstick %.3g, bar %.3g | %s | smallest error / bar over the launch %.3g" % (n_fft, tag, yard, bar, broken, miss))
            caught[json.dumps(broken)] = max(caught[json.dumps(broken)], miss)
    for broken in FAULTS:
        if ("e_clamp" in broken or "p_clamp" in broken) and n_fft != 512:
            continue                                         # (the launch that lies under both bounds runs at N = 512: see above)
        assert caught[json.dumps(broken)] > 10, (n_fft, broken, caught[json.dumps(broken)])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the inputs are tie-free
# ---------------------------------------------------------------------------------------------------------------------
LN_MARGIN, REL_MARGIN = 1e-6, 1e-3
# The spectrum is rounded to float32 once per bin: m carries 2^-24 relative, E (a sum of positive terms in double) no more, l_hr -
# l_sr at most 1.2e-7: a |l_hr - l_sr| of 1e-6 and an E or p that is 1e-3 (relative) from its bound are decided as float64 decides.


def check_margins(tag, pairs, banks):
    worst = [math.inf, math.inf, math.inf, 0.0, 0.0]
    for hr, sr in pairs:
        for n_fft, hop, W in banks:
            ln, e, p, under_e, under_p = tie_margins(hr, sr, n_fft, hop, W)
            assert ln >= LN_MARGIN and e >= REL_MARGIN and p >= REL_MARGIN, (tag, len(hr), n_fft, hop, ln, e, p)
            worst = [min(worst[0], ln), min(worst[1], e), min(worst[2], p), max(worst[3], under_e), max(worst[4], under_p)]
    print("tie margins %s: smallest |l_hr - l_sr| %.3g, |E / floor - 1| %.3g, |p / clamp - 1| %.3g; at most %.3g of E_sr under the "
          "floor, %.3g of p_sr under the clamp" % ((tag,) + tuple(worst)))
    return worst


@pytest.mark.parametrize("which", [512, 1024, 2048, "mean"])
def test_gpu_inputs_are_tie_free(which):
    for kind in KINDS:
        for res in gpu_resolutions(which):
            check_margins("%s %s %s" % (which, kind, res), gpu_pairs(which, kind), banks_of(res))


def test_odd_filterbank_inputs_are_tie_free_and_cross_both_bounds():
    from mdctgan_amd.metrics import mel_band_tables
    _, band_j = mel_band_tables(odd_fbank("three"))
    assert int((band_j[:, 1] - band_j[:, 0]).max()) == 3
    check_margins("odd one", odd_pairs("one"), [(512, 128, odd_fbank("one"))])
    worst = check_margins("odd three", odd_pairs("three"), [(512, 128, odd_fbank("three"))])
    assert 0.02 < worst[3] < 0.9 and 0.02 < worst[4] < 0.9          # energies under the floor and over it, bins under the clamp and over it
    check_margins("J = 256", gpu_pairs(2048, "mixed"), [(2048, 512, wide_fbank())])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the exact zeros
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_zero_cases():
    banks = banks_of(((512, 128, 40),))
    hr, _ = signal_pair("mixed", 1500, 3, 512)
    zero = np.zeros(1500, np.float32)
    for a, b, loss_is_zero in ((hr, hr.copy(), True), (zero, zero, True), (hr, zero, False)):
        loss, g, _ = mel_autograd(a, b, banks, torch.float64)
        two = mel_grad_two_stage(a, b, banks)
        assert np.all(g == 0.0) and np.all(two == 0.0) and math.isfinite(loss)
        assert (loss == 0.0) if loss_is_zero else (loss > 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the option, the model's refusals, header, bindings, argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_and_defaults_to_zero():
    from mdctgan_amd.options import make_opt
    assert make_opt("--lambda_mel", "0.25").lambda_mel == 0.25
    assert make_opt().lambda_mel == 0.0 and make_opt().lambda_mrstft == 0.0 and make_opt().lambda_lsd == 0.0


def test_loss_filter_places_the_term_after_the_mrstft():
    from mdctgan_amd.pix2pixHD_model import Pix2PixHDModel
    with_feat, without = types.SimpleNamespace(no_ganFeat_loss=False), types.SimpleNamespace(no_ganFeat_loss=True)
    assert Pix2PixHDModel.loss_filter(with_feat, 1, 2, 3, 4) == [1, 2, 3, 4]
    assert Pix2PixHDModel.loss_filter(with_feat, 1, 2, 3, 4, 5, 6, 7) == [1, 2, 5, 6, 7, 3, 4]
    assert Pix2PixHDModel.loss_filter(with_feat, 1, 2, 3, 4, g_mel=7) == [1, 2, 7, 3, 4]
    assert Pix2PixHDModel.loss_filter(without, 1, 2, 3, 4, g_lsd=5, g_mel=7) == [1, 5, 7, 3, 4]


def _check(in_kernel=True, n_fft=512, hop=256, **over):
    from mdctgan_amd.pix2pixHD_model import Audio2MDCT, Pix2PixHDModel
    pre = types.SimpleNamespace(_in_kernel=in_kernel, win_length=n_fft, hop_length=hop)
    pre.audio_length = lambda T: Audio2MDCT.audio_length(pre, T)
    opt = types.SimpleNamespace(**dict(dict(lambda_mel=1.0, segment_length=7936, hr_sampling_rate=48000), **over))
    return Pix2PixHDModel._check_lambda_mel(types.SimpleNamespace(preprocess=pre), opt)


def test_refusals_when_the_model_is_built():
    assert _check() == 1.0 and _check(lambda_mel=0.25) == 0.25
    for rate in (16000, 44100, 48000):
        assert _check(hr_sampling_rate=rate) == 1.0
    assert _check(n_fft=2048, hop=1024) == 1.0 and _check(n_fft=128, hop=64) == 1.0       # its own transforms, as --lambda_mrstft
    # 0 switches the term off whatever else is set: the default path checks nothing new
    assert _check(in_kernel=False, lambda_mel=0.0, segment_length=16, hr_sampling_rate=100) == 0.0
    for bad in (-1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="lambda_mel"):
            _check(lambda_mel=bad)
    with pytest.raises(NotImplementedError, match="lambda_mel"):
        _check(in_kernel=False)                                         # the dB and explicit-encoding codecs
    for short in (1024, 768, 256):                                      # decoded clips of at most 1024 samples
        with pytest.raises(ValueError, match="lambda_mel.*segment_length"):
            _check(segment_length=short)
    assert _check(segment_length=1280) == 1.0
    # at 200 kHz the lowest of the 40 filters of the 512-point transform falls between two bins
    with pytest.raises(ValueError, match=r"lambda_mel.*hr_sampling_rate.*resolution \(512, 128, 40\).*filter \d+ is empty"):
        _check(hr_sampling_rate=200000)


def test_too_short_an_utterance_names_utterance_and_resolution():
    from mdctgan_amd.metrics import MEL_RESOLUTIONS, plan_mel
    assert MEL_RESOLUTIONS == DEFAULT
    assert [p.frames for p in plan_mel([1025, 3000])] == [[9, 24], [5, 12], [3, 6]]
    with pytest.raises(ValueError, match=r"resolution \(2048, 512, 160\): utterance 1"):
        plan_mel([3000, 1024])
    with pytest.raises(ValueError, match=r"resolution \(512, 128, 40\): utterance 0"):
        plan_mel([256, 3000])
    with pytest.raises(NotImplementedError):
        plan_mel([3000], ((256, 64, 20),))
    for bad in (((512, 0, 40),), ((512, 128, 0),), ((512, 128, 257),), ((512, 128),), ()):
        with pytest.raises(ValueError):
            plan_mel([3000], bad)


def test_new_entry_points_are_declared_bound_and_exported():
    from mdctgan_amd import _lib
    text = open(os.path.join(REPO, "include", "mdctgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    declared = set(re.findall(r"\b(mg_mel_\w+)\s*\(", code))
    assert declared == set(NEW) == {n for n in _lib.SIGNATURES if n.startswith("mg_mel_")}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if " mg_mel_" in ln} == set(NEW)
    assert _lib.ABI_VERSION == 4 and lib.mg_abi_version() == 4


P = 4096                         # a non-null, 16-byte aligned "pointer"
FRAMES, NFFT, NMELS = 40, 1024, 80
WS_F, WS_B = FRAMES * 8, FRAMES * NFFT * 4
COMMON_BAD = [(0, None), (2, None), (4, None), (6, None), (8, None), (12, None), (13, None), (14, None),      # null pointers
              (12, P + 2), (13, P + 1), (14, P + 3),                                                         # misaligned tables
              (9, 256), (9, 4096), (9, 1000), (9, 0),                                                        # other transform sizes
              (1, 0), (1, -5), (3, 0), (3, -5), (5, 0), (5, -1), (7, 0), (7, -3), (10, 0), (10, -512),       # counts, totals, hop
              (15, 0), (15, -1), (15, 257)]                                                                  # the number of filters
# hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop, center, fbank, band_k, band_j, n_mels, ...
HEAD = [P, 30000, P, 30000, P, 3, P, FRAMES, P, NFFT, 512, 1, P, P, P, NMELS]
# ..., row_out, workspace, bytes, stream
FWD_GOOD = HEAD + [P, P, WS_F, None]
FWD_BAD = COMMON_BAD + [(16, None), (17, None), (18, WS_F - 1), (18, 0), (17, P + 4)]
# ..., grad_rows, accumulate, grad_sr, workspace, bytes, stream
BWD_GOOD = HEAD + [P, 0, P, P, WS_B, None]
BWD_BAD = COMMON_BAD + [(16, None), (18, None), (19, None), (20, WS_B - 1), (20, 0), (19, P + 4)]
# ..., go, scale, n_res, accumulate, grad_sr, workspace, bytes, stream
SEED_GOOD = HEAD + [P, 0.5, 3, 1, P, P, WS_B, None]
SEED_BAD = COMMON_BAD + [(16, None), (20, None), (21, None), (18, 0), (18, -1), (22, WS_B - 1), (22, 0), (21, P + 4)]
JOBS = [["mg_mel_loss_rows", FWD_GOOD, FWD_BAD], ["mg_mel_loss_rows_backward", BWD_GOOD, BWD_BAD],
        ["mg_mel_loss_rows_backward_seeded", SEED_GOOD, SEED_BAD]]

CHILD = """
import json, sys
sys.path.insert(0, %r)
from mdctgan_amd import _lib
lib = _lib.load()
for name, good, bad in json.loads(sys.argv[1]):
    for pos, value in bad:
        args = list(good)
        args[pos] = value
        print("rc %%s %%d %%d" %% (name, pos, getattr(lib, name)(*args)), flush=True)
q, b = lib.mg_mel_loss_rows_workspace, lib.mg_mel_loss_rows_backward_workspace
print("ws %%d %%d %%d %%d %%d %%d %%d %%d" %% (q(40), q(0), q(-1), b(40, 1024), b(0, 1024), b(-1, 512), b(40, 256), b(7, 512)))
""" % REPO


@pytest.fixture(scope="module")
def child():
    p = subprocess.run([sys.executable, "-c", CHILD, json.dumps(JOBS)], capture_output=True, text=True, cwd=REPO, timeout=300)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("name,bad", [(j[0], j[2]) for j in JOBS], ids=[j[0] for j in JOBS])
def test_bad_arguments_are_rejected_before_any_launch(child, name, bad):
    rc, out, errtxt = child
    assert rc == 0, "child exit status %d\n%s" % (rc, errtxt[-2000:])
    lines = [ln.split()[2:] for ln in out.splitlines() if ln.startswith("rc %s " % name)]
    assert lines == [[str(pos), str(H.MG_ERR_ARG)] for pos, _ in bad]


def test_workspace_queries(child):
    _, out, _ = child
    ws = [ln.split()[1:] for ln in out.splitlines() if ln.startswith("ws ")]
    assert ws == [[str(v) for v in (WS_F, 0, 0, WS_B, 0, 0, 0, 7 * 512 * 4)]]
