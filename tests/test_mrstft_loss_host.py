"""The multi-resolution STFT loss without a GPU (metrics.mrstft_many / mrstft_loss / mrstft_loss_term, --lambda_mrstft;
csrc/stft_loss_rows.hip).

For one resolution (N, hop): periodic Hann window of N samples (float64, rounded to float32 once), centred frames reflected at
the utterance's own ends, K = N/2 + 1 bins, F frames, p = re^2 + im^2, m = sqrt(max(p, 1e-7)),
    loss = sqrt(sum (m_hr - m_sr)^2 / sum m_hr^2) + sum |ln m_hr - ln m_sr| / (F K),
and the multi-resolution loss is the mean over the resolutions.  Gradient in sr only.  At the non-smooth points, by definition: a
first term whose numerator is 0 contributes exactly 0, a bin with ln m_hr == ln m_sr contributes 0, a bin with p_sr < 1e-7
contributes 0.

1. The yardstick: that definition under torch.stft + autograd in float64 and float32 (mrstft_autograd), and the kernels' two-stage
   algorithm restated in float64 numpy (one window-weighted gradient frame per frame, then test_lsd_loss_host.gather); the two
   agree to 1e-11 of the largest element.
2. The bars of tests/test_mrstft_loss_gpu.py have teeth: the restatement without the reflection, without the second window
   product, with the clamp left out and with the sign dropped from the L1 term each miss the gradient bar (four times the
   error of float32 CPU autograd) by more than 10x on every case; the spectral-convergence denominator taken from sr misses the
   forward's 2e-4 bound by more than 100x (the gradient bar does not see it: see the test).
3. The inputs of the GPU test are tie-free on the float64 reference: every bin has |ln m_hr - ln m_sr| >= 1e-6 or exactly 0, and
   no p lies within 1e-3 (relative) of the clamp -- otherwise a sign or clamp decision taken in float32 is a coin toss.
4. The exact-zero cases.  5. --lambda_mrstft parses and the model's refusals.  6. Header, bindings, exports, argument errors.
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

import test_lsd_loss_host as H

REPO = H.REPO
CLAMP = 1e-7
DEFAULT = ((512, 128), (1024, 256), (2048, 512))
NEW = ("mg_stft_loss_rows_workspace", "mg_stft_loss_rows", "mg_stft_loss_rows_backward_workspace", "mg_stft_loss_rows_backward",
       "mg_stft_loss_rows_backward_seeded", "mg_stft_loss_mean")


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def hann32(n_fft):
    """the float32 window the kernels multiply with: periodic Hann in float64, rounded once"""
    n = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)).astype(np.float32)


def _spectrum(a, n_fft, hop, dtype, center=True):
    w = torch.from_numpy(hann32(n_fft)).to(dtype)
    return torch.stft(a, n_fft, hop_length=hop, win_length=n_fft, window=w, center=center, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)


def mrstft_autograd(hr, sr, resolutions, dtype, center=True):
    """The definition for one utterance in `dtype` on the CPU -> (loss, d loss / d sr, [loss per resolution]), float64 numpy.
    hr, sr: float32 numpy.  (re^2 + im^2, not abs()^2: abs has no gradient at 0.  torch's clamp passes no gradient below the bound,
    its abs has sign(0) = 0; the 0 / 0 of sqrt at A == 0 is the one convention stated by hand.)"""
    x = torch.from_numpy(sr).to(dtype).requires_grad_()
    h = torch.from_numpy(hr).to(dtype)
    per = []
    for n_fft, hop in resolutions:
        def mag(a):
            s = _spectrum(a, n_fft, hop, dtype, center)
            return torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=CLAMP))
        mh, ms = mag(h), mag(x)
        A, B = ((mh - ms) ** 2).sum(), (mh ** 2).sum()
        l1 = (torch.log(mh) - torch.log(ms)).abs().sum() / mh.numel()
        per.append(l1 + torch.sqrt(A / B) if float(A.detach()) > 0 else l1)
    loss = sum(per) / len(per)
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), g.double().numpy(), [float(p.detach()) for p in per]


def frame_gradients(hr, sr, n_fft, hop, upstream=1.0, second_window=True, den_from_sr=False, clamp=True, sign=True):
    """Stage one of the kernels in float64: [frames, n_fft], frame f = y_f[n] window[n], y_f the gradient of upstream * loss with
    respect to the windowed frame f of sr.  The keyword arguments are the faults of test 2."""
    w = hann32(n_fft).astype(np.float64)
    M = n_fft // 2

    def spectra(x):
        x = np.pad(x.astype(np.float64), (M, M), mode="reflect")
        F = 1 + (len(x) - n_fft) // hop
        return np.fft.rfft(x[hop * np.arange(F)[:, None] + np.arange(n_fft)[None, :]] * w, axis=-1)
    Xh, Xs = spectra(hr), spectra(sr)
    ph, ps = np.abs(Xh) ** 2, np.abs(Xs) ** 2
    floor = CLAMP if clamp else 1e-300
    mh, ms = np.sqrt(np.maximum(ph, floor)), np.sqrt(np.maximum(ps, floor))
    A, B = ((mh - ms) ** 2).sum(), ((ms if den_from_sr else mh) ** 2).sum()
    dl = np.log(mh) - np.log(ms)
    sg = np.sign(dl) if sign else np.ones_like(dl)
    c_sc = upstream / math.sqrt(A * B) if A > 0 else 0.0
    c = (c_sc * (ms - mh) - (upstream / mh.size) * sg / ms) / ms
    c[ps < floor] = 0.0
    G = c * Xs
    Hs = G / 2
    Hs[:, 0], Hs[:, M] = G[:, 0].real, G[:, M].real
    y = n_fft * np.fft.irfft(Hs, n=n_fft, axis=-1)
    return y * w if second_window else y


def mrstft_grad_two_stage(hr, sr, resolutions, **broken):
    reflected = broken.pop("reflected", True)
    out = np.zeros(len(sr))
    for n_fft, hop in resolutions:
        frames = frame_gradients(hr, sr, n_fft, hop, upstream=1.0 / len(resolutions), **broken)
        out += H.gather(frames, len(sr), n_fft, hop, True, reflected=reflected)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the inputs (shared with tests/test_mrstft_loss_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
MIXES = {"below": (0.6, 0.2), "above": (1.5, 0.3), "mixed": (1.0, 0.7)}
KINDS = list(MIXES) + ["tone"]


def signal_pair(kind, n, seed, n_fft):
    """float32 (hr, sr).  Noise of amplitude 0.1 with sr = a hr + b delay(hr, 1): mostly below, mostly above, mixed signs of
    ln m_hr - ln m_sr.  Tone: hr 0.5 sin at bin 37.3 of an n_fft transform, sr 0.4 sin there plus 0.05 sin at bin 90.7 (about half
    of the bins sit under the clamp)."""
    if kind == "tone":
        t = np.arange(n, dtype=np.float64)
        hr = 0.5 * np.sin(2 * np.pi * 37.3 * t / n_fft)
        sr = 0.4 * np.sin(2 * np.pi * 37.3 * t / n_fft) + 0.05 * np.sin(2 * np.pi * 90.7 * t / n_fft)
        return hr.astype(np.float32), sr.astype(np.float32)
    a, b = MIXES[kind]
    hr = (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    delayed = np.concatenate([[0.0], hr[:-1].astype(np.float64)])
    return hr, (a * hr.astype(np.float64) + b * delayed).astype(np.float32)


LENGTHS = {512: [257, 300, 1500, 2560, 4097], 1024: [513, 3001, 2560, 5000, 1025], 2048: [1025, 5000, 4096, 2049, 6001]}
SEED0 = {512: 5120, 1024: 10240, 2048: 20480, "mean": 77}      # utterance u of kind k: SEED0 + 16 k + u (chosen: test 3 holds)
MEAN_LENGTHS = LENGTHS[2048]                                   # every one longer than 1024: all three default resolutions


def gpu_pairs(which, kind):
    """The five utterances of one launch of the GPU test: which = 512 / 1024 / 2048 (one resolution, hop N/4 or N/2) or "mean" (the
    three default resolutions)."""
    lengths = MEAN_LENGTHS if which == "mean" else LENGTHS[which]
    n_fft = 1024 if which == "mean" else which
    return [signal_pair(kind, n, SEED0[which] + 16 * KINDS.index(kind) + u, n_fft) for u, n in enumerate(lengths)]


def gpu_resolutions(which):
    return [DEFAULT] if which == "mean" else [((which, which // 4),), ((which, which // 2),)]


def tie_margins(hr, sr, n_fft, hop):
    """float64 -> (smallest non-zero |ln m_hr - ln m_sr|, smallest relative distance of a p (hr's or sr's) to the clamp, fraction of
    positive signs, fraction of clamped sr bins)"""
    with torch.no_grad():
        sh = _spectrum(torch.from_numpy(hr).double(), n_fft, hop, torch.float64)
        ss = _spectrum(torch.from_numpy(sr).double(), n_fft, hop, torch.float64)
    ph, ps = (sh.real ** 2 + sh.imag ** 2).numpy(), (ss.real ** 2 + ss.imag ** 2).numpy()
    dl = 0.5 * (np.log(np.maximum(ph, CLAMP)) - np.log(np.maximum(ps, CLAMP)))
    nz = np.abs(dl[dl != 0.0])
    return (float(nz.min()) if nz.size else math.inf, float(min(np.abs(ps / CLAMP - 1.0).min(), np.abs(ph / CLAMP - 1.0).min())), float((dl > 0).mean()),
            float((ps < CLAMP).mean()))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the two-stage restatement against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------
HOST_CASES = [(n_fft, n) for n_fft in (512, 1024, 2048) for n in (n_fft // 2 + 1, n_fft + 300)]


@pytest.mark.parametrize("n_fft,n", HOST_CASES)
def test_two_stage_restatement_equals_float64_autograd(n_fft, n):
    res = ((n_fft, n_fft // 4),)
    for kind in KINDS:
        hr, sr = signal_pair(kind, n, n_fft + n, n_fft)
        loss, want, _ = mrstft_autograd(hr, sr, res, torch.float64)
        got = mrstft_grad_two_stage(hr, sr, res)
        err = H.rel_err(got, want)
        print("restatement N=%d T=%d %s: loss %.4f, error %.2e of the largest element" % (n_fft, n, kind, loss, err))
        assert np.all(np.isfinite(got)) and err <= 1e-11, (kind, err)


def test_two_stage_restatement_of_the_three_resolution_mean():
    hr, sr = signal_pair("mixed", 1500, 3, 1024)
    _, want, per = mrstft_autograd(hr, sr, DEFAULT, torch.float64)
    assert len(per) == 3 and H.rel_err(mrstft_grad_two_stage(hr, sr, DEFAULT), want) <= 1e-11


# ---------------------------------------------------------------------------------------------------------------------
# 2. the GPU bar has teeth
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = [{"reflected": False}, {"second_window": False}, {"clamp": False}, {"sign": False}]


def loss_with_denominator_from_sr(hr, sr, n_fft, hop):
    """the loss of one resolution in float64 numpy, right and with sum m_sr^2 under the spectral convergence"""
    with torch.no_grad():
        mags = []
        for a in (hr, sr):
            s = _spectrum(torch.from_numpy(a).double(), n_fft, hop, torch.float64)
            mags.append(np.sqrt(np.maximum((s.real ** 2 + s.imag ** 2).numpy(), CLAMP)))
    mh, ms = mags
    A, l1 = ((mh - ms) ** 2).sum(), np.abs(np.log(mh) - np.log(ms)).mean()
    return l1 + math.sqrt(A / (mh ** 2).sum()), l1 + math.sqrt(A / (ms ** 2).sum())


@pytest.mark.parametrize("n_fft,n", HOST_CASES)
def test_gpu_bars_reject_every_fault(n_fft, n):
    """Per case the gradient bar is 4 e32, e32 the error of float32 CPU autograd against float64.  A restatement without the
    reflected taps, without the second window product, without the clamp or without the sign misses it by more than 10x on every
    case (leaving the clamp out changes nothing where no sr bin lies under it: measured on the cases that have such bins -- every
    tone pair does).  Smallest factors measured over these cases: reflection 24 (tone) and 149 (noise), window 297, clamp 901,
    sign 12.7 (the "mixed" noise, where half of the signs are right by chance).
    The FIFTH fault, the spectral-convergence denominator taken from sr, is NOT the gradient bar's to catch: the 1/m weights of
    the L1 term dominate the largest element, and the max-norm error of a wrong denominator lies between 0.01 (a tone) and 5000
    times the bar, below the bar on two tone cases.  The kernels read the denominator that the forward stored (row_sums), so it is the forward's bound that has the
    teeth: a loss with sum m_sr^2 in the denominator misses the 2e-4 relative bound of the GPU test by more than 100x."""
    res = ((n_fft, n_fft // 4),)
    for kind in KINDS:
        hr, sr = signal_pair(kind, n, n_fft + n, n_fft)
        _, g64, _ = mrstft_autograd(hr, sr, res, torch.float64)
        _, g32, _ = mrstft_autograd(hr, sr, res, torch.float32)
        bar = 4 * H.rel_err(g32, g64)
        assert 0 < bar < 1.0           # (a yardstick of 1 would let an all-zero gradient pass; e32 varies between hosts, up to 1e-2 here)
        assert H.rel_err(mrstft_grad_two_stage(hr, sr, res), g64) <= bar
        clamped = tie_margins(hr, sr, *res[0])[3]
        for broken in FAULTS:
            if "clamp" in broken and clamped == 0.0:
                continue
            miss = H.rel_err(mrstft_grad_two_stage(hr, sr, res, **broken), g64) / bar
            print("gradient bar %.2e | N=%d T=%d %s | %s | error / bar %.3g" % (bar, n_fft, n, kind, broken, miss))
            assert miss > 10, (kind, broken, miss)
        right, wrong = loss_with_denominator_from_sr(hr, sr, *res[0])
        miss = abs(wrong - right) / (2e-4 * right)
        g_miss = H.rel_err(mrstft_grad_two_stage(hr, sr, res, den_from_sr=True), g64) / bar
        print("forward bound 2e-4 | N=%d T=%d %s | denominator from sr | error / bound %.3g (gradient: error / bar %.3g)"
              % (n_fft, n, kind, miss, g_miss))
        assert miss > 100, (kind, miss)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the inputs are tie-free
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [512, 1024, 2048, "mean"])
def test_gpu_inputs_are_tie_free(which):
    worst_ln, worst_p = math.inf, math.inf
    for kind in KINDS:
        for hr, sr in gpu_pairs(which, kind):
            for res in gpu_resolutions(which):
                for n_fft, hop in res:
                    ln, p, pos, under = tie_margins(hr, sr, n_fft, hop)
                    worst_ln, worst_p = min(worst_ln, ln), min(worst_p, p)
                    assert ln >= 1e-6 and p >= 1e-3, (which, kind, len(hr), n_fft, hop, ln, p)
    print("tie margins %s: smallest |ln m_hr - ln m_sr| %.3g, smallest |p / clamp - 1| %.3g" % (which, worst_ln, worst_p))


def test_float32_autograd_takes_the_noise_decisions_as_float64_does():
    """N in {512, 1024, 2048}, hop N/4, lengths N/2 + 1, N + 300, 5N + 1.  On the noise constructions float32 CPU autograd takes every
    sign (of the bins that are not clamped) and every clamp decision as float64 does.  On the tone pair it does NOT, margins or
    no margins: the skirt of a 0.5 tone lies eleven decades of power above the clamp, so float32's error on a bin near the clamp
    is percents of the bin (measured: 5 signs flip over these nine tone cases, no clamp decision).  That is the heavy tail of e32
    on the tone cases, and why the GPU test takes the largest e32 of a launch as its yardstick."""
    flips = {"noise": 0, "tone": 0}
    for n_fft in (512, 1024, 2048):
        for n in (n_fft // 2 + 1, n_fft + 300, 5 * n_fft + 1):
            for kind in KINDS:
                hr, sr = signal_pair(kind, n, n_fft + n, n_fft)
                seen = []
                for dtype in (torch.float64, torch.float32):
                    with torch.no_grad():
                        ph, ps = (_spectrum(torch.from_numpy(a).to(dtype), n_fft, n_fft // 4, dtype) for a in (hr, sr))
                        ph, ps = (ph.real ** 2 + ph.imag ** 2).numpy(), (ps.real ** 2 + ps.imag ** 2).numpy()
                    seen.append((np.sign(np.log(np.maximum(ph, CLAMP)) - np.log(np.maximum(ps, CLAMP))), ps < CLAMP))
                live = ~seen[0][1] & ~seen[1][1]
                flips["tone" if kind == "tone" else "noise"] += (int(((seen[0][0] != seen[1][0]) & live).sum())
                                                                 + int((seen[0][1] != seen[1][1]).sum()))
    print("float32 against float64 decisions that differ: %s" % flips)
    assert flips["noise"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. the exact zeros
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_zero_cases():
    res = ((512, 128),)
    hr, _ = signal_pair("mixed", 1500, 3, 512)
    zero = np.zeros(1500, np.float32)
    for a, b, loss_is_zero in ((hr, hr.copy(), True), (zero, zero, True), (hr, zero, False)):
        loss, g, _ = mrstft_autograd(a, b, res, torch.float64)
        two = mrstft_grad_two_stage(a, b, res)
        assert np.all(g == 0.0) and np.all(two == 0.0) and math.isfinite(loss)
        assert (loss == 0.0) if loss_is_zero else (loss > 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the option and the model's refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_and_defaults_to_zero():
    from mdctgan_amd.options import make_opt
    assert make_opt("--lambda_mrstft", "0.25").lambda_mrstft == 0.25
    assert make_opt().lambda_mrstft == 0.0 and make_opt().lambda_lsd == 0.0


def test_loss_filter_places_the_term_after_the_lsd():
    from mdctgan_amd.pix2pixHD_model import Pix2PixHDModel
    with_feat, without = types.SimpleNamespace(no_ganFeat_loss=False), types.SimpleNamespace(no_ganFeat_loss=True)
    assert Pix2PixHDModel.loss_filter(with_feat, 1, 2, 3, 4) == [1, 2, 3, 4]
    assert Pix2PixHDModel.loss_filter(with_feat, 1, 2, 3, 4, 5, 6) == [1, 2, 5, 6, 3, 4]
    assert Pix2PixHDModel.loss_filter(without, 1, 2, 3, 4, g_mrstft=6) == [1, 6, 3, 4]


def _check(in_kernel=True, n_fft=512, hop=256, **over):
    from mdctgan_amd.pix2pixHD_model import Audio2MDCT, Pix2PixHDModel
    pre = types.SimpleNamespace(_in_kernel=in_kernel, win_length=n_fft, hop_length=hop)
    pre.audio_length = lambda T: Audio2MDCT.audio_length(pre, T)
    opt = types.SimpleNamespace(**dict(dict(lambda_mrstft=1.0, segment_length=7936), **over))
    return Pix2PixHDModel._check_lambda_mrstft(types.SimpleNamespace(preprocess=pre), opt)


def test_refusals_when_the_model_is_built():
    assert _check() == 1.0 and _check(lambda_mrstft=0.25) == 0.25
    # the term has its own transforms: codec sizes that --lambda_lsd refuses are served
    assert _check(n_fft=2048, hop=1024) == 1.0 and _check(n_fft=128, hop=64) == 1.0
    # 0 switches the term off whatever else is set: the default path checks nothing new
    assert _check(in_kernel=False, lambda_mrstft=0.0, segment_length=16) == 0.0
    for bad in (-1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="lambda_mrstft"):
            _check(lambda_mrstft=bad)
    with pytest.raises(NotImplementedError, match="lambda_mrstft"):
        _check(in_kernel=False)                                         # the dB and explicit-encoding codecs
    for short in (1024, 768, 256):                                      # decoded clips of at most 1024 samples
        with pytest.raises(ValueError, match="lambda_mrstft.*segment_length"):
            _check(segment_length=short)
    assert _check(segment_length=1280) == 1.0


def test_too_short_an_utterance_names_utterance_and_resolution():
    from mdctgan_amd.metrics import STFT_RESOLUTIONS, plan_mrstft
    assert STFT_RESOLUTIONS == DEFAULT
    assert [p.frames for p in plan_mrstft([1025, 3000])] == [[9, 24], [5, 12], [3, 6]]
    with pytest.raises(ValueError, match=r"resolution \(2048, 512\): utterance 1"):
        plan_mrstft([3000, 1024])
    with pytest.raises(ValueError, match=r"resolution \(512, 128\): utterance 0"):
        plan_mrstft([256, 3000])
    with pytest.raises(NotImplementedError):
        plan_mrstft([3000], ((256, 64),))
    with pytest.raises(ValueError):
        plan_mrstft([3000], ((512, 0),))
    with pytest.raises(ValueError):
        plan_mrstft([3000], ())


# ---------------------------------------------------------------------------------------------------------------------
# 6. header, bindings, argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported():
    from mdctgan_amd import _lib
    text = open(os.path.join(REPO, "include", "mdctgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 4 and lib.mg_abi_version() == 4


P = 4096                         # a non-null, 16-byte aligned "pointer"
FRAMES, NFFT = 40, 1024
WS_F, WS_B = FRAMES * 3 * 8, FRAMES * NFFT * 4
# hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop, center, row_out, workspace, bytes, stream
FWD_GOOD = [P, 30000, P, 30000, P, 3, P, FRAMES, P, NFFT, 512, 1, P, P, WS_F, None]
FWD_BAD = [(0, None), (2, None), (4, None), (6, None), (8, None), (12, None), (13, None),                     # null pointers
           (9, 256), (9, 4096), (9, 1000), (9, 0),                                                            # other transform sizes
           (1, 0), (1, -5), (3, 0), (3, -5), (5, 0), (5, -1), (7, 0), (7, -3), (10, 0), (10, -512),           # counts, totals, hop
           (14, WS_F - 1), (14, 0), (13, P + 4)]                                                              # short / misaligned workspace
# ..., center, row_sums, grad_rows, accumulate, grad_sr, workspace, bytes, stream
BWD_GOOD = [P, 30000, P, 30000, P, 3, P, FRAMES, P, NFFT, 512, 1, P, P, 0, P, P, WS_B, None]
BWD_BAD = [(0, None), (2, None), (4, None), (6, None), (8, None), (12, None), (13, None), (15, None), (16, None),
           (9, 256), (9, 4096), (9, 1000), (9, 0),
           (1, 0), (1, -5), (3, 0), (3, -5), (5, 0), (5, -1), (7, 0), (7, -3), (10, 0), (10, -512),
           (17, WS_B - 1), (17, 0), (16, P + 4)]
# ..., center, row_sums, go, scale, n_res, accumulate, grad_sr, workspace, bytes, stream
SEED_GOOD = [P, 30000, P, 30000, P, 3, P, FRAMES, P, NFFT, 512, 1, P, P, 0.5, 3, 1, P, P, WS_B, None]
SEED_BAD = [(0, None), (2, None), (4, None), (6, None), (8, None), (12, None), (13, None), (17, None), (18, None),
            (9, 256), (9, 4096), (9, 1000), (9, 0),
            (1, 0), (1, -5), (3, 0), (3, -5), (5, 0), (5, -1), (7, 0), (7, -3), (10, 0), (10, -512), (15, 0), (15, -1),
            (19, WS_B - 1), (19, 0), (18, P + 4)]
# row_out, n_rows, n_res, scale, loss, stream
MEAN_GOOD = [P, 8, 3, 0.5, P, None]
MEAN_BAD = [(0, None), (4, None), (1, 0), (1, -7), (2, 0), (2, -1)]
JOBS = [["mg_stft_loss_rows", FWD_GOOD, FWD_BAD], ["mg_stft_loss_rows_backward", BWD_GOOD, BWD_BAD],
        ["mg_stft_loss_rows_backward_seeded", SEED_GOOD, SEED_BAD], ["mg_stft_loss_mean", MEAN_GOOD, MEAN_BAD]]

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
q, b = lib.mg_stft_loss_rows_workspace, lib.mg_stft_loss_rows_backward_workspace
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
