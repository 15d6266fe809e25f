"""The LSD loss without a GPU (metrics.lsd_many / lsd_loss, csrc/lsd_rows_grad.hip).

1. The two new entry points are declared in the header, bound in _lib.SIGNATURES and exported by the library; they reject null
   pointers, other transform sizes, non-positive counts, totals and hops and a short workspace with MG_ERR_ARG before any launch
   (child processes with arbitrary non-null integers as pointers, never dereferenced because the call returns first).
2. The two-stage algorithm of the kernels, restated here in float64 numpy -- stage one stores one window-weighted gradient frame
   per frame, stage two gathers every sample from its three candidate positions -- equals float64 autograd through
   torch.stft(pad_mode="reflect") of the reference's expression (util/util.py:171-175) to 1e-12 of the largest element.  This pins
   the adjoint of the reflection and the half weights of the bins 0 and N/2.
3. The bar of tests/test_lsd_loss_gpu.py (four times the error of float32 CPU autograd) has teeth: the restatement without the
   reflected candidates, and the one without the second window product, each miss it by more than 100x.
4. sr == hr gives an all-zero, finite gradient, where autograd has NaN.
"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MG_ERR_ARG = -1
NEW = ("mg_lsd_rows_backward_workspace", "mg_lsd_rows_backward")


# ---------------------------------------------------------------------------------------------------------------------
# the reference's expression under autograd, and the restatement of the two kernels
# ---------------------------------------------------------------------------------------------------------------------
def window32(n_fft):
    """the float32 window the kernels multiply with"""
    from mdctgan_amd.mdct import kbdwin
    return kbdwin(n_fft).to(torch.float32).numpy()


def lsd_autograd(hr, sr, window, n_fft, hop, center, dtype):
    """util/util.py:171-175 for one utterance in `dtype` on the CPU -> (lsd, d lsd / d sr), both float64 numpy.  hr, sr, window:
    float32 numpy."""
    w = torch.from_numpy(window).to(dtype)
    x = torch.from_numpy(sr).to(dtype).requires_grad_()

    def power(a):
        s = torch.stft(a, n_fft, hop_length=hop, win_length=n_fft, window=w, center=center, pad_mode="reflect",
                       normalized=False, onesided=True, return_complex=True)
        return s.abs().pow(2)                                          # aF.spectrogram(power=2): [bins, frames]
    d = torch.log10(power(torch.from_numpy(hr).to(dtype)) + 1e-6) - torch.log10(power(x) + 1e-6)
    lsd = torch.sqrt(torch.mean(d ** 2, dim=-2)).mean()
    (g,) = torch.autograd.grad(lsd, x)
    return float(lsd.detach()), g.double().numpy()


def frame_gradients(hr, sr, window, n_fft, hop, center, upstream=1.0, second_window=True):
    """Stage one in float64: [frames, n_fft], frame f = y_f[n] window[n] with y_f the gradient of upstream * mean_f L_f with
    respect to the windowed frame f of sr.  A frame with L_f == 0 contributes exactly 0."""
    w = window.astype(np.float64)
    M, NB = n_fft // 2, n_fft // 2 + 1

    def spectra(x):
        x = x.astype(np.float64)
        if center:
            x = np.pad(x, (M, M), mode="reflect")
        F = 1 + (len(x) - n_fft) // hop
        return np.fft.rfft(x[hop * np.arange(F)[:, None] + np.arange(n_fft)[None, :]] * w, axis=-1)
    Xh, Xs = spectra(hr), spectra(sr)
    ph, ps = np.abs(Xh) ** 2, np.abs(Xs) ** 2
    d = np.log10(ph + 1e-6) - np.log10(ps + 1e-6)
    L = np.sqrt((d ** 2).sum(-1) / NB)
    g_f = upstream / len(L)
    live = L > 0
    c = np.zeros_like(d)
    c[live] = -g_f * d[live] / (L[live, None] * NB * math.log(10.0) * (ps[live] + 1e-6))
    G = 2 * c * Xs
    # y[n] = Re sum_{k=0..N/2} G_k exp(+2 pi i k n / N) = N irfft(H), H = G / 2 inside, Re G at k = 0 and N/2
    H = G / 2
    H[:, 0], H[:, M] = G[:, 0].real, G[:, M].real
    y = n_fft * np.fft.irfft(H, n=n_fft, axis=-1)
    return y * w if second_window else y


def gather(frames, length, n_fft, hop, center, reflected=True):
    """Stage two in float64: sample t sums the taps that framing mapped to it -- the direct position, then (centred) -t for
    1 <= t <= N/2, then 2 (len - 1) - t for t < len - 1 inside the right padding; per candidate every covering frame, ascending."""
    nf, half = frames.shape[0], n_fft // 2
    off = half if center else 0
    out = np.zeros(length)
    for t in range(length):
        cand = [t]
        if center and reflected:
            if 1 <= t <= half:
                cand.append(-t)
            r = 2 * (length - 1) - t
            if t < length - 1 and r <= length - 1 + half:
                cand.append(r)
        acc = 0.0
        for r in cand:
            q = r + off                                                    # position in the padded row
            for f in range(max(0, -((n_fft - 1 - q) // hop)), min(nf - 1, q // hop) + 1):
                acc += frames[f, q - f * hop]
        out[t] = acc
    return out


def lsd_grad_two_stage(hr, sr, window, n_fft, hop, center, **broken):
    frames = frame_gradients(hr, sr, window, n_fft, hop, center, second_window=broken.get("second_window", True))
    return gather(frames, len(sr), n_fft, hop, center, reflected=broken.get("reflected", True))


def rel_err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def host_pair(n, seed):
    rng = np.random.default_rng(seed)
    hr = 0.1 * rng.standard_normal(n)
    return hr.astype(np.float32), (hr + 0.01 * rng.standard_normal(n)).astype(np.float32)


HOST_LENGTHS = [257, 300, 1500, 2560]            # 257: the shortest legal centred length (two frames); 2560: a multiple of hop


# ---------------------------------------------------------------------------------------------------------------------
# 1. header, bindings, argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported():
    from mdctgan_amd import _lib
    text = open(os.path.join(REPO, "include", "mdctgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    # the binding's argument count is the declaration's
    for name in NEW:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 4 and lib.mg_abi_version() == 4


P = 4096                         # a non-null, 16-byte aligned "pointer"
FRAMES, NFFT = 40, 1024
WS = FRAMES * NFFT * 4
# hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, hr_shift, window, n_fft, hop, center, grad_rows, grad_sr,
# workspace, workspace_bytes, stream
GOOD = [P, 30000, P, 30000, P, 3, P, FRAMES, None, P, NFFT, 512, 1, P, P, P, WS, None]
BAD = [(0, None), (2, None), (4, None), (6, None), (9, None), (13, None), (14, None), (15, None),          # null pointers
       (10, 256), (10, 4096), (10, 1000), (10, 0),                                                       # other transform sizes
       (1, 0), (1, -5), (3, 0), (3, -5), (5, 0), (5, -1), (7, 0), (7, -3), (11, 0), (11, -512),          # counts, totals, hop
       (16, WS - 1), (16, 0), (15, P + 4)]                                                               # short / misaligned workspace

CHILD = """
import json, sys
sys.path.insert(0, %r)
from mdctgan_amd import _lib
lib = _lib.load()
good, bad = json.loads(sys.argv[1])
for pos, value in bad:
    args = list(good)
    args[pos] = value
    print("rc %%d %%d" %% (pos, lib.mg_lsd_rows_backward(*args)), flush=True)
q = lib.mg_lsd_rows_backward_workspace
print("ws %%d %%d %%d %%d %%d" %% (q(40, 1024), q(0, 1024), q(-1, 512), q(40, 4096), q(7, 512)))
""" % REPO


@pytest.fixture(scope="module")
def child():
    import json
    p = subprocess.run([sys.executable, "-c", CHILD, json.dumps([GOOD, BAD])], capture_output=True, text=True, cwd=REPO, timeout=300)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("case", range(len(BAD)), ids=["%d=%s" % pv for pv in BAD])
def test_backward_rejects_bad_arguments(child, case):
    rc, out, errtxt = child
    assert rc == 0, "child exit status %d\n%s" % (rc, errtxt[-2000:])
    lines = [ln.split() for ln in out.splitlines() if ln.startswith("rc ")]
    assert len(lines) == len(BAD)
    assert lines[case] == ["rc", str(BAD[case][0]), str(MG_ERR_ARG)]


def test_backward_workspace_query(child):
    _, out, _ = child
    ws = [ln.split() for ln in out.splitlines() if ln.startswith("ws ")]
    assert ws == [["ws", str(WS), "0", "0", "0", str(7 * 512 * 4)]]          # one float32 frame of n_fft samples per frame


# ---------------------------------------------------------------------------------------------------------------------
# 2. the two-stage restatement against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("hop_div", [2, 4])
def test_two_stage_restatement_equals_float64_autograd(hop_div, center):
    n_fft, hop = 512, 512 // hop_div
    window = window32(n_fft)
    for n in HOST_LENGTHS:
        n = n if center else max(n, n_fft)
        hr, sr = host_pair(n, n + hop + center)
        lsd, want = lsd_autograd(hr, sr, window, n_fft, hop, center, torch.float64)
        got = lsd_grad_two_stage(hr, sr, window, n_fft, hop, center)
        err = rel_err(got, want)
        print("restatement N=%d hop=%d center=%d T=%d: lsd %.4f, error %.2e of the largest element" % (n_fft, hop, center, n, lsd, err))
        assert np.all(np.isfinite(got)) and err <= 1e-12, (n, err)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the GPU bar has teeth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 1500])
def test_gpu_bar_rejects_a_missing_reflection_and_a_missing_window(n):
    n_fft, hop, center = 512, 256, True
    window = window32(n_fft)
    hr, sr = host_pair(n, 7 + n)
    _, g64 = lsd_autograd(hr, sr, window, n_fft, hop, center, torch.float64)
    _, g32 = lsd_autograd(hr, sr, window, n_fft, hop, center, torch.float32)
    bar = 4 * rel_err(g32, g64)
    assert 0 < bar < 1e-3
    assert rel_err(lsd_grad_two_stage(hr, sr, window, n_fft, hop, center), g64) <= bar
    for broken in ({"reflected": False}, {"second_window": False}):
        miss = rel_err(lsd_grad_two_stage(hr, sr, window, n_fft, hop, center, **broken), g64) / bar
        print("GPU bar %.2e | T=%d | %s | error / bar %.3g" % (bar, n, broken, miss))
        assert miss > 100, (broken, miss)


# ---------------------------------------------------------------------------------------------------------------------
# 4. sr == hr
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("center", [True, False])
def test_equal_signals_give_a_zero_gradient(center):
    n_fft, hop = 512, 128
    hr, _ = host_pair(1500, 3)
    got = lsd_grad_two_stage(hr, hr.copy(), window32(n_fft), n_fft, hop, center)
    assert got.shape == (1500,) and np.all(np.isfinite(got)) and np.all(got == 0.0)
    zero = np.zeros(1500, np.float32)
    got = lsd_grad_two_stage(zero, zero, window32(n_fft), n_fft, hop, center)
    assert np.all(got == 0.0)
