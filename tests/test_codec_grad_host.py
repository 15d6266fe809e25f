"""The adjoint identities the backward passes of MDCT4 / IMDCT4 rely on (mdctgan_amd/mdct.py: imdct4_backward / mdct4_backward,
csrc/mdct_ct.h: the backward kernels), checked on the float64 oracle with dense Jacobians.  CPU only.

* win == 2 hop:  IMDCT4^T(gy) = 4/N MDCT4(gy)  (gy zero past out_length, the forward's frame count)  and
  MDCT4^T(gX) = N/4 IMDCT4(gX) cropped to T -- exact.
* hop != win / 2: that shortcut fails (the IMDCT crops win // 2, the MDCT pads hop); the explicit adjoint holds everywhere:
  IMDCT4^T = frames of gy with start padding win // 2 (centre), window, x C, x 4/N;  MDCT4^T = x C^T, window, overlap-add with
  crop hop (centre), length T.
The hop = win / 4 family of the class default 2048 / 512 / 2048 runs at 1024 / 256 / 1024 and 512 / 128 / 512 here: the same
structure at a fraction of the dense Jacobians' host time (tests/test_codec_grad_gpu.py runs 2048 / 512 / 2048 on the kernels)."""
import numpy as np
import pytest

from oracle import transform as T


def jac_mdct(t, w, n_fft, hop, center=True):
    """d MDCT4(x) / dx as [F * M, t] (the transform is linear; a unit impulse times a float32 window is exact)."""
    X, _ = T.mdct4(np.eye(t, dtype=np.float32), w, n_fft, hop, center)
    return X.reshape(t, -1).T


def jac_imdct(F, w, n_fft, hop, center=True, out_length=None):
    """d IMDCT4(spec) / d spec as [T_out, F * M]."""
    m = n_fft // 2
    y, _ = T.imdct4(np.eye(F * m).reshape(F * m, F, m), w, n_fft, hop, center, out_length)
    return y[:, 0, 0, :].T


def imdct_adjoint(gy, w, n_fft, hop, F, center=True):
    """The explicit IMDCT4^T: frame gy [B, T_out] with start padding win // 2, window, contract with C, scale 4/N."""
    win = len(w)
    start = win // 2 if center else 0
    gp = np.pad(gy, [(0, 0), (start, (F - 1) * hop + win)])
    idx = np.arange(win)[None, :] + hop * np.arange(F)[:, None]
    frames = gp[:, idx] * np.asarray(w, np.float64)
    return 4.0 / n_fft * frames @ T.mdct_matrix(n_fft)[:win]


def mdct_adjoint(gX, w, n_fft, hop, t, center=True):
    """The explicit MDCT4^T: contract gX [B, F, M] with C^T, window, overlap-add, crop the MDCT's start padding, length t."""
    win = len(w)
    z = (gX @ T.mdct_matrix(n_fft)[:win].T) * np.asarray(w, np.float64)
    B, F, _ = z.shape
    full = np.zeros((B, (F - 1) * hop + win + t))
    for f in range(F):
        full[:, f * hop:f * hop + win] += z[:, f]
    start = hop if center else 0
    return full[:, start:start + t]


@pytest.mark.parametrize("n_fft,hop,win", [(512, 256, 512), (1024, 256, 512)])
def test_raw_transforms_are_adjoint_up_to_scale_when_win_is_two_hops(n_fft, hop, win):
    w = T.kbd_window(win)
    t = 1024
    A = jac_mdct(t, w, n_fft, hop)
    F = A.shape[0] // (n_fft // 2)
    S = jac_imdct(F, w, n_fft, hop)
    assert S.shape == (t, F * n_fft // 2)             # (F - 1) hop + win - win == t
    assert np.abs(S.T - 4.0 / n_fft * A).max() == 0.0
    # out_length: the rows past it are zero gradient, i.e. the MDCT of gy padded with zeros
    S2 = jac_imdct(F, w, n_fft, hop, out_length=768)
    assert np.abs(S2.T - 4.0 / n_fft * A[:, :768]).max() == 0.0


@pytest.mark.parametrize("n_fft,hop,win", [(1024, 256, 1024), (512, 128, 512)])
def test_shortcut_fails_when_hop_is_not_half_the_window(n_fft, hop, win):
    w = T.kbd_window(win)
    t = max(1024, n_fft)
    A = jac_mdct(t, w, n_fft, hop)
    F = A.shape[0] // (n_fft // 2)
    S = jac_imdct(F, w, n_fft, hop)
    n = min(S.shape[0], t)
    assert np.abs(S[:n].T - 4.0 / n_fft * A[:, :n]).max() > 1e-3 * np.abs(A).max() * 4.0 / n_fft


@pytest.mark.parametrize("n_fft,hop,win,center", [(512, 256, 512, True), (1024, 256, 512, True), (1024, 256, 1024, True),
                                                  (512, 128, 512, True), (512, 256, 512, False), (1024, 256, 512, False)])
def test_explicit_adjoints_equal_the_dense_jacobians(n_fft, hop, win, center):
    rng = np.random.default_rng(n_fft + hop + win + center)
    w = T.kbd_window(win)
    t = max(1024, n_fft)
    A = jac_mdct(t, w, n_fft, hop, center)
    m = n_fft // 2
    F = A.shape[0] // m
    S = jac_imdct(F, w, n_fft, hop, center)
    gy = rng.standard_normal((2, S.shape[0]))
    got = imdct_adjoint(gy, w, n_fft, hop, F, center).reshape(2, -1)
    want = gy @ S
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    gX = rng.standard_normal((2, F, m))
    got = mdct_adjoint(gX, w, n_fft, hop, t, center)
    want = gX.reshape(2, -1) @ A
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
