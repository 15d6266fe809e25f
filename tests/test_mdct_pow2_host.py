"""K1' / K2' (csrc/mdct_pow2.hip) without a GPU: the C ABI carries the new entry points, the host query and the `.fast`
attribute route the right geometries, and the decomposition the kernels run -- TDAC fold, pre-twiddle, Stockham stages with the
radices and the twiddle tables the library hands out (mg_mdct_pow2_twiddles, before their one rounding to float32), post-twiddle --
reproduces oracle.transform.mdct4_folded in float64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mdctgan_amd import _lib
from oracle import transform as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mg_mdct_pow2_supported", "mg_mdct_pow2_twiddle_floats", "mg_mdct_pow2_twiddles", "mg_mdct4_pow2_forward",
       "mg_imdct4_pow2_forward", "mg_imdct4_pow2_stitched"]


def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "mdctgan_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW:
            assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 4


def test_supported_geometries():
    lib = _lib.load()
    for g in ((256, 128, 256), (1024, 512, 1024), (2048, 1024, 2048)):
        assert lib.mg_mdct_pow2_supported(*g, 1) == 1, g
        assert lib.mg_mdct_pow2_supported(*g, 0) == 0, g
        assert lib.mg_mdct_pow2_twiddle_floats(g[0]) == 3 * g[0] // 2
    for g in ((512, 256, 512), (1024, 256, 512), (2048, 512, 2048), (1000, 500, 1000)):
        assert lib.mg_mdct_pow2_supported(*g, 1) == 0, g
    assert lib.mg_mdct_pow2_twiddle_floats(512) == 0
    assert lib.mg_mdct_pow2_twiddles(512, ctypes.c_void_p(torch.empty(8).data_ptr()), 0) == -2      # MG_ERR_UNSUPPORTED


def test_fast_attribute_follows_the_switch(monkeypatch):
    from mdctgan_amd.mdct import IMDCT4, MDCT4, kbdwin
    monkeypatch.delenv("MG_MDCT_POW2", raising=False)
    for cls in (MDCT4, IMDCT4):
        m = cls(2048, 1024, 2048, kbdwin, device="cpu")
        assert m.fused is False and m.fast is True
        monkeypatch.setenv("MG_MDCT_POW2", "0")
        assert m.fused is False and m.fast is False
        monkeypatch.delenv("MG_MDCT_POW2")
        assert m.fast is True
        assert cls(512, 256, 512, kbdwin, device="cpu").fast is False          # K1 / K2's geometry
        assert cls(512, 256, 512, kbdwin, device="cpu").fused is True
        assert cls(2048, 512, 2048, kbdwin, device="cpu").fast is False
        assert cls(1024, 512, 1024, kbdwin, center=False, device="cpu").fast is False


def test_audio2mdct_routes(monkeypatch):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import Audio2MDCT
    monkeypatch.delenv("MG_MDCT_POW2", raising=False)

    def pre(n_fft, hop, *extra):
        return Audio2MDCT(options.make_opt(*options.SPECTRAL_FLAGS, "--n_fft", n_fft, "--hop_length", hop, "--win_length", n_fft,
                                           "--lr_sampling_rate", "12000", *extra, gpu_ids=[]))
    p = pre(1024, 512)
    assert not p.fused and p.fast and p.fast_codec and p.has_stitched_decoder
    monkeypatch.setenv("MG_MDCT_POW2", "0")
    assert not p.fast and not p.has_stitched_decoder
    with pytest.raises(NotImplementedError, match="stitched decode"):
        p._to_audio(torch.zeros(1, 1, 3, 512), {"min": torch.zeros(1), "max": torch.ones(1)}, None, (torch.zeros(8), 0, 0))
    monkeypatch.delenv("MG_MDCT_POW2")
    q = pre(512, 256)
    assert q.fused and not q.fast and q.has_stitched_decoder
    assert not pre(1024, 256).fast


@pytest.mark.parametrize("n_fft", [256, 1024, 2048])
def test_decomposition_in_float64(n_fft):
    from mdctgan_amd.mdct import pow2_radices, pow2_twiddles_host
    M, N2 = n_fft // 2, n_fft // 4
    radices = pow2_radices(n_fft)
    assert int(np.prod(radices)) == N2 and all(r == 8 for r in radices[1:]) and radices[0] in (2, 4, 8)
    tw = pow2_twiddles_host(n_fft, torch.float64).numpy()
    # the device buffer is this table rounded once
    np.testing.assert_array_equal(pow2_twiddles_host(n_fft).numpy(), tw.astype(np.float32))
    pre, post, root = (t[:, 0] + 1j * t[:, 1] for t in tw)
    n = np.arange(N2)
    # (1e-15: the numpy value on the right rounds its unreduced argument, a few ulp of pi)
    assert np.abs(pre - np.exp(-1j * np.pi * (4 * n + 1) / (4 * M))).max() <= 1e-15
    assert np.abs(post - np.exp(-1j * np.pi * n / M)).max() <= 1e-15
    assert np.abs(root - np.exp(-2j * np.pi * n / N2)).max() <= 1e-15
    assert root[0] == 1 and root[N2 // 4] == -1j and post[0] == 1          # exact at the octant boundaries
    x = np.random.default_rng(n_fft).standard_normal((2, 6 * n_fft + 37)).astype(np.float32)
    w = T.kbd_window(n_fft)
    want = T.mdct4_folded(x, w, n_fft, M)
    frames = (T.frame_signal(x, n_fft, M, True) * w).astype(np.float32).astype(np.float64)
    u = T.tdac_fold(frames)
    a = (u[..., 0::2] + 1j * u[..., ::-1][..., 0::2]) * pre                 # c[n] = (u[2n] + i u[M-1-2n]) pre[n]
    ns = 1
    for R in radices:                                                       # pw_stage in csrc/mdct_pow2.hip
        nb = N2 // R
        j = np.arange(nb)
        k = j % ns
        v = np.stack([a[..., j + r * nb] * root[r * k * (N2 // (ns * R))] for r in range(R)], -1)
        wr = np.exp(-2j * np.pi * np.outer(np.arange(R), np.arange(R)) / R)
        o = v @ wr
        b = np.empty_like(a)
        d = (j // ns) * ns * R + k
        for r in range(R):
            b[..., d + r * ns] = o[..., r]
        a, ns = b, ns * R
    Y = a * post
    X = np.empty_like(u)
    X[..., 0::2] = Y.real
    X[..., ::-1][..., 0::2] = -Y.imag                                       # X[M-1-2k] = -Im Y[k]
    err = np.abs(X - want).max() / np.abs(want).max()
    assert err <= 1e-12, err
    # the DCT-IV is its own inverse up to 2 / M: the same stages decode (K2')
    assert np.abs(T.dct4_matrix(M) @ T.dct4_matrix(M) - np.eye(M) * M / 2).max() <= 1e-9
