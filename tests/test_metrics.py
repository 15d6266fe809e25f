"""F2: compute_matrics (util/util.py:132-177) -- oracle sanity on the CPU, the HIP path against the oracle on
the GPU.  The LSD's spectrogram is torchaudio's in the reference; torchaudio is not installed, the oracle restates it
through torch.stft (oracle/metrics.py header), so that term is pinned to torch.stft only."""
import types

import numpy as np
import pytest
import torch

from oracle import metrics as M


def _signals(B=3, T=32512, seed=0):
    rng = np.random.default_rng(seed)
    hr = 0.1 * rng.standard_normal((B, T))
    sr = hr + 0.01 * rng.standard_normal((B, T))
    lr = hr + 0.03 * rng.standard_normal((B, T))
    return hr.astype(np.float32), lr.astype(np.float32), sr.astype(np.float32)


def test_oracle_metrics_sanity():
    hr, lr, sr = _signals()
    mse, snr_sr, snr_lr, a, b, c, lsd = M.compute_matrics(hr, lr, sr)
    assert (a, b, c) == (0, 0, 0)
    assert abs(mse - 1e-4) < 1e-5                                  # noise variance 0.01^2
    assert abs(snr_sr - 20.0) < 0.2 and abs(snr_lr - 10.46) < 0.2     # 10 log10(0.1^2 / sigma^2)
    assert 0.05 < lsd < 0.5
    assert M.compute_matrics(hr, lr, hr + 0.0)[6] == 0.0
    p = M.spectrogram_power(hr, 1024, 512, 1024, np.ones(1024))
    assert p.shape == (3, 513, 64)
    # Parseval on one interior frame (rectangular window, onesided): sum_k c_k |X_k|^2 = N sum_n x_n^2
    x = hr[0, 512 * 4 - 512: 512 * 4 + 512].astype(np.float64)
    c = np.ones(513); c[1:-1] = 2.0
    assert abs((c * p[0, :, 4]).sum() - 1024 * (x ** 2).sum()) < 1e-6 * 1024 * (x ** 2).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("center", [True, False])
def test_compute_matrics_on_device(center):
    from mdctgan_amd.metrics import compute_matrics
    hr, lr, sr = _signals(seed=3)
    opt = types.SimpleNamespace(n_fft=512, hop_length=256, win_length=512, center=center)
    want = M.compute_matrics(hr, lr, sr, center=center)
    got = compute_matrics(torch.from_numpy(hr), torch.from_numpy(lr), torch.from_numpy(sr).to("cuda"), opt)
    assert len(got) == 7 and got[3:6] == (0, 0, 0)
    assert abs(got[0] - want[0]) <= 1e-5 * want[0]
    assert abs(got[1] - want[1]) <= 1e-4 and abs(got[2] - want[2]) <= 1e-4          # dB
    assert abs(got[6] - want[6]) <= 2e-4 * want[6]
    # 1-D waveforms (generate_audio.py:60 passes [1, n] / squeezed tensors)
    got1 = compute_matrics(torch.from_numpy(hr[0]), torch.from_numpy(lr[0]), torch.from_numpy(sr[0]).to("cuda"), opt)
    want1 = M.compute_matrics(hr[0], lr[0], sr[0], center=center)
    assert abs(got1[6] - want1[6]) <= 2e-4 * want1[6] and abs(got1[1] - want1[1]) <= 1e-4


@pytest.mark.gpu
def test_eval_model_loop(tmp_path):
    """train.py:104-134 on the device: inference + compute_matrics per batch, the five averaged columns, a CSV row per
    call, eval mode inside the loop and the previous mode restored -- checked against the per-batch metrics computed here
    from the model's own inference outputs."""
    from mdctgan_amd import options
    from mdctgan_amd.metrics import compute_matrics, eval_model
    from mdctgan_amd.pix2pixHD_model import create_model
    from oracle import nets as onets
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                           "--n_blocks_global", "2", "--n_blocks_attn_g", "1", "--heads_g", "2", "--dim_head_g", "8",
                           "--num_D", "2", "--ndf", "8", "--batchSize", "2", "--bins", "32", "--segment_length", "7936",
                           "--gpu_ids", "0", "--eval_size", "1")
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    rng = np.random.default_rng(1)
    batches = [{"LR_audio": torch.from_numpy(0.05 * rng.standard_normal((2, 7936)).astype(np.float32)),
                "HR_audio": torch.from_numpy(0.05 * rng.standard_normal((2, 7936)).astype(np.float32))} for _ in range(4)]
    path = str(tmp_path / "eval.csv")
    assert model.training
    res = eval_model(model, batches, opt, path)
    assert model.training                                   # restored
    assert set(res) == {"err", "snr", "snr_seg", "pesq", "lsd"} and res["pesq"] == 0 and res["snr_seg"] == 0
    # eval_size = 1 -> batches 0 and 1 are scored (the reference breaks after j >= eval_size)
    model.eval()
    want = []
    for b in batches[:2]:
        with torch.no_grad():
            sr = model.inference(b["LR_audio"].cuda())[1]
        want.append(compute_matrics(b["HR_audio"], b["LR_audio"], sr.squeeze(), opt))
    assert abs(res["err"] - np.mean([w[0] for w in want])) <= 1e-6 * res["err"]
    assert abs(res["lsd"] - np.mean([w[6] for w in want])) <= 1e-5 * res["lsd"]
    assert abs(res["snr"] - np.mean([(w[2], w[1]) for w in want])) <= 1e-4
    eval_model(model, batches, opt, path)
    rows = open(path).read().strip().splitlines()
    assert rows[0] == "err,snr,snr_seg,pesq,lsd" and len(rows) == 3


@pytest.mark.gpu
def test_compute_matrics_against_the_reference_fixture(golden):
    """G12: the reference's own compute_matrics (float32 on the host).  The device path accumulates its sums in double and
    runs the STFT as an exact-float32 GEMM, so it sits closer to the float64 yardstick than the reference does: MSE / SNR to
    float32 rounding of the REFERENCE's sums, the LSD within the reference's own float32 error (1.5e-3 on the quiet case)."""
    from mdctgan_amd.metrics import compute_matrics
    g = golden("g12_metrics")
    opt = types.SimpleNamespace(n_fft=int(g["n_fft"]), hop_length=int(g["hop_length"]), win_length=int(g["win_length"]),
                                center=bool(g["center"]))
    cases = [(g["hr0"], g["lr0"], g["sr0"], g["metrics0"]), (g["hr1"], g["lr1"], g["sr1"], g["metrics1"]),
             (g["hr2"], 0.5 * g["hr2"], 0.9 * g["hr2"], g["metrics2"])]
    for hr, lr, sr, want in cases:
        got = compute_matrics(torch.from_numpy(hr), torch.from_numpy(lr), torch.from_numpy(sr).to("cuda"), opt)
        exact = M.compute_matrics(hr, lr, sr, center=opt.center)
        assert got[3:6] == (0, 0, 0)
        assert abs(got[0] - want[0]) <= 2e-6 * want[0]
        assert abs(got[1] - want[1]) <= 2e-5 and abs(got[2] - want[2]) <= 2e-5                # dB
        assert abs(got[6] - want[6]) <= 1.5e-3 * want[6]
        assert abs(got[6] - exact[6]) <= 2e-4 * exact[6]


# ---- the metrics kernels one at a time (csrc/metrics.hip) against numpy float64 restatements ------------------------------------
def stft_frames_ref(x, window, n_fft, hop, center):
    """[B, T] float32 -> [B, F, n_fft] float32: numpy reflect padding, framing, one float32 product per output."""
    if center:
        x = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    F = 1 + (x.shape[1] - n_fft) // hop
    idx = hop * np.arange(F)[:, None] + np.arange(n_fft)[None, :]
    out = x[:, idx] * window[None, None, :]
    assert out.dtype == np.float32
    return out


def stft_lengths(n_fft, hop, center):
    return ([n_fft // 2 + 1] if center else []) + [n_fft, n_fft + 1, 7 * hop + 5, 4000]      # n_fft / 2 + 1: the deepest legal reflection


def device_frames(x, window, n_fft, hop, center, F):
    from mdctgan_amd import _lib
    lib = _lib.load()
    B, T = x.shape
    frames = torch.full((B * max(F, 1), n_fft), 3.25, device="cuda")
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(window).cuda()
    rc = lib.mg_stft_frames(_lib.ptr(xd), B, T, _lib.ptr(wd), n_fft, hop, int(center), _lib.ptr(frames), _lib.stream())
    return rc, frames


@pytest.mark.gpu
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("n_fft,hop", [(64, 32), (64, 16), (1024, 512)])
def test_stft_frames_bit_exact(n_fft, hop, center):
    """mg_stft_num_frames == torch.stft's frame count, and mg_stft_frames == reflect padding + framing + a float32 multiply by the
    window, bit for bit -- a wrong reflected sample in an edge frame cannot hide in a mean over frames.  Both rejected argument
    sets return MG_ERR_ARG and write nothing."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(n_fft + hop + center)
    window = rng.uniform(0.1, 1.0, n_fft).astype(np.float32)
    for T in stft_lengths(n_fft, hop, center):
        x = rng.standard_normal((3, T)).astype(np.float32)
        want = stft_frames_ref(x, window, n_fft, hop, center)
        F = lib.mg_stft_num_frames(T, n_fft, hop, int(center))
        ts = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, win_length=n_fft, window=torch.from_numpy(window), center=center,
                        pad_mode="reflect", return_complex=True)
        assert F == ts.shape[-1] == want.shape[1], (T, F, ts.shape, want.shape)
        rc, frames = device_frames(x, window, n_fft, hop, center, F)
        assert rc == 0
        assert np.array_equal(frames.cpu().numpy().reshape(3, F, n_fft), want), T
    T = n_fft // 2 if center else n_fft - 1                # center: the reflection would need sample T; else: not one whole frame
    x = rng.standard_normal((3, T)).astype(np.float32)
    if not center:
        assert lib.mg_stft_num_frames(T, n_fft, hop, 0) == -1
    rc, frames = device_frames(x, window, n_fft, hop, center, 1)
    assert rc == -1 and bool((frames == 3.25).all())
    assert lib.mg_stft_num_frames(0, n_fft, hop, int(center)) == -1 and lib.mg_stft_num_frames(T, n_fft, 0, int(center)) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop,T,center", [(64, 32, 229, True), (64, 16, 117, False), (1024, 512, 4000, True)])
def test_power_spectra_against_rfft(n_fft, hop, T, center):
    """metrics.power_spectra == numpy.fft.rfft (float64) of the same windowed frames, (re, im) interleaved; 3e-5 of max|ref|: an
    exact-float32 MFMA contraction over n_fft terms (tests/test_conv_gpu.py)."""
    from mdctgan_amd.metrics import power_spectra
    rng = np.random.default_rng(T)
    window = rng.uniform(0.1, 1.0, n_fft).astype(np.float32)
    x = rng.standard_normal((3, T)).astype(np.float32)
    frames = stft_frames_ref(x, window, n_fft, hop, center)
    spec = np.fft.rfft(frames.astype(np.float64), axis=-1).reshape(-1, n_fft // 2 + 1)
    want = np.stack((spec.real, spec.imag), axis=-1).reshape(spec.shape[0], -1)
    got, F = power_spectra(torch.from_numpy(x).cuda(), n_fft, hop, torch.from_numpy(window), center)
    assert F == frames.shape[1] and tuple(got.shape) == want.shape
    err = np.abs(got.double().cpu().numpy() - want).max()
    print("power_spectra n_fft=%d: err %.3g of max %.3g" % (n_fft, err, np.abs(want).max()))
    assert err <= 3e-5 * np.abs(want).max()
    if not center:
        with pytest.raises(ValueError):
            power_spectra(torch.from_numpy(x[:, :n_fft - 1]).cuda(), n_fft, hop, torch.from_numpy(window), center)
    else:
        with pytest.raises(ValueError):
            power_spectra(torch.from_numpy(x[:, :n_fft // 2].copy()).cuda(), n_fft, hop, torch.from_numpy(window), center)


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames", [1, 130])
@pytest.mark.parametrize("n_bins", [1, 63, 64, 65, 513])
def test_lsd_frames_against_float64(n_bins, n_frames):
    """mg_lsd_frames on given float32 spectra == sqrt(mean_k (log10(|a_k|^2 + 1e-6) - log10(|b_k|^2 + 1e-6))^2) in float64: bin counts
    around the 64-lane wave, frames that are all zero in one input or in both (the 1e-6 floor decides), a bin 10 orders below the
    floor.  The kernel computes in double and rounds once to float32: 2^-22 relative."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1000 * n_bins + n_frames)
    variants = [((3, 7), (5, 7))] if n_frames > 1 else [((), ()), ((0,), ()), ((), (0,)), ((0,), (0,))]
    for zero_a, zero_b in variants:
        a = (rng.standard_normal((n_frames, n_bins, 2)) * 10.0 ** rng.uniform(-3, 1, (n_frames, 1, 1))).astype(np.float32)
        b = (rng.standard_normal((n_frames, n_bins, 2)) * 10.0 ** rng.uniform(-3, 1, (n_frames, 1, 1))).astype(np.float32)
        if n_bins > 1:           # (a lone bin below the floor in both inputs would make the answer a difference of rounding errors)
            a[:, min(2, n_bins - 1)] = (1e-8, -1e-8)                # power 2e-16
            b[:, 0] = (0.0, 3e-9)
        a[list(zero_a)] = 0.0
        b[list(zero_b)] = 0.0
        if n_frames > 9:
            b[9] = a[9]                                             # identical frames: exactly 0
        pa = (a.astype(np.float64) ** 2).sum(-1)
        pb = (b.astype(np.float64) ** 2).sum(-1)
        want = np.sqrt(((np.log10(pa + 1e-6) - np.log10(pb + 1e-6)) ** 2).mean(-1))
        out = torch.full((n_frames,), -1.0, device="cuda")
        ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        _lib.check(lib.mg_lsd_frames(_lib.ptr(ad), _lib.ptr(bd), n_frames, n_bins, _lib.ptr(out), _lib.stream()), "mg_lsd_frames")
        got = out.double().cpu().numpy()
        assert np.all(np.abs(got - want) <= 2.0 ** -22 * want), (zero_a, zero_b, np.abs(got - want).max())
        if zero_a and zero_a == zero_b:
            assert got[0] == 0.0
        if n_frames > 9:
            assert got[7] == 0.0 and got[9] == 0.0 and got[3] > 0.0 and got[5] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 7001])
def test_metrics_rows_against_float64(T, B):
    """mg_metrics_rows == float64 numpy sums of hr^2, (sr - hr)^2, (lr - hr)^2 per row to 1e-12 (double accumulation; only the order
    of the additions differs), lengths around the 256-thread block.  A row with sr == hr sums to exactly 0 and its SNR is inf."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(10 * T + B)
    for exact_row in (None, B - 1):
        hr = (0.1 * rng.standard_normal((B, T))).astype(np.float32)
        sr = (hr + 0.01 * rng.standard_normal((B, T))).astype(np.float32)
        lr = (hr + 0.03 * rng.standard_normal((B, T))).astype(np.float32)
        if exact_row is not None:
            sr[exact_row] = hr[exact_row]
        h, s, l = (t.astype(np.float64) for t in (hr, sr, lr))
        want = np.stack(((h * h).sum(1), ((s - h) ** 2).sum(1), ((l - h) ** 2).sum(1)), axis=1)
        sums = torch.full((B, 3), -1.0, dtype=torch.float64, device="cuda")
        hd, ld, sd = (torch.from_numpy(t).cuda() for t in (hr, lr, sr))
        _lib.check(lib.mg_metrics_rows(_lib.ptr(hd), _lib.ptr(ld), _lib.ptr(sd), B, T, _lib.ptr(sums), _lib.stream()), "mg_metrics_rows")
        got = sums.cpu().numpy()
        assert np.all(np.abs(got - want) <= 1e-12 * want), (exact_row, np.abs(got - want).max())
        snr = (10 * torch.log10(sums[:, 0] / sums[:, 1])).cpu().numpy()          # as metrics.compute_matrics forms it
        with np.errstate(divide="ignore"):
            snr_want = 10 * np.log10(want[:, 0] / want[:, 1])
        if exact_row is not None:
            assert got[exact_row, 1] == 0.0 and snr[exact_row] == np.inf and snr_want[exact_row] == np.inf
        fin = np.isfinite(snr_want)
        assert np.array_equal(fin, np.isfinite(snr)) and np.all(np.abs(snr[fin] - snr_want[fin]) <= 1e-9)
