"""The packed front end for many utterances: mg_resample_rows, mg_rows_moments, mg_add_noise_rows, resample.front_end_many,
the noise step of make_training_pair / make_test_segments, and generate_audio.super_resolve_many.

Oracles.  The resampler: oracle/resample.py, whose parity with torchaudio is UNPINNED (torchaudio is not installed; see that
file's header) -- and the row-table kernel against the single-utterance kernel bit for bit.  The noise of --add_noise
(data/audio_dataset.py:73-78, 179-184): a float64 numpy restatement of those five lines written here (noise_ref64), so this
parity too is unpinned beyond the restatement; noise_ref32 is the reference's own lines on torch CPU float32, the yardstick of
the bar (tests/test_front_end_host.py shows that the bar has teeth).

Bars.  Row-table resampling: torch.equal.  Moments: N double additions of exactly represented terms, each at most 2^-53 of the
running sum: N 2^-52 of sum |x| (sum x^2).  Noise: max-abs error against float64 <= 4 e(float32 restatement) + 4 2^-23 max|want|,
the project's bar for an op whose float32 output cannot beat its own rounding (tests/test_bot_attn_gpu.py).  The chain against
the oracle: 4e-6 max|want|, the chain tolerance of tests/test_resample.py.
"""
import math

import numpy as np
import pytest
import torch

from oracle import resample as R

DEV = "cuda"
SEG = 7936
SENTINEL = 1234.5
GUARD = 64

ROW_LENGTHS = [1, 37, 4096, 7001, 20000]
ROW_PAIRS = [(48000, 8000), (8000, 48000), (48000, 12000), (16000, 48000), (44100, 48000)]
MOMENT_LENGTHS = [1, 2, 255, 4095, 4096, 4097, 12289, 70000]
NOISE_LENGTHS = [3000, 7936, 50000]
SNRS = [55.0, 10.0]


# ---------------------------------------------------------------------------------------------------------------------
# restatements and the bar (no GPU needed: tests/test_front_end_host.py imports them)
# ---------------------------------------------------------------------------------------------------------------------
def noise_ref64(lr, noise, snr, segment_length):
    """data/audio_dataset.py:73-78 in float64 numpy for one waveform."""
    lr, noise = np.asarray(lr, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    noise = noise - noise.mean()
    signal_power = np.sum(lr ** 2) / segment_length
    noise_var = signal_power / 10 ** (snr / 10)
    noise = np.sqrt(noise_var) / noise.std(ddof=1) * noise
    return lr + noise


def noise_ref32(lr, noise, snr, segment_length, fault=None):
    """The reference's own lines on torch CPU float32.  fault: "length" divides the signal power by the waveform's length instead
    of segment_length, "biased" takes the biased standard deviation."""
    lr_waveform, noise = torch.as_tensor(lr, dtype=torch.float32), torch.as_tensor(noise, dtype=torch.float32)
    noise = noise - noise.mean()
    signal_power = torch.sum(lr_waveform ** 2) / (lr_waveform.numel() if fault == "length" else segment_length)
    noise_var = signal_power / 10 ** (snr / 10)
    noise = torch.sqrt(noise_var) / (noise.std(unbiased=False) if fault == "biased" else noise.std()) * noise
    return (lr_waveform + noise).numpy()


def noise_passes(got, f32, f64):
    """-> (passes, error / bar)."""
    got, f32, f64 = (np.asarray(a, dtype=np.float64) for a in (got, f32, f64))
    bar = 4 * np.abs(f32 - f64).max() + 4 * 2.0 ** -23 * np.abs(f64).max()
    e = np.abs(got - f64).max()
    return bool(e <= bar), e / bar


def noise_inputs(n, seed=11):
    gen = torch.Generator().manual_seed(seed + n)
    return 0.05 * torch.randn(n, generator=gen), torch.randn(n, generator=gen)


def aligned_starts(lengths, align=64):
    starts, pos = [], 0
    for n in lengths:
        starts.append(pos)
        pos = -(-(pos + n) // align) * align
    return starts, pos


def _gpu(fn):
    return pytest.mark.gpu(fn)


def _wave(n, seed):
    return 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------
# 1. mg_resample_rows
# ---------------------------------------------------------------------------------------------------------------------
def _pack(waves, starts, total, fill=0.0, guard=GUARD):
    """[guard | packed waveforms, `fill` in the gaps | guard] on the device; -> (whole buffer, the packed part)."""
    buf = torch.full((total + 2 * guard,), fill, dtype=torch.float32)
    for w, s in zip(waves, starts):
        buf[guard + s:guard + s + w.numel()] = w
    buf = buf.to(DEV)
    return buf, buf[guard:guard + total]


@_gpu
@pytest.mark.parametrize("orig,new", ROW_PAIRS)
def test_resample_rows_equals_resample_per_utterance(orig, new):
    """Five utterances and a dead row in one launch: every window has the bits of resample() on that utterance alone, without
    and with a per-row shift; the alignment gaps and 64 floats on both sides of both buffers keep their sentinel; a second call
    onto NaNs gives the same bits; an utterance packed alone has the bits it has in the pack."""
    from mdctgan_amd.resample import resample, resample_length, resample_rows
    waves = [_wave(n, 100 + i) for i, n in enumerate(ROW_LENGTHS)]
    out_len = [resample_length(n, orig, new) for n in ROW_LENGTHS]
    in_start, in_total = aligned_starts(ROW_LENGTHS)
    out_start, out_total = aligned_starts(out_len)
    rows = [(a, n, b, m) for a, n, b, m in zip(in_start, ROW_LENGTHS, out_start, out_len)]
    rows.insert(2, (in_start[3], 0, out_start[3], 0))                       # a dead row that points into a live window
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    live = [0, 1, 3, 4, 5]
    shift = torch.tensor([0.25, -1e-4, 7.0, 3e-3, -0.5, 1e-4], device=DEV)
    # (the input gaps hold the sentinel too: a kernel that reads past a row's end shows in the result)
    x_all, x = _pack(waves, in_start, in_total, fill=SENTINEL)
    inside = torch.zeros(out_total + 2 * GUARD, dtype=torch.bool, device=DEV)
    for s, m in zip(out_start, out_len):
        inside[GUARD + s:GUARD + s + m] = True
    for sh in (None, shift):
        out_all = torch.full((out_total + 2 * GUARD,), SENTINEL, device=DEV)
        out = out_all[GUARD:GUARD + out_total]
        resample_rows(x, table, max(out_len), orig, new, out, shift=sh)
        for u, w in enumerate(waves):
            xin = w.to(DEV) if sh is None else w.to(DEV) + sh[live[u]]
            want = resample(xin[None], orig, new)[0]
            got = out[out_start[u]:out_start[u] + out_len[u]]
            assert want.shape == got.shape and torch.equal(got, want), (u, (got - want).abs().max().item())
        assert (out_all[~inside] == SENTINEL).all()
        assert (x_all[:GUARD] == SENTINEL).all() and (x_all[GUARD + in_total:] == SENTINEL).all()
        again_all = torch.full_like(out_all, float("nan"))
        resample_rows(x, table, max(out_len), orig, new, again_all[GUARD:GUARD + out_total], shift=sh)
        assert torch.equal(again_all[inside], out_all[inside]) and again_all[~inside].isnan().all()
        # alone: one row at position 0 of buffers of its own
        u = 3
        alone = torch.empty(out_len[u], device=DEV)
        resample_rows(waves[u].to(DEV), torch.tensor([(0, ROW_LENGTHS[u], 0, out_len[u])], dtype=torch.int64, device=DEV),
                      out_len[u], orig, new, alone, shift=None if sh is None else sh[live[u]:live[u] + 1].clone())
        assert torch.equal(alone, out[out_start[u]:out_start[u] + out_len[u]])


@_gpu
def test_resample_rows_cuts_bad_windows_to_the_buffers():
    """Windows that stick out of either buffer are cut to it, equal rates copy, a malformed table is refused on the host."""
    from mdctgan_amd.resample import resample_rows
    x_all, x = _pack([_wave(1000, 1)], [0], 1000, fill=SENTINEL)
    out_all = torch.full((500 + 2 * GUARD,), SENTINEL, device=DEV)
    out = out_all[GUARD:GUARD + 500]
    rows = [(-200, 600, -50, 100), (900, 600, 450, 100), (10 ** 15, 5, 0, 5), (0, 5, -10 ** 15, 5), (2 ** 40, 2 ** 40, 0, 2 ** 40)]
    resample_rows(x, torch.tensor(rows, dtype=torch.int64, device=DEV), 600, 48000, 8000, out)
    assert (out_all[:GUARD] == SENTINEL).all() and (out_all[GUARD + 500:] == SENTINEL).all()
    assert (out[50:450] == SENTINEL).all()
    assert (out[:50] != SENTINEL).all() and (out[450:] != SENTINEL).all() and out[:50].abs().max() < 1.0
    same = torch.full((1000,), SENTINEL, device=DEV)
    resample_rows(x, torch.tensor([(100, 300, 7, 300)], dtype=torch.int64, device=DEV), 300, 16000, 16000, same,
                  shift=torch.tensor([0.5], device=DEV))
    assert torch.equal(same[7:307], x[100:400] + 0.5) and (same[:7] == SENTINEL).all() and (same[307:] == SENTINEL).all()
    with pytest.raises(ValueError):
        resample_rows(x, torch.tensor(rows[:2], dtype=torch.int32, device=DEV), 600, 48000, 8000, out)
    with pytest.raises(ValueError):
        resample_rows(x, torch.tensor(rows, dtype=torch.int64, device=DEV)[:, :3].contiguous(), 600, 48000, 8000, out)


# ---------------------------------------------------------------------------------------------------------------------
# 2. mg_rows_moments
# ---------------------------------------------------------------------------------------------------------------------
@_gpu
@pytest.mark.parametrize("align", [64, 1])
def test_rows_moments_against_float64_sums(align):
    """Rows of 1 to 70000 samples (below, at and above the 4096-sample chunk, several chunks, a dead row) against numpy float64
    sums; alone == in the pack and repeat == repeat, bit for bit.  align 1 packs back to back: rows at positions that are no
    multiple of 4 (scalar loads of the same samples in the same order)."""
    from mdctgan_amd.resample import rows_moments
    waves = [_wave(n, 200 + i) + 0.01 for i, n in enumerate(MOMENT_LENGTHS)]
    starts, total = aligned_starts(MOMENT_LENGTHS, align)
    _, x = _pack(waves, starts, total, fill=SENTINEL)
    rows = [(0, s, s + n) for s, n in zip(starts, MOMENT_LENGTHS)] + [(0, 5, 5)]
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    got = rows_moments(x, table, max(MOMENT_LENGTHS))
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(rows), 2)
    assert torch.equal(got, rows_moments(x, table, max(MOMENT_LENGTHS)))
    host = got.cpu().numpy()
    assert host[-1, 0] == 0.0 and host[-1, 1] == 0.0
    for u, w in enumerate(waves):
        d = w.numpy().astype(np.float64)
        n = d.size
        e1, e2 = abs(host[u, 0] - d.sum()), abs(host[u, 1] - (d * d).sum())
        print("moments n=%d align=%d | sum %.3e of bar | sum sq %.3e of bar"
              % (n, align, e1 / (n * 2.0 ** -52 * np.abs(d).sum()), e2 / (n * 2.0 ** -52 * (d * d).sum())))
        assert e1 <= n * 2.0 ** -52 * np.abs(d).sum(), (n, e1)
        assert e2 <= n * 2.0 ** -52 * (d * d).sum(), (n, e2)
        alone = rows_moments(w.to(DEV), torch.tensor([(0, 0, n)], dtype=torch.int64, device=DEV), n)
        assert torch.equal(alone[0], got[u]), n
    # a window that sticks out of the buffer is cut to it
    cut = rows_moments(x, torch.tensor([(0, total - 10, total + 10 ** 12)], dtype=torch.int64, device=DEV), 4096).cpu().numpy()
    tail = x[total - 10:].cpu().numpy().astype(np.float64)
    assert abs(cut[0, 0] - tail.sum()) <= 10 * 2.0 ** -52 * np.abs(tail).sum()


# ---------------------------------------------------------------------------------------------------------------------
# 3. mg_add_noise_rows
# ---------------------------------------------------------------------------------------------------------------------
@_gpu
@pytest.mark.parametrize("snr", SNRS)
def test_add_noise_rows_against_the_restatement(snr):
    """Rows of 3000, 7936 and 50000 samples and a dead row, noise from a seeded CPU generator: the bar against float64, the
    realised SNR (with the reference's divisor, segment_length) to 1e-3 dB, a zero-mean added signal, gaps and dead rows
    untouched, and the same bits for a row alone."""
    from mdctgan_amd.resample import add_noise_rows, rows_moments
    pairs = [noise_inputs(n) for n in NOISE_LENGTHS]
    starts, total = aligned_starts(NOISE_LENGTHS)
    lr_all, lr = _pack([p[0] for p in pairs], starts, total, fill=SENTINEL)
    _, z = _pack([p[1] for p in pairs], starts, total, fill=SENTINEL)
    rows = [(0, s, s + n) for s, n in zip(starts, NOISE_LENGTHS)]
    rows.insert(1, (0, starts[2] + 5, starts[2] + 5))                          # dead, inside a live window
    rows.append((0, starts[0] + 100, starts[0] + 101))                          # one sample: no standard deviation, left alone
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    before = lr_all.clone()
    m_lr, m_z = rows_moments(lr, table, max(NOISE_LENGTHS)), rows_moments(z, table, max(NOISE_LENGTHS))
    assert add_noise_rows(lr, z, table, max(NOISE_LENGTHS), m_lr, m_z, snr, SEG) is lr
    inside = torch.zeros_like(lr_all, dtype=torch.bool)
    for (a, b), s, n in zip(pairs, starts, NOISE_LENGTHS):
        inside[GUARD + s:GUARD + s + n] = True
        got = lr[s:s + n].cpu().numpy()
        f64, f32 = noise_ref64(a, b, snr, SEG), noise_ref32(a, b, snr, SEG)
        ok, margin = noise_passes(got, f32, f64)
        added = got.astype(np.float64) - a.numpy().astype(np.float64)
        realised = 10 * math.log10((np.sum(a.numpy().astype(np.float64) ** 2) / SEG) / added.var(ddof=1))
        print("add_noise n=%d snr=%g | error / bar %.3e | realised snr %.6f dB | mean / std %.3e"
              % (n, snr, margin, realised, abs(added.mean()) / added.std(ddof=1)))
        assert ok, (n, snr, margin)
        assert abs(realised - snr) <= 1e-3, (n, snr, realised)
        assert abs(added.mean()) <= 1e-6 * added.std(ddof=1), (n, snr)
        # alone
        one = a.to(DEV)
        t1 = torch.tensor([(0, 0, n)], dtype=torch.int64, device=DEV)
        add_noise_rows(one, b.to(DEV), t1, n, rows_moments(one, t1, n), rows_moments(b.to(DEV), t1, n), snr, SEG)
        assert torch.equal(one, lr[s:s + n]), n
    assert torch.equal(lr_all[~inside], before[~inside])


# ---------------------------------------------------------------------------------------------------------------------
# 4. front_end_many
# ---------------------------------------------------------------------------------------------------------------------
HR, LR = 48000, 12000
# (rate, raw length): final lengths below, at and above a segment (3000, 7936, 21772 / 21769, 30004 / 30001, 12000)
MIX = [(16000, 1000), (48000, SEG), (44100, 20000), (48000, 30001), (16000, 4000)]


def mix_raws(seed=31):
    return [_wave(n, seed + i) + 0.02 for i, (_, n) in enumerate(MIX)], [r for r, _ in MIX]


_oracle_cache = {}


def oracle_front_end(is_lr_input, overlap):
    """R.inference_segments per utterance of MIX, computed once per (is_lr_input, overlap) and shared."""
    key = (bool(is_lr_input), overlap)
    if key not in _oracle_cache:
        raws, rates = mix_raws()
        _oracle_cache[key] = [R.inference_segments(w.numpy()[None], fs, HR, LR, SEG, overlap, is_lr_input)
                              for w, fs in zip(raws, rates)]
    return _oracle_cache[key]


def front_end_opt(is_lr_input, overlap, **more):
    return dict(lr_sampling_rate=LR, hr_sampling_rate=HR, is_lr_input=is_lr_input, segment_length=SEG, gen_overlap=overlap,
                batch_size=5, **more)


@_gpu
@pytest.mark.parametrize("is_lr_input", [False, True])
def test_front_end_many_matches_the_dataset_chain(is_lr_input):
    """Five utterances at 16 / 48 / 44.1 kHz (is_lr_input: one of the steps is a copy for the 48 kHz files) against the oracle's
    AudioTestDataset chain per utterance: exactly its shapes, within the chain tolerance of tests/test_resample.py; the gather
    over the plan's row table gives its segments at overlap 0 and 1024, the zero padding exactly zero."""
    from mdctgan_amd.mdct import seg_row_table, segments_gather
    from mdctgan_amd.resample import front_end_many
    raws, rates = mix_raws()
    for overlap in (0, 1024):
        want = oracle_front_end(is_lr_input, overlap)
        host_and_device = [w.to(DEV) if i % 2 else w[None] for i, w in enumerate(raws)]
        packed, views, plan = front_end_many(host_and_device, rates, front_end_opt(is_lr_input, overlap))
        assert packed.numel() == plan.utterances.in_total and len(views) == len(raws)
        assert plan.n_launches == (3 if is_lr_input else 4)         # three raw rates, then one 12 kHz -> 48 kHz launch
        inside = torch.zeros(packed.numel(), dtype=torch.bool, device=DEV)
        for u, (lr_audio, _) in enumerate(want):
            assert tuple(views[u].shape) == lr_audio.shape, u
            assert views[u].data_ptr() == packed[plan.utterances.in_start[u]:].data_ptr()
            e = np.abs(views[u].cpu().numpy() - lr_audio).max()
            assert e <= 4e-6 * np.abs(lr_audio).max(), (u, e)
            inside[plan.utterances.in_start[u]:plan.utterances.in_start[u] + lr_audio.shape[1]] = True
        assert not packed[~inside].any()
        segs = segments_gather(packed, seg_row_table(plan.in_rows, DEV), SEG).cpu().numpy()
        row = 0
        for u, (lr_audio, want_segs) in enumerate(want):
            got = segs[row:row + want_segs.shape[0]]
            row += want_segs.shape[0]
            assert got.shape == want_segs.shape and np.abs(got - want_segs).max() <= 4e-6 * np.abs(lr_audio).max(), (u, overlap)
            assert not got[want_segs == 0].any(), (u, overlap)
        assert row == plan.utterances.n_live
        assert not segs[plan.utterances.n_live:].any()


@_gpu
def test_front_end_many_with_noise_and_alone():
    """add_noise with the caller's noise: every utterance is the float64 restatement of the five lines on the noiseless front
    end's own output, under the noise bar; an utterance alone has the bits it has in the mix; without `noise` the device
    generator's stream is used and the result is reproducible from its seed."""
    from mdctgan_amd.resample import front_end_many
    raws, rates = mix_raws()
    _, clean, plan = front_end_many(raws, rates, front_end_opt(False, 0))
    gen = torch.Generator().manual_seed(77)
    noise = [torch.randn(n, generator=gen) for n in plan.final_lengths]
    _, noisy, _ = front_end_many(raws, rates, front_end_opt(False, 0, add_noise=True, snr=30.0), noise=noise)
    for u, (c, y) in enumerate(zip(clean, noisy)):
        c = c[0].cpu()
        ok, margin = noise_passes(y[0].cpu().numpy(), noise_ref32(c, noise[u], 30.0, SEG), noise_ref64(c, noise[u], 30.0, SEG))
        print("front_end_many add_noise u=%d | error / bar %.3e" % (u, margin))
        assert ok, (u, margin)
    _, alone, _ = front_end_many(raws[2:3], rates[2:3], front_end_opt(False, 0, add_noise=True, snr=30.0), noise=noise[2:3])
    assert torch.equal(alone[0], noisy[2])
    runs = [front_end_many(raws, rates, front_end_opt(False, 0, add_noise=True),
                           generator=torch.Generator(device=DEV).manual_seed(5))[0] for _ in range(2)]
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0][:3000], clean[0][0])
    with pytest.raises(ValueError):
        front_end_many(raws, rates, front_end_opt(False, 0, add_noise=True), noise=noise[:-1])
    with pytest.raises(ValueError):            # one sample at 48 kHz stays one sample: no standard deviation
        front_end_many([torch.ones(1)], [HR], front_end_opt(True, 0, add_noise=True))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the noise step of the per-waveform functions
# ---------------------------------------------------------------------------------------------------------------------
@_gpu
def test_training_pair_and_test_segments_with_noise():
    from mdctgan_amd.resample import make_test_segments, make_training_pair, resample
    gen = torch.Generator().manual_seed(9)
    wav = (0.1 * torch.randn(2, 9000, generator=gen)).to(DEV)
    noise = torch.randn(2, 9000, generator=gen)
    lr0, hr0 = make_training_pair(wav, HR, HR, LR, SEG)
    lr1, hr1 = make_training_pair(wav, HR, HR, LR, SEG, add_noise=False, snr=10.0, noise=noise)
    assert torch.equal(lr0, lr1) and torch.equal(hr0, hr1)
    full = resample(resample(wav, HR, LR), LR, HR).cpu()
    assert full.shape == noise.shape
    for snr in SNRS:
        lr, hr = make_training_pair(wav, HR, HR, LR, SEG, add_noise=True, snr=snr, noise=noise)
        assert torch.equal(hr, hr0) and lr.shape == lr0.shape
        for b in range(2):
            f64, f32 = noise_ref64(full[b], noise[b], snr, SEG), noise_ref32(full[b], noise[b], snr, SEG)
            ok, margin = noise_passes(lr[b].cpu().numpy(), f32[:SEG], f64[:SEG])
            print("make_training_pair add_noise row %d snr=%g | error / bar %.3e" % (b, snr, margin))
            assert ok, (b, snr, margin)
    # all rates equal: the low-rate waveform IS the input, which the noise must not touch
    keep = wav.clone()
    lr, hr = make_training_pair(wav, HR, HR, HR, SEG, add_noise=True, noise=noise)
    assert torch.equal(wav, keep) and torch.equal(hr, wav[:, :SEG]) and not torch.equal(lr, hr)
    # one waveform of the test dataset: the noise goes on the whole low-rate waveform, the segments are cut from it
    raw = wav[:1]
    lr_audio0, segs0 = make_test_segments(raw, HR, HR, LR, SEG, 1024)
    lr_audio, segs = make_test_segments(raw, HR, HR, LR, SEG, 1024, add_noise=True, snr=10.0, noise=noise[:1])
    assert lr_audio.shape == lr_audio0.shape and segs.shape == segs0.shape
    c = lr_audio0[0].cpu()
    ok, margin = noise_passes(lr_audio[0].cpu().numpy(), noise_ref32(c, noise[0], 10.0, SEG), noise_ref64(c, noise[0], 10.0, SEG))
    assert ok, margin
    from mdctgan_amd.generate_audio import segment_audio
    assert torch.equal(segs, segment_audio(lr_audio, SEG, 1024))
    with pytest.raises(ValueError):
        make_training_pair(wav, HR, HR, LR, SEG, add_noise=True, noise=noise[:, :100])


# ---------------------------------------------------------------------------------------------------------------------
# 6. super_resolve_many
# ---------------------------------------------------------------------------------------------------------------------
@_gpu
@pytest.mark.parametrize("add_noise", [False, True])
def test_super_resolve_many_is_front_end_then_generate_many(add_noise, monkeypatch):
    """The toy model of tests/test_generate_many_gpu.py (ngf 4, segment 7936, 12 kHz -> 48 kHz): raw files in, stitched
    waveforms out, bit for bit generate_many on the front end's views, through the fused row-table decode and through the
    composition (MG_NO_STITCHED_K2=1)."""
    from test_generate_many_gpu import make_model
    from mdctgan_amd import _lib
    from mdctgan_amd.generate_audio import generate_many, super_resolve_many
    from mdctgan_amd.resample import front_end_many
    model = make_model()
    assert (model.opt.lr_sampling_rate, model.opt.hr_sampling_rate, model.opt.segment_length) == (LR, HR, SEG)
    model.opt.add_noise, model.opt.snr = add_noise, 20.0
    raws, rates = mix_raws()
    overlap = 1024
    _, views, plan = front_end_many(raws, rates, front_end_opt(False, overlap))
    noise = None
    if add_noise:
        gen = torch.Generator().manual_seed(78)
        noise = [torch.randn(n, generator=gen) for n in plan.final_lengths]
        _, views, _ = front_end_many(raws, rates, front_end_opt(False, overlap, add_noise=True, snr=20.0), noise=noise)
    for no_fused in (False, True):
        if no_fused:
            monkeypatch.setenv("MG_NO_STITCHED_K2", "1")
        want = generate_many(model, views, batch_size=5, gen_overlap=overlap)
        got = super_resolve_many(model, raws, rates, batch_size=5, gen_overlap=overlap, noise=noise)
        assert ("<stitched rows>" in _lib.load().mg_mdct_last_kernel(1).decode()) != no_fused
        assert len(got) == len(want) == len(raws)
        for u, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape == (1, plan.utterances.out_length[u]), u
            assert torch.isfinite(g).all() and torch.equal(g, w), (u, no_fused)
