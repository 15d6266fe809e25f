"""Packed metrics on the device (csrc/metrics_rows.hip, metrics.compute_matrics_many, generate_audio.evaluate_many): the row sums
against float64 numpy, the per-frame LSD against numpy.fft.rfft (float64) of the float32 windowed frames, the utterance
boundaries, pack invariance, the float64 oracle and the reference fixture, and the whole chain on the small generator."""
import types

import numpy as np
import pytest
import torch

from oracle import metrics as M

_gpu = pytest.mark.gpu
GUARD = 1e3                      # what fills every sample a kernel must not read


def metric_lengths(n_fft, hop, center):
    """tests/test_metrics_many_host.py's grid, and a fifth utterance of exactly two frames where there is no n_fft / 2 + 1."""
    return ([n_fft // 2 + 1] if center else [n_fft + hop]) + [n_fft, n_fft + 1, 7 * hop + 5, 9000]


def frames_ref(x, window, n_fft, hop, center):
    """[T] float32 -> [F, n_fft] float32: numpy reflect padding at the utterance's own ends, framing, one float32 product."""
    if center:
        x = np.pad(x, (n_fft // 2, n_fft // 2), mode="reflect")
    F = 1 + (x.shape[0] - n_fft) // hop
    idx = hop * np.arange(F)[:, None] + np.arange(n_fft)[None, :]
    out = x[idx] * window[None, :]
    assert out.dtype == np.float32
    return out


def lsd_ref(hr, sr, window, n_fft, hop, center):
    """per-frame LSD in float64 from the float32 windowed frames."""
    pa = np.abs(np.fft.rfft(frames_ref(hr, window, n_fft, hop, center).astype(np.float64), axis=-1)) ** 2
    pb = np.abs(np.fft.rfft(frames_ref(sr, window, n_fft, hop, center).astype(np.float64), axis=-1)) ** 2
    return np.sqrt(((np.log10(pa + 1e-6) - np.log10(pb + 1e-6)) ** 2).mean(-1))


def pack(waves, lead, align, fill, tail=0):
    """-> (float32 buffer, starts): wave u at lead + (aligned) running position, `fill` everywhere else."""
    starts, pos = [], lead
    for w in waves:
        starts.append(pos)
        pos = -(-(pos + len(w)) // align) * align
    buf = np.full(pos + tail, fill, dtype=np.float32)
    for s, w in zip(starts, waves):
        buf[s:s + len(w)] = w
    return buf, starts


def lsd_rows(hr_buf, sr_buf, hr_starts, sr_starts, lengths, n_fft, hop, center, window, shift=None):
    """mg_lsd_rows on packed numpy buffers -> (per-frame float32 tensor, MetricsPlan); the output lies inside a guard-filled array."""
    from mdctgan_amd import _lib
    from mdctgan_amd.metrics import plan_metrics
    lib = _lib.load()
    plan = plan_metrics(lengths, n_fft, hop, center)
    U = len(lengths)
    rows = torch.tensor([[h, 0, s, n] for h, s, n in zip(hr_starts, sr_starts, lengths)], dtype=torch.int64).cuda()
    fs = torch.tensor(plan.frame_start, dtype=torch.int64).cuda()
    hd, sd, wd = torch.from_numpy(hr_buf).cuda(), torch.from_numpy(sr_buf).cuda(), torch.from_numpy(window).cuda()
    sh = None if shift is None else torch.from_numpy(shift).cuda()
    out = torch.full((plan.total_frames + 16,), -5.0, device="cuda")
    _lib.check(lib.mg_lsd_rows(_lib.ptr(hd), hd.numel(), _lib.ptr(sd), sd.numel(), _lib.ptr(rows), U, _lib.ptr(fs),
                               plan.total_frames, _lib.ptr(sh), _lib.ptr(wd), n_fft, hop, int(center), _lib.ptr(out[8:]),
                               _lib.stream()), "mg_lsd_rows")
    assert bool((out[:8] == -5.0).all()) and bool((out[8 + plan.total_frames:] == -5.0).all())
    return out[8:8 + plan.total_frames], plan


# ---------------------------------------------------------------------------------------------------------------------
# 1. mg_metrics_rows_packed
# ---------------------------------------------------------------------------------------------------------------------
@_gpu
@pytest.mark.parametrize("with_shift", [False, True])
def test_metrics_rows_packed_against_float64(with_shift):
    """One launch over rows around the 256-thread block and MG_MOMENTS_CHUNK plus a dead row == float64 numpy sums to 1e-12 (the
    bound of test_metrics_rows_against_float64: double accumulation, only the order differs).  hr at aligned starts, sr four
    samples in, lr packed tightly from sample 3 (rows 1, 4 and 7 are quad-aligned in all three buffers, the others take the scalar
    loads); everything between the rows is 1e3.  A row with sr == hr gives exactly 0 and an infinite SNR; the outputs lie in a
    guard-filled array."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5 + with_shift)
    lengths = [1, 255, 256, 257, 4095, 4096, 4097, 9000]
    shift = (1e-3 * rng.standard_normal(len(lengths) + 1)).astype(np.float32) if with_shift else None
    hr = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    sr = [(h + 0.01 * rng.standard_normal(len(h))).astype(np.float32) for h in hr]
    lr = [(h + 0.03 * rng.standard_normal(len(h))).astype(np.float32) for h in hr]
    same = 3
    sr[same] = hr[same] + shift[same] if with_shift else hr[same].copy()
    assert sr[same].dtype == np.float32
    hb, hs = pack(hr, 0, 64, GUARD)
    sb, ss = pack(sr, 4, 64, GUARD, tail=7)
    lb, ls = pack(lr, 3, 1, GUARD, tail=2)
    assert [(a | b | c) & 3 == 0 for a, b, c in zip(hs, ls, ss)] == [False, True, False, False, True, False, False, True]
    # the dead row sits in the middle of the table and points at real samples
    table = [[h, l, s, n] for h, l, s, n in zip(hs, ls, ss, lengths)]
    table.insert(4, [hs[2], ls[2], ss[2], 0])
    if with_shift:
        shift = np.insert(shift[:len(lengths)], 4, np.float32(0.5))
    live = [0, 1, 2, 3, 5, 6, 7, 8]
    U = len(table)
    rows = torch.tensor(table, dtype=torch.int64).cuda()
    hd, ld, sd = (torch.from_numpy(b).cuda() for b in (hb, lb, sb))
    shd = None if shift is None else torch.from_numpy(shift).cuda()
    nbytes = lib.mg_metrics_rows_packed_workspace(U, max(lengths))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((U + 2, 3), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.mg_metrics_rows_packed(_lib.ptr(hd), hd.numel(), _lib.ptr(ld), ld.numel(), _lib.ptr(sd), sd.numel(),
                                          _lib.ptr(rows), U, max(lengths), _lib.ptr(shd), _lib.ptr(out[1:]), _lib.ptr(ws), nbytes,
                                          _lib.stream()), "mg_metrics_rows_packed")
    got = out.cpu().numpy()
    assert np.all(got[0] == -7.0) and np.all(got[-1] == -7.0)
    got = got[1:-1]
    assert np.all(got[4] == 0.0)
    worst = 0.0
    for k, r in enumerate(live):
        h = (hr[k] + shift[r]) if with_shift else hr[k]
        assert h.dtype == np.float32
        h, s, l = h.astype(np.float64), sr[k].astype(np.float64), lr[k].astype(np.float64)
        want = np.array([(h * h).sum(), ((s - h) ** 2).sum(), ((l - h) ** 2).sum()])
        err = np.abs(got[r] - want)
        worst = max(worst, float((err / np.maximum(want, 1e-300)).max()))
        assert np.all(err <= 1e-12 * want), (lengths[k], got[r], want)
    print("mg_metrics_rows_packed shift=%s: worst relative error %.3g" % (with_shift, worst))
    sums = out[1:-1]
    snr = (10 * torch.log10(sums[:, 0] / sums[:, 1])).cpu().numpy()
    assert got[same, 1] == 0.0 and snr[same] == np.inf and got[same, 0] > 0.0 and got[same, 2] > 0.0
    assert np.all(np.isfinite(np.delete(snr, [same, 4])))


# ---------------------------------------------------------------------------------------------------------------------
# 2. mg_lsd_rows per frame
# ---------------------------------------------------------------------------------------------------------------------
def signal_pair(kind, n, rng):
    t = np.arange(n)
    tone = 0.5 * np.sin(2 * np.pi * 440.0 * t / 48000.0)
    if kind == "noise":
        hr = 0.1 * rng.standard_normal(n)
        sr = hr + 0.01 * rng.standard_normal(n)
    elif kind == "sr 80 dB down":
        hr = 0.1 * rng.standard_normal(n)
        sr = 1e-4 * hr
    elif kind == "both at 1e-3":
        hr, sr = 1e-3 * rng.standard_normal(n), 1e-3 * rng.standard_normal(n)
    elif kind == "tone":
        hr, sr = tone + 0.01 * rng.standard_normal(n), tone
    else:
        hr = 0.1 * rng.standard_normal(n)
        sr = hr
    return hr.astype(np.float32), sr.astype(np.float32)


KINDS = ["noise", "sr 80 dB down", "both at 1e-3", "tone", "sr == hr"]


@_gpu
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("hop_div", [2, 4])
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_lsd_rows_per_frame_against_rfft(n_fft, hop_div, center):
    """Every frame of five utterances per launch: |got - want| <= 2e-4 want + 1e-5 against the float64 transform of the float32
    windowed frames.  2e-4 is the project's LSD bound (tests/test_metrics.py), here per frame, so that a wrong reflected sample in
    an edge frame cannot hide in a mean; 1e-5 absolute covers frames whose distance is (nearly) 0.  The kernel runs the same
    real transform on hr and on sr, so sr == hr must give exactly 0.  Measured on the MI355X, worst frame of the whole grid: 1.5e-5 relative (noise,
    n_fft 1024, hop 256, not centred), thirteen times inside the bound."""
    from mdctgan_amd.mdct import kbdwin
    hop = n_fft // hop_div
    window = kbdwin(n_fft).numpy().astype(np.float32)
    lengths = metric_lengths(n_fft, hop, center)
    rng = np.random.default_rng(n_fft + hop + center)
    for kind in KINDS:
        pairs = [signal_pair(kind, n, rng) for n in lengths]
        hb, hs = pack([p[0] for p in pairs], 0, 64, 0.0)
        sb, ss = pack([p[1] for p in pairs], 5, 64, 0.0)
        got, plan = lsd_rows(hb, sb, hs, ss, lengths, n_fft, hop, center, window)
        got = got.double().cpu().numpy()
        worst_rel = worst_abs = 0.0
        for u, (h, s) in enumerate(pairs):
            want = lsd_ref(h, s, window, n_fft, hop, center)
            g = got[plan.frame_start[u]:plan.frame_start[u + 1]]
            assert g.shape == want.shape
            err = np.abs(g - want)
            worst_abs = max(worst_abs, float(err.max()))
            if kind != "sr == hr":
                worst_rel = max(worst_rel, float((err / want).max()))
            assert np.all(err <= 2e-4 * want + 1e-5), (kind, u, lengths[u], int(np.argmax(err - 2e-4 * want)), err.max())
            if kind == "sr == hr":
                assert np.all(g == 0.0) and np.all(want == 0.0)
        print("mg_lsd_rows N=%d hop=%d center=%d %-14s worst rel %.3g abs %.3g" % (n_fft, hop, center, kind, worst_rel, worst_abs))


@_gpu
def test_lsd_rows_refuses_other_sizes():
    from mdctgan_amd import _lib
    lib = _lib.load()
    x = torch.zeros(9000, device="cuda")
    rows = torch.tensor([[0, 0, 0, 9000]], dtype=torch.int64).cuda()
    fs = torch.tensor([0, 4], dtype=torch.int64).cuda()
    out = torch.full((4,), -5.0, device="cuda")
    for n_fft in (256, 4096, 1000):
        w = torch.ones(n_fft, device="cuda")
        assert lib.mg_lsd_rows(_lib.ptr(x), 9000, _lib.ptr(x), 9000, _lib.ptr(rows), 1, _lib.ptr(fs), 4, None, _lib.ptr(w), n_fft,
                               n_fft // 2, 1, _lib.ptr(out), _lib.stream()) == -1
    assert bool((out == -5.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. boundaries
# ---------------------------------------------------------------------------------------------------------------------
@_gpu
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("n_fft,hop", [(512, 128), (1024, 512), (2048, 512)])
def test_lsd_rows_never_reads_across_an_utterance_boundary(n_fft, hop, center):
    """The gaps, the neighbours' surroundings and sr's samples beyond len are 1e3: every per-frame value equals, bit for bit, the
    launch with the utterance alone in a buffer of exactly its samples -- with and without the ground truth's shift."""
    from mdctgan_amd.mdct import kbdwin
    window = kbdwin(n_fft).numpy().astype(np.float32)
    lengths = metric_lengths(n_fft, hop, center)
    rng = np.random.default_rng(3 * n_fft + hop + center)
    pairs = [signal_pair("noise", n, rng) for n in lengths]
    shift = (1e-3 * rng.standard_normal(len(lengths))).astype(np.float32)
    hb, hs = pack([p[0] for p in pairs], 3, 1, GUARD, tail=5)               # tightly packed: the neighbour IS the next sample
    sb, ss = pack([np.concatenate([p[1], np.full(37, GUARD, np.float32)]) for p in pairs], 64, 64, GUARD, tail=64)
    for sh in (None, shift):
        got, plan = lsd_rows(hb, sb, hs, ss, lengths, n_fft, hop, center, window, sh)
        assert bool(torch.isfinite(got).all())
        for u, (h, s) in enumerate(pairs):
            alone, _ = lsd_rows(h, s, [0], [0], [lengths[u]], n_fft, hop, center, window, None if sh is None else sh[u:u + 1])
            assert torch.equal(got[plan.frame_start[u]:plan.frame_start[u + 1]], alone), (u, lengths[u])


# ---------------------------------------------------------------------------------------------------------------------
# 4. pack invariance
# ---------------------------------------------------------------------------------------------------------------------
def opt_for(n_fft, center):
    return types.SimpleNamespace(n_fft=n_fft // 2, hop_length=n_fft // 4, win_length=n_fft // 2, center=center)


def triples(lengths, seed):
    rng = np.random.default_rng(seed)
    hr = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    sr = [(h + 0.01 * rng.standard_normal(len(h))).astype(np.float32) for h in hr]
    lr = [(h + 0.03 * rng.standard_normal(len(h))).astype(np.float32) for h in hr]
    return hr, lr, sr


@_gpu
def test_compute_matrics_many_is_pack_invariant():
    """Seven utterances of different lengths: every row has the same bits alone, in the mix and in the reversed mix (lr and sr
    longer than hr here and there: they are cropped)."""
    from mdctgan_amd.metrics import compute_matrics_many
    lengths = [600, 1024, 4097, 9000, 12289, 2500, 20001]
    hr, lr, sr = triples(lengths, 11)
    lr[2] = np.concatenate([lr[2], np.ones(11, np.float32)])
    sr[5] = np.concatenate([sr[5], np.ones(300, np.float32)])
    t = lambda ws: [torch.from_numpy(w) for w in ws]
    opt = opt_for(1024, True)
    mix = compute_matrics_many(t(hr), t(lr), t(sr), opt)
    rev = compute_matrics_many(t(hr[::-1]), t(lr[::-1]), t(sr[::-1]), opt)
    assert mix.shape == (7, 7) and mix.dtype == torch.float64 and mix.is_cuda
    assert bool(torch.isfinite(mix).all()) and bool((mix[:, 3:6] == 0).all()) and bool((mix[:, 6] > 0).all())
    assert torch.equal(mix, rev.flip(0))
    for u in range(7):
        alone = compute_matrics_many(t(hr[u:u + 1]), t(lr[u:u + 1]), [torch.from_numpy(sr[u]).cuda().view(1, -1)], opt)
        assert torch.equal(alone[0], mix[u]), u


# ---------------------------------------------------------------------------------------------------------------------
# 5. against the float64 oracle and the reference fixture
# ---------------------------------------------------------------------------------------------------------------------
@_gpu
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("n_fft", [1024, 512])
def test_compute_matrics_many_against_the_oracle(n_fft, center):
    """Per utterance at the bounds of test_compute_matrics_on_device: MSE 1e-5 relative, SNRs 1e-4 dB, LSD 2e-4 relative."""
    from mdctgan_amd.metrics import compute_matrics_many
    lengths = [n_fft // 2 + 1 if center else n_fft, 4097, 9000, 32512]
    hr, lr, sr = triples(lengths, 3 + n_fft + center)
    opt = opt_for(n_fft, center)
    got = compute_matrics_many(*([torch.from_numpy(w) for w in ws] for ws in (hr, lr, sr)), opt).cpu().numpy()
    for u in range(len(lengths)):
        want = M.compute_matrics(hr[u], lr[u], sr[u], n_fft=opt.n_fft, hop_length=opt.hop_length, win_length=opt.win_length,
                                 center=center)
        g = got[u]
        print("N=%d center=%d T=%d: mse %.3g  snr %.3g %.3g dB  lsd %.3g" % (
            n_fft, center, lengths[u], abs(g[0] - want[0]) / want[0], abs(g[1] - want[1]), abs(g[2] - want[2]),
            abs(g[6] - want[6]) / want[6]))
        assert tuple(g[3:6]) == (0, 0, 0)
        assert abs(g[0] - want[0]) <= 1e-5 * want[0]
        assert abs(g[1] - want[1]) <= 1e-4 and abs(g[2] - want[2]) <= 1e-4          # dB
        assert abs(g[6] - want[6]) <= 2e-4 * want[6]


@_gpu
def test_compute_matrics_many_against_the_reference_fixture(golden):
    """G12 at the bounds of test_compute_matrics_against_the_reference_fixture, every fixture row an utterance of one call: the mean
    over a case's rows is the reference's batch value (equal lengths)."""
    from mdctgan_amd.metrics import compute_matrics_many
    g = golden("g12_metrics")
    opt = types.SimpleNamespace(n_fft=int(g["n_fft"]), hop_length=int(g["hop_length"]), win_length=int(g["win_length"]),
                                center=bool(g["center"]))
    cases = [(g["hr0"], g["lr0"], g["sr0"], g["metrics0"]), (g["hr1"], g["lr1"], g["sr1"], g["metrics1"]),
             (g["hr2"][None], 0.5 * g["hr2"][None], 0.9 * g["hr2"][None], g["metrics2"])]
    hrs, lrs, srs = ([torch.from_numpy(np.ascontiguousarray(row)) for c in cases for row in c[k]] for k in range(3))
    got = compute_matrics_many(hrs, lrs, srs, opt).cpu().numpy()
    at = 0
    for hr, lr, sr, want in cases:
        rows = got[at:at + hr.shape[0]].mean(0)
        at += hr.shape[0]
        exact = M.compute_matrics(hr, lr, sr, center=opt.center)
        assert abs(rows[0] - want[0]) <= 2e-6 * want[0]
        assert abs(rows[1] - want[1]) <= 2e-5 and abs(rows[2] - want[2]) <= 2e-5                # dB
        assert abs(rows[6] - want[6]) <= 1.5e-3 * want[6]
        assert abs(rows[6] - exact[6]) <= 2e-4 * exact[6]


# ---------------------------------------------------------------------------------------------------------------------
# 6. evaluate_many
# ---------------------------------------------------------------------------------------------------------------------
@_gpu
def test_evaluate_many_on_the_small_generator(tmp_path):
    """The small generator of test_eval_model_loop, four files at the hr rate: the waveforms are super_resolve_many's, the scores
    are compute_matrics_many on the materialised operands (raw + shift as a float32 add, the front end's view, the stitched view)
    bit for bit, and the existing compute_matrics per utterance within the bounds of the oracle test."""
    from mdctgan_amd import options
    from mdctgan_amd.generate_audio import _front_end_kwargs, evaluate_many, super_resolve_many
    from mdctgan_amd.metrics import compute_matrics, compute_matrics_many
    from mdctgan_amd.pix2pixHD_model import create_model
    from mdctgan_amd.resample import front_end_many
    from oracle import nets as onets
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                           "--n_blocks_global", "2", "--n_blocks_attn_g", "1", "--heads_g", "2", "--dim_head_g", "8",
                           "--num_D", "2", "--ndf", "8", "--batchSize", "2", "--bins", "32", "--segment_length", "7936",
                           "--gpu_ids", "0", "--eval_size", "1")
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    hr_rate = int(opt.hr_sampling_rate)
    rng = np.random.default_rng(21)
    lengths = [5000, 20000, 7937, 12001]
    raws = [torch.from_numpy((0.05 * rng.standard_normal(n) + 0.01).astype(np.float32)) for n in lengths]
    rates = [hr_rate] * 4
    path = str(tmp_path / "metric.txt")
    waves, scores = evaluate_many(model, raws, rates, batch_size=3, metric_path=path)
    want_waves = super_resolve_many(model, raws, rates, batch_size=3)
    assert len(waves) == len(want_waves) == 4
    for g, w in zip(waves, want_waves):
        assert torch.equal(g, w)
    assert scores.shape == (4, 7) and scores.dtype == torch.float64 and bool(torch.isfinite(scores).all())

    kw = _front_end_kwargs(model, 3, None)
    packed, views, plan = front_end_many(raws, rates, kw, keep_raw=True)
    packed0, _, plan0 = front_end_many(raws, rates, kw)
    assert torch.equal(packed, packed0) and plan0.raw is None
    assert plan.raw.shift.shape == (4,) and plan.raw.starts == plan.starts[0] and plan.raw.lengths == lengths
    hrs = [raws[u].cuda() + plan.raw.shift[u] for u in range(4)]
    assert all(h.dtype == torch.float32 for h in hrs)
    many = compute_matrics_many(hrs, views, want_waves, opt)
    assert torch.equal(scores, many)
    for u, n in enumerate(lengths):
        one = compute_matrics(hrs[u], views[u][..., :n], want_waves[u][..., :n], opt)
        g = scores[u].tolist()
        assert abs(g[0] - one[0]) <= 1e-5 * one[0]
        assert abs(g[1] - one[1]) <= 1e-4 and abs(g[2] - one[2]) <= 1e-4
        assert abs(g[6] - one[6]) <= 2e-4 * one[6]
    lines = open(path).read().splitlines()
    assert len(lines) == 4
    for line, row in zip(lines, scores.tolist()):
        assert line == "%f,%f,%f" % (row[0], row[1], row[6])
    with pytest.raises(ValueError, match="utterance 2"):
        evaluate_many(model, raws, [hr_rate, hr_rate, 44100, hr_rate], batch_size=3)


@_gpu
def test_keep_raw_shift_is_in_utterance_order():
    """Mixed rates: the DC-mean table runs in group order, plan.raw.shift in utterance order."""
    from mdctgan_amd.resample import front_end_many
    rng = np.random.default_rng(2)
    lengths, rates = [5000, 7001, 6000, 4100], [48000, 44100, 48000, 16000]
    raws = [torch.from_numpy((0.05 * rng.standard_normal(n) + 0.02 * (u + 1)).astype(np.float32)) for u, n in enumerate(lengths)]
    kw = dict(lr_sampling_rate=12000, hr_sampling_rate=48000, segment_length=7936)
    packed, _, plan = front_end_many(raws, rates, kw, keep_raw=True)
    packed0, _, plan0 = front_end_many(raws, rates, kw)
    assert plan.order != [0, 1, 2, 3] and plan0.raw is None and torch.equal(packed, packed0)
    shift = plan.raw.shift.cpu().numpy()
    for u, w in enumerate(raws):
        want = 1e-4 - w.double().mean().item()
        assert abs(shift[u] - want) <= 1e-6 * abs(want), u
        s0 = plan.raw.starts[u]
        assert torch.equal(plan.raw.buffer[s0:s0 + lengths[u]].cpu(), w)
