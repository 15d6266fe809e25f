"""Training batches cut from a packed corpus (mdctgan_amd/train_data.py, csrc/train_rows.hip): every row of the shared launches
has the bits resample.make_training_pair gives for its window alone, whatever lies next to the window in the corpus."""
import numpy as np
import pytest
import torch

from mdctgan_amd import train_data as T
from mdctgan_amd.resample import make_training_pair

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.0


def _noise_corpus(lengths, rates, seed=0):
    """Files of non-zero noise; lengths that are multiples of 64 sit back to back, so a tap read across a window edge changes bits."""
    gen = torch.Generator().manual_seed(seed)
    return T.pack_corpus([0.1 * torch.randn(n, generator=gen) + 0.01 for n in lengths], rates, DEV)


def _opt(hr, lr, seg, **kw):
    return dict(hr_sampling_rate=hr, lr_sampling_rate=lr, segment_length=seg, **kw)


def _alone(corpus, f, off, n, hr, lr, seg, **kw):
    s0 = corpus.starts[f] + off
    return make_training_pair(corpus.buffer[s0:s0 + n].clone().view(1, -1), corpus.rates[f], hr, lr, seg, **kw)


def _check_rows(corpus, windows, hr, lr, seg):
    idx, off, ln = ([w[k] for w in windows] for k in range(3))
    got_lr, got_hr = T.training_batch_many(corpus, idx, _opt(hr, lr, seg), offsets=off, lengths=ln)
    assert tuple(got_lr.shape) == tuple(got_hr.shape) == (len(windows), seg)
    for b, (f, o, n) in enumerate(windows):
        want_lr, want_hr = _alone(corpus, f, o, n, hr, lr, seg)
        assert torch.equal(got_hr[b], want_hr[0]), ("hr", b, f, o, n)
        assert torch.equal(got_lr[b], want_lr[0]), ("lr", b, f, o, n)
    return got_lr, got_hr


# files of 4096, 2048, 640 and 1088 samples: 7872 = 123 * 64 in all, no gaps.  Windows (file, offset, length): from sample 0 of the
# corpus; up to the last sample of file 0, where file 1 begins; from the first sample of file 1; inside file 0; the short file
# whole; up to the last sample of the corpus.
EDGE_LENGTHS = [4096, 2048, 640, 1088]
EDGE_WINDOWS = [(0, 0, 1000), (0, 3096, 1000), (1, 0, 1000), (0, 1500, 1000), (2, 0, 640), (3, 88, 1000), (1, 1048, 1000)]


@pytest.mark.parametrize("fs,hr,lr", [(48000, 48000, 12000), (48000, 48000, 8000), (16000, 48000, 8000), (44100, 48000, 8000),
                                      (96000, 48000, 8000), (16000, 48000, 48000), (48000, 48000, 48000), (8000, 48000, 8000),
                                      (12000, 48000, 8000)])
def test_rows_are_make_training_pair_bit_for_bit(fs, hr, lr):
    corpus = _noise_corpus(EDGE_LENGTHS, [fs] * 4, seed=fs // 100 + lr // 1000)
    assert corpus.buffer.numel() == sum(EDGE_LENGTHS) and EDGE_WINDOWS[5][1] + 1000 == EDGE_LENGTHS[3]
    got_lr, got_hr = _check_rows(corpus, EDGE_WINDOWS, hr, lr, 1000)
    hr_len, _, lr_len = T.pair_lengths(1000, fs, hr, lr)
    if hr_len < 1000:                                           # 96 kHz: half a segment, then zeros
        assert float(got_hr[0, hr_len:].abs().max()) == 0.0 and float(got_hr[0, :hr_len].abs().max()) > 0.0
    if lr_len < 1000:
        assert float(got_lr[0, lr_len:].abs().max()) == 0.0
    short = T.pair_lengths(640, fs, hr, lr)
    if short[0] < 1000:                                         # the file shorter than the segment
        assert float(got_hr[4, short[0]:].abs().max()) == 0.0


def test_segment_of_one_sample_and_segments_off_the_tile():
    corpus = _noise_corpus([8192, 4096, 320], [48000] * 3, seed=3)
    _check_rows(corpus, [(0, 0, 1), (0, 8191, 1), (1, 0, 1), (2, 319, 1)], 48000, 8000, 1)
    # 2500 = 2 * 1024 + 452: three tiles of the fused kernel, the last one partial; 1025: one sample into the second tile
    _check_rows(corpus, [(0, 0, 2500), (0, 5692, 2500), (1, 0, 2500), (1, 1596, 2500), (2, 0, 320)], 48000, 8000, 2500)
    _check_rows(corpus, [(0, 0, 1025), (1, 3071, 1025)], 48000, 12000, 1025)
    # 16 kHz at a long segment: the low-rate leg stops mid-tile, the crop cuts the tripled signal
    slow = _noise_corpus([4096, 2048], [16000] * 2, seed=4)
    _check_rows(slow, [(0, 0, 2500), (0, 1596, 2500), (1, 0, 2048), (1, 1000, 700)], 48000, 8000, 2500)


def test_mixed_file_rates_in_one_batch():
    rates = [48000, 16000, 44100, 96000, 48000, 16000]
    corpus = _noise_corpus([2048, 2048, 2048, 2048, 1024, 1024], rates, seed=5)
    windows = [(0, 0, 1000), (1, 1048, 1000), (2, 500, 1000), (3, 0, 1000), (4, 24, 1000), (5, 0, 1000), (2, 1048, 1000), (2, 0, 700)]
    idx, off, ln = ([w[k] for w in windows] for k in range(3))
    plan = T.plan_training_batch(corpus, idx, off, ln, 1000, 48000, 8000)
    assert plan.n_launches == 4
    _check_rows(corpus, windows, 48000, 8000, 1000)


def test_golden_dataset_chain(golden):
    g = golden("g13_dataset_chain")
    seg, hr_rate, lr_rate = int(g["segment_length"]), int(g["hr_rate"]), int(g["lr_rate"])
    corpus = T.pack_corpus([torch.from_numpy(g["file%d" % i]) for i in range(3)], [int(g["fs%d" % i]) for i in range(3)], DEV)
    torch.manual_seed(1234)
    lr, hr = T.training_batch_many(corpus, [0, 1, 2], _opt(hr_rate, lr_rate, seg))
    for i in range(3):
        for got, want in ((hr[i], g["HR%d" % i]), (lr[i], g["LR%d" % i])):
            got = got.cpu().numpy()
            err, peak = float(np.abs(got - want).max()), float(np.abs(want).max())
            print("g13 row %d: max error %.3e of peak %.3e (%.3e)" % (i, err, peak, err / peak))
            assert got.shape == (seg,) and err <= 4e-6 * peak, i
            assert np.array_equal(got == 0, want == 0) or np.abs(got[want == 0]).max() <= 4e-6 * peak
    assert hr_rate == 48000 and float(hr[1, 5000:].abs().max()) == 0.0 and float(np.abs(g["HR1"][5000:]).max()) == 0.0


@pytest.mark.parametrize("snr", [5.0, 55.0])
def test_add_noise_rows_are_make_training_pair_bit_for_bit(snr):
    corpus = _noise_corpus([4096, 2048, 640, 2048], [48000, 16000, 48000, 44100], seed=6)
    windows = [(0, 0, 1000), (1, 1048, 1000), (2, 0, 640), (0, 3096, 1000), (3, 100, 1000), (1, 0, 1000)]
    idx, off, ln = ([w[k] for w in windows] for k in range(3))
    seg, hr, lr = 1000, 48000, 8000
    plan = T.plan_training_batch(corpus, idx, off, ln, seg, hr, lr, add_noise=True)
    assert plan.lr_len[1] == 3000 and plan.lr_len[0] == 1002          # the 16 kHz row: power over three times the segment
    gen = torch.Generator().manual_seed(int(snr))
    noise = [torch.randn(n, generator=gen).to(DEV) for n in plan.lr_len]
    got_lr, got_hr = T.training_batch_many(corpus, idx, _opt(hr, lr, seg, add_noise=True, snr=snr), offsets=off, lengths=ln,
                                           noise=noise)
    clean_lr, _ = T.training_batch_many(corpus, idx, _opt(hr, lr, seg), offsets=off, lengths=ln)
    for b, (f, o, n) in enumerate(windows):
        want_lr, want_hr = _alone(corpus, f, o, n, hr, lr, seg, add_noise=True, snr=snr, noise=noise[b].view(1, -1))
        assert torch.equal(got_hr[b], want_hr[0]), b
        assert torch.equal(got_lr[b], want_lr[0]), b
        assert not torch.equal(got_lr[b], clean_lr[b])


def test_a_row_alone_has_its_bits_in_a_batch_of_40_and_a_dead_row_writes_nothing():
    corpus = _noise_corpus([4096, 2048, 640, 1088], [48000] * 4, seed=7)
    seg, hr, lr = 1000, 48000, 8000
    rng = np.random.RandomState(0)
    windows = []
    for b in range(40):
        f = b % 4
        n = min(1000, corpus.lengths[f])
        windows.append((f, int(rng.randint(0, corpus.lengths[f] - n + 1)), n))
    idx, off, ln = ([w[k] for w in windows] for k in range(3))
    got_lr, got_hr = T.training_batch_many(corpus, idx, _opt(hr, lr, seg), offsets=off, lengths=ln)
    for b in (0, 7, 22, 39):
        one_lr, one_hr = T.training_batch_many(corpus, idx[b:b + 1], _opt(hr, lr, seg), offsets=off[b:b + 1], lengths=ln[b:b + 1])
        assert torch.equal(one_lr[0], got_lr[b]) and torch.equal(one_hr[0], got_hr[b]), b
    # dead rows (in_len == 0), whatever their other fields say: rows 1 and 3 of the outputs stay as they were
    table = torch.tensor([(0, 1000, 0, 0, 0), (64, 0, 1, 0, 0), (128, 1000, 2, 0, 0), (0, 0, 3, 0, 1000)], dtype=torch.int64, device=DEV)
    out_lr, out_hr = (torch.full((4, seg), float("nan"), device=DEV) for _ in range(2))
    T.train_pair_rows(corpus.buffer, table, seg, 48000, hr, lr, out_hr, out_lr)
    for t in (out_lr, out_hr):
        assert bool(torch.isnan(t[1]).all()) and bool(torch.isnan(t[3]).all())
        assert bool(torch.isfinite(t[0]).all()) and bool(torch.isfinite(t[2]).all())
    want_lr, want_hr = _alone(corpus, 0, 128, 1000, hr, lr, seg)
    assert torch.equal(out_lr[2], want_lr[0]) and torch.equal(out_hr[2], want_hr[0])


@pytest.mark.parametrize("full", [False, True])
def test_outputs_stay_inside_their_buffers(full):
    corpus = _noise_corpus([4096, 2048, 640], [16000] * 3, seed=8)
    seg, hr, lr, pad = 1000, 48000, 8000, 64
    windows = [(0, 0, 1000), (1, 1048, 1000), (2, 0, 640), (0, 3096, 1000)]
    idx, off, ln = ([w[k] for w in windows] for k in range(3))
    plan = T.plan_training_batch(corpus, idx, off, ln, seg, hr, lr, add_noise=full)
    B, rows = len(windows), plan.table()
    # lr | 64 sentinels | hr | 64 sentinels, NaN where the results go; the same for lr_full and the table
    arena = torch.full((2 * (B * seg + pad),), SENTINEL, device=DEV)
    out_lr, out_hr = arena[:B * seg].view(B, seg), arena[B * seg + pad:2 * B * seg + pad].view(B, seg)
    out_lr.fill_(float("nan"))
    out_hr.fill_(float("nan"))
    n_full = max(plan.full_total, 1)
    full_arena = torch.full((n_full + pad,), SENTINEL, device=DEV)
    table_arena = torch.full((rows.size + pad,), -7, dtype=torch.int64, device=DEV)
    table_arena[:rows.size] = torch.from_numpy(rows.reshape(-1)).to(DEV)
    table = table_arena[:rows.size].view(B, T.ROW_COLS)
    T.train_pair_rows(corpus.buffer, table, seg, 16000, hr, lr, out_hr, None if full else out_lr,
                      full_arena[:n_full] if full else None, max(plan.lr_len))
    assert bool((arena[B * seg:B * seg + pad] == SENTINEL).all()) and bool((arena[-pad:] == SENTINEL).all())
    assert bool((full_arena[n_full:] == SENTINEL).all()) and bool((table_arena[rows.size:] == -7).all())
    assert torch.equal(table_arena[:rows.size].cpu(), torch.from_numpy(rows.reshape(-1)))
    assert bool(torch.isfinite(out_hr).all())
    if full:
        assert bool(torch.isnan(out_lr).all())                     # the dense rows are left alone
        live = torch.zeros(n_full, dtype=torch.bool, device=DEV)
        for s0, n in zip(plan.full_start, plan.lr_len):
            live[s0:s0 + n] = True
        assert bool((full_arena[:n_full][live] != SENTINEL).all())
        assert bool((full_arena[:n_full][~live] == SENTINEL).all())  # the gaps between the rows' windows
    else:
        assert bool(torch.isfinite(out_lr).all()) and bool((full_arena == SENTINEL).all())


def test_graph_replays_equal_the_eager_call():
    corpus = _noise_corpus([4096, 2048, 640, 1088], [48000] * 4, seed=9)
    opt = _opt(48000, 8000, 1000)
    run = T.make_graphed_training_batch(corpus, 6, opt)
    tables = [([0, 1, 2, 3, 0, 1], [0, 1048, 0, 88, 3095, 5]),
              ([3, 3, 1, 0, 2, 0], [1, 87, 777, 2048, 0, 1500]),
              ([1, 0, 3], [1047, 3000, 40])]                       # fewer rows than the capture: the rest are dead
    for idx, off in tables:
        lr, hr = run(idx, offsets=off)
        assert tuple(lr.shape) == tuple(hr.shape) == (6, 1000)
        want_lr, want_hr = T.training_batch_many(corpus, idx, opt, offsets=off)
        assert torch.equal(lr[:len(idx)], want_lr) and torch.equal(hr[:len(idx)], want_hr), idx
    # drawn windows: the same CPU stream in both
    lr, hr = run([0, 1, 2, 3, 1, 0], generator=torch.Generator().manual_seed(11))
    want_lr, want_hr = T.training_batch_many(corpus, [0, 1, 2, 3, 1, 0], opt, generator=torch.Generator().manual_seed(11))
    assert torch.equal(lr, want_lr) and torch.equal(hr, want_hr)
    with pytest.raises(ValueError):
        run(list(range(4)) * 2)
    mixed = _noise_corpus([2048, 2048], [48000, 16000], seed=10)
    with pytest.raises(ValueError, match="16000.*48000"):
        T.make_graphed_training_batch(mixed, 4, opt)
    with pytest.raises(NotImplementedError):
        T.make_graphed_training_batch(corpus, 4, dict(opt, add_noise=True))


def test_out_writes_the_callers_tensors():
    corpus = _noise_corpus([4096, 2048], [48000] * 2, seed=12)
    opt, idx, off = _opt(48000, 8000, 1000), [0, 1, 0, 1], [0, 1048, 3095, 7]
    want_lr, want_hr = T.training_batch_many(corpus, idx, opt, offsets=off)
    lr, hr = (torch.full((4, 1000), float("nan"), device=DEV) for _ in range(2))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = T.training_batch_many(corpus, idx, opt, offsets=off, out=(lr, hr))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - before < lr.numel() * 4      # (the row table at most: no result tensor)
    assert got[0] is lr and got[1] is hr
    assert torch.equal(lr, want_lr) and torch.equal(hr, want_hr)
    with pytest.raises(ValueError):
        T.training_batch_many(corpus, idx, opt, offsets=off, out=(lr, hr[:3]))
    with pytest.raises(ValueError):
        T.training_batch_many(corpus, idx, opt, offsets=off, out=(lr.double(), hr))
