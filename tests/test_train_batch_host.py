"""Host side of the packed training batches (mdctgan_amd/train_data.py): readaudio's random crop restated against the fixture
captured from the reference's AudioDataset, and the row tables of plan_training_batch.  No device call."""
import numpy as np
import pytest
import torch

from mdctgan_amd import train_data as T
from oracle import resample as R


def _g13_corpus(g):
    waves = [torch.from_numpy(g["file%d" % i]) for i in range(3)]
    return T.pack_corpus(waves, [int(g["fs%d" % i]) for i in range(3)], "cpu")


def test_draw_windows_is_readaudio_on_the_golden_chain(golden):
    g = golden("g13_dataset_chain")
    seg, hr_rate = int(g["segment_length"]), int(g["hr_rate"])
    corpus = _g13_corpus(g)
    torch.manual_seed(1234)                                   # AudioDataset.__init__: torch.manual_seed(opt.seed)
    offsets, lengths = T.draw_windows(corpus, [0, 1, 2], seg, hr_rate)
    assert offsets.dtype == lengths.dtype == torch.int64
    assert offsets.tolist() == [int(g["offset%d" % i]) for i in range(3)]
    for i in range(3):
        s0 = corpus.starts[i] + int(offsets[i])
        window = corpus.buffer[s0:s0 + int(lengths[i])].numpy()
        assert np.array_equal(window, g["loaded%d" % i].reshape(-1)), i
    # the same draws from a generator of the caller's, and none for a file that is loaded whole
    gen = torch.Generator().manual_seed(1234)
    again, _ = T.draw_windows(corpus, [0, 1, 2], seg, hr_rate, generator=gen)
    assert again.tolist() == offsets.tolist()
    state = torch.get_rng_state()
    T.draw_windows(corpus, [1], seg, hr_rate)
    assert int(g["offset1"]) == 0 and torch.equal(state, torch.get_rng_state())
    # windows_at: the caller's offsets, readaudio's lengths
    off2, len2 = T.windows_at(corpus, [0, 1, 2], offsets, seg, hr_rate)
    assert off2.tolist() == offsets.tolist() and len2.tolist() == lengths.tolist()


def test_crop_window_equals_the_oracle():
    seen = set()
    for fs in (8000, 16000, 44100, 48000, 96000):
        for hr in (44100, 48000):
            for seg in (1, 1000, 32512):
                for n in (1, seg // 3, seg - 1, seg, seg + 1, int(seg * fs / hr), int(seg * fs / hr) + 1, 2 * seg + 7, 500000):
                    if n <= 0:
                        continue
                    got = T.crop_window(n, fs, seg, hr)
                    assert got == R.crop_window(n, fs, seg, hr) and isinstance(got, int)
                    seen.add((got > 0) - (got < 0))
                    seen.add("fs>hr" if fs > hr else "fs<=hr")
    assert seen == {-1, 0, 1, "fs>hr", "fs<=hr"}


def _corpus(lengths, rates, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return T.pack_corpus([torch.randn(n, generator=gen) for n in lengths], rates, "cpu")


def test_pack_corpus_layout():
    corpus = _corpus([100, 64, 7], [48000, 16000, 48000])
    assert corpus.starts == [0, 128, 192] and corpus.buffer.numel() == 256 and len(corpus) == 3
    assert corpus.distinct_rates == [16000, 48000]
    assert float(corpus.buffer[100:128].abs().max()) == 0.0
    with pytest.raises(ValueError):
        T.pack_corpus([], [], "cpu")
    with pytest.raises(ValueError):
        T.pack_corpus([torch.zeros(4)], [48000, 16000], "cpu")


def test_plan_groups_rows_by_file_rate_and_launches_do_not_grow():
    corpus = _corpus([5000, 3000, 4000, 900], [48000, 16000, 48000, 96000])
    seg, hr, lr = 1000, 48000, 8000
    plans = {}
    for B in (1, 64):
        idx = [b % 4 for b in range(B)] if B > 1 else [0]
        off, ln = T.draw_windows(corpus, idx, seg, hr, generator=torch.Generator().manual_seed(B))
        plans[B] = (idx, off, ln, T.plan_training_batch(corpus, idx, off, ln, seg, hr, lr))
    idx, off, ln, plan = plans[64]
    assert [g.file_rate for g in plan.groups] == [48000, 16000, 96000] and plan.n_launches == 3
    one_rate = _corpus([5000, 3000], [48000, 48000])
    for B in (1, 64):
        o, n = T.draw_windows(one_rate, [b % 2 for b in range(B)], seg, hr)
        assert T.plan_training_batch(one_rate, [b % 2 for b in range(B)], o, n, seg, hr, lr).n_launches == 1
    assert plans[1][3].n_launches == 1
    seen = []
    for g in plan.groups:
        assert g.rows.dtype == np.int64 and g.rows.shape == (len(g.index), T.ROW_COLS)
        for row, b in zip(g.rows, g.index):
            f = idx[b]
            assert corpus.rates[f] == g.file_rate
            assert row.tolist() == [corpus.starts[f] + int(off[b]), int(ln[b]), b, 0, 0]
        seen += g.index
    assert sorted(seen) == list(range(64))
    assert plan.table().shape == (64, T.ROW_COLS) and plan.rows == 64


def test_plan_lengths_are_mid_len_and_the_up_sampled_mid_len():
    corpus = _corpus([1000, 2000, 999], [48000, 16000, 44100])
    plan = T.plan_training_batch(corpus, [0, 1, 2], [0, 0, 0], [1000, 1000, 999], 1000, 48000, 8000, add_noise=True)
    # L = 1000 at 48 k / 8 k: ceil(1000 / 6) = 167 intermediates, 6 * 167 = 1002 low-rate samples beside 1000 high-rate ones
    assert (plan.hr_len[0], plan.mid_len[0], plan.lr_len[0]) == (1000, 167, 1002)
    assert (plan.hr_len[1], plan.mid_len[1], plan.lr_len[1]) == (3000, 500, 3000)
    mid = -(-80 * 999 // 441)
    assert (plan.hr_len[2], plan.mid_len[2], plan.lr_len[2]) == (-(-160 * 999 // 147), mid, 6 * mid)
    for b in range(3):
        assert T.pair_lengths([1000, 1000, 999][b], corpus.rates[b], 48000, 8000) == (plan.hr_len[b], plan.mid_len[b], plan.lr_len[b])
        hr_o, lr_o = (R._resample32(np.zeros((1, [1000, 1000, 999][b]), np.float32), corpus.rates[b], 48000),
                      R._resample32(R._resample32(np.zeros((1, [1000, 1000, 999][b]), np.float32), corpus.rates[b], 8000), 8000, 48000))
        assert hr_o.shape[1] == plan.hr_len[b] and lr_o.shape[1] == plan.lr_len[b]
    # under add_noise every row's full-length signal has an aligned window of the packed buffer
    assert plan.full_start == [0, 1024, 4032] and plan.full_total == 4032 + -(-6 * mid // 64) * 64
    rows = {int(r[2]): r for g in plan.groups for r in g.rows}
    assert [int(rows[b][3]) for b in range(3)] == plan.full_start and [int(rows[b][4]) for b in range(3)] == plan.lr_len
    assert [g.max_full_len for g in plan.groups] == [1002, 3000, 6 * mid]
    # degenerate legs
    assert T.pair_lengths(1000, 48000, 48000, 48000) == (1000, 1000, 1000)
    assert T.pair_lengths(1000, 8000, 48000, 8000) == (6000, 1000, 6000)


def test_plan_marks_dead_rows():
    corpus = _corpus([5000, 3000], [48000, 48000])
    plan = T.plan_training_batch(corpus, [1, 0, 1], [5, 6, 7], [1000, 1000, 1000], 1000, 48000, 8000, pad_to=8)
    table = plan.table()
    assert table.shape == (8, T.ROW_COLS) and plan.rows == 8 and plan.batch == 3 and plan.n_launches == 1
    assert table[:3, 1].tolist() == [1000, 1000, 1000] and table[:3, 2].tolist() == [0, 1, 2]
    assert not table[3:].any()                                  # in_len == 0: dead
    with pytest.raises(ValueError):
        T.plan_training_batch(corpus, [1, 0, 1], [5, 6, 7], [1000] * 3, 1000, 48000, 8000, pad_to=2)
    with pytest.raises(ValueError):
        T.plan_training_batch(corpus, [1, 0, 1], [5, 6, 7], [1000] * 3, 1000, 48000, 8000, add_noise=True, pad_to=8)


def test_argument_errors():
    corpus = _corpus([5000, 3000], [48000, 48000])
    opt = dict(lr_sampling_rate=8000, hr_sampling_rate=48000, segment_length=1000)
    with pytest.raises(ValueError):
        T.draw_windows(corpus, [], 1000, 48000)
    with pytest.raises(ValueError):
        T.training_batch_many(corpus, [], opt)
    for bad in ([2], [-1], [0, 5]):
        with pytest.raises(IndexError):
            T.draw_windows(corpus, bad, 1000, 48000)
        with pytest.raises(IndexError):
            T.training_batch_many(corpus, bad, opt)
    with pytest.raises(ValueError):
        T.plan_training_batch(corpus, [0], [4500], [1000], 1000, 48000, 8000)            # the window leaves the file
    with pytest.raises(ValueError):
        T.plan_training_batch(corpus, [0, 1], [0], [1000], 1000, 48000, 8000)
    with pytest.raises(ValueError):
        T.windows_at(corpus, [0], [5000], 1000, 48000)
    # noise of the wrong size, and noise without add_noise: refused before any device call
    noisy = dict(opt, add_noise=True, snr=5.0)
    with pytest.raises(ValueError, match="one waveform per batch row"):
        T.training_batch_many(corpus, [0, 1], noisy, offsets=[0, 0], noise=[torch.zeros(1002), torch.zeros(1000)])
    with pytest.raises(ValueError, match="one waveform per batch row"):
        T.training_batch_many(corpus, [0, 1], noisy, offsets=[0, 0], noise=[torch.zeros(1002)])
    with pytest.raises(ValueError):
        T.training_batch_many(corpus, [0], opt, offsets=[0], noise=[torch.zeros(1002)])
    with pytest.raises(ValueError):
        T.training_batch_many(corpus, [0], dict(lr_sampling_rate=8000, hr_sampling_rate=48000), offsets=[0])
    with pytest.raises(ValueError):
        T.training_batch_many(corpus, [0], opt, offsets=[0], out=(torch.zeros(1, 1000), torch.zeros(2, 1000)))


def test_graphed_variant_refusals_need_no_device():
    opt = dict(lr_sampling_rate=8000, hr_sampling_rate=48000, segment_length=1000)
    mixed = _corpus([5000, 3000], [48000, 16000])
    with pytest.raises(ValueError, match="16000.*48000"):
        T.make_graphed_training_batch(mixed, 4, opt)
    with pytest.raises(NotImplementedError):
        T.make_graphed_training_batch(_corpus([5000], [48000]), 4, dict(opt, add_noise=True))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """mg_train_pair_rows returns MG_ERR_ARG / MG_ERR_UNSUPPORTED from its host-side checks: no pointer below is ever followed."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    p = 0x1000                                                   # "some non-null pointer"
    copy, sinc = _lib.ResampleBank(None, 1, 1, 0), _lib.ResampleBank(p, 6, 1, 37)
    good = dict(corpus=p, total=4096, rows=p, n_rows=4, seg=1000, to_hr=copy, to_lr=sinc, up=_lib.ResampleBank(p, 1, 6, 7), lr=p, hr=p,
                out_rows=4, lr_full=None, full_total=0, max_full=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mg_train_pair_rows(a["corpus"], a["total"], a["rows"], a["n_rows"], a["seg"], a["to_hr"], a["to_lr"], a["up"],
                                      a["lr"], a["hr"], a["out_rows"], a["lr_full"], a["full_total"], a["max_full"], None)
    for bad in (dict(corpus=None), dict(rows=None), dict(hr=None), dict(lr=None), dict(n_rows=0), dict(n_rows=-3), dict(seg=0),
                dict(seg=-1), dict(seg=(1 << 30) + 1), dict(total=0), dict(out_rows=0), dict(to_hr=None), dict(to_lr=None),
                dict(up=None), dict(to_lr=_lib.ResampleBank(p, 0, 1, 37)), dict(up=_lib.ResampleBank(p, 1, 6, -1)),
                dict(lr_full=p, full_total=0, max_full=10), dict(lr_full=p, full_total=10, max_full=0)):
        assert call(**bad) == -1, bad
    # an lr -> hr bank whose taps of one output do not fit the tile of intermediates
    assert call(up=_lib.ResampleBank(p, 5000, 1, 0)) == -2
    with pytest.raises(NotImplementedError):
        _lib.check(-2, "mg_train_pair_rows")
