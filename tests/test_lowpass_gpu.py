"""Low-pass rows on the device: mg_sos_rows (csrc/sos_rows.hip) against the float64 restatement of tests/test_lowpass_host.py
(which is pinned to SciPy's outputs there), and the training path built on it.

The bar: |y - ref| <= 2^-23 max |ref| per row -- twice the rounding bound of the float32 output; the double recursion's own
error (about 1e-13) is invisible beside it, and a float32 recursion misses it by 68 x to 1244 x
(test_lowpass_host.test_float32_recursion_misses_the_gpu_bar).
"""
import numpy as np
import pytest
import torch

import test_lowpass_host as H
from mdctgan_amd import lowpass
from mdctgan_amd.lowpass import LowpassSpec, lowpass_sos, pad_sos
from mdctgan_amd.packed import aligned_layout

pytestmark = pytest.mark.gpu

C = lowpass.MG_SOS_CHUNK
# 1, 2, 3: shorter than a staged tile; C - 1, C, C + 1: one chunk and the first sample of a second; 2C - 1 (511), 2C + 1: around
# the third; 1200: the fixture's whole input (five chunks, the last partial)
LENGTHS = sorted({1, 2, 3, 255, 256, 257, 511, 513, 1200, C - 1, C, C + 1, 2 * C + 1})
GUARD = 12345.0


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def run_pack(rows, arena=None, x_total=None, zero_phase=True):
    """rows: (samples float32 [n], sections, in_pos, out_pos), or None for a dead row, packed as the table says -> the output
    arena, guard-filled outside what the kernel wrote."""
    live = [r for r in rows if r is not None]
    x_total = x_total or max(p + len(x) for x, _, p, _ in live) + 7
    buf = np.full(x_total, 777.0, dtype=np.float32)                        # (nothing outside a row's window may enter it)
    for x, _, p, _ in live:
        lo, hi = max(p, 0), min(p + len(x), x_total)
        buf[lo:hi] = x[lo - p:hi - p]
    table = np.asarray([(0, 0, 0) if r is None else (r[2], len(r[0]), r[3]) for r in rows], dtype=np.int64)
    sos = np.stack([pad_sos(H.CASES[0].sos) if r is None else pad_sos(r[1]) for r in rows])
    arena = arena or max(q + len(x) for x, _, _, q in live) + 5
    out = torch.full((arena,), GUARD, dtype=torch.float32, device=dev())
    lowpass.sos_rows(torch.from_numpy(buf).to(dev()), table, sos, out=out, zero_phase=zero_phase)
    return out


def check_row(y, ref, what):
    peak = np.abs(ref).max()
    e = np.abs(y.astype(np.float64) - ref).max() / peak
    assert np.isfinite(y).all(), what
    assert e <= H.GPU_BAR, "%s: %.3e of the peak, %.2f x the bar" % (what, e, e / H.GPU_BAR)
    return e / H.GPU_BAR


# ------------------------------------------------------------------------------------------------------------------
# per-element accuracy: every fixture filter at every length, one pack per mode
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_phase", [False, True], ids=["one_pass", "zero_phase"])
def test_sos_rows_matches_the_float64_reference(zero_phase):
    cells = [(c, n) for c in H.CASES for n in LENGTHS]
    lay = aligned_layout([n for _, n in cells])
    out = run_pack([(c.x[:n], c.sos, s, s) for (c, n), s in zip(cells, lay.starts)], arena=lay.total + 64,
                   zero_phase=zero_phase).cpu().numpy()
    worst = {}
    for (c, n), s in zip(cells, lay.starts):
        r = check_row(out[s:s + n], H.reference(c, n, zero_phase), "%s, %d samples" % (c.id, n))
        worst[c.id] = max(worst.get(c.id, 0.0), r)
    for cid, r in worst.items():
        print("lowpass sos_rows %s | zero_phase %d | worst error / bar %.3f" % (cid, zero_phase, r))
    written = np.zeros(out.shape[0], dtype=bool)
    for (_, n), s in zip(cells, lay.starts):
        written[s:s + n] = True
    assert (out[~written] == GUARD).all()


def test_sections_designed_here_pass_the_same_bar():
    """lowpass_sos' own sections (every section of gain 1) on the sharpest filters, and lowpass_waveform's one-row form."""
    for c in [c for c in H.CASES if c.order >= 11 and c.cutoff == 1000.0]:
        sos = H.design_of(c)
        x = torch.from_numpy(c.x).to(dev())
        for zero_phase in (False, True):
            ref = H.sos_zero_phase(sos, c.x.astype(np.float64)) if zero_phase else H.sos_cascade(sos, c.x)
            y = lowpass.lowpass_waveform(x[None], sos, zero_phase=zero_phase)
            assert y.shape == (1, len(c.x)) and y.dtype == torch.float32
            r = check_row(y[0].cpu().numpy(), ref, c.id)
            print("lowpass own sections %s | zero_phase %d | error / bar %.3f" % (c.id, zero_phase, r))
    # a [B, L] batch is B rows of one filter
    c = H.CASES[3]
    xb = torch.from_numpy(np.stack([c.x[:600], c.x[600:]])).to(dev())
    yb = lowpass.lowpass_waveform(xb, c.sos)
    for k in range(2):
        assert torch.equal(yb[k], lowpass.lowpass_waveform(xb[k], c.sos))


def test_long_rows_take_the_second_workgroup_and_the_second_carry_batch():
    """A workgroup runs 64 chunks and the carry holds the states of 128 chunks at a time: 64 C + 1 samples are the first row with
    a second workgroup, 128 C + 1 the first with a second carry batch.  The sharpest fixture filter, one pack, both modes."""
    c = H.CASES[16]
    n_long = 128 * C + 1
    x = (0.5 * np.random.default_rng(77).standard_normal(n_long)).astype(np.float32)
    forward = H.sos_cascade(c.sos, x)
    lengths = [64 * C + 1, n_long, 64 * C]
    lay = aligned_layout(lengths)
    for zero_phase in (False, True):
        out = run_pack([(x[:n], c.sos, s + 1, s) for n, s in zip(lengths, lay.starts)], arena=lay.total + 8,
                       zero_phase=zero_phase).cpu().numpy()
        for n, s in zip(lengths, lay.starts):
            ref = H.sos_zero_phase(c.sos, None, forward=forward[:n]) if zero_phase else forward[:n]
            r = check_row(out[s:s + n], ref, "%d samples" % n)
            print("lowpass long row %d | zero_phase %d | error / bar %.3f" % (n, zero_phase, r))


# ------------------------------------------------------------------------------------------------------------------
# a mixed pack, the buffer guard, windows cut to their buffers
# ------------------------------------------------------------------------------------------------------------------
def mixed_rows():
    """Different filters and lengths; rows packed with no gap (513 + 257 + 1 + 1200 samples from the odd position 3 on: odd and
    unaligned in_pos); a dead row; out_pos in another order than in_pos."""
    cs = H.CASES
    picks = [(cs[16], 513), (cs[6], 257), (cs[0], 1), None, (cs[15], 1200), (cs[9], 255), (cs[13], 2)]
    rows, pos = [], 3
    out_pos = {0: 2001, 1: 1, 2: 300, 4: 3000, 5: 2600, 6: 2900}
    for k, pk in enumerate(picks):
        if pk is None:
            rows.append(None)
            continue
        c, n = pk
        rows.append((c.x[:n], c.sos, pos, out_pos[k]))
        pos += n
    return picks, rows


def test_mixed_pack_and_buffer_guard():
    picks, rows = mixed_rows()
    for zero_phase in (True, False):
        out = run_pack(rows, arena=4300, zero_phase=zero_phase).cpu().numpy()
        written = np.zeros(out.shape[0], dtype=bool)
        for pk, r in zip(picks, rows):
            if pk is None:
                continue
            (c, n), q = pk, r[3]
            check_row(out[q:q + n], H.reference(c, n, zero_phase), "%s, %d samples, in_pos %d" % (c.id, n, r[2]))
            assert not written[q:q + n].any()
            written[q:q + n] = True
        assert (out[~written] == GUARD).all()


def test_windows_are_cut_to_their_buffers():
    """A window that starts before its buffer reads zeros there (the signal is zero outside the window, and nothing outside the
    buffer is touched); an output window that sticks out of the arena loses its tail and nothing else."""
    c = H.CASES[10]
    n = 300
    x = c.x[:n]
    # in: the row starts 5 samples before the buffer; out: the last 40 samples do not fit
    out = run_pack([(x, c.sos, -5, 20)], arena=20 + n - 40, x_total=n + 10).cpu().numpy()
    shifted = x.copy()
    shifted[:5] = 0.0
    ref = H.sos_zero_phase(c.sos, shifted.astype(np.float64))
    e = np.abs(out[20:].astype(np.float64) - ref[:n - 40]).max() / np.abs(ref).max()
    assert e <= H.GPU_BAR, e
    assert (out[:20] == GUARD).all()
    # a row longer than max_len is dropped, the others are not
    o2 = torch.full((1000,), GUARD, dtype=torch.float32, device=dev())
    buf = torch.from_numpy(np.concatenate([x, x])).to(dev())
    lowpass.sos_rows(buf, np.asarray([[0, 300, 0], [300, 200, 400]]), np.stack([pad_sos(c.sos)] * 2), out=o2, max_len=200)
    o2 = o2.cpu().numpy()
    assert (o2[:400] == GUARD).all() and (o2[600:] == GUARD).all()
    check_row(o2[400:600], H.reference(c, 200, True), "the row that fits")


# ------------------------------------------------------------------------------------------------------------------
# pack invariance
# ------------------------------------------------------------------------------------------------------------------
def test_a_row_has_the_same_bits_alone_in_any_pack_and_run_to_run():
    c, n = H.CASES[16], 1200
    picks, rows = mixed_rows()
    for zero_phase in (True, False):
        alone = run_pack([(c.x[:n], c.sos, 0, 0)], zero_phase=zero_phase)[:n]
        assert torch.equal(alone, run_pack([(c.x[:n], c.sos, 0, 0)], zero_phase=zero_phase)[:n])        # a rerun
        # behind other rows, at an odd position, written elsewhere
        a = run_pack(rows + [(c.x[:n], c.sos, 2301, 4301)], zero_phase=zero_phase)
        assert torch.equal(a[4301:4301 + n], alone)
        # in front of them, in another order of the table
        moved = [None if r is None else (r[0], r[1], r[2] + 1300, r[3] + 1300) for r in rows[::-1]]
        b = run_pack([(c.x[:n], c.sos, 64, 10)] + moved, zero_phase=zero_phase)
        assert torch.equal(b[10:10 + n], alone)
        for k, r in enumerate(rows):
            if r is not None:
                assert torch.equal(a[r[3]:r[3] + len(r[0])], b[r[3] + 1300:r[3] + 1300 + len(r[0])]), k


# ------------------------------------------------------------------------------------------------------------------
# the training path
# ------------------------------------------------------------------------------------------------------------------
OPT = dict(lr_sampling_rate=8000, hr_sampling_rate=48000, segment_length=1024)


@pytest.fixture(scope="module")
def corpus():
    from mdctgan_amd.train_data import pack_corpus
    rng = np.random.default_rng(5)
    waves = [torch.from_numpy((0.3 * rng.standard_normal(n)).astype(np.float32)) for n in (3000, 2900, 3100, 700)]
    return pack_corpus(waves, [48000, 16000, 48000, 16000], dev())


def batch_table(rates):
    """One filter per row at the row's file rate: both kinds, odd and even orders, an identity row."""
    menu = [("cheby1", 10, 3900.0, 0.5), ("butter", 7, 3600.0, None), ("cheby1", 3, 3990.0, 0.01), ("butter", 12, 3700.0, None),
            None, ("cheby1", 12, 3800.0, 1.0)]
    return np.stack([lowpass.identity_sos() if m is None else pad_sos(lowpass_sos(m[0], m[1], m[2], fs, m[3]))
                     for m, fs in zip(menu, rates)])


@pytest.mark.parametrize("add_noise", [False, True], ids=["plain", "add_noise"])
def test_training_batch_many_with_a_coefficient_table(corpus, add_noise):
    from mdctgan_amd.train_data import (draw_windows, make_training_pair, plan_training_batch, training_batch_many)
    idx = [0, 1, 2, 3, 1, 2]
    table = batch_table([corpus.rates[i] for i in idx])
    offs, lens = draw_windows(corpus, idx, 1024, 48000, torch.Generator().manual_seed(21))
    opt = dict(OPT, add_noise=add_noise, snr=30.0)
    noise = None
    if add_noise:
        plan = plan_training_batch(corpus, idx, offs, lens, 1024, 48000, 8000, add_noise=True)
        rng = np.random.default_rng(9)
        noise = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev()) for n in plan.lr_len]
    lr, hr = training_batch_many(corpus, idx, opt, offsets=offs, lengths=lens, noise=noise, lowpass=table)
    lr0, hr0 = training_batch_many(corpus, idx, opt, offsets=offs, lengths=lens, noise=noise)
    assert torch.equal(hr, hr0)                                             # hr has the bits it has without the feature
    assert not torch.equal(lr, lr0)
    assert torch.equal(lr[4], lr0[4])                                       # the identity row: x through 1 * x + 0 in double
    for b, i in enumerate(idx):
        s = corpus.starts[i] + int(offs[b])
        window = corpus.buffer[s:s + int(lens[b])][None]
        one_lr, one_hr = make_training_pair(window, corpus.rates[i], 48000, 8000, 1024, add_noise=add_noise, snr=30.0,
                                            noise=None if noise is None else noise[b][None], lowpass_sos=table[b])
        assert torch.equal(lr[b], one_lr[0]), b
        assert torch.equal(hr[b], one_hr[0]), b
    # a spec instead of a table: the filters are drawn after the windows, from the same generator
    spec = LowpassSpec()
    g = torch.Generator().manual_seed(33)
    offs2, lens2 = draw_windows(corpus, idx, 1024, 48000, g)
    drawn = lowpass.draw_lowpass([corpus.rates[i] for i in idx], 8000, spec, g)
    if not add_noise:
        a = training_batch_many(corpus, idx, opt, generator=torch.Generator().manual_seed(33), lowpass=spec)
        b = training_batch_many(corpus, idx, opt, offsets=offs2, lengths=lens2, lowpass=drawn)
        c = training_batch_many(corpus, idx, dict(opt, lowpass_aug="butter,cheby1"), generator=torch.Generator().manual_seed(33))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    # an unstable table is refused on the host
    bad = table.copy()
    bad[2, 1, 5] = 1.0
    with pytest.raises(ValueError, match="unstable"):
        training_batch_many(corpus, idx, opt, offsets=offs, lengths=lens, noise=noise, lowpass=bad)


def test_graphed_training_batch_with_lowpass():
    from mdctgan_amd.train_data import make_graphed_training_batch, pack_corpus, training_batch_many
    rng = np.random.default_rng(6)
    waves = [torch.from_numpy((0.3 * rng.standard_normal(n)).astype(np.float32)) for n in (3000, 2500, 900)]
    corp = pack_corpus(waves, [48000] * 3, dev())
    spec = LowpassSpec(("butter", "cheby1"), (1, 12), (0.01, 1.0), (0.8, 1.0))
    run = make_graphed_training_batch(corp, 4, OPT, lowpass=spec)
    for seed, idx in ((1, [0, 1, 2, 0]), (2, [2, 1, 1]), (3, [1, 0, 0, 2])):
        lr, hr = run(idx, generator=torch.Generator().manual_seed(seed))
        e_lr, e_hr = training_batch_many(corp, idx, OPT, generator=torch.Generator().manual_seed(seed), lowpass=spec)
        n = len(idx)
        assert torch.equal(lr[:n], e_lr) and torch.equal(hr[:n], e_hr), seed
        assert run.last_lowpass.shape == (n, 6, 6)
    # the device and dtype checks of a caller's buffers
    from mdctgan_amd import _lib
    need = _lib.load().mg_sos_rows_workspace(4, 1024)
    for bad_ws in (torch.empty(need - 1, dtype=torch.uint8, device=dev()), torch.empty(need, dtype=torch.float32, device=dev()),
                   torch.empty(need, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="workspace"):
            lowpass.sos_rows(corp.buffer, run.table[:, :3].contiguous(), torch.zeros(4, 6, 6, dtype=torch.float64, device=dev()),
                             out=run.filtered, max_len=1024, workspace=bad_ws)
    # the capture without the feature is what it was
    plain = make_graphed_training_batch(corp, 4, OPT)
    lr, hr = plain([0, 1, 2, 0], generator=torch.Generator().manual_seed(1))
    e_lr, e_hr = training_batch_many(corp, [0, 1, 2, 0], OPT, generator=torch.Generator().manual_seed(1))
    assert torch.equal(lr, e_lr) and torch.equal(hr, e_hr)


def test_the_capture_keeps_every_buffer_its_kernels_touch():
    """The graph holds raw pointers.  Whatever is allocated after make_graphed_training_batch has returned must survive a replay:
    the filter's workspace (268 doubles per chunk) lives as long as `run`, it does not go back to the allocator."""
    from mdctgan_amd import _lib
    from mdctgan_amd.train_data import make_graphed_training_batch, pack_corpus, training_batch_many
    L, B = 8192, 4
    opt = dict(OPT, segment_length=L)
    rng = np.random.default_rng(8)
    waves = [torch.from_numpy((0.3 * rng.standard_normal(n)).astype(np.float32)) for n in (20000, 17000, 9000)]
    corp = pack_corpus(waves, [48000] * 3, dev())
    idx = [0, 1, 2, 0]
    table = np.stack([pad_sos(lowpass_sos("cheby1", 10, 3800.0, 48000, 0.5))] * B)
    run = make_graphed_training_batch(corp, B, opt, lowpass=LowpassSpec())
    need = _lib.load().mg_sos_rows_workspace(B, L)
    assert run.workspace.numel() >= need and run.workspace.dtype == torch.uint8 and run.filtered.numel() >= B * L
    # blocks of every size up to the workspace's, taken after the capture: a freed workspace would be handed out here
    guards = [torch.full((need // 4 >> k,), GUARD, dtype=torch.float32, device=dev()) for k in range(6)]
    g = torch.Generator().manual_seed(4)
    lr, hr = run(idx, generator=g)
    first = (lr.clone(), hr.clone())
    e_lr, e_hr = training_batch_many(corp, idx, opt, generator=torch.Generator().manual_seed(4), lowpass=LowpassSpec())
    assert torch.equal(first[0], e_lr) and torch.equal(first[1], e_hr)
    # eager results allocated AFTER the capture, then a bare replay of the same tables: the same batch, and nothing else is written
    want = training_batch_many(corp, idx, opt, generator=torch.Generator().manual_seed(4), lowpass=LowpassSpec())
    kept = (want[0].clone(), want[1].clone())
    run.graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(want[0], kept[0]) and torch.equal(want[1], kept[1])
    assert torch.equal(lr, kept[0]) and torch.equal(hr, kept[1])
    for t in guards:
        assert bool((t == GUARD).all())
    # ... and with an explicit table
    want = training_batch_many(corp, idx, opt, generator=torch.Generator().manual_seed(5), lowpass=table)
    got = run(idx, generator=torch.Generator().manual_seed(5), lowpass=table)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for t in guards:
        assert bool((t == GUARD).all())


def test_the_legs_alone_have_the_pair_call_s_bits(corpus):
    """mg_train_hr_rows and mg_train_lr_rows are mg_train_pair_rows' two kernels: the same bits, lr_full included."""
    from mdctgan_amd.packed import upload_tables
    from mdctgan_amd.train_data import plan_training_batch, train_hr_rows, train_lr_rows, train_pair_rows, windows_at
    idx = [0, 2, 0]
    offs, lens = windows_at(corpus, idx, [5, 1000, 1975], 1024, 48000)
    for add_noise in (False, True):
        plan = plan_training_batch(corpus, idx, offs, lens, 1024, 48000, 8000, add_noise=add_noise)
        g = plan.groups[0]
        rows, = upload_tables([g.rows], dev())
        lr, hr, lr2, hr2 = (torch.full((3, 1024), GUARD, dtype=torch.float32, device=dev()) for _ in range(4))
        full, full2 = (torch.full((max(plan.full_total, 1),), GUARD, dtype=torch.float32, device=dev()) for _ in range(2))
        train_pair_rows(corpus.buffer, rows, 1024, 48000, 48000, 8000, hr, None if add_noise else lr, full if add_noise else None,
                        g.max_full_len)
        train_hr_rows(corpus.buffer, rows, 1024, 48000, 48000, hr2)
        train_lr_rows(corpus.buffer, rows, 1024, 48000, 48000, 8000, None if add_noise else lr2, full2 if add_noise else None,
                      g.max_full_len, out_rows=3)
        assert torch.equal(hr, hr2) and torch.equal(lr, lr2) and torch.equal(full, full2)


# ------------------------------------------------------------------------------------------------------------------
# argument refusals (a child process, fake pointers: no call gets as far as a launch)
# ------------------------------------------------------------------------------------------------------------------
child = H.child


@pytest.mark.parametrize("name", H.REFUSED)
def test_entry_points_return_mg_err_arg(child, name):
    assert int(child[name]) == H.MG_ERR_ARG
