"""tests/test_rows_geometry_gpu.py without a GPU: its restatements of the launch grids against hand-computed values, every one of
its case tables against the regime it is built for (a second trip of the loop it names, rows ending on, short of and past a trip),
and the row-wise forms of the imported references against those references.

The restatements mirror csrc/rows.h (rows_grid), csrc/resample.hip (mg_resample's bx), csrc/frames_common.h (frames_grid),
csrc/metrics_rows.hip (mg_lsd_rows' blocks) and csrc/train_rows.hip (tile_for) as they stand today; a cap that changes there is
not noticed here."""
import numpy as np
import pytest

import test_front_end_gpu as FE
import test_lowpass_host as LP
import test_mel_loss_host as MH
import test_mrstft_loss_host as SH
import test_rows_geometry_gpu as G


# ---------------------------------------------------------------------------------------------------------------------
# 0. the restatements
# ---------------------------------------------------------------------------------------------------------------------
def test_rows_grid_against_hand_computed_values():
    assert G.rows_grid(5, 20000, 256) == (79, 5)                    # ceil(20000 / 256) = 79 < 8192 // 5
    assert G.rows_grid(1030, 9000, 256) == (8, 1030)                # 8192 // 1030 = 7: the floor of 8 blocks
    assert G.rows_grid(70000, 3, 4096) == (1, 65535)
    assert G.rows_grid(1, 10 ** 9, 256) == (1024, 1)                # the ceiling of 1024 blocks
    assert G.rows_grid(6, 20000, 256) == (79, 6) and G.rows_grid(9, 70000, 4096) == (18, 9)      # test_front_end_gpu's launches
    assert G.rows_grid(40, 1000, 256) == (4, 40) and G.rows_grid(40, 10 ** 6, 256) == (204, 40)  # test_train_batch_gpu's: cap 204
    assert G.rows_grid(65535, 3, 256) == (1, 65535) and G.rows_grid(65536, 3, 256) == (1, 65535)


def test_the_other_grids_against_hand_computed_values():
    assert G.resample_blocks(1) == 1 and G.resample_blocks(262144) == 1024 and G.resample_blocks(262145) == 1024
    assert G.resample_blocks(7001 * 4) == 110
    # (frames per tile, tiles, blocks): the first frame counts with more tiles than blocks at n_fft = 2048
    assert G.lsd_rows_grid(6144, 2048) == (2, 3072, 3072) and G.lsd_rows_grid(6145, 2048) == (2, 3073, 3072)
    assert G.frames_grid(4096, 2048, 4096, 2) == (2, 2048, 2048) and G.frames_grid(4097, 2048, 4096, 2) == (2, 2049, 2048)
    assert G.frames_grid(3072, 2048, 2048, 3) == (1, 3072, 3072) and G.frames_grid(3073, 2048, 2048, 3) == (1, 3073, 3072)
    assert G.lsd_rows_grid(24577, 512) == (8, 3073, 3072) and G.frames_grid(12289, 512, 2048, 3) == (4, 3073, 3072)
    # tile_for: 12 kHz and 8 kHz up to 48 kHz (orig 1, width 7), 44.1 kHz (147 : 160), and a bank too long for the LDS window
    assert G.tile_for(1, 4, 7) == 1024 and G.tile_for(1, 6, 7) == 1024 and G.tile_for(147, 160, 7) == 1024
    assert G.tile_for(1, 1, 2046) == 3 and G.tile_for(1, 1, 2048) == 0      # K = 4093: three intermediates fit; K = 4097: none
    assert G.up_tile(12000) == G.up_tile(8000) == G.up_tile(44100) == 1024


def test_layout_and_packing_against_the_loops():
    lengths = [1, 37, 64, 65, 0, 128, 3]
    starts, total = G.layout(lengths)
    want_starts, want_total = FE.aligned_starts(lengths)
    assert list(starts) == want_starts and total == want_total
    flat = np.arange(sum(lengths), dtype=np.float32)
    buf = G.pack_rows(flat, starts, lengths, total)
    want = np.full(total + 2 * G.GUARD, G.SENTINEL, dtype=np.float32)
    at = 0
    for s, n in zip(starts, lengths):
        want[G.GUARD + s:G.GUARD + s + n] = flat[at:at + n]
        at += n
    assert np.array_equal(buf, want)
    assert np.array_equal(G.inside_mask(starts, lengths, total), want != G.SENTINEL)
    tight, end = G.layout(lengths, align=1, lead=3)
    assert list(tight) == [3, 4, 41, 105, 170, 170, 298] and end == 301
    assert np.array_equal(G.rows_2d(buf, starts, [1], 37)[0], flat[1:38])


# ---------------------------------------------------------------------------------------------------------------------
# 1. - 3. every case table is in its regime (the builders assert it; here they run without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", G.RESAMPLE_PAIRS)
def test_resample_rows_case_is_in_the_regime(orig, new):
    in_len, out_len = G.resample_rows_case(orig, new)
    assert len(out_len) == 1030 and {2047, 2048, 2049, 4097, 6143} <= set(out_len.tolist())
    assert (out_len[0], out_len[515], out_len[-1]) == (2049, 4097, 6143)
    assert in_len.sum() < 3e6 and G.layout(out_len)[1] < 3e6


def test_capped_cases_are_in_the_regime():
    assert G.resample_long_case()[3] == 280004
    for seed in (3, 4, 5):
        lengths = G.chunk_case(seed)
        assert {32767, 32768, 32769, 65537, 98303} <= set(lengths.tolist()) and G.layout(lengths)[1] < 3e6
    assert {8191, 8192, 8193, 16385, 24575} <= set(G.noise_case().tolist()) and G.noise_case().min() >= 2
    with pytest.raises(AssertionError):                             # the helper refuses what the older suites launch
        G.assert_later_x_trips(np.asarray(FE.MOMENT_LENGTHS), G.CHUNK)
    with pytest.raises(AssertionError):                             # ... and a table shrunk back under the cap
        G.assert_later_x_trips(np.minimum(G.chunk_case(3), 32768), G.CHUNK)


@pytest.mark.parametrize("fs,lr_rate", G.TRAIN_CONFIGS)
def test_train_cases_are_in_the_regime(fs, lr_rate):
    wins, table = G.pair_case(fs, lr_rate)
    assert len(table) == 1030 and len(set(wins)) == len(wins) == 9
    for f, off, n in wins:
        assert 0 <= off and off + n <= G.FILES[f]
    assert any(off + n == G.FILES[0] for f, off, n in wins if f == 0) and any(off == 0 for f, off, n in wins if f == 1)
    assert [G.hr_case(seg) for seg in G.HR_SEGS] == [2048] * 3


@pytest.mark.parametrize("fs,lr_rate,boundary", G.FULL_CONFIGS)
def test_lr_full_case_is_in_the_regime(fs, lr_rate, boundary):
    from mdctgan_amd.train_data import pair_lengths
    wins, table = G.full_case(fs, lr_rate, boundary)
    assert len(table) == 1030 and len(set(wins)) == len(wins) == 9
    for f, off, n in wins:
        assert 0 <= off and off + n <= G.FULL_FILES[f]
    full = sorted(pair_lengths(w[2], fs, G.HR_RATE, lr_rate)[2] for w in wins[4:])
    assert full == sorted([8192 + boundary[0], 8192, 8192 + boundary[2], 2 * 8192 + boundary[2], 3 * 8192 + boundary[0]])


def test_many_row_cases_are_in_the_regime():
    for seed, per_block, shortest in ((20, 256, 1), (23, G.CHUNK, 1), (25, 1024, 2), (27, G.CHUNK, 1), (35, 256, 1)):
        lengths = G.many_case(seed, per_block, shortest)
        assert len(lengths) == 65540 and lengths.max() == 3 and lengths[np.arange(65540) != G.DEAD].min() == shortest
    lengths, starts, total, rows = G.pcm_many_case()
    assert rows.shape == (65540, 6) and rows[G.DEAD, 1] == 0 and total < 3e6
    which, rows = G.train_many_case()
    assert rows.shape == (65540, 5) and rows[G.DEAD, 1] == 0 and (which[:6] == np.arange(6)).all()
    with pytest.raises(AssertionError):
        G.assert_later_y_trips(G.many_lengths(20)[:65535], 256)


@pytest.mark.parametrize("kernel", sorted(G.FRAME_KERNELS))
@pytest.mark.parametrize("n_fft", [2048, 512])
def test_frame_cases_are_past_the_block_cap(n_fft, kernel):
    lengths = G.frame_case(n_fft, kernel)
    assert sum(lengths) < 3e6
    with pytest.raises(AssertionError):                             # five rows of the shortest legal length stay under mg_lsd_rows' cap
        G.frame_case(n_fft, "lsd", [n_fft // 2 + 2] * 5)


# ---------------------------------------------------------------------------------------------------------------------
# the references taken row-wise are the imported references
# ---------------------------------------------------------------------------------------------------------------------
def test_row_wise_noise_references_equal_the_imported_ones():
    rng = np.random.default_rng(1)
    for n in (2, 3, 40):
        lr = (0.05 * rng.standard_normal((64, n))).astype(np.float32)
        z = rng.standard_normal((64, n)).astype(np.float32)
        for snr in FE.SNRS:
            G.pin_noise_refs(lr, z, snr, FE.SEG, range(64))


def test_the_cascade_runs_over_rows_side_by_side():
    c = LP.CASES[16]
    x = (0.5 * np.random.default_rng(2).standard_normal((5, 3))).astype(np.float32)
    one = LP.sos_cascade(c.sos, x.T).T
    two = LP.sos_zero_phase(c.sos, x.T.astype(np.float64)).T
    for r in range(5):
        assert np.array_equal(one[r], LP.sos_cascade(c.sos, x[r]))
        assert np.array_equal(two[r], LP.sos_zero_phase(c.sos, x[r].astype(np.float64)))


@pytest.mark.parametrize("n_fft", G.FRAME_SIZES)
def test_frame_inputs_are_tie_free(n_fft):
    """the margins tests/test_mrstft_loss_host.py and tests/test_mel_loss_host.py ask of their GPU inputs, at hop 1: a bin is
    -ln SCALES[u] from a tie unless one of its two powers is under the clamp"""
    pairs = G.frame_pairs(n_fft)
    assert len(pairs) <= len(G.SCALES) and min(abs(np.log(a)) for a in G.SCALES) > 0.22
    for hr, sr in pairs:
        ln, p, _, _ = SH.tie_margins(hr, sr, n_fft, G.HOP)
        assert ln >= 1e-6 and p >= 1e-3, (n_fft, len(hr), ln, p)
    MH.check_margins("%d hop 1" % n_fft, pairs, [(n_fft, G.HOP, G.mel_bank(n_fft))])
