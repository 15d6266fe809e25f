"""The later trips of every stride loop of the packed-rows and frame-tile kernels.

Every row-table kernel walks its work with stride loops over a capped grid (csrc/rows.h: rows_grid; csrc/frames_common.h:
frames_grid); the other suites stay inside the first trip of each.  Here every case is built to take a second (and third) trip
of the loop it is named for, and says so through the restatements of section 0 before it launches anything:
  1. capped x grids: packs of 1030 rows (x cap: 8 blocks), about 1025 of them 1 to 40 samples long, five around the trip
     boundaries T = 8 * per_block (T + 1 first in the table, T - 1, 2 T + 1 in the middle, T, 3 T - 1 last);
  2. more than 65535 rows (r += gridDim.y): 65540 rows of 1 to 3 samples, row 65536 dead;
  3. the frame-tile kernels past their block cap, where a tile of a later trip straddles two rows.
The references and the bars are the ones the kernels' own suites use, imported from them: oracle/resample.py at the bar of
tests/test_resample.py, the moments and noise bars of tests/test_front_end_gpu.py, the float64 sums of
tests/test_metrics_many_gpu.py, the restatements of tests/test_wavio_host.py and tests/test_lowpass_host.py, make_training_pair
bit for bit (tests/test_train_batch_gpu.py), and the float64 / float32 autograd yardsticks of the three loss suites.  Nothing here
is a new tolerance.  tests/test_rows_geometry_host.py checks the restatements against hand-computed grids and every case table
below against its regime without a GPU; it cannot notice a cap that changes in the C source.
"""
import functools
import math

import numpy as np
import pytest
import torch

import test_front_end_gpu as FE
import test_lowpass_host as LP
import test_lsd_loss_host as LH
import test_mel_loss_host as MH
import test_mrstft_loss_host as SH
import test_wavio_host as WH
from oracle import resample as R

_gpu = pytest.mark.gpu
DEV = "cuda"
SENTINEL, GUARD, SEG = FE.SENTINEL, FE.GUARD, FE.SEG
CHUNK = 4096                                     # MG_MOMENTS_CHUNK


# ---------------------------------------------------------------------------------------------------------------------
# 0. the grids, restated, and what a case must show before it runs
# ---------------------------------------------------------------------------------------------------------------------
def rows_grid(n_rows, max_len, per_block):
    """csrc/rows.h: rows_grid -> (blocks in x, blocks in y)"""
    gy = min(n_rows, 65535)
    bx = -(-max_len // per_block)
    bx = min(bx, max(8192 // gy, 8))
    return max(1, min(bx, 1024)), gy


def resample_blocks(out_len):
    """csrc/resample.hip: mg_resample's `bx`, blocks of 256 output samples"""
    return min(-(-out_len // 256), 1024)


def frames_grid(total_frames, n_fft, tile, wg_per_cu):
    """csrc/frames_common.h: frames_grid -> (frames per tile, tiles, blocks)"""
    ft = tile // n_fft
    n_tiles = -(-total_frames // ft)
    return ft, n_tiles, min(n_tiles, wg_per_cu * 256 * 4)


def lsd_rows_grid(total_frames, n_fft):
    """csrc/metrics_rows.hip: mg_lsd_rows' `ft`, `n_tiles` and `blocks` (LSD_TILE = 4096, three workgroups per CU)"""
    return frames_grid(total_frames, n_fft, 4096, 3)


def tile_for(orig, new, width):
    """csrc/train_rows.hip: tile_for (kMidCap = 4096 intermediates in LDS, kTile = 1024)"""
    m = (4096 - (2 * width + orig)) // orig - 1
    return 0 if m < 0 else min((m + 1) * new, 1024)


N_ROWS = 1030                                    # gy = 1030: the x cap is max(8192 // 1030, 8) = 8 blocks
LONG_AT = (0, 257, 515, 772, 1029)               # where the long rows sit: first, last, the middle and two more
N_MANY, DEAD = 65540, 65536                      # part 2: two trips of r += gridDim.y; block y = 1 meets the dead row on its second


def capped_lengths(T, seed, shortest=1):
    """1030 row lengths: 1025 of `shortest` to 40 samples and, at LONG_AT, T + 1, T - 1, 2 T + 1, T and 3 T - 1"""
    n = np.random.default_rng(seed).integers(shortest, 41, N_ROWS).astype(np.int64)
    n[list(LONG_AT)] = [T + 1, T - 1, 2 * T + 1, T, 3 * T - 1]
    return n


def assert_later_x_trips(lengths, per_block, boundary=(-1, 0, 1)):
    """The launch over `lengths` is capped at 8 x blocks of `per_block` samples, rows end `boundary` samples off the first trip's
    end T = 8 * per_block, and rows take two and three trips.  -> T"""
    lengths = np.asarray(lengths, dtype=np.int64)
    bx, gy = rows_grid(len(lengths), int(lengths.max()), per_block)
    assert (bx, gy) == (8, len(lengths)), (bx, gy)
    T = bx * per_block
    trips = -(-lengths // T)
    for d in boundary:
        assert T + d in lengths, (T, d)
    assert trips[lengths == T + boundary[1]].max() == 1 and trips[lengths == T + boundary[2]].min() == 2
    assert 3 in trips and np.median(lengths) <= 40
    assert min(lengths[0], lengths[len(lengths) // 2], lengths[-1]) >= T + boundary[0]       # a long row first, in the middle, last
    return T


def many_lengths(seed, shortest=1):
    """65540 row lengths of `shortest` to 3 samples; row 65536 is dead, rows 0 and 65535 (block y = 0 on both trips) are alike, the
    last row (block y = 4 on its second trip) has 3 samples where row 4 and its neighbours have `shortest` or 2"""
    n = np.random.default_rng(seed).integers(shortest, 4, N_MANY).astype(np.int64)
    n[3:6] = (shortest, 2, shortest)
    n[65535] = n[0]
    n[DEAD] = 0
    n[-1] = 3
    return n


def assert_later_y_trips(lengths, per_block):
    """More rows than the y grid has blocks: every block takes a second trip of r += gridDim.y for some row"""
    lengths = np.asarray(lengths, dtype=np.int64)
    bx, gy = rows_grid(len(lengths), int(lengths.max()), per_block)
    assert (bx, gy) == (1, 65535) and -(-len(lengths) // gy) == 2
    assert lengths[DEAD] == 0 and lengths[0] == lengths[65535] and lengths[-1] != lengths[len(lengths) - 1 - gy]
    return gy


# ---------------------------------------------------------------------------------------------------------------------
# packing, vectorised: rows at aligned starts of one buffer, a sentinel in the gaps and in 64 guard samples on both sides
# ---------------------------------------------------------------------------------------------------------------------
def layout(lengths, align=64, lead=0):
    """test_front_end_gpu.aligned_starts without the loop -> (starts int64 [n], total)"""
    lengths = np.asarray(lengths, dtype=np.int64)
    span = -(-lengths // align) * align
    return lead + np.cumsum(span) - span, int(lead + span.sum())


def firsts(lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    return np.cumsum(lengths) - lengths


def positions(starts, lengths):
    """the buffer position of every sample of every row, rows in table order"""
    lengths = np.asarray(lengths, dtype=np.int64)
    return np.repeat(np.asarray(starts, dtype=np.int64) - firsts(lengths), lengths) + np.arange(int(lengths.sum()))


def pack_rows(flat, starts, lengths, total, fill=SENTINEL, guard=GUARD):
    """[guard | rows, `fill` in the gaps | guard] on the host, `flat` holding the rows' samples one after the other"""
    buf = np.full(total + 2 * guard, fill, dtype=flat.dtype)
    buf[guard + positions(starts, lengths)] = flat
    return buf


def inside_mask(starts, lengths, total, guard=GUARD):
    m = np.zeros(total + 2 * guard, dtype=bool)
    m[guard + positions(starts, lengths)] = True
    return m


def on_device(buf, guard=GUARD):
    """-> (the whole buffer on the device, the part between the guards)"""
    whole = torch.from_numpy(buf).to(DEV)
    return whole, whole[guard:whole.numel() - guard]


def groups_of(lengths):
    """[(length, rows of that length)] for the live rows: equal lengths reshape to 2-D"""
    lengths = np.asarray(lengths)
    return [(int(n), np.flatnonzero(lengths == n)) for n in np.unique(lengths) if n > 0]


def rows_2d(buf, starts, rows, n, guard=GUARD):
    """[len(rows), n]: the windows of `rows` (all n samples long) of a guarded host buffer"""
    return buf[guard + np.asarray(starts)[rows][:, None] + np.arange(n)[None, :]]


def noise_wave(n, seed, scale=0.1, offset=0.0):
    return (scale * np.random.default_rng(seed).standard_normal(n) + offset).astype(np.float32)


def moments_bar(seg, got, what):
    """the moments bar of test_front_end_gpu: N 2^-52 of sum |x| (sum x^2)"""
    d = seg.astype(np.float64)
    n = d.size
    e1, e2 = abs(got[0] - d.sum()), abs(got[1] - (d * d).sum())
    assert e1 <= n * 2.0 ** -52 * np.abs(d).sum(), (what, n, e1)
    assert e2 <= n * 2.0 ** -52 * (d * d).sum(), (what, n, e2)


def moments_bar_2d(x, got, what):
    """moments_bar for rows of one length: x [k, n] float32, got [k, 2]"""
    d = x.astype(np.float64)
    n = d.shape[1]
    e1, e2 = np.abs(got[:, 0] - d.sum(1)), np.abs(got[:, 1] - (d * d).sum(1))
    assert (e1 <= n * 2.0 ** -52 * np.abs(d).sum(1)).all(), (what, n, e1.max())
    assert (e2 <= n * 2.0 ** -52 * (d * d).sum(1)).all(), (what, n, e2.max())


# ---------------------------------------------------------------------------------------------------------------------
# 1a. mg_resample_rows: o += gridDim.x * blockDim.x
# ---------------------------------------------------------------------------------------------------------------------
RESAMPLE_PAIRS = [(48000, 8000), (8000, 48000), (44100, 48000)]          # the last: the filter bank stays in L2


def resample_rows_case(orig, new):
    """-> (in_len, out_len) of 1030 rows, T = 8 * 256 output samples.  The table's out_len is the wanted one: 6 L and
    ceil(160 L / 147) do not reach every length, so a row reads the shortest input that has at least that many outputs and its
    window is the first out_len of them (what the training path's crop does)."""
    g = math.gcd(orig, new)
    out_len = capped_lengths(2048, orig // 100 + new // 1000)
    assert assert_later_x_trips(out_len, 256) == 2048
    in_len = -(-out_len * (orig // g) // (new // g))
    assert (-(-in_len * (new // g) // (orig // g)) >= out_len).all()
    return in_len, out_len


def oracle_rows(got, flat, in_len, out_len, out_start, shift, orig, new, what):
    """every row against oracle.resample in float64 at the bar of tests/test_resample.py (3e-6 of the call's largest sample), rows
    of one length as one [k, L] call"""
    first = firsts(in_len)
    for m, rows in groups_of(out_len):
        n = int(in_len[rows[0]])
        x = flat[first[rows][:, None] + np.arange(n)[None, :]]
        if shift is not None:
            x = x + shift[rows][:, None]
        assert x.dtype == np.float32
        want = R.resample(x, orig, new)[:, :m]
        g = rows_2d(got, out_start, rows, m)
        assert g.shape == want.shape
        assert np.abs(g - want).max() <= 3e-6 * np.abs(want).max(), (what, m, len(rows))


@_gpu
@pytest.mark.parametrize("with_shift", [False, True], ids=["plain", "shift"])
@pytest.mark.parametrize("orig,new", RESAMPLE_PAIRS)
def test_resample_rows_later_x_trips(orig, new, with_shift):
    """1030 rows, 8 x blocks per row: rows of 2047, 2048, 2049, 4097 and 6143 output samples among 1025 short ones.  Every window
    has the bits of resample() on that row alone (n_rows = 1, an uncapped grid, one trip) and lies within the oracle's bar;
    nothing outside the windows changes in either buffer."""
    from mdctgan_amd.resample import resample, resample_rows
    in_len, out_len = resample_rows_case(orig, new)
    flat = noise_wave(int(in_len.sum()), orig + new + with_shift)
    in_start, in_total = layout(in_len)
    out_start, out_total = layout(out_len)
    x_all, x = on_device(pack_rows(flat, in_start, in_len, in_total))
    x_before = x_all.clone()
    table = torch.from_numpy(np.stack([in_start, in_len, out_start, out_len], axis=1)).to(DEV)
    shift_h = (1e-3 * np.random.default_rng(7).standard_normal(N_ROWS)).astype(np.float32) if with_shift else None
    shift = None if shift_h is None else torch.from_numpy(shift_h).to(DEV)
    out_all = torch.full((out_total + 2 * GUARD,), SENTINEL, device=DEV)
    resample_rows(x, table, int(out_len.max()), orig, new, out_all[GUARD:GUARD + out_total], shift=shift)
    want_all = torch.full_like(out_all, SENTINEL)
    for u in range(N_ROWS):
        a, n, b, m = int(in_start[u]), int(in_len[u]), GUARD + int(out_start[u]), int(out_len[u])
        alone = x[a:a + n].clone() if shift is None else x[a:a + n] + shift[u]
        want_all[b:b + m] = resample(alone[None], orig, new)[0, :m]
    if not torch.equal(out_all, want_all):
        bad = torch.nonzero(out_all != want_all).flatten()
        first_bad = int(bad[0]) - GUARD
        u = int(np.searchsorted(out_start, first_bad, side="right")) - 1
        raise AssertionError("%d samples differ, the first at sample %d of row %d (%d output samples)"
                             % (bad.numel(), first_bad - int(out_start[u]), u, int(out_len[u])))
    assert torch.equal(x_all, x_before)
    oracle_rows(out_all.cpu().numpy(), flat, in_len, out_len, out_start, shift_h, orig, new, (orig, new, with_shift))


# ---------------------------------------------------------------------------------------------------------------------
# 1b. mg_resample: o += gridDim.x * blockDim.x of resample_kernel
# ---------------------------------------------------------------------------------------------------------------------
RESAMPLE_LONG = (70001, 12000, 48000)            # [2, L] at 12 kHz -> 280004 samples a row, past the 1024 * 256 of one trip


def resample_long_case():
    L, orig, new = RESAMPLE_LONG
    out_len = -(-L * new // orig)
    assert out_len > resample_blocks(out_len) * 256 and resample_blocks(out_len) == 1024
    return L, orig, new, out_len


@_gpu
def test_resample_past_its_block_cap():
    from mdctgan_amd.resample import resample
    L, orig, new, out_len = resample_long_case()
    x = noise_wave(2 * L, 12).reshape(2, L)
    want = R.resample(x, orig, new)
    got = resample(torch.from_numpy(x).to(DEV), orig, new).cpu().numpy()
    assert got.shape == want.shape == (2, out_len)
    e = np.abs(got - want)
    print("mg_resample 2 x %d -> %d: error %.3e of the peak (second trip alone: %.3e)"
          % (L, out_len, e.max() / np.abs(want).max(), e[:, 1024 * 256:].max() / np.abs(want).max()))
    assert e.max() <= 3e-6 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------------
# 1c. mg_rows_moments: c += gridDim.x
# ---------------------------------------------------------------------------------------------------------------------
def chunk_case(seed, shortest=1):
    lengths = capped_lengths(8 * CHUNK, seed, shortest)
    assert assert_later_x_trips(lengths, CHUNK) == 32768
    return lengths


@_gpu
def test_rows_moments_later_chunk_trips():
    """Rows of 32767, 32768, 32769, 65537 and 98303 samples (8, 8, 9, 17 and 24 chunks over 8 blocks) among 1025 short ones against
    numpy float64 at the moments bar; every long row (and three short ones) alone has the bits it has in the pack."""
    from mdctgan_amd.resample import rows_moments
    lengths = chunk_case(3)
    flat = noise_wave(int(lengths.sum()), 30, offset=0.01)
    starts, total = layout(lengths)
    _, x = on_device(pack_rows(flat, starts, lengths, total))
    table = torch.from_numpy(np.stack([np.zeros_like(starts), starts, starts + lengths], axis=1)).to(DEV)
    got = rows_moments(x, table, int(lengths.max()))
    assert got.dtype == torch.float64 and tuple(got.shape) == (N_ROWS, 2)
    assert torch.equal(got, rows_moments(x, table, int(lengths.max())))
    host, first = got.cpu().numpy(), firsts(lengths)
    for u in range(N_ROWS):
        moments_bar(flat[first[u]:first[u] + lengths[u]], host[u], u)
    for u in LONG_AT + (1, 514, 1028):
        n = int(lengths[u])
        w = x[int(starts[u]):int(starts[u]) + n].clone()
        alone = rows_moments(w, torch.tensor([(0, 0, n)], dtype=torch.int64, device=DEV), n)
        assert torch.equal(alone[0], got[u]), (u, n)


# ---------------------------------------------------------------------------------------------------------------------
# 1d. mg_metrics_rows_packed: c += gridDim.x
# ---------------------------------------------------------------------------------------------------------------------
def metrics_packed(hb, lb, sb, table, max_len, shift):
    """mg_metrics_rows_packed on host buffers -> float64 [rows, 3] (host), the output inside a guard-filled array"""
    from mdctgan_amd import _lib
    lib = _lib.load()
    U = table.shape[0]
    rows = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)).to(DEV)
    hd, ld, sd = (torch.from_numpy(b).to(DEV) for b in (hb, lb, sb))
    shd = None if shift is None else torch.from_numpy(shift).to(DEV)
    nbytes = lib.mg_metrics_rows_packed_workspace(U, int(max_len))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((U + 2, 3), -7.0, dtype=torch.float64, device=DEV)
    _lib.check(lib.mg_metrics_rows_packed(_lib.ptr(hd), hd.numel(), _lib.ptr(ld), ld.numel(), _lib.ptr(sd), sd.numel(),
                                          _lib.ptr(rows), U, int(max_len), _lib.ptr(shd), _lib.ptr(out[1:]), _lib.ptr(ws), nbytes,
                                          _lib.stream()), "mg_metrics_rows_packed")
    got = out.cpu().numpy()
    assert np.all(got[0] == -7.0) and np.all(got[-1] == -7.0)
    return got[1:-1]


def metric_triples(lengths, seed):
    """hr, lr, sr as flat float32 arrays, the rows one after the other (test_metrics_many_gpu's signals)"""
    rng = np.random.default_rng(seed)
    n = int(np.asarray(lengths).sum())
    hr = (0.1 * rng.standard_normal(n)).astype(np.float32)
    sr = (hr + 0.01 * rng.standard_normal(n)).astype(np.float32)
    lr = (hr + 0.03 * rng.standard_normal(n)).astype(np.float32)
    return hr, lr, sr


def metric_packs(hr, lr, sr, lengths):
    """hr at 64-sample starts, sr four samples in, lr packed tightly from sample 3 (test_metrics_many_gpu's layout); 1e3 between
    the rows.  -> the three buffers and the table hr_pos, lr_pos, sr_pos, len"""
    hs, ht = layout(lengths)
    ss, st = layout(lengths, lead=4)
    ls, lt = layout(lengths, align=1, lead=3)
    hb = pack_rows(hr, hs, lengths, ht, fill=np.float32(1e3), guard=0)
    sb = pack_rows(sr, ss, lengths, st + 7, fill=np.float32(1e3), guard=0)
    lb = pack_rows(lr, ls, lengths, lt + 2, fill=np.float32(1e3), guard=0)
    return hb, lb, sb, np.stack([hs, ls, ss, np.asarray(lengths, dtype=np.int64)], axis=1)


def metric_sums(h, l, s, axis=None):
    h, l, s = (a.astype(np.float64) for a in (h, l, s))
    return np.stack([(h * h).sum(axis), ((s - h) ** 2).sum(axis), ((l - h) ** 2).sum(axis)], axis=-1)


@_gpu
@pytest.mark.parametrize("with_shift", [False, True], ids=["plain", "shift"])
def test_metrics_rows_packed_later_chunk_trips(with_shift):
    """The chunk_case rows through mg_metrics_rows_packed: float64 numpy sums to 1e-12 (the bound of
    test_metrics_rows_packed_against_float64), and every long row alone has the bits it has in the pack."""
    lengths = chunk_case(4)
    hr, lr, sr = metric_triples(lengths, 40 + with_shift)
    shift = (1e-3 * np.random.default_rng(41).standard_normal(N_ROWS)).astype(np.float32) if with_shift else None
    hb, lb, sb, table = metric_packs(hr, lr, sr, lengths)
    got = metrics_packed(hb, lb, sb, table, lengths.max(), shift)
    first = firsts(lengths)
    worst = 0.0
    for u in range(N_ROWS):
        w = slice(first[u], first[u] + lengths[u])
        h = hr[w] + shift[u] if with_shift else hr[w]
        assert h.dtype == np.float32
        want = metric_sums(h, lr[w], sr[w])
        err = np.abs(got[u] - want)
        worst = max(worst, float((err / want).max()))
        assert np.all(err <= 1e-12 * want), (u, lengths[u], got[u], want)
    print("mg_metrics_rows_packed 1030 rows shift=%s: worst relative error %.3g" % (with_shift, worst))
    for u in LONG_AT:
        w = slice(first[u], first[u] + lengths[u])
        one = np.asarray([[0, 0, 0, lengths[u]]], dtype=np.int64)
        alone = metrics_packed(hr[w].copy(), lr[w].copy(), sr[w].copy(), one, lengths[u], None if shift is None else shift[u:u + 1])
        assert np.array_equal(alone[0], got[u]), (u, lengths[u])


# ---------------------------------------------------------------------------------------------------------------------
# 1e. mg_pcm_decode_rows with moments: c += gridDim.x
# ---------------------------------------------------------------------------------------------------------------------
def pcm_layouts():
    from mdctgan_amd.wavio import MG_PCM_S16, MG_PCM_S24, MG_PCM_S32, MG_PCM_U8
    return [(MG_PCM_S16, 1, 0), (MG_PCM_S24, 2, 1), (MG_PCM_S32, 1, 0), (MG_PCM_U8, 3, 2)]      # format, channels, the channel taken


@_gpu
def test_pcm_decode_rows_later_chunk_trips():
    """The chunk_case rows (frames) as 16-bit mono, 24-bit stereo, 32-bit mono and 8-bit three-channel payloads in one launch: the
    bits of the numpy restatement, the sentinel in every gap, rows_moments' bits, numpy float64 at the moments bar, and every long
    row alone with the bits it has in the pack."""
    from mdctgan_amd.packed import rows_moments
    from mdctgan_amd.wavio import SAMPLE_BYTES
    from test_wavio_gpu import raw_decode, stage, windows
    lengths = chunk_case(5)
    kinds = pcm_layouts()
    files = [kinds[u % 4] + (int(n),) for u, n in enumerate(lengths)]
    assert len({files[u][0] for u in LONG_AT}) == 3                                # the long rows: three sample formats
    payloads = [WH.payload_for(code, ch, n, seed=u) for u, (code, ch, _, n) in enumerate(files)]
    data, byte_starts = stage(payloads)
    starts, total = layout(lengths)
    rows = np.asarray([[s, n, ch, c, code, d] for (code, ch, c, n), s, d in zip(files, byte_starts, starts)], dtype=np.int64)
    want = [WH.np_decode(p, code, ch)[c] for p, (code, ch, c, _) in zip(payloads, files)]
    data_t = torch.from_numpy(data).to(DEV)
    out, mom = raw_decode(data_t, rows, total, prefill=SENTINEL)
    got = out.cpu().numpy()
    for u in range(N_ROWS):
        assert WH.bits_equal(got[starts[u]:starts[u] + lengths[u]], want[u]), (u, files[u])
    assert (got[~inside_mask(starts, lengths, total, guard=0)] == SENTINEL).all()
    ref = rows_moments(out, windows(rows), int(lengths.max()))
    assert torch.equal(mom.view(torch.int64), ref.view(torch.int64))
    host = mom.cpu().numpy()
    for u in range(N_ROWS):
        moments_bar(want[u], host[u], (u, files[u]))
    for u in LONG_AT:
        code, ch, c, n = files[u]
        assert len(payloads[u]) == n * ch * SAMPLE_BYTES[code]
        alone = torch.from_numpy(np.frombuffer(payloads[u], dtype=np.uint8).copy()).to(DEV)
        o, m = raw_decode(alone, np.asarray([[0, n, ch, c, code, 0]], dtype=np.int64), n)
        assert torch.equal(o.view(torch.int32), out[int(starts[u]):int(starts[u]) + n].view(torch.int32)), (u, files[u])
        assert torch.equal(m.view(torch.int64), mom[u:u + 1].view(torch.int64)), (u, files[u])


# ---------------------------------------------------------------------------------------------------------------------
# 1f. mg_add_noise_rows: p += 4 * gridDim.x * blockDim.x
# ---------------------------------------------------------------------------------------------------------------------
def noise_case():
    lengths = capped_lengths(8 * 1024, 6, shortest=2)
    assert assert_later_x_trips(lengths, 1024) == 8192
    return lengths


def noise_flats(lengths, seed):
    rng = np.random.default_rng(seed)
    n = int(np.asarray(lengths).sum())
    return (0.05 * rng.standard_normal(n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)


@_gpu
def test_add_noise_rows_later_x_trips():
    """Rows of 8191, 8192, 8193, 16385 and 24575 samples among 1025 of 2 to 40 (rows start on 64 samples, so a trip is 8192 samples
    from the row's first): every row against noise_ref64 under noise_passes, nothing outside the windows changes, and every long
    row alone has the bits it has in the pack."""
    from mdctgan_amd.resample import add_noise_rows, rows_moments
    snr = 10.0
    lengths = noise_case()
    a, z = noise_flats(lengths, 60)
    starts, total = layout(lengths)
    lr_all, lr = on_device(pack_rows(a, starts, lengths, total))
    z_all, zd = on_device(pack_rows(z, starts, lengths, total))
    before, z_before = lr_all.clone(), z_all.clone()
    table = torch.from_numpy(np.stack([np.zeros_like(starts), starts, starts + lengths], axis=1)).to(DEV)
    longest = int(lengths.max())
    add_noise_rows(lr, zd, table, longest, rows_moments(lr, table, longest), rows_moments(zd, table, longest), snr, SEG)
    got = lr_all.cpu().numpy()
    first, worst = firsts(lengths), 0.0
    for u in range(N_ROWS):
        w = slice(first[u], first[u] + lengths[u])
        ok, margin = FE.noise_passes(got[GUARD + starts[u]:GUARD + starts[u] + lengths[u]], FE.noise_ref32(a[w], z[w], snr, SEG),
                                     FE.noise_ref64(a[w], z[w], snr, SEG))
        worst = max(worst, margin)
        assert ok, (u, lengths[u], margin)
    print("mg_add_noise_rows 1030 rows: worst error / bar %.3e" % worst)
    outside = torch.from_numpy(~inside_mask(starts, lengths, total)).to(DEV)
    assert torch.equal(lr_all[outside], before[outside]) and torch.equal(z_all, z_before)
    for u in LONG_AT:
        n, w = int(lengths[u]), slice(first[u], first[u] + lengths[u])
        one, zone = torch.from_numpy(a[w].copy()).to(DEV), torch.from_numpy(z[w].copy()).to(DEV)
        t1 = torch.tensor([(0, 0, n)], dtype=torch.int64, device=DEV)
        add_noise_rows(one, zone, t1, n, rows_moments(one, t1, n), rows_moments(zone, t1, n), snr, SEG)
        assert torch.equal(one, lr[int(starts[u]):int(starts[u]) + n]), (u, n)


# ---------------------------------------------------------------------------------------------------------------------
# 1g. mg_train_pair_rows, mg_train_hr_rows, mg_train_lr_rows: o += gridDim.x * kThreads and tile += gridDim.x
# ---------------------------------------------------------------------------------------------------------------------
HR_RATE = 48000
PAIR_SEG = 8 * 1024 + 1                          # one sample past 8 tiles of the low-rate leg; 33 blocks of 256 of the high-rate leg
TRAIN_CONFIGS = [(48000, 12000), (16000, 8000)]  # (file rate, low rate): hr is a copy / a 1:3 bank
FILES = [16384, 12288, 4096]                     # multiples of 64: the files sit back to back


def up_tile(lr_rate):
    """tile_for of the lr -> hr bank: 12000 -> 48000 is (orig 1, new 4, width 7), 8000 -> 48000 (1, 6, 7); both give
    (4096 - 15) / 1 = 4081 intermediates' worth of outputs, cut to kTile = 1024.  44100 -> 48000 (147, 160, 7): 26 * 160, cut to 1024."""
    _, width, orig, new = R.sinc_resample_kernel(lr_rate, HR_RATE)
    return tile_for(orig, new, width)


def train_windows(fs):
    """(file, offset, length): windows whose high-rate length lies around the legs' trip ends, at the first sample of the corpus,
    up to the last sample of file 0 (where file 1 begins), from the first sample of file 1, and the short file whole"""
    want_hr = [37, 2047, 2048, 2049, 4097, 8191, PAIR_SEG, PAIR_SEG + 807]
    lens = [-(-t * fs // HR_RATE) for t in want_hr]
    wins = []
    for i, n in enumerate(lens):
        f = i % 2
        wins.append((f, 0 if i % 4 < 2 else FILES[f] - n, n))
    return wins + [(2, 0, FILES[2])]


def pair_case(fs, lr_rate):
    tile = up_tile(lr_rate)
    assert tile == 1024
    bh, _ = rows_grid(N_ROWS, PAIR_SEG, 256)
    bl, _ = rows_grid(N_ROWS, PAIR_SEG, tile)
    assert (bh, bl) == (8, 8)
    assert -(-(-(-PAIR_SEG // 256)) // bh) == 5 and -(-(-(-PAIR_SEG // tile)) // bl) == 2       # trips of the two legs
    assert PAIR_SEG == bl * tile + 1
    wins = train_windows(fs)
    return wins, [wins[b % len(wins)] for b in range(N_ROWS)]


def noise_corpus(lengths, fs, seed):
    from mdctgan_amd import train_data as T
    gen = torch.Generator().manual_seed(seed)
    return T.pack_corpus([0.1 * torch.randn(n, generator=gen) + 0.01 for n in lengths], [fs] * len(lengths), DEV)


def window_alone(corpus, f, off, n):
    s0 = corpus.starts[f] + off
    return corpus.buffer[s0:s0 + n].clone().view(1, -1)


def assert_duplicates(got, n_distinct, what):
    """row b of a table that cycles through n_distinct windows equals row b % n_distinct"""
    B = got.shape[0]
    assert torch.equal(got, got[torch.arange(B, device=got.device) % n_distinct]), what


@_gpu
@pytest.mark.parametrize("fs,lr_rate", TRAIN_CONFIGS)
def test_train_pair_rows_later_x_trips(fs, lr_rate):
    """1030 rows of 8193 samples (the loop bound of both legs is the segment, shared by a launch: five trips of the high-rate leg,
    two of the low-rate leg's tiles) cycling through nine windows whose signals end around 2048, 4096 and 8192 samples: every
    distinct window has make_training_pair's bits, the duplicates equal their first occurrence, and the single-leg entry points
    give the pair call's bits.  (1030 dense rows of more than 8 * 1024 samples are 8.4 M floats a leg: the kernels' output is
    dense, so this is the least such a launch can write.)"""
    from mdctgan_amd import train_data as T
    from mdctgan_amd.packed import upload_tables
    from mdctgan_amd.resample import make_training_pair
    wins, table = pair_case(fs, lr_rate)
    corpus = noise_corpus(FILES, fs, fs // 1000 + lr_rate // 1000)
    idx, off, ln = ([w[k] for w in table] for k in range(3))
    opt = dict(hr_sampling_rate=HR_RATE, lr_sampling_rate=lr_rate, segment_length=PAIR_SEG)
    got_lr, got_hr = T.training_batch_many(corpus, idx, opt, offsets=off, lengths=ln)
    assert tuple(got_lr.shape) == tuple(got_hr.shape) == (N_ROWS, PAIR_SEG)
    for b, (f, o, n) in enumerate(wins):
        want_lr, want_hr = make_training_pair(window_alone(corpus, f, o, n), fs, HR_RATE, lr_rate, PAIR_SEG)
        assert torch.equal(got_hr[b], want_hr[0]), ("hr", b, f, o, n)
        assert torch.equal(got_lr[b], want_lr[0]), ("lr", b, f, o, n)
    assert_duplicates(got_hr, len(wins), "hr")
    assert_duplicates(got_lr, len(wins), "lr")
    plan = T.plan_training_batch(corpus, idx, off, ln, PAIR_SEG, HR_RATE, lr_rate)
    rows, = upload_tables([plan.groups[0].rows], DEV)
    assert plan.n_launches == 1 and rows.shape[0] == N_ROWS
    hr2, lr2 = (torch.full((N_ROWS, PAIR_SEG), float("nan"), device=DEV) for _ in range(2))
    T.train_hr_rows(corpus.buffer, rows, PAIR_SEG, fs, HR_RATE, hr2)
    T.train_lr_rows(corpus.buffer, rows, PAIR_SEG, fs, HR_RATE, lr_rate, lr2)
    assert torch.equal(hr2, got_hr) and torch.equal(lr2, got_lr)


HR_SEGS = [2 * 2048 - 1, 2 * 2048, 2 * 2048 + 1]          # the high-rate leg ends a sample short of, on and past its second trip


def hr_case(seg):
    bx, _ = rows_grid(N_ROWS, seg, 256)
    assert bx == 8 and -(-(-(-seg // 256)) // bx) == (2 if seg <= 4096 else 3)
    return bx * 256


@_gpu
@pytest.mark.parametrize("seg", HR_SEGS)
@pytest.mark.parametrize("fs", [48000, 16000])
def test_train_hr_rows_ends_around_a_trip(fs, seg):
    """mg_train_hr_rows alone at segments of 4095, 4096 and 4097 samples (T = 2048): the high-rate row of make_training_pair bit
    for bit, duplicates equal their first occurrence"""
    from mdctgan_amd import train_data as T
    from mdctgan_amd.packed import upload_tables
    from mdctgan_amd.resample import make_training_pair
    assert hr_case(seg) == 2048
    wins = [w for w in train_windows(fs) if w[2] <= FILES[w[0]]]
    table = [wins[b % len(wins)] for b in range(N_ROWS)]
    corpus = noise_corpus(FILES, fs, seg)
    idx, off, ln = ([w[k] for w in table] for k in range(3))
    plan = T.plan_training_batch(corpus, idx, off, ln, seg, HR_RATE, 12000)
    rows, = upload_tables([plan.groups[0].rows], DEV)
    hr = torch.full((N_ROWS, seg), float("nan"), device=DEV)
    T.train_hr_rows(corpus.buffer, rows, seg, fs, HR_RATE, hr)
    for b, (f, o, n) in enumerate(wins):
        _, want_hr = make_training_pair(window_alone(corpus, f, o, n), fs, HR_RATE, HR_RATE, seg)
        assert torch.equal(hr[b], want_hr[0]), (b, f, o, n)
    assert_duplicates(hr, len(wins), seg)


FULL_CONFIGS = [(48000, 12000, (-4, 0, 4)), (48000, 44100, (-1, 0, 1))]
FULL_FILES = [32768, 8192]


def full_case(fs, lr_rate, boundary):
    """lr_full: every row has its own length, the low-rate signal's.  -> (distinct windows, the table's windows).  12000 -> 48000
    makes multiples of 4 only, so the rows next to the trip's end T = 8 * 1024 are T - 4 and T + 4; through 44100 Hz (147 : 160,
    both banks in L2) the lengths T - 1, T and T + 1 exist."""
    from mdctgan_amd.train_data import pair_lengths
    T_ = 8 * up_tile(lr_rate)
    assert T_ == 8192
    targets = [T_ + boundary[2], T_ + boundary[0], 2 * T_ + boundary[2], T_ + boundary[1], 3 * T_ + boundary[0]]
    long_wins = []
    for i, t in enumerate(targets):
        n = next(n for n in range(t * fs // HR_RATE - 8, FULL_FILES[0] + 1) if pair_lengths(n, fs, HR_RATE, lr_rate)[2] >= t)
        assert pair_lengths(n, fs, HR_RATE, lr_rate)[2] == t, (t, n)
        long_wins.append((0, 0 if i % 2 else FULL_FILES[0] - n, n))
    short_wins = [(1, 0, 5), (1, FULL_FILES[1] - 17, 17), (0, 3000, 29), (1, 100, 40)]
    table = [short_wins[b % 4] for b in range(N_ROWS)]
    for b, w in zip(LONG_AT, long_wins):
        table[b] = w
    full_len = np.asarray([pair_lengths(w[2], fs, HR_RATE, lr_rate)[2] for w in table], dtype=np.int64)
    assert assert_later_x_trips(full_len, up_tile(lr_rate), boundary) == T_
    return short_wins + long_wins, table


@_gpu
@pytest.mark.parametrize("fs,lr_rate,boundary", FULL_CONFIGS)
def test_train_rows_lr_full_later_tile_trips(fs, lr_rate, boundary):
    """The lr_full variant over 1030 rows, five of them with low-rate signals of one, two and three trips of 8 tiles: every distinct
    window's signal is resample(resample(window)) bit for bit (what make_training_pair computes before its crop), duplicates equal
    their first occurrence, the gaps of the packed buffer and 64 samples behind it keep their sentinel, and mg_train_lr_rows alone
    writes the same bits."""
    from mdctgan_amd import train_data as T
    from mdctgan_amd.packed import upload_tables
    from mdctgan_amd.resample import resample
    wins, table = full_case(fs, lr_rate, boundary)
    corpus = noise_corpus(FULL_FILES, fs, lr_rate // 100)
    idx, off, ln = ([w[k] for w in table] for k in range(3))
    seg = 64
    plan = T.plan_training_batch(corpus, idx, off, ln, seg, HR_RATE, lr_rate, add_noise=True)
    rows, = upload_tables([plan.table()], DEV)
    arenas = [torch.full((plan.full_total + GUARD,), SENTINEL, device=DEV) for _ in range(2)]
    hr = torch.full((N_ROWS, seg), float("nan"), device=DEV)
    T.train_pair_rows(corpus.buffer, rows, seg, fs, HR_RATE, lr_rate, hr, None, arenas[0][:plan.full_total], max(plan.lr_len))
    T.train_lr_rows(corpus.buffer, rows, seg, fs, HR_RATE, lr_rate, None, arenas[1][:plan.full_total], max(plan.lr_len),
                    out_rows=N_ROWS)
    assert torch.equal(arenas[0], arenas[1]) and bool(torch.isfinite(hr).all())
    want = {w: resample(resample(window_alone(corpus, *w), fs, lr_rate), lr_rate, HR_RATE)[0] for w in wins}
    want_all = torch.full_like(arenas[0], SENTINEL)
    for b, w in enumerate(table):
        assert want[w].numel() == plan.lr_len[b]
        want_all[plan.full_start[b]:plan.full_start[b] + plan.lr_len[b]] = want[w]
    assert torch.equal(arenas[0], want_all)


# ---------------------------------------------------------------------------------------------------------------------
# 2. more than 65535 rows: r += gridDim.y (and sos_carry_kernel's and pcm_encode_rows_kernel's r += gridDim.x)
# ---------------------------------------------------------------------------------------------------------------------
def many_flat(lengths, seed, scale=0.1, offset=0.0):
    """the rows' samples one after the other, rows 0 and 65535 alike"""
    flat = noise_wave(int(lengths.sum()), seed, scale, offset)
    first = firsts(lengths)
    flat[first[65535]:first[65535] + lengths[65535]] = flat[:lengths[0]]
    return flat


def many_case(seed, per_block, shortest=1):
    lengths = many_lengths(seed, shortest)
    assert_later_y_trips(lengths, per_block)
    return lengths


@_gpu
def test_resample_rows_more_rows_than_y_blocks():
    """65540 rows of 1 to 3 samples at 8 kHz to 6, 12 and 18 at 48 kHz, without and with the per-row shift: the rows of one length are
    one [k, L] call of resample() (a y block of its own and one trip for every row) and one call of the oracle"""
    from mdctgan_amd.resample import resample, resample_rows
    orig, new = 8000, 48000
    in_len = many_case(20, 256)
    out_len = 6 * in_len
    assert rows_grid(N_MANY, int(out_len.max()), 256) == (1, 65535)
    flat = many_flat(in_len, 21)
    in_start, in_total = layout(in_len, 8)
    out_start, out_total = layout(out_len, 32)
    x_buf = pack_rows(flat, in_start, in_len, in_total)
    x_all, x = on_device(x_buf)
    x_before = x_all.clone()
    table = torch.from_numpy(np.stack([in_start, in_len, out_start, out_len], axis=1)).to(DEV)
    shift_h = (1e-3 * np.random.default_rng(22).standard_normal(N_MANY)).astype(np.float32)
    shift_h[65535] = shift_h[0]
    for sh in (None, shift_h):
        out_all = torch.full((out_total + 2 * GUARD,), SENTINEL, device=DEV)
        resample_rows(x, table, int(out_len.max()), orig, new, out_all[GUARD:GUARD + out_total],
                      shift=None if sh is None else torch.from_numpy(sh).to(DEV))
        want_all = torch.full_like(out_all, SENTINEL)
        for n, rows in groups_of(in_len):
            xin = rows_2d(x_buf, in_start, rows, n)
            if sh is not None:
                xin = xin + sh[rows][:, None]
            y = resample(torch.from_numpy(xin).to(DEV), orig, new)
            at = torch.from_numpy(GUARD + out_start[rows][:, None] + np.arange(6 * n)[None, :]).to(DEV)
            want_all[at] = y
        assert torch.equal(out_all, want_all), "shift" if sh is not None else "plain"
        assert torch.equal(x_all, x_before)
        got = out_all.cpu().numpy()
        assert np.array_equal(rows_2d(got, out_start, [0], int(out_len[0])), rows_2d(got, out_start, [65535], int(out_len[0])))
        oracle_rows(got, flat, in_len, out_len, out_start, sh, orig, new, "65540 rows")


@_gpu
def test_rows_moments_more_rows_than_y_blocks():
    from mdctgan_amd.resample import rows_moments
    lengths = many_case(23, CHUNK)
    flat = many_flat(lengths, 24, offset=0.01)
    starts, total = layout(lengths, 8)
    buf = pack_rows(flat, starts, lengths, total)
    _, x = on_device(buf)
    table = torch.from_numpy(np.stack([np.zeros_like(starts), starts, starts + lengths], axis=1)).to(DEV)
    got = rows_moments(x, table, 3)
    assert torch.equal(got, rows_moments(x, table, 3))
    host = got.cpu().numpy()
    assert host[DEAD, 0] == 0.0 and host[DEAD, 1] == 0.0 and np.array_equal(host[0], host[65535])
    for n, rows in groups_of(lengths):
        moments_bar_2d(rows_2d(buf, starts, rows, n), host[rows], "65540 rows")


def noise_refs_2d(lr, noise, snr, segment_length):
    """FE.noise_ref64 and FE.noise_ref32 for the rows of a [k, n] pair at once, the same statements along axis 1 -> (f64, f32).
    pin_noise_refs holds them to the imported functions bit for bit."""
    a, z = lr.astype(np.float64), noise.astype(np.float64)
    z = z - z.mean(1, keepdims=True)
    f64 = a + np.sqrt((np.sum(a ** 2, 1, keepdims=True) / segment_length) / 10 ** (snr / 10)) / z.std(1, ddof=1, keepdims=True) * z
    a32, z32 = torch.from_numpy(lr), torch.from_numpy(noise)
    z32 = z32 - z32.mean(1, keepdim=True)
    var = (torch.sum(a32 ** 2, 1, keepdim=True) / segment_length) / 10 ** (snr / 10)
    f32 = (a32 + torch.sqrt(var) / z32.std(1, keepdim=True) * z32).numpy()
    return f64, f32


def noise_margins_2d(got, f32, f64):
    """FE.noise_passes' error / bar for every row of [k, n] arrays"""
    got, f32, f64 = (np.asarray(a, dtype=np.float64) for a in (got, f32, f64))
    bar = 4 * np.abs(f32 - f64).max(1) + 4 * 2.0 ** -23 * np.abs(f64).max(1)
    return np.abs(got - f64).max(1) / bar


def pin_noise_refs(lr, noise, snr, segment_length, rows):
    """the row-wise forms above equal the imported per-waveform functions on `rows`, bit for bit"""
    f64, f32 = noise_refs_2d(lr, noise, snr, segment_length)
    fake = f64 + 1e-9
    for r in rows:
        assert np.array_equal(f64[r], FE.noise_ref64(lr[r], noise[r], snr, segment_length)), r
        assert np.array_equal(f32[r], FE.noise_ref32(lr[r], noise[r], snr, segment_length)), r
        ok, margin = FE.noise_passes(fake[r], f32[r], f64[r])
        assert margin == noise_margins_2d(fake[r:r + 1], f32[r:r + 1], f64[r:r + 1])[0] and ok == (margin <= 1.0)


@_gpu
def test_add_noise_rows_more_rows_than_y_blocks():
    """65540 rows of 2 and 3 samples: every row against the float64 restatement under the noise bar (both taken row-wise over
    rows of one length, and held to test_front_end_gpu's functions on 48 rows of each length), the dead row and every gap untouched"""
    from mdctgan_amd.resample import add_noise_rows, rows_moments
    snr = 10.0
    lengths = many_case(25, 1024, shortest=2)
    a, z = noise_flats(lengths, 26)
    first = firsts(lengths)
    for flat in (a, z):
        flat[first[65535]:first[65535] + lengths[65535]] = flat[:lengths[0]]
    starts, total = layout(lengths, 8)
    a_buf, z_buf = pack_rows(a, starts, lengths, total), pack_rows(z, starts, lengths, total)
    lr_all, lr = on_device(a_buf)
    z_all, zd = on_device(z_buf)
    z_before = z_all.clone()
    table = torch.from_numpy(np.stack([np.zeros_like(starts), starts, starts + lengths], axis=1)).to(DEV)
    add_noise_rows(lr, zd, table, 3, rows_moments(lr, table, 3), rows_moments(zd, table, 3), snr, SEG)
    got = lr_all.cpu().numpy()
    for n, rows in groups_of(lengths):
        lr2, z2 = rows_2d(a_buf, starts, rows, n), rows_2d(z_buf, starts, rows, n)
        pin_noise_refs(lr2, z2, snr, SEG, list(range(24)) + list(range(len(rows) - 24, len(rows))))
        f64, f32 = noise_refs_2d(lr2, z2, snr, SEG)
        margin = noise_margins_2d(rows_2d(got, starts, rows, n), f32, f64)
        print("mg_add_noise_rows %d rows of %d samples: worst error / bar %.3e" % (len(rows), n, margin.max()))
        assert (margin <= 1.0).all(), (n, int(rows[np.argmax(margin)]), margin.max())
    outside = ~inside_mask(starts, lengths, total)
    assert np.array_equal(got[outside], a_buf[outside]) and torch.equal(z_all, z_before)
    assert np.array_equal(rows_2d(got, starts, [0], int(lengths[0])), rows_2d(got, starts, [65535], int(lengths[0])))


@_gpu
def test_metrics_rows_packed_more_rows_than_y_blocks():
    """65540 rows with the per-row shift (shift[r] belongs to the row, not to the block): float64 sums to 1e-12, zeros for the dead row"""
    lengths = many_case(27, CHUNK)
    hr, lr, sr = metric_triples(lengths, 28)
    shift = (1e-3 * np.random.default_rng(29).standard_normal(N_MANY)).astype(np.float32)
    hb, lb, sb, table = metric_packs(hr, lr, sr, lengths)
    got = metrics_packed(hb, lb, sb, table, 3, shift)
    assert np.all(got[DEAD] == 0.0)
    for n, rows in groups_of(lengths):
        h = rows_2d(hb, table[:, 0], rows, n, guard=0) + shift[rows][:, None]
        assert h.dtype == np.float32
        want = metric_sums(h, rows_2d(lb, table[:, 1], rows, n, guard=0), rows_2d(sb, table[:, 2], rows, n, guard=0), axis=1)
        assert np.all(np.abs(got[rows] - want) <= 1e-12 * want), n


def pcm_many_case():
    """16-bit mono payloads packed tightly (a row's bytes start where the row before ends); mg_pcm_row: src_pos, frames, channels,
    channel, format, dst_pos"""
    from mdctgan_amd.wavio import MG_PCM_S16
    lengths = many_case(31, CHUNK)
    starts, total = layout(lengths, 8)
    n = len(lengths)
    rows = np.stack([2 * firsts(lengths), lengths, np.ones(n, np.int64), np.zeros(n, np.int64), np.full(n, MG_PCM_S16, np.int64),
                     starts], axis=1)
    return lengths, starts, total, rows


@_gpu
def test_pcm_decode_rows_more_rows_than_y_blocks():
    """65540 rows of 1 to 3 frames, one payload after the other: the restatement's bits at every row's place, the sentinel in every
    gap, and rows_moments' bits (zeros for the dead row)"""
    from mdctgan_amd.packed import rows_moments
    from mdctgan_amd.wavio import MG_PCM_S16
    from test_wavio_gpu import raw_decode, windows
    lengths, starts, total, rows = pcm_many_case()
    payload = WH.payload_for(MG_PCM_S16, 1, int(lengths.sum()), seed=32)
    want = WH.np_decode(payload, MG_PCM_S16, 1)[0]
    data = torch.from_numpy(np.frombuffer(payload + bytes(16), dtype=np.uint8).copy()).to(DEV)
    out, mom = raw_decode(data, rows, total, prefill=SENTINEL)
    assert WH.bits_equal(out.cpu().numpy(), pack_rows(want, starts, lengths, total, guard=0))
    ref = rows_moments(out, windows(rows), 3)
    assert torch.equal(mom.view(torch.int64), ref.view(torch.int64)) and bool((mom[DEAD] == 0).all())
    host, buf = mom.cpu().numpy(), out.cpu().numpy()
    for n, r in groups_of(lengths):
        moments_bar_2d(rows_2d(buf, starts, r, n, guard=0), host[r], "65540 rows")


@_gpu
def test_pcm_encode_rows_more_rows_than_blocks():
    """mg_pcm_encode_rows launches min(n_rows, 65535) workgroups: 65540 rows of 1 to 3 samples (the wrapper refuses a row without
    frames, so row 65536 is live here) as 16-bit payloads at 8-byte starts: the restatement's bytes, 0xA5 everywhere else, and its
    count of clamped and NaN samples for every row"""
    from mdctgan_amd import wavio
    lengths = many_lengths(33)
    lengths[DEAD] = 2
    assert len(lengths) > 65535 and -(-len(lengths) // 65535) == 2
    x = many_flat(lengths, 34, scale=0.6)
    x[::97], x[5::1013], x[-1] = 1.5, np.nan, -1.5
    starts, total = layout(lengths, 8)
    byte_starts, byte_total = layout(2 * lengths, 8)
    n = len(lengths)
    rows = np.stack([starts, lengths, np.ones(n, np.int64), np.zeros(n, np.int64), np.full(n, wavio.MG_PCM_S16, np.int64),
                     byte_starts], axis=1)
    _, xd = on_device(pack_rows(x, starts, lengths, total))
    big = torch.full((byte_total + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    clipped = wavio.pcm_encode_rows(xd, rows, big[:byte_total]).cpu().numpy()
    want = np.full(byte_total + GUARD, 0xA5, dtype=np.uint8)
    want[positions(byte_starts, 2 * lengths)] = WH.np_encode(x[None], wavio.MG_PCM_S16)[0]
    assert np.array_equal(big.cpu().numpy(), want)
    _, bad = WH.np_quantise(x, 16)
    counts = np.bincount(np.repeat(np.arange(n), lengths), weights=bad, minlength=n).astype(np.int64)
    assert np.array_equal(clipped, counts) and counts[:65535].sum() > 1000 and counts[65535:].sum() > 0


@_gpu
@pytest.mark.parametrize("zero_phase", [False, True], ids=["one_pass", "zero_phase"])
def test_sos_rows_more_rows_than_y_blocks(zero_phase):
    """65540 rows of 1 to 3 samples through a twelfth-order fixture filter, all six sections (sos_pass_kernel's r += gridDim.y,
    sos_carry_kernel's r += gridDim.x): test_lowpass_host's float64 cascade, run over the rows of one length side by side, at the
    bar of tests/test_lowpass_gpu.py; the dead row and every gap keep the sentinel.  (Not the sharpest filter, fixture 16: its
    first-sample gain is 5.6e-18, so a zero-phase row of one sample below 4e-4 comes out under 2^-126, where no float32 output can
    meet a bar relative to the row's peak -- measured 12.8 x the bar on such a row.  Fixture 13's gain is 1.4e-8.)"""
    from mdctgan_amd import lowpass
    c = LP.CASES[13]
    assert c.sos.shape[0] == 6 and np.prod(c.sos[:, 0]) ** 2 > 1e-16
    lengths = many_case(35, 256)
    flat = many_flat(lengths, 36, scale=0.5)
    starts, total = layout(lengths, 8)
    buf = pack_rows(flat, starts, lengths, total)
    _, x = on_device(buf)
    out_all = torch.full((total + 2 * GUARD,), SENTINEL, device=DEV)
    table = np.stack([starts, lengths, starts], axis=1)
    lowpass.sos_rows(x, table, lowpass.pad_sos(c.sos), out=out_all[GUARD:GUARD + total], zero_phase=zero_phase)
    got = out_all.cpu().numpy()
    assert (got[~inside_mask(starts, lengths, total)] == SENTINEL).all()
    for n, rows in groups_of(lengths):
        xs = rows_2d(buf, starts, rows, n).T                                   # [n, k]: the cascade runs along axis 0
        ref = (LP.sos_zero_phase(c.sos, xs.astype(np.float64)) if zero_phase else LP.sos_cascade(c.sos, xs)).T
        y = rows_2d(got, starts, rows, n).astype(np.float64)
        assert np.isfinite(y).all()
        e = np.abs(y - ref).max(1) / np.abs(ref).max(1)
        print("mg_sos_rows %d rows of %d samples zero_phase=%d: worst error / bar %.3f" % (len(rows), n, zero_phase, e.max() / LP.GPU_BAR))
        assert (e <= LP.GPU_BAR).all(), (n, int(rows[np.argmax(e)]), e.max() / LP.GPU_BAR)
    assert np.array_equal(rows_2d(got, starts, [0], int(lengths[0])), rows_2d(got, starts, [65535], int(lengths[0])))


MANY_SEG = 8
MANY_WINDOWS = [(0, 1), (5, 2), (100, 3), (4093, 3), (64, 1), (2000, 2)]         # (offset, length) in one file of 4096 samples


def train_many_case():
    """-> int64 [65540, 5] rows in_pos, in_len, out_row, full_pos, full_len cycling through MANY_WINDOWS; row 65536 is dead, rows 0
    and 65535 are the same window, the last row (window 1, two samples) differs from row 4's (one sample)"""
    which = np.arange(N_MANY) % len(MANY_WINDOWS)
    which[65535] = 0
    w = np.asarray(MANY_WINDOWS, dtype=np.int64)[which]
    rows = np.stack([w[:, 0], w[:, 1], np.arange(N_MANY), np.zeros(N_MANY, np.int64), np.zeros(N_MANY, np.int64)], axis=1)
    rows[DEAD, 1] = 0
    assert rows_grid(N_MANY, MANY_SEG, 256) == (1, 65535) and rows_grid(N_MANY, MANY_SEG, up_tile(12000)) == (1, 65535)
    assert rows[-1, 1] != rows[N_MANY - 1 - 65535, 1] and (rows[0, :2] == rows[65535, :2]).all()
    return which, rows


@_gpu
def test_train_rows_more_rows_than_y_blocks():
    """65540 rows of 8 samples from six windows of 1 to 3 samples: every distinct window has make_training_pair's bits, every row
    equals its window's first occurrence, the dead row's outputs keep their NaN, the single-leg entry points give the same bits"""
    from mdctgan_amd import train_data as T
    from mdctgan_amd.resample import make_training_pair
    which, rows_h = train_many_case()
    corpus = noise_corpus([4096], 48000, 37)
    rows = torch.from_numpy(rows_h).to(DEV)
    outs = [torch.full((N_MANY, MANY_SEG), float("nan"), device=DEV) for _ in range(4)]
    T.train_pair_rows(corpus.buffer, rows, MANY_SEG, 48000, HR_RATE, 12000, outs[0], outs[1])
    T.train_hr_rows(corpus.buffer, rows, MANY_SEG, 48000, HR_RATE, outs[2])
    T.train_lr_rows(corpus.buffer, rows, MANY_SEG, 48000, HR_RATE, 12000, outs[3])
    live = torch.from_numpy(np.arange(N_MANY) != DEAD).to(DEV)
    first = torch.from_numpy(which).to(DEV)
    for got, leg, alone in ((outs[0], 1, outs[2]), (outs[1], 0, outs[3])):
        assert bool(torch.isnan(got[DEAD]).all()) and bool(torch.isfinite(got[live]).all())
        for k, (o, n) in enumerate(MANY_WINDOWS):
            want = make_training_pair(window_alone(corpus, 0, o, n), 48000, HR_RATE, 12000, MANY_SEG)[leg]
            assert torch.equal(got[k], want[0]), (leg, k, o, n)
        assert torch.equal(got[live], got[first][live]), leg
        assert torch.equal(got[live], alone[live]) and bool(torch.isnan(alone[DEAD]).all()), leg


@_gpu
def test_segments_gather_refuses_more_than_65535_rows():
    """mdct.hip launches one y block per row and answers MG_ERR_UNSUPPORTED above 65535: the Python caller reports it as
    NotImplementedError and nothing is launched (the output keeps its fill)"""
    from mdctgan_amd.mdct import segments_gather
    wave = torch.ones(64, device=DEV)
    out = torch.full((65536, 4), SENTINEL, device=DEV)
    table = torch.zeros(65536, 3, dtype=torch.int64, device=DEV)
    table[:, 2] = 4
    with pytest.raises(NotImplementedError, match="MG_ERR_UNSUPPORTED"):
        segments_gather(wave, table, 4, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert bool((segments_gather(wave, table[:65535], 4, out=out[:65535]) == 1.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. the frame-tile kernels past their block cap: tile += gridDim.x
# ---------------------------------------------------------------------------------------------------------------------
HOP = 1                                          # the smallest hop plan_metrics and the resolution parsers accept
# centred frames of a row of n samples at hop 1: n + 1.  Both sizes run in every test below (each case well under a second on the
# MI355X).  Measured there: mg_lsd_rows within 3e-5 relative per frame (bound 2e-4); mg_lsd_rows_backward at most 1.33 e32 (bar 4);
# the STFT loss's gradient within 7.5e-8 and the mel loss's within 7.1e-8 of the largest element (ceiling 1e-4), 0.003 and 0.075 of
# the launch's largest e32 (bar 4).
FRAME_COUNTS = {2048: [1300, 1301, 1500, 1027, 1027, 1100],                   # 7255 frames; rows begin at 1300, 2601, 4101, 5128, 6155
                512: [4101, 4100, 4105, 4099, 4102, 4100, 1000]}              # 25607 frames; 4101, 8201, 12306, 16405, 20507, 24607
FRAME_KERNELS = {"lsd": (4096, 3), "lsd_backward": (4096, 2), "stft": (2048, 3), "mel": (2048, 3)}    # tile (complex points), workgroups per CU
FRAME_SIZES = [2048, 512]
SCALES = (0.5, 2.0, 0.25, 0.75, 1.5, 0.625, 1.25)                 # sr = SCALES[u] * hr for row u


def frame_case(n_fft, kernel, counts=None):
    """-> the row lengths (for the frame counts FRAME_COUNTS[n_fft]).  The launch has more tiles than blocks by at least one tile,
    and -- where a tile holds more than one frame -- a tile of a later trip straddles two rows (at n_fft = 2048 the STFT and mel
    tiles are one frame: no tile straddles)."""
    from mdctgan_amd.metrics import plan_metrics
    counts = FRAME_COUNTS[n_fft] if counts is None else counts
    lengths = [f - 1 for f in counts]
    assert 5 <= len(lengths) <= 7 and min(lengths) > n_fft // 2
    plan = plan_metrics(lengths, n_fft, HOP, True)
    assert plan.frames == list(counts)
    tile, wg = FRAME_KERNELS[kernel]
    ft, n_tiles, blocks = lsd_rows_grid(plan.total_frames, n_fft) if kernel == "lsd" else frames_grid(plan.total_frames, n_fft, tile, wg)
    assert blocks == wg * 1024 and n_tiles >= blocks + 2, (n_tiles, blocks)
    assert plan.total_frames >= {("lsd", 2048): 6145, ("lsd_backward", 2048): 4097, ("stft", 2048): 3073, ("mel", 2048): 3073}.get(
        (kernel, n_fft), 0) + ft
    straddled = [b for b in plan.frame_start[1:-1] if b % ft and b // ft >= blocks]
    assert straddled or ft == 1, (kernel, n_fft)
    return lengths


@functools.lru_cache(maxsize=None)
def frame_pairs(n_fft):
    """float32 (hr, sr) per row for the STFT and mel losses: noise of amplitude 0.1 and sr = SCALES[u] * hr, a different factor for
    every row.  At hop 1 a row has more than a million bins, and the loss suites' noise mixes (sr = a hr + b delay(hr)) then always
    hold some bin whose |ln m_hr - ln m_sr| is under the 1e-6 those suites ask for (measured: 2.5e-7 to 3.6e-7 on every row), where
    a sign taken from float32 bins is a coin toss.  Here ln m_hr - ln m_sr = -ln SCALES[u], at least 0.22 from 0, in every bin
    whose two powers are above the clamp, so every decision is float64's and the suites' bars apply as they stand;
    tests/test_rows_geometry_host.py asserts the suites' margins on these inputs."""
    waves = [noise_wave(f - 1, 7000 + n_fft + u) for u, f in enumerate(FRAME_COUNTS[n_fft])]
    return [(hr, (SCALES[u] * hr).astype(np.float32)) for u, hr in enumerate(waves)]


@_gpu
@pytest.mark.parametrize("n_fft", [2048, 512])
def test_lsd_rows_past_its_block_cap(n_fft):
    """mg_lsd_rows over 7255 (25607) frames, 3072 blocks of 2 (8) frames: every frame against the float64 transform at the bound of
    test_lsd_rows_per_frame_against_rfft, with and without the shift; the rows of the later trips alone have the bits of the pack"""
    from mdctgan_amd.mdct import kbdwin
    from test_metrics_many_gpu import lsd_ref, lsd_rows, pack, signal_pair
    lengths = frame_case(n_fft, "lsd")
    window = kbdwin(n_fft).numpy().astype(np.float32)
    rng = np.random.default_rng(n_fft)
    pairs = [signal_pair("noise", n, rng) for n in lengths]
    shift = (1e-3 * rng.standard_normal(len(lengths))).astype(np.float32)
    hb, hs = pack([p[0] for p in pairs], 3, 1, 1e3, tail=5)
    sb, ss = pack([np.concatenate([p[1], np.full(37, 1e3, np.float32)]) for p in pairs], 64, 64, 1e3, tail=64)
    for sh in (None, shift):
        got_t, plan = lsd_rows(hb, sb, hs, ss, lengths, n_fft, HOP, True, window, sh)
        got = got_t.double().cpu().numpy()
        worst = 0.0
        for u, (h, s) in enumerate(pairs):
            want = lsd_ref(h if sh is None else h + sh[u], s, window, n_fft, HOP, True)
            g = got[plan.frame_start[u]:plan.frame_start[u + 1]]
            assert g.shape == want.shape
            err = np.abs(g - want)
            worst = max(worst, float((err / want).max()))
            assert np.all(err <= 2e-4 * want + 1e-5), (u, lengths[u], int(np.argmax(err - 2e-4 * want)), err.max())
        print("mg_lsd_rows N=%d hop=1 %d frames shift=%s: worst rel %.3g" % (n_fft, plan.total_frames, sh is not None, worst))
        for u in range(len(lengths) - 3, len(lengths)):
            alone, _ = lsd_rows(pairs[u][0], pairs[u][1], [0], [0], [lengths[u]], n_fft, HOP, True, window,
                                None if sh is None else sh[u:u + 1])
            assert torch.equal(got_t[plan.frame_start[u]:plan.frame_start[u + 1]], alone), (u, lengths[u])


def seeded_rows(go, scale, n_rows, divisors):
    """the header's formula for the seeded entry points: ((go * scale) / n_rows) / divisor in double, rounded to float32 once"""
    return np.asarray([((np.float64(np.float32(go)) * scale) / n_rows) / d for d in divisors], dtype=np.float64).astype(np.float32)


@_gpu
@pytest.mark.parametrize("n_fft", [2048, 512])
def test_lsd_rows_backward_past_its_block_cap(n_fft):
    """mg_lsd_rows_backward over 2048 blocks of 2 (8) frames: per row max|got - g64| / max|g64| <= 4 e32, the bar of
    tests/test_lsd_loss_gpu.py; the seeded entry point gives the bits of the plain one with the upstream gradient its header states"""
    from mdctgan_amd import _lib
    from test_lsd_loss_gpu import UNWRITTEN, lsd_backward, written_only_inside
    from test_metrics_many_gpu import pack, signal_pair
    lengths = frame_case(n_fft, "lsd_backward")
    frames = FRAME_COUNTS[n_fft]
    window = LH.window32(n_fft)
    rng = np.random.default_rng(n_fft + 1)
    pairs = [signal_pair("noise", n, rng) for n in lengths]
    hb, hs = pack([p[0] for p in pairs], 3, 1, 1e3, tail=5)
    sb, ss = pack([np.concatenate([p[1], np.full(37, 1e3, np.float32)]) for p in pairs], 5, 64, 1e3, tail=64)
    table = list(zip(hs, ss, lengths))
    got_t = lsd_backward(hb, sb, table, frames, n_fft, HOP, True, window, [1.0 / f for f in frames])
    assert written_only_inside(got_t, ss, lengths)
    got = got_t.double().cpu().numpy()
    worst = 0.0
    for u, (h, s) in enumerate(pairs):
        g = got[ss[u]:ss[u] + lengths[u]]
        assert np.all(np.isfinite(g))
        _, g64 = LH.lsd_autograd(h, s, window, n_fft, HOP, True, torch.float64)
        _, g32 = LH.lsd_autograd(h, s, window, n_fft, HOP, True, torch.float32)
        e32, e = LH.rel_err(g32, g64), LH.rel_err(g, g64)
        worst = max(worst, e / e32)
        print("mg_lsd_rows_backward N=%d hop=1 T=%d: e %.3g, e32 %.3g" % (n_fft, lengths[u], e, e32))
        assert e <= 4 * e32, (u, lengths[u], e, e32)
    print("mg_lsd_rows_backward N=%d hop=1 %d frames: worst e / e32 %.3f" % (n_fft, sum(frames), worst))
    # seeded: go = 1, scale = 0.5 against the plain call with the same upstream gradient
    lib = _lib.load()
    U, total = len(table), sum(frames)
    up = seeded_rows(1.0, 0.5, U, frames)
    plain = lsd_backward(hb, sb, table, frames, n_fft, HOP, True, window, up)
    rows = torch.tensor([[h, 0, s, n] for h, s, n in table], dtype=torch.int64).cuda()
    fsd = torch.from_numpy(np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)).cuda()
    hd, sd, wd = torch.from_numpy(hb).cuda(), torch.from_numpy(sb).cuda(), torch.from_numpy(window).cuda()
    nbytes = lib.mg_lsd_rows_backward_workspace(total, n_fft)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    grad = torch.full((len(sb),), UNWRITTEN, dtype=torch.float32, device=DEV)
    go = torch.tensor([1.0], dtype=torch.float32, device=DEV)
    _lib.check(lib.mg_lsd_rows_backward_seeded(_lib.ptr(hd), hd.numel(), _lib.ptr(sd), sd.numel(), _lib.ptr(rows), U, _lib.ptr(fsd),
                                               total, None, _lib.ptr(wd), n_fft, HOP, 1, _lib.ptr(go), 0.5, _lib.ptr(grad),
                                               _lib.ptr(ws), nbytes, _lib.stream()), "mg_lsd_rows_backward_seeded")
    assert torch.equal(grad, plain)


@functools.lru_cache(maxsize=None)
def stft_refs(n_fft):
    res = ((n_fft, HOP),)
    return [SH.mrstft_autograd(hr, sr, res, torch.float64)[:2] + SH.mrstft_autograd(hr, sr, res, torch.float32)[:2]
            for hr, sr in frame_pairs(n_fft)]


@_gpu
@pytest.mark.parametrize("n_fft", FRAME_SIZES)
def test_stft_loss_rows_past_its_block_cap(n_fft, kind="scaled"):
    """mg_stft_loss_rows and both backwards over 3072 blocks of 1 (4) frames: the value within 2e-4 and the gradient under the bar
    of tests/test_mrstft_loss_gpu.py (4 e32 of the launch and the absolute ceiling) per row; the seeded backward has the bits of the
    plain one with the upstream gradient its header states"""
    from mdctgan_amd import _lib
    from test_lsd_loss_gpu import written_only_inside
    from test_mrstft_loss_gpu import UNWRITTEN, device_tables, judge, packed_case, show, stft_backward, stft_forward
    lengths = frame_case(n_fft, "stft")
    frames = FRAME_COUNTS[n_fft]
    pairs, refs = frame_pairs(n_fft), stft_refs(n_fft)
    hb, hs, sb, ss = packed_case(pairs)
    table = list(zip(hs, ss, lengths))
    row_out = stft_forward(hb, sb, table, frames, n_fft, HOP)
    for u, r in enumerate(refs):
        got = row_out[u, 3].item()
        print("mg_stft_loss_rows N=%d hop=1 %s T=%d: loss %.9g, float64 %.9g" % (n_fft, kind, lengths[u], got, r[0]))
        assert abs(got - r[0]) <= 2e-4 * r[0], (kind, u)
    grad = stft_backward(hb, sb, table, frames, n_fft, HOP, row_out, [1.0] * len(lengths))
    assert written_only_inside(grad, ss, lengths)
    g = grad.double().cpu().numpy()
    tag = "mg_stft_loss_rows N=%d hop=1" % n_fft
    show(tag + " " + kind, judge(tag, kind, [g[s:s + n] for s, n in zip(ss, lengths)], refs, lengths, (0.0, None, 0)), len(lengths))
    # seeded: go = the number of rows, scale = 0.5, one resolution.  This entry point keeps ((go * scale) / n_rows) / n_res in double,
    # unrounded (csrc/stft_loss_rows.hip), so it has the plain call's bits where the quotient is a float32: here 0.5
    lib = _lib.load()
    U = len(table)
    assert seeded_rows(float(U), 0.5, U, [1] * U).tolist() == [0.5] * U
    plain = stft_backward(hb, sb, table, frames, n_fft, HOP, row_out, seeded_rows(float(U), 0.5, U, [1] * U))
    rows, fsd, total = device_tables(table, frames)
    hd, sd, wd = torch.from_numpy(hb).cuda(), torch.from_numpy(sb).cuda(), torch.from_numpy(SH.hann32(n_fft)).cuda()
    nbytes = lib.mg_stft_loss_rows_backward_workspace(total, n_fft)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    seeded = torch.full((len(sb),), UNWRITTEN, dtype=torch.float32, device=DEV)
    go = torch.tensor([float(U)], dtype=torch.float32, device=DEV)
    _lib.check(lib.mg_stft_loss_rows_backward_seeded(_lib.ptr(hd), hd.numel(), _lib.ptr(sd), sd.numel(), _lib.ptr(rows), U,
                                                     _lib.ptr(fsd), total, _lib.ptr(wd), n_fft, HOP, 1, _lib.ptr(row_out),
                                                     _lib.ptr(go), 0.5, 1, 0, _lib.ptr(seeded), _lib.ptr(ws), nbytes,
                                                     _lib.stream()), "mg_stft_loss_rows_backward_seeded")
    assert torch.equal(seeded, plain)


def mel_bank(n_fft):
    return MH.fbank32(MH.RATE, n_fft, MH.MELS[n_fft])


@functools.lru_cache(maxsize=None)
def mel_refs(n_fft):
    banks = [(n_fft, HOP, mel_bank(n_fft))]
    return [MH.mel_autograd(hr, sr, banks, torch.float64)[:2] + MH.mel_autograd(hr, sr, banks, torch.float32)[:2]
            for hr, sr in frame_pairs(n_fft)]


@_gpu
@pytest.mark.parametrize("n_fft", FRAME_SIZES)
def test_mel_loss_rows_past_its_block_cap(n_fft, kind="scaled"):
    """mg_mel_loss_rows and both backwards over 3072 blocks of 1 (4) frames, the default filterbank of the size at 16 kHz: value and
    gradient under the bars of tests/test_mel_loss_gpu.py per row; the seeded backward has the bits of the plain one"""
    from mdctgan_amd import _lib
    from test_lsd_loss_gpu import written_only_inside
    from test_mel_loss_gpu import UNWRITTEN, bank_tensors, judge, mel_backward, mel_forward
    from test_mrstft_loss_gpu import device_tables, packed_case
    lengths = frame_case(n_fft, "mel")
    frames = FRAME_COUNTS[n_fft]
    W = mel_bank(n_fft)
    pairs, refs = frame_pairs(n_fft), mel_refs(n_fft)
    hb, hs, sb, ss = packed_case(pairs)
    table = list(zip(hs, ss, lengths))
    row_out = mel_forward(hb, sb, table, frames, n_fft, HOP, W)
    for u, r in enumerate(refs):
        got = row_out[u, 3].item()
        print("mg_mel_loss_rows N=%d hop=1 %s T=%d: loss %.9g, float64 %.9g" % (n_fft, kind, lengths[u], got, r[0]))
        assert abs(got - r[0]) <= 2e-4 * r[0], (kind, u)
    grad = mel_backward(hb, sb, table, frames, n_fft, HOP, W, [1.0] * len(lengths))
    assert written_only_inside(grad, ss, lengths)
    g = grad.double().cpu().numpy()
    judge("mg_mel_loss_rows N=%d hop=1" % n_fft, kind, [g[s:s + n] for s, n in zip(ss, lengths)], refs, lengths)
    # seeded: go = 2, scale = 0.5, one resolution
    lib = _lib.load()
    U = len(table)
    plain = mel_backward(hb, sb, table, frames, n_fft, HOP, W, seeded_rows(2.0, 0.5, U, [1] * U))
    rows, fsd, total = device_tables(table, frames)
    hd, sd, wd = torch.from_numpy(hb).cuda(), torch.from_numpy(sb).cuda(), torch.from_numpy(SH.hann32(n_fft)).cuda()
    Wd, bk, bj = bank_tensors(W)
    nbytes = lib.mg_mel_loss_rows_backward_workspace(total, n_fft)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    seeded = torch.full((len(sb),), UNWRITTEN, dtype=torch.float32, device=DEV)
    go = torch.tensor([2.0], dtype=torch.float32, device=DEV)
    _lib.check(lib.mg_mel_loss_rows_backward_seeded(_lib.ptr(hd), hd.numel(), _lib.ptr(sd), sd.numel(), _lib.ptr(rows), U,
                                                    _lib.ptr(fsd), total, _lib.ptr(wd), n_fft, HOP, 1, _lib.ptr(Wd), _lib.ptr(bk),
                                                    _lib.ptr(bj), W.shape[0], _lib.ptr(go), 0.5, 1, 0, _lib.ptr(seeded),
                                                    _lib.ptr(ws), nbytes, _lib.stream()), "mg_mel_loss_rows_backward_seeded")
    assert torch.equal(seeded, plain)
