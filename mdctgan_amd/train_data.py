"""Training batches cut from a device-resident corpus in shared launches: AudioDataset.readaudio + __getitem__
(data/audio_dataset.py:34-82) for a whole batch.

The corpus is packed once into one float32 buffer in HBM (``pack_corpus``).  Every step a small device table of crop windows --
one ``mg_train_row`` per batch row -- turns into the ``(LR_audio, HR_audio)`` batch (``training_batch_many``): two launches of
``mg_train_pair_rows`` per distinct file rate, whatever the batch size, the low-rate leg (down to lr_rate and back up) as one fused
kernel.  Every row has the bits ``resample.make_training_pair`` gives for its window alone.  The random crop of ``readaudio`` is
restated on the host (``crop_window``, ``draw_windows``): the same draws from the same CPU stream as the reference.  Under
``--add_noise`` the low-rate leg is written at full length first, because the reference takes the noise power over the waveform
before the crop; ``mg_rows_moments`` (twice), ``mg_add_noise_rows`` and ``mg_segments_gather`` finish the batch.
``make_graphed_training_batch`` captures the launches once over a fixed-size table; a replay only copies a new table in.
``lowpass=`` (or ``--lowpass_aug``; not in the reference) puts a different zero-phase IIR low-pass per row in front of the low-rate leg:
``mg_sos_rows`` filters the B windows into a packed scratch buffer, ``mg_train_lr_rows`` reads that and ``mg_train_hr_rows`` the corpus.
Decoding files stays outside: the caller hands over loaded waveforms.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

import numpy as np
import torch

from . import _lib
from .lowpass import MG_SOS_MAX_SECTIONS, LowpassSpec, check_sos, draw_lowpass, identity_sos, sos_rows, sos_table_bits
from .packed import (PackedLayout, add_noise_packed, aligned_layout, check_table, noise_buffer, pack_waves, upload_tables,
                     window_table)
from .resample import data_options, filter_bank, make_training_pair, resample, resample_length

__all__ = ["TrainingCorpus", "TrainingBatchPlan", "pack_corpus", "crop_window", "draw_windows", "windows_at", "pair_lengths",
           "plan_training_batch", "train_pair_rows", "train_hr_rows", "train_lr_rows", "training_batch_many", "make_graphed_training_batch",
           "make_training_pair", "resample"]         # (the last two: resample.py's per-waveform path, the yardstick of every row)

ROW_COLS = 5            # mg_train_row: in_pos, in_len, out_row, full_pos, full_len


@dataclass
class TrainingCorpus:
    """pack_corpus' result: file f is buffer[starts[f] : starts[f] + lengths[f]] at rates[f] Hz (starts rounded up to `align`
    samples, zeros in the gaps -- which no row ever reads: a row's window is its whole signal)."""
    buffer: torch.Tensor
    starts: List[int]
    lengths: List[int]
    rates: List[int]

    def __len__(self):
        return len(self.lengths)

    @property
    def distinct_rates(self) -> List[int]:
        return sorted(set(self.rates))


def pack_corpus(waveforms, rates, device, align: int = 64) -> TrainingCorpus:
    """Loaded waveforms ([T] or [1, T], on the host or the device) at `rates` Hz -> one packed float32 buffer on `device`."""
    waveforms = list(waveforms)
    rates = [int(r) for r in rates]
    if not waveforms or len(waveforms) != len(rates):
        raise ValueError("pack_corpus needs one sampling rate per waveform, and at least one waveform")
    lengths = [int(w.numel()) for w in waveforms]
    if min(lengths) <= 0 or min(rates) <= 0:
        raise ValueError("lengths and sampling rates must be positive")
    layout = aligned_layout(lengths, align)
    return TrainingCorpus(pack_waves(waveforms, layout, device), layout.starts, lengths, rates)


def pack_corpus_files(paths, device) -> TrainingCorpus:
    """pack_corpus straight from WAV files (wavio.read_wav_many: one copy of the payload bytes, one decode launch): channel 0 of
    every file -- what seg_pad_audio keeps (:104) -- whole, at the sampling rate its header names.  The crop stays draw_windows'."""
    from .wavio import read_wav_many
    pack = read_wav_many(paths, device, channels="first")
    return TrainingCorpus(pack.buffer, pack.starts, pack.lengths, pack.rates)


def crop_window(audio_length: int, fs: int, segment_length: int, hr_rate: int) -> int:
    """data/audio_dataset.py:43: the exclusive upper bound of readaudio's random start frame (<= 0: the whole file is loaded)."""
    return int(audio_length - segment_length * fs / hr_rate)


def _indices(corpus: TrainingCorpus, indices) -> List[int]:
    idx = [int(i) for i in (indices.tolist() if torch.is_tensor(indices) else indices)]
    if not idx:
        raise ValueError("a training batch needs at least one file index")
    bad = [i for i in idx if not 0 <= i < len(corpus)]
    if bad:
        raise IndexError("file index %d is outside the corpus of %d files" % (bad[0], len(corpus)))
    return idx


def draw_windows(corpus: TrainingCorpus, indices, segment_length: int, hr_rate: int, generator=None):
    """AudioDataset.readaudio (:34-52) for the files `indices`, in that order: one torch.randint(0, hi, (1,)) on the CPU per file
    with hi = crop_window(...) > 0 -- from the global CPU stream, as the reference draws, or from `generator` -- and a window of
    segment_length frames AT THE FILE'S RATE from there, cut to the file (torchaudio.load returns what is left); hi <= 0 loads the
    whole file.  -> (offsets, lengths), int64 [B] on the host."""
    offsets, lengths = [], []
    for i in _indices(corpus, indices):
        n = corpus.lengths[i]
        hi = crop_window(n, corpus.rates[i], segment_length, hr_rate)
        if hi > 0:
            off = int(torch.randint(0, hi, (1,), generator=generator).item())
            offsets.append(off)
            lengths.append(min(int(segment_length), n - off))
        else:
            offsets.append(0)
            lengths.append(n)
    return torch.tensor(offsets, dtype=torch.int64), torch.tensor(lengths, dtype=torch.int64)


def windows_at(corpus: TrainingCorpus, indices, offsets, segment_length: int, hr_rate: int):
    """draw_windows with the caller's start frames in place of the draws (a file that readaudio loads whole ignores its offset)."""
    idx = _indices(corpus, indices)
    offs = [int(o) for o in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]
    if len(offs) != len(idx):
        raise ValueError("one offset per file index (%d indices, %d offsets)" % (len(idx), len(offs)))
    out_off, out_len = [], []
    for i, off in zip(idx, offs):
        n = corpus.lengths[i]
        if crop_window(n, corpus.rates[i], segment_length, hr_rate) > 0:
            if not 0 <= off < n:
                raise ValueError("offset %d is outside file %d of %d samples" % (off, i, n))
            out_off.append(off)
            out_len.append(min(int(segment_length), n - off))
        else:
            out_off.append(0)
            out_len.append(n)
    return torch.tensor(out_off, dtype=torch.int64), torch.tensor(out_len, dtype=torch.int64)


def pair_lengths(length: int, fs: int, hr_rate: int, lr_rate: int):
    """(hr_len, mid_len, lr_len) of a window of `length` samples at fs Hz: ceil(hr L / fs), mid_len = ceil(lr L / fs) and
    ceil(hr mid_len / lr) -- the lengths aF.resample returns in :66-71.  The first and the last differ in general."""
    mid = resample_length(length, fs, lr_rate)
    return resample_length(length, fs, hr_rate), mid, resample_length(mid, lr_rate, hr_rate)


@dataclass
class TrainGroup:
    """The rows of one mg_train_pair_rows call: batch rows `index` (in table order) come from files of file_rate Hz."""
    file_rate: int
    index: List[int]
    rows: np.ndarray                # int64 [n, 5] = in_pos, in_len, out_row, full_pos, full_len (in_len == 0: a dead row)
    max_full_len: int


@dataclass
class TrainingBatchPlan:
    """plan_training_batch's result.  `groups`: one TrainGroup per distinct file rate.  `hr_len` / `mid_len` / `lr_len`: per batch
    row, pair_lengths of its window.  `full_start` / `full_total`: under add_noise, where every row's full-length low-rate signal
    sits in the packed lr_full buffer.  `rows`: the number of table rows (batch rows plus dead padding rows)."""
    batch: int
    segment_length: int
    groups: List[TrainGroup]
    hr_len: List[int]
    mid_len: List[int]
    lr_len: List[int]
    full_start: List[int] = field(default_factory=list)
    full_total: int = 0
    rows: int = 0

    @property
    def n_launches(self) -> int:
        """mg_train_pair_rows calls: one per distinct file rate, whatever the batch size."""
        return len(self.groups)

    def table(self) -> np.ndarray:
        """Every group's rows in launch order: the one array that travels to the device."""
        return np.concatenate([g.rows for g in self.groups], axis=0)


def plan_training_batch(corpus: TrainingCorpus, indices, offsets, lengths, segment_length: int, hr_rate: int, lr_rate: int,
                        add_noise: bool = False, pad_to=None, align: int = 64) -> TrainingBatchPlan:
    """The row tables of one batch (host only: no device call).  Batch row b loads `lengths[b]` samples from sample `offsets[b]`
    of file indices[b] and writes row b of (lr, hr).  Rows are grouped by file rate, one mg_train_pair_rows call per distinct
    rate.  pad_to: the first group's table is filled up with dead rows (in_len == 0, which write nothing) to pad_to rows in all --
    the fixed-size table of a captured graph."""
    idx = _indices(corpus, indices)
    offs = [int(o) for o in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]
    lens = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    if len(offs) != len(idx) or len(lens) != len(idx):
        raise ValueError("one offset and one length per file index (%d, %d, %d)" % (len(idx), len(offs), len(lens)))
    if int(segment_length) <= 0 or int(hr_rate) <= 0 or int(lr_rate) <= 0:
        raise ValueError("segment_length and sampling rates must be positive")
    for i, off, n in zip(idx, offs, lens):
        if n <= 0 or off < 0 or off + n > corpus.lengths[i]:
            raise ValueError("window [%d, %d) is outside file %d of %d samples" % (off, off + n, i, corpus.lengths[i]))
    B = len(idx)
    if pad_to is not None and (int(pad_to) < B or add_noise):
        raise ValueError("pad_to is at least the batch (%d) and not for add_noise" % B)
    trio = [pair_lengths(n, corpus.rates[i], hr_rate, lr_rate) for i, n in zip(idx, lens)]
    hr_len, mid_len, lr_len = ([t[k] for t in trio] for k in range(3))
    full = aligned_layout(lr_len, align) if add_noise else PackedLayout([0] * B, lr_len, 0)
    full_start, full_total = full.starts, full.total
    members = {}
    for b, i in enumerate(idx):
        members.setdefault(corpus.rates[i], []).append(b)
    groups = []
    for rate, rows_of in members.items():
        rows = np.asarray([(corpus.starts[idx[b]] + offs[b], lens[b], b, full_start[b], lr_len[b] if add_noise else 0)
                           for b in rows_of], dtype=np.int64).reshape(-1, ROW_COLS)
        groups.append(TrainGroup(rate, rows_of, rows, max(lr_len[b] for b in rows_of)))
    n_rows = B
    if pad_to is not None and int(pad_to) > B:
        groups[0].rows = np.concatenate([groups[0].rows, np.zeros((int(pad_to) - B, ROW_COLS), dtype=np.int64)], axis=0)
        n_rows = int(pad_to)
    return TrainingBatchPlan(B, int(segment_length), groups, hr_len, mid_len, lr_len, full_start if add_noise else [], full_total,
                             n_rows)


def _bank(orig_freq: int, new_freq: int, device):
    """mg_resample_bank of one step, from resample.filter_bank; its identity bank (equal rates) travels as the copy bank."""
    kern, width, orig, new = filter_bank(orig_freq, new_freq, device)
    return _lib.ResampleBank(kern.data_ptr() if (orig, new) != (1, 1) else None, orig, new, width)


def _check_pair_args(what, corpus_buffer, table, L, dense, lr_full):
    """The tensor checks the three leg wrappers share; dense: (tensor, name) of the [rows, L] outputs the call writes."""
    n = check_table(table, ROW_COLS, what).shape[0]
    if corpus_buffer.dtype != torch.float32 or not corpus_buffer.is_contiguous():
        raise ValueError("%s: the corpus is a contiguous float32 buffer" % what)
    for t, name in dense:
        if t is None or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != L or not t.is_contiguous():
            raise ValueError("%s: %s is a contiguous float32 [rows, %d] tensor" % (what, name, L))
    if len({t.shape[0] for t, _ in dense}) > 1:
        raise ValueError("%s: lr and hr have the same number of rows" % what)
    if lr_full is not None and (lr_full.dtype != torch.float32 or not lr_full.is_contiguous()):
        raise ValueError("%s: lr_full is a contiguous float32 buffer" % what)
    return n


def train_pair_rows(corpus_buffer: torch.Tensor, table: torch.Tensor, segment_length: int, file_rate: int, hr_rate: int,
                    lr_rate: int, hr: torch.Tensor, lr=None, lr_full=None, max_full_len: int = 0):
    """mg_train_pair_rows: every row of `table` (int64 [n, 5] on the device: in_pos, in_len, out_row, full_pos, full_len) reads its
    window of the packed corpus and writes row out_row of hr and lr ([rows, segment_length] float32) -- or, with lr_full (a packed
    float32 buffer), its whole low-rate signal to lr_full[full_pos : full_pos + full_len] in place of lr."""
    lib = _lib.load()
    L = int(segment_length)
    n = _check_pair_args("train_pair_rows", corpus_buffer, table, L,
                          [(hr, "hr")] + ([(lr, "lr")] if lr is not None or lr_full is None else []), lr_full)
    dev = corpus_buffer.device
    to_hr, to_lr, up = _bank(file_rate, hr_rate, dev), _bank(file_rate, lr_rate, dev), _bank(lr_rate, hr_rate, dev)
    _lib.check(lib.mg_train_pair_rows(_lib.ptr(corpus_buffer), corpus_buffer.numel(), _lib.ptr(table), n, L, to_hr, to_lr, up,
                                      _lib.ptr(lr), _lib.ptr(hr), hr.shape[0], _lib.ptr(lr_full),
                                      0 if lr_full is None else lr_full.numel(), int(max_full_len), _lib.stream()),
               "mg_train_pair_rows")
    return lr, hr


def train_hr_rows(corpus_buffer: torch.Tensor, table: torch.Tensor, segment_length: int, file_rate: int, hr_rate: int,
                  hr: torch.Tensor):
    """mg_train_hr_rows: the high-rate leg of train_pair_rows alone (the same kernel, the same bits)."""
    lib = _lib.load()
    L = int(segment_length)
    n = _check_pair_args("train_hr_rows", corpus_buffer, table, L, [(hr, "hr")], None)
    _lib.check(lib.mg_train_hr_rows(_lib.ptr(corpus_buffer), corpus_buffer.numel(), _lib.ptr(table), n, L,
                                    _bank(file_rate, hr_rate, corpus_buffer.device), _lib.ptr(hr), hr.shape[0], _lib.stream()),
               "mg_train_hr_rows")
    return hr


def train_lr_rows(buffer: torch.Tensor, table: torch.Tensor, segment_length: int, file_rate: int, hr_rate: int, lr_rate: int,
                  lr=None, lr_full=None, max_full_len: int = 0, out_rows=None):
    """mg_train_lr_rows: the low-rate leg of train_pair_rows alone (the same kernel, the same bits, lr_full included), over any
    packed buffer -- the low-passed windows of training_batch_many(lowpass=), say.  out_rows: the rows of the batch when lr is
    None (with lr_full; default: the table's)."""
    lib = _lib.load()
    L = int(segment_length)
    n = _check_pair_args("train_lr_rows", buffer, table, L, [(lr, "lr")] if lr is not None or lr_full is None else [], lr_full)
    dev = buffer.device
    _lib.check(lib.mg_train_lr_rows(_lib.ptr(buffer), buffer.numel(), _lib.ptr(table), n, L, _bank(file_rate, lr_rate, dev),
                                    _bank(lr_rate, hr_rate, dev), _lib.ptr(lr), lr.shape[0] if lr is not None else int(out_rows or n),
                                    _lib.ptr(lr_full), 0 if lr_full is None else lr_full.numel(), int(max_full_len),
                                    _lib.stream()), "mg_train_lr_rows")
    return lr if lr is not None else lr_full


def _windows(corpus, idx, o, offsets, lengths, generator):
    L, hr_rate = int(o["segment_length"]), int(o["hr_sampling_rate"])
    if lengths is not None:
        if offsets is None:
            raise ValueError("explicit lengths need explicit offsets")
        return offsets, lengths
    if offsets is None:
        return draw_windows(corpus, idx, L, hr_rate, generator)
    return windows_at(corpus, idx, offsets, L, hr_rate)


def _out_pair(out, B, L, device):
    if out is None:
        return (torch.empty(B, L, dtype=torch.float32, device=device), torch.empty(B, L, dtype=torch.float32, device=device))
    lr, hr = out
    for t in (lr, hr):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == (B, L) and t.is_contiguous()
                and t.device == device):
            raise ValueError("out=(lr, hr): two contiguous float32 [%d, %d] tensors on %s" % (B, L, device))
    return lr, hr


def _lowpass_table(lowpass, corpus, idx, lr_rate, generator):
    """The coefficient table float64 [B, 6, 6] of a batch: drawn from a LowpassSpec (after the window draws, from the same stream), or
    the caller's, refused on the host when a section is unstable or not finite."""
    if isinstance(lowpass, LowpassSpec):
        return draw_lowpass([corpus.rates[i] for i in idx], lr_rate, lowpass, generator)
    coef = check_sos(lowpass)
    if coef.shape[0] != len(idx):
        raise ValueError("lowpass: one [%d, 6] set of sections per batch row (%d rows, %d sets)"
                         % (MG_SOS_MAX_SECTIONS, len(idx), coef.shape[0]))
    return coef


def _lowpass_rows(plan: TrainingBatchPlan, starts):
    """Where the low-passed windows sit: batch row b is filtered from its corpus window into scratch[starts[b] : starts[b] + len].
    -> (the mg_sos_row table int64 [plan.rows, 3] in batch-row order, rows past the batch dead; every group's mg_train_row table
    with in_pos moved to the scratch buffer -- what the low-rate leg reads)."""
    starts = np.asarray(starts, dtype=np.int64)
    sos_tab = np.zeros((plan.rows, 3), dtype=np.int64)
    moved = []
    for g in plan.groups:
        rows = g.rows.copy()
        live = rows[:, 1] > 0
        b = rows[live, 2]
        sos_tab[b] = np.stack([rows[live, 0], rows[live, 1], starts[b]], axis=1)
        rows[live, 0] = starts[b]
        moved.append(rows)
    return sos_tab, moved


def training_batch_many(corpus: TrainingCorpus, indices, opt_or_kwargs, offsets=None, generator=None, noise=None, out=None,
                        lengths=None, noise_generator=None, lowpass=None):
    """AudioDataset.readaudio + __getitem__ (data/audio_dataset.py:34-82) for the files `indices` of a packed corpus ->
    (lr, hr), each float32 [B, segment_length] on the corpus' device; row b is resample.make_training_pair on its window alone,
    bit for bit.  opt_or_kwargs: an options namespace or a dict with lr_sampling_rate, hr_sampling_rate, segment_length and
    optionally add_noise / snr.
    offsets: the start frame per file instead of draw_windows' draws (from the global CPU stream, or the CPU `generator`);
    lengths: with offsets, explicit window lengths in place of readaudio's rule.  out=(lr, hr): the caller's tensors are written
    (the static inputs of make_graphed_step, say) and returned.
    add_noise: `noise` is a list of one waveform per batch row of the row's full low-rate length (plan.lr_len; for tests: the
    reference draws from the CPU stream, which a device cannot reproduce), otherwise torch.randn(..., generator=noise_generator)
    on the device.
    lowpass (default: the options' --lowpass_aug; not in the reference): a lowpass.LowpassSpec -- one filter per row is drawn
    from the same CPU stream, after the windows -- or an explicit coefficient table float64 [B, 6, 6] (lowpass.pad_sos of
    lowpass.lowpass_sos at the row's file rate).  Row b of lr is then make_training_pair(window_b, lowpass_sos=table[b]), bit for
    bit; hr keeps its bits.  The noise of add_noise comes after the filter.
    Launches: one table copy and mg_train_pair_rows per distinct file rate; under add_noise also two mg_rows_moments,
    mg_add_noise_rows and mg_segments_gather -- whatever the batch size.  With lowpass: the coefficients travel in the same copy,
    mg_sos_rows (6 launches) filters all windows into a scratch buffer of aligned_layout, and every rate's mg_train_pair_rows
    becomes mg_train_hr_rows over the corpus and mg_train_lr_rows over the scratch buffer.  Nothing is read back."""
    from .mdct import segments_gather
    o = data_options(opt_or_kwargs)
    L, hr_rate, lr_rate = int(o["segment_length"]), int(o["hr_sampling_rate"]), int(o["lr_sampling_rate"])
    idx = _indices(corpus, indices)
    offsets, lengths = _windows(corpus, idx, o, offsets, lengths, generator)
    plan = plan_training_batch(corpus, idx, offsets, lengths, L, hr_rate, lr_rate, o["add_noise"])
    B, dev = plan.batch, corpus.buffer.device
    if o["add_noise"]:
        if min(plan.lr_len) < 2:
            raise ValueError("add_noise: a waveform of fewer than 2 samples has no standard deviation")
        if noise is not None and [int(z.numel()) for z in noise] != plan.lr_len:
            raise ValueError("add_noise: noise holds one waveform per batch row, of the lengths %s" % plan.lr_len)
    elif noise is not None:
        raise ValueError("noise= is for add_noise")
    lowpass = o["lowpass"] if lowpass is None else lowpass
    coef = None if lowpass is None else _lowpass_table(lowpass, corpus, idx, lr_rate, generator)
    lr, hr = _out_pair(out, B, L, dev)

    # every table in one copy: each group's rows, then under add_noise the windows of lr_full in batch order
    full = PackedLayout(plan.full_start, plan.lr_len, plan.full_total)
    win_part = [window_table(full.starts, full.lengths) if o["add_noise"] else []]
    lr_full = torch.empty(full.total, dtype=torch.float32, device=dev) if o["add_noise"] else None
    if coef is None:
        *group_rows, win = upload_tables([g.rows for g in plan.groups] + win_part, dev)
        for g, rows in zip(plan.groups, group_rows):
            train_pair_rows(corpus.buffer, rows, L, g.file_rate, hr_rate, lr_rate, hr, None if o["add_noise"] else lr, lr_full,
                            g.max_full_len)
    else:
        # ... and with lowpass the scratch windows, the groups' rows over the scratch buffer and the coefficients
        scratch = aligned_layout([int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)])
        sos_tab, moved = _lowpass_rows(plan, scratch.starts)
        n_g = len(plan.groups)
        *tables, sos_dev, coef_dev, win = upload_tables([g.rows for g in plan.groups] + moved + [sos_tab, sos_table_bits(coef)]
                                                        + win_part, dev)
        filtered = torch.empty(scratch.total, dtype=torch.float32, device=dev)
        sos_rows(corpus.buffer, sos_dev, coef_dev.view(torch.float64), out=filtered, max_len=max(scratch.lengths))
        for g, rows, rows_lp in zip(plan.groups, tables[:n_g], tables[n_g:]):
            train_hr_rows(corpus.buffer, rows, L, g.file_rate, hr_rate, hr)
            train_lr_rows(filtered, rows_lp, L, g.file_rate, hr_rate, lr_rate, None if o["add_noise"] else lr, lr_full,
                          g.max_full_len, out_rows=B)
    if o["add_noise"]:
        add_noise_packed(lr_full, win, max(plan.lr_len), o["snr"], L, noise_buffer(noise, full, dev, noise_generator))
        segments_gather(lr_full, win, L, out=lr)
    return lr, hr


def make_graphed_training_batch(corpus: TrainingCorpus, batch: int, opt_or_kwargs, lowpass=None):
    """Capture the launches of training_batch_many once, over a table of `batch` rows, and return run(indices, offsets=None,
    generator=None, lengths=None) -> (lr, hr): it plans the windows on the host, copies the new table in and replays.  The
    returned tensors are the captured outputs, [batch, segment_length], rewritten by every replay; fewer than `batch` indices
    leave the remaining rows dead (they keep what they held).  The graph is a plain chain of two kernels.
    lowpass (a lowpass.LowpassSpec; default: the options' --lowpass_aug): the six launches of mg_sos_rows join the chain in front of
    mg_train_hr_rows and mg_train_lr_rows -- still a plain chain -- over a scratch buffer of `batch` aligned rows of segment_length
    samples (a window of more frames is refused); run(...) draws the filters after the windows, or takes run(..., lowpass=table),
    and copies windows and coefficients in one copy.  run.last_lowpass: the table of the last replay; run.filtered: the scratch
    buffer, row b's low-passed window at aligned_layout([segment_length] * batch).starts[b]; run.workspace: mg_sos_rows' workspace.
    Defined for a corpus with ONE file rate (the launches of a capture are fixed; the row grouping of mixed rates is not);
    add_noise draws from a random stream inside the capture, which is out of scope."""
    o = data_options(opt_or_kwargs)
    if len(corpus.distinct_rates) != 1:
        raise ValueError("make_graphed_training_batch needs a corpus with one file rate, this one has %s" % corpus.distinct_rates)
    if o["add_noise"]:
        raise NotImplementedError("--add_noise inside a captured training batch (the random stream of a capture) is not built")
    batch = int(batch)
    if batch <= 0:
        raise ValueError("batch must be positive")
    spec = o["lowpass"] if lowpass is None else lowpass
    if spec is not None and not isinstance(spec, LowpassSpec):
        raise ValueError("make_graphed_training_batch: lowpass is a LowpassSpec (an explicit table goes to run(..., lowpass=))")
    L, hr_rate, lr_rate = int(o["segment_length"]), int(o["hr_sampling_rate"]), int(o["lr_sampling_rate"])
    dev, rate = corpus.buffer.device, corpus.rates[0]
    lr = torch.zeros(batch, L, dtype=torch.float32, device=dev)
    hr = torch.zeros(batch, L, dtype=torch.float32, device=dev)
    if spec is None:
        table = torch.zeros(batch, ROW_COLS, dtype=torch.int64, device=dev)          # all rows dead

        def launch():
            train_pair_rows(corpus.buffer, table, L, rate, hr_rate, lr_rate, hr, lr)
    else:
        # one storage for every table of a replay: the rows over the corpus, the rows over the scratch buffer, the filter's rows
        # and the coefficients (identity sections until the first replay)
        shapes = [(batch, ROW_COLS), (batch, ROW_COLS), (batch, 3), (batch, MG_SOS_MAX_SECTIONS, 6)]
        sizes = [int(np.prod(sh)) for sh in shapes]
        storage = torch.zeros(sum(sizes), dtype=torch.int64, device=dev)
        table, table_lp, sos_tab, coef_bits = (storage[e - n:e].view(sh) for sh, n, e in zip(shapes, sizes, np.cumsum(sizes)))
        coef = coef_bits.view(torch.float64)
        coef.copy_(torch.from_numpy(np.broadcast_to(identity_sos(), shapes[3]).copy()))
        scratch = aligned_layout([L] * batch)
        filtered = torch.zeros(scratch.total, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.load().mg_sos_rows_workspace(batch, L), dtype=torch.uint8, device=dev)

        def launch():
            sos_rows(corpus.buffer, sos_tab, coef, out=filtered, max_len=L, workspace=ws)
            train_hr_rows(corpus.buffer, table, L, rate, hr_rate, hr)
            train_lr_rows(filtered, table_lp, L, rate, hr_rate, lr_rate, lr)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launch()                                                                    # (builds the filter banks outside the capture)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()

    def run(indices, offsets=None, generator=None, lengths=None, lowpass=None):
        idx = _indices(corpus, indices)
        if len(idx) > batch:
            raise ValueError("the capture holds %d rows, got %d indices" % (batch, len(idx)))
        offs, lens = _windows(corpus, idx, o, offsets, lengths, generator)
        plan = plan_training_batch(corpus, idx, offs, lens, L, hr_rate, lr_rate, pad_to=batch)
        if spec is None:
            if lowpass is not None:
                raise ValueError("this capture was made without lowpass")
            table.copy_(torch.from_numpy(plan.table()))
        else:
            if max(int(n) for n in (lens.tolist() if torch.is_tensor(lens) else lens)) > L:
                raise ValueError("a window of more than segment_length (%d) frames does not fit the captured scratch buffer" % L)
            picked = _lowpass_table(spec if lowpass is None else lowpass, corpus, idx, lr_rate, generator)
            rows_f, (rows_lp,) = _lowpass_rows(plan, scratch.starts)
            full = np.broadcast_to(identity_sos(), shapes[3]).copy()
            full[:len(idx)] = picked
            storage.copy_(torch.from_numpy(np.concatenate([plan.table().reshape(-1), rows_lp.reshape(-1), rows_f.reshape(-1),
                                                           sos_table_bits(full).reshape(-1)])))
            run.last_lowpass = picked
        graph.replay()
        return lr, hr
    run.graph, run.table, run.batch, run.last_lowpass = graph, table, batch, None
    # the capture holds raw pointers: every buffer its kernels touch lives as long as `run`
    run.filtered, run.workspace = (filtered, ws) if spec is not None else (None, None)
    return run
