"""Packed rows: what ``generate_many``, ``front_end_many``, ``compute_matrics_many`` and ``training_batch_many`` share on the host.

Many waveforms sit at aligned starts of one float32 buffer (``PackedLayout``, ``aligned_layout``, ``pack_waves``), and small int64
row tables tell the kernels where every row reads and writes (``window_table``, ``check_table``); all the tables of one call
travel in one host array and one copy (``upload_tables``).  The row kernels over such a buffer that more than one module uses --
``mg_rows_moments``, ``mg_add_noise_rows`` and the ``--add_noise`` tail made of them -- are bound here as well.  A leaf module:
nothing else of the package is imported.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from . import _lib


@dataclass
class PackedLayout:
    """Waveform u is buffer[starts[u] : starts[u] + lengths[u]] of a packed buffer of `total` samples."""
    starts: List[int]
    lengths: List[int]
    total: int


def aligned_layout(lengths, align: int = 64) -> PackedLayout:
    """THE alignment rule: every waveform starts at the end of the one before, rounded up to `align` samples (so that a row keeps
    the alignment it has alone: the 16-byte paths of the kernels); `total` is the rounded end of the last one."""
    lengths, align = [int(n) for n in lengths], int(align)
    starts, pos = [], 0
    for n in lengths:
        starts.append(pos)
        pos = -(-(pos + n) // align) * align
    return PackedLayout(starts, lengths, pos)


def pack_waves(waves, layout: PackedLayout, device, out=None) -> torch.Tensor:
    """The packed buffer: every waveform at its start, zeros in the gaps, written once -- one concatenation straight into `out`
    (a device buffer of at least layout.total samples; default: a new one).  A list of host waveforms is concatenated on the
    host and travels in one copy; a list that mixes devices is moved to `device` waveform by waveform."""
    device = torch.device(device)
    buf = torch.empty(layout.total, dtype=torch.float32, device=device) if out is None else out[:layout.total]
    flat = [w.reshape(-1) for w in waves]
    on_host = all(w.device.type == "cpu" for w in flat)
    where = torch.device("cpu") if on_host else device
    gap = torch.zeros(max(int(s1 - s0 - n) for s0, s1, n in
                          zip(layout.starts, layout.starts[1:] + [layout.total], layout.lengths)) or 1,
                      dtype=torch.float32, device=where)
    parts = []
    for w, s0, s1 in zip(flat, layout.starts, layout.starts[1:] + [layout.total]):
        parts.append(w.to(device=where, dtype=torch.float32))
        if s1 - s0 > w.numel():
            parts.append(gap[:s1 - s0 - w.numel()])
    if on_host and device.type != "cpu":
        buf.copy_(torch.cat(parts), non_blocking=True)
    else:
        torch.cat(parts, out=buf)
    return buf


def window_table(starts, lengths, order=None) -> np.ndarray:
    """int64 [n, 3] rows of pos, lo, hi (mg_seg_row) on the host: the window [starts[u], starts[u] + lengths[u]) of every u, read
    from its first sample, in the order `order` (default: as given)."""
    first, n = np.asarray(starts, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    if order is not None:
        order = np.asarray(order, dtype=np.int64)
        first, n = first[order], n[order]
    return np.stack([first, first, first + n], axis=1)


def upload_tables(parts, device) -> List[torch.Tensor]:
    """Every table of a call in one host array and ONE non_blocking copy: int64 host arrays of any shape -> one device view per
    part, in the part's own shape, all of one storage."""
    parts = [np.asarray(p, dtype=np.int64) for p in parts]
    flat = torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts])).to(device, non_blocking=True)
    ends = np.cumsum([p.size for p in parts])
    return [flat[e - p.size:e].view(p.shape) for p, e in zip(parts, ends)]


def check_table(table, cols: int, what: str):
    if not (torch.is_tensor(table) and table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == cols
            and table.shape[0] > 0 and table.is_contiguous()):
        raise ValueError("%s: the row table is a contiguous int64 [n, %d] tensor with at least one row" % (what, cols))
    return table


def rows_moments(x: torch.Tensor, table: torch.Tensor, max_len: int) -> torch.Tensor:
    """mg_rows_moments: float64 [n, 2] = {sum x, sum x^2} over the window [lo, hi) of every row of `table` (int64 [n, 3] = pos, lo,
    hi on the device) of the packed float32 buffer `x`."""
    lib = _lib.load()
    n = check_table(table, 3, "rows_moments").shape[0]
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("rows_moments: x is a contiguous float32 buffer")
    nbytes = lib.mg_rows_moments_workspace(n, int(max_len))
    ws = _lib.workspace(nbytes, x.device)
    out = torch.empty(n, 2, dtype=torch.float64, device=x.device)
    _lib.check(lib.mg_rows_moments(_lib.ptr(x), x.numel(), _lib.ptr(table), n, int(max_len), _lib.ptr(out), _lib.ptr(ws), nbytes,
                                   _lib.stream()), "mg_rows_moments")
    return out


def add_noise_rows(lr: torch.Tensor, noise: torch.Tensor, table: torch.Tensor, max_len: int, lr_moments: torch.Tensor,
                   noise_moments: torch.Tensor, snr: float, segment_length: int) -> torch.Tensor:
    """mg_add_noise_rows, in place on the packed buffer `lr`: every row's window [lo, hi) becomes lr + a (noise - mean(noise)),
    a = sqrt((sum lr^2 / segment_length) / 10^(snr / 10)) / std(noise), from rows_moments(lr, ...) and rows_moments(noise, ...)."""
    lib = _lib.load()
    n = check_table(table, 3, "add_noise_rows").shape[0]
    if lr.dtype != torch.float32 or noise.dtype != torch.float32 or not lr.is_contiguous() or not noise.is_contiguous():
        raise ValueError("add_noise_rows: lr and noise are contiguous float32 buffers")
    if noise.numel() < lr.numel():
        raise ValueError("add_noise_rows: the noise buffer has lr's layout (%d samples, got %d)" % (lr.numel(), noise.numel()))
    for m in (lr_moments, noise_moments):
        if m.dtype != torch.float64 or tuple(m.shape) != (n, 2) or not m.is_contiguous():
            raise ValueError("add_noise_rows: moments are contiguous float64 [%d, 2] tensors" % n)
    _lib.check(lib.mg_add_noise_rows(_lib.ptr(lr), _lib.ptr(noise), lr.numel(), _lib.ptr(table), n, int(max_len),
                                     _lib.ptr(lr_moments), _lib.ptr(noise_moments), float(snr), int(segment_length),
                                     _lib.stream()), "mg_add_noise_rows")
    return lr


def add_noise_packed(buf: torch.Tensor, win: torch.Tensor, longest: int, snr: float, segment_length: int,
                     z: torch.Tensor) -> torch.Tensor:
    """The --add_noise tail (data/audio_dataset.py:73-78 / :179-184) over a packed buffer, in place: the moments of `buf` and of the
    noise `z` (buf's layout) over the windows `win` (device int64 [n, 3], the longest of `longest` samples), then
    add_noise_rows."""
    return add_noise_rows(buf, z, win, longest, rows_moments(buf, win, longest), rows_moments(z, win, longest), snr,
                          segment_length)


def noise_buffer(noise, layout: PackedLayout, device, generator=None) -> torch.Tensor:
    """The noise of a packed buffer of `layout`: the caller's waveforms (one per row, packed alike) or, without them,
    torch.randn(layout.total, generator=generator) on the device."""
    if noise is None:
        return torch.randn(layout.total, dtype=torch.float32, device=device, generator=generator)
    return pack_waves(list(noise), layout, device)
