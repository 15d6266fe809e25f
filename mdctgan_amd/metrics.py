"""``compute_matrics`` (util/util.py:132-177) on the device: MSE, SNR of the super-resolved and of the low-rate waveform,
log-spectral distance.  Same call and return tuple as the reference -- ``(mse, snr_sr, snr_lr, 0, 0, 0, lsd)``, Python
floats -- but the waveforms stay in HBM: three row reductions in double precision, and for the LSD the power
spectrograms of ``aF.spectrogram(n_fft=2*opt.n_fft, hop=2*opt.hop_length, window=kbdwin(2*opt.win_length), center,
power=2)`` as windowed reflect-padded frames times a dense DFT table on the f32 MFMA pipe.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from . import _lib, ops
from .mdct import kbdwin
from .packed import aligned_layout, pack_waves, rows_moments, upload_tables, window_table

_tables = {}


def _dft_table(n_fft: int, device):
    """[2 * (n_fft/2 + 1), n_fft]: rows 2k = cos(2 pi k n / N), 2k+1 = -sin(2 pi k n / N) (float64 on the host, once)."""
    key = (n_fft, str(device))
    t = _tables.get(key)
    if t is None:
        k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)[:, None]
        n = torch.arange(n_fft, dtype=torch.float64)[None, :]
        ang = 2.0 * math.pi * k * n / n_fft
        t = torch.stack((torch.cos(ang), -torch.sin(ang)), dim=1).reshape(-1, n_fft).to(torch.float32).to(device).contiguous()
        _tables[key] = t
    return t


def power_spectra(audio: torch.Tensor, n_fft: int, hop_length: int, window: torch.Tensor, center: bool = True):
    """[B, T] -> interleaved (re, im) STFT coefficients [B * F, 2 * (n_fft/2 + 1)] and F."""
    lib = _lib.load()
    x = _lib.f32c(audio)
    B, T = x.shape
    F = lib.mg_stft_num_frames(T, n_fft, hop_length, int(center))
    if F <= 0:
        raise ValueError("signal of %d samples is too short for n_fft=%d" % (T, n_fft))
    frames = torch.empty(B * F, n_fft, dtype=torch.float32, device=x.device)
    w = _lib.f32c(window.to(x.device))
    _lib.check(lib.mg_stft_frames(_lib.ptr(x), B, T, _lib.ptr(w), n_fft, hop_length, int(center), _lib.ptr(frames),
                                  _lib.stream()), "mg_stft_frames")
    table = _dft_table(n_fft, x.device)
    g = ops.conv_geom(1, 1, B * F, n_fft, table.shape[0], 1, 1, 1, 0, False)
    spec = ops.conv_fwd(g, frames.view(1, 1, B * F, n_fft), table.view(table.shape[0], 1, 1, n_fft))
    return spec.view(B * F, table.shape[0]), F


def compute_matrics(hr_audio, lr_audio, sr_audio, opt):
    lib = _lib.load()
    dev = sr_audio.device
    hr = _lib.f32c(hr_audio.to(dev).reshape(-1, hr_audio.shape[-1]))
    lr = _lib.f32c(lr_audio.to(dev).reshape(-1, lr_audio.shape[-1]))
    sr = _lib.f32c(sr_audio.reshape(-1, sr_audio.shape[-1]))
    B, T = sr.shape
    sums = torch.empty(B, 3, dtype=torch.float64, device=dev)
    _lib.check(lib.mg_metrics_rows(_lib.ptr(hr), _lib.ptr(lr), _lib.ptr(sr), B, T, _lib.ptr(sums), _lib.stream()),
               "mg_metrics_rows")
    mse = (sums[:, 1].sum() / (B * T)).item()
    snr_sr = (10 * torch.log10(sums[:, 0] / sums[:, 1])).mean().item()
    snr_lr = (10 * torch.log10(sums[:, 0] / sums[:, 2])).mean().item()
    n_fft, hop, win = 2 * opt.n_fft, 2 * opt.hop_length, 2 * opt.win_length
    if win != n_fft:
        raise NotImplementedError("win_length != n_fft")
    window = kbdwin(win)
    sa, _ = power_spectra(hr, n_fft, hop, window, bool(opt.center))
    sb, _ = power_spectra(sr, n_fft, hop, window, bool(opt.center))
    per_frame = torch.empty(sa.shape[0], dtype=torch.float32, device=dev)
    _lib.check(lib.mg_lsd_frames(_lib.ptr(sa), _lib.ptr(sb), sa.shape[0], n_fft // 2 + 1, _lib.ptr(per_frame),
                                 _lib.stream()), "mg_lsd_frames")
    lsd = per_frame.double().mean().item()
    return mse, snr_sr, snr_lr, 0, 0, 0, lsd


# ---------------------------------------------------------------------------------------------------------------------
# Many utterances in shared launches
# ---------------------------------------------------------------------------------------------------------------------
LSD_ROWS_N_FFT = (512, 1024, 2048)         # the transform sizes of mg_lsd_rows (csrc/metrics_rows.hip)


@dataclass
class MetricsPlan:
    """plan_metrics' result: `frames[u]` = mg_stft_num_frames(lengths[u], n_fft, hop, center), `frame_start` its prefix sums
    (U + 1 entries: utterance u's per-frame values are [frame_start[u], frame_start[u + 1]) of the packed per-frame array)."""
    lengths: List[int]
    n_fft: int
    hop: int
    center: bool
    frames: List[int]
    frame_start: List[int]

    @property
    def total_frames(self) -> int:
        return self.frame_start[-1]


def plan_metrics(lengths, n_fft: int, hop: int, center: bool) -> MetricsPlan:
    """How many STFT frames every utterance has and where they sit in the packed per-frame array (host only: no device call).
    n_fft / hop: the transform's, i.e. 2 * opt.n_fft / 2 * opt.hop_length.  ValueError (naming the utterance) where mg_stft_frames
    refuses: a length without a frame, or a centred transform whose reflection (n_fft / 2 samples) does not fit the utterance."""
    n_fft, hop, center = int(n_fft), int(hop), bool(center)
    lengths = [int(n) for n in lengths]
    if not lengths:
        raise ValueError("plan_metrics needs at least one utterance")
    if n_fft <= 0 or hop <= 0:
        raise ValueError("n_fft and hop must be positive")
    frames, start = [], [0]
    for u, n in enumerate(lengths):
        padded = n + 2 * (n_fft // 2) if center else n
        if n <= 0 or padded < n_fft:
            raise ValueError("utterance %d: %d samples are too short for n_fft=%d" % (u, n, n_fft))
        if center and n_fft // 2 >= n:
            raise ValueError("utterance %d: %d samples cannot be reflect-padded by n_fft / 2 = %d" % (u, n, n_fft // 2))
        frames.append(1 + (padded - n_fft) // hop)
        start.append(start[-1] + frames[-1])
    return MetricsPlan(lengths, n_fft, hop, center, frames, start)


def _packed_operand(x, what: str):
    """A list of waveforms ([T_u] or [1, T_u]) -> (None, waves, lengths available); a packed `(buffer, starts)` or `(buffer,
    starts, lengths)` tuple -> (buffer, starts, lengths available).  Without lengths, an utterance of a packed buffer is taken to
    reach the next start (the end of the buffer for the last one)."""
    if isinstance(x, tuple) and len(x) in (2, 3) and torch.is_tensor(x[0]) and not torch.is_tensor(x[1]):
        buf, starts = x[0], [int(s) for s in x[1]]
        if buf.dim() != 1 or buf.dtype != torch.float32 or not buf.is_contiguous() or not buf.is_cuda:
            raise ValueError("%s: a packed operand is a contiguous float32 [total] device buffer" % what)
        if len(x) == 3:
            avail = [int(n) for n in x[2]]
            if len(avail) != len(starts):
                raise ValueError("%s: one length per start" % what)
        else:
            avail = [b - a for a, b in zip(starts, starts[1:] + [buf.numel()])]
        if any(s < 0 or n < 0 or s + n > buf.numel() for s, n in zip(starts, avail)):
            raise ValueError("%s: an utterance lies outside its packed buffer" % what)
        return buf, starts, avail
    waves = list(x)
    return None, waves, [int(w.numel()) for w in waves]


def _checked_operands(operands):
    """The operand forms, counts and lengths of ((hrs, "hrs"), ..., (srs, "srs")) -> (_packed_operand of each, hr's lengths)."""
    ops_ = [_packed_operand(x, name) for x, name in operands]
    hrs = operands[0][0]
    if isinstance(hrs, tuple) and ops_[0][0] is not None and len(hrs) != 3:
        raise ValueError("hrs: a packed ground truth names its lengths: (buffer, starts, lengths)")
    lengths = ops_[0][2]
    U = len(lengths)
    if U == 0:
        raise ValueError("no waveforms")
    for (_, _, avail), (_, name) in zip(ops_[1:], operands[1:]):
        name = name[:-1]
        if len(avail) != U:
            raise ValueError("%d hr waveforms but %d %s waveforms" % (U, len(avail), name))
        for u in range(U):
            if avail[u] < lengths[u]:
                raise ValueError("utterance %d: %s has %d samples, fewer than hr's %d" % (u, name, avail[u], lengths[u]))
    return ops_, lengths


def _pack_operands(ops_, differentiable):
    """Packs what came as a list (packed.aligned_layout's layout) -> (device, buffers, starts) in the operands' order."""
    device = next((t.device for buf, ws, _ in ops_ for t in ([buf] if buf is not None else ws) if t.is_cuda), None)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    bufs, starts = [], []
    for buf, ws, avail in ops_:
        if buf is None:
            layout = aligned_layout(avail)
            with_grad = differentiable and torch.is_grad_enabled() and any(w.requires_grad for w in ws)
            buf, ws = (_pack_with_grad if with_grad else pack_waves)(ws, layout, device), layout.starts
        bufs.append(buf)
        starts.append(ws)
    return device, bufs, starts


def _metric_operands(operands, opt, hr_shift, differentiable=False):
    """What compute_matrics_many and the LSD loss do before their launches, stated once so that the two stay in step.  operands:
    ((hrs, "hrs"), ..., (srs, "srs")), the ground truth first; every other one is cropped to its lengths and must not be shorter.
    Checks the transform (2 * opt.n_fft in LSD_ROWS_N_FFT, win_length == n_fft), the operand forms, the counts, the lengths and
    hr_shift, plans the frames, and packs what came as a list (packed.aligned_layout's layout; `differentiable`: a list with an
    entry that requires grad is packed by one differentiable concatenation).
    -> (n_fft, hop, win, plan, device, buffers, starts), buffers / starts in the operands' order."""
    n_fft, hop, win = 2 * int(opt.n_fft), 2 * int(opt.hop_length), 2 * int(opt.win_length)
    if win != n_fft:
        raise NotImplementedError("win_length != n_fft")
    if n_fft not in LSD_ROWS_N_FFT:
        raise NotImplementedError("mg_lsd_rows serves n_fft in %s (got %d)" % (LSD_ROWS_N_FFT, n_fft))
    ops_, lengths = _checked_operands(operands)
    U = len(lengths)
    plan = plan_metrics(lengths, n_fft, hop, bool(opt.center))
    device, bufs, starts = _pack_operands(ops_, differentiable)
    if hr_shift is not None and (not hr_shift.is_cuda or hr_shift.dtype != torch.float32 or hr_shift.numel() != U
                                 or not hr_shift.is_contiguous()):
        raise ValueError("hr_shift is a contiguous float32 [%d] device tensor" % U)
    return n_fft, hop, win, plan, device, bufs, starts


def compute_matrics_many(hrs, lrs, srs, opt, hr_shift=None):
    """``compute_matrics`` for every utterance of a test set on its own (generate_audio.py:57-67), in shared launches.
    hrs / lrs / srs: lists of waveforms ([T_u] or [1, T_u], host or device; packed here with packed.aligned_layout's layout), or packed
    operands that are read where they lie -- ``(buffer, starts, lengths)`` (hrs), ``(buffer, starts)`` or ``(buffer, starts,
    lengths)`` (lrs, srs) with a contiguous float32 device buffer and host lists, as front_end_many and generate_many leave them.
    Utterance u is scored over len_u = len(hr_u) samples; lr_u and sr_u are cropped to that and must not be shorter (ValueError).
    hr_shift: float32 [U] on the device; every ground-truth sample enters as hr + hr_shift[u] (one float32 add) -- read_audio's
    un-materialised DC shift.  -> float64 device tensor [U, 7], row u = (mse, snr_sr, snr_lr, 0, 0, 0, lsd) of utterance u alone,
    with the same bits whatever else shares the call.  Launches: one table copy (plus one packing copy per operand given as a
    list), mg_metrics_rows_packed, mg_lsd_rows, mg_rows_moments and a few element-wise launches over [U], whatever U is; nothing
    is read back."""
    n_fft, hop, win, plan, device, (hr, lr, sr), starts = _metric_operands(((hrs, "hrs"), (lrs, "lrs"), (srs, "srs")), opt,
                                                                           hr_shift)
    lengths = plan.lengths
    U = len(lengths)

    # every table in one copy: the metric rows, frame_start, and the windows of the per-frame array
    rows = np.stack([np.asarray(t, dtype=np.int64) for t in (*starts, lengths)], axis=1)
    row_t, fs_t, frame_t = upload_tables([rows, plan.frame_start, window_table(plan.frame_start[:-1], plan.frames)], device)

    lib = _lib.load()
    max_len = max(lengths)
    nbytes = lib.mg_metrics_rows_packed_workspace(U, max_len)
    ws = _lib.workspace(nbytes, device)
    sums = torch.empty(U, 3, dtype=torch.float64, device=device)
    _lib.check(lib.mg_metrics_rows_packed(_lib.ptr(hr), hr.numel(), _lib.ptr(lr), lr.numel(), _lib.ptr(sr), sr.numel(),
                                          _lib.ptr(row_t), U, max_len, _lib.ptr(hr_shift), _lib.ptr(sums), _lib.ptr(ws), nbytes,
                                          _lib.stream()), "mg_metrics_rows_packed")
    window = _window(win, device)
    per_frame = torch.empty(plan.total_frames, dtype=torch.float32, device=device)
    _lib.check(lib.mg_lsd_rows(_lib.ptr(hr), hr.numel(), _lib.ptr(sr), sr.numel(), _lib.ptr(row_t), U, _lib.ptr(fs_t),
                               plan.total_frames, _lib.ptr(hr_shift), _lib.ptr(window), n_fft, hop, int(bool(opt.center)),
                               _lib.ptr(per_frame), _lib.stream()), "mg_lsd_rows")
    lsd_sum = rows_moments(per_frame, frame_t, max(plan.frames))[:, 0]

    out = torch.zeros(U, 7, dtype=torch.float64, device=device)
    out[:, 0] = sums[:, 1] / row_t[:, 3].double()
    out[:, 1] = 10 * torch.log10(sums[:, 0] / sums[:, 1])
    out[:, 2] = 10 * torch.log10(sums[:, 0] / sums[:, 2])
    out[:, 6] = lsd_sum / (frame_t[:, 2] - frame_t[:, 1]).double()
    return out


_windows = {}


def _window(win: int, device):
    key = (win, str(device))
    if key not in _windows:
        _windows[key] = kbdwin(win).to(device=device, dtype=torch.float32).contiguous()
    return _windows[key]


# ---------------------------------------------------------------------------------------------------------------------
# The log-spectral distance as a loss: mg_lsd_rows forward, mg_lsd_rows_backward (csrc/lsd_rows_grad.hip) backward
# ---------------------------------------------------------------------------------------------------------------------
class _LsdRows(torch.autograd.Function):
    """Per-utterance LSD [U] (float64) of a packed sr buffer against a packed, constant hr buffer.  Forward: mg_lsd_rows and
    rows_moments, compute_matrics_many's statements.  Backward: the upstream gradient divided by every row's frame count, then
    mg_lsd_rows_backward into a zero-filled buffer of sr's size."""

    @staticmethod
    def forward(ctx, sr, hr, row_t, fs_t, frame_t, hr_shift, window, geom):
        n_fft, hop, center, total_frames, max_frames = geom
        lib = _lib.load()
        per_frame = torch.empty(total_frames, dtype=torch.float32, device=sr.device)
        _lib.check(lib.mg_lsd_rows(_lib.ptr(hr), hr.numel(), _lib.ptr(sr), sr.numel(), _lib.ptr(row_t), row_t.shape[0],
                                   _lib.ptr(fs_t), total_frames, _lib.ptr(hr_shift), _lib.ptr(window), n_fft, hop, int(center),
                                   _lib.ptr(per_frame), _lib.stream()), "mg_lsd_rows")
        lsd_sum = rows_moments(per_frame, frame_t, max_frames)[:, 0]
        ctx.save_for_backward(sr, hr, row_t, fs_t, frame_t, hr_shift, window)
        ctx.geom = geom
        return lsd_sum / (frame_t[:, 2] - frame_t[:, 1]).double()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        sr, hr, row_t, fs_t, frame_t, hr_shift, window = ctx.saved_tensors
        n_fft, hop, center, total_frames, _ = ctx.geom
        lib = _lib.load()
        grad_rows = (grad.double() / (frame_t[:, 2] - frame_t[:, 1]).double()).float().contiguous()
        grad_sr = torch.zeros_like(sr)
        nbytes = lib.mg_lsd_rows_backward_workspace(total_frames, n_fft)
        ws = _lib.workspace(nbytes, sr.device)
        _lib.check(lib.mg_lsd_rows_backward(_lib.ptr(hr), hr.numel(), _lib.ptr(sr), sr.numel(), _lib.ptr(row_t), row_t.shape[0],
                                            _lib.ptr(fs_t), total_frames, _lib.ptr(hr_shift), _lib.ptr(window), n_fft, hop,
                                            int(center), _lib.ptr(grad_rows), _lib.ptr(grad_sr), _lib.ptr(ws), nbytes,
                                            _lib.stream()), "mg_lsd_rows_backward")
        return grad_sr, None, None, None, None, None, None, None


def _pack_with_grad(waves, layout, device):
    """pack_waves' buffer as one differentiable concatenation (the gradient of the packed buffer is cut back to the waveforms)."""
    gap = torch.zeros(max(layout.total - sum(layout.lengths), 1), dtype=torch.float32, device=device)
    parts = []
    for w, s0, s1 in zip(waves, layout.starts, layout.starts[1:] + [layout.total]):
        parts.append(w.reshape(-1).to(device=device, dtype=torch.float32))
        if s1 - s0 > w.numel():
            parts.append(gap[:s1 - s0 - w.numel()])
    return torch.cat(parts)


_loss_tables = {}           # the device tables of the losses' dense geometries, (loss, geometry) -> tensors, uploaded once


def _row_tables(key, starts, lengths, more, device):
    """The tables of a loss in one copy -> device tensors: the metric rows {hr start, 0, sr start, length} (compute_matrics_many's
    without the lr column), then what more() lists.  A caller that names its geometry (key is not None) finds the same tensors
    again -- a captured graph goes on reading them.  The cache is ONE for all losses: the insertion of a 65th geometry by any
    loss drops every loss's tables (never those being inserted), so a graph captured over one of the 64 dropped geometries must
    be captured again; a training run has a few geometries and never gets there."""
    tables = _loss_tables.get(key) if key is not None else None
    if tables is None:
        rows = np.stack([np.asarray(t, dtype=np.int64) for t in (starts[0], [0] * len(lengths), starts[1], lengths)], axis=1)
        tables = upload_tables([rows] + more(), device)
        if key is not None:
            if len(_loss_tables) >= 64:         # a training run has a few geometries; a sweep over many must not pile tables up
                _loss_tables.clear()            # (before the insertion: never the geometry in use)
            _loss_tables[key] = tables
    return tables


def _hr_is_constant(hr_op, what):
    """hr_op: _packed_operand's result for the ground truth."""
    if any(t.requires_grad for t in ([hr_op[0]] if hr_op[0] is not None else hr_op[1])):
        raise NotImplementedError("the %s has no gradient with respect to hr: detach the ground truth" % what)


def _finite_scale(scale) -> float:
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError("scale must be finite")
    return scale


def _lsd_operands(hrs, srs, opt, hr_shift, table_key=None):
    """What every LSD loss node is applied to: -> (sr, hr, row_t, fs_t, frame_t, hr_shift, window, geom)."""
    _hr_is_constant(_packed_operand(hrs, "hrs"), "LSD")
    n_fft, hop, win, plan, device, (hr, sr), starts = _metric_operands(((hrs, "hrs"), (srs, "srs")), opt, hr_shift,
                                                                       differentiable=True)
    row_t, fs_t, frame_t = _row_tables(table_key, starts, plan.lengths,
                                       lambda: [plan.frame_start, window_table(plan.frame_start[:-1], plan.frames)], device)
    geom = (n_fft, hop, plan.center, plan.total_frames, max(plan.frames))
    return sr, hr, row_t, fs_t, frame_t, hr_shift, _window(win, device), geom


def _lsd_rows(hrs, srs, opt, hr_shift, table_key=None):
    return _LsdRows.apply(*_lsd_operands(hrs, srs, opt, hr_shift, table_key))


def lsd_many(hrs, srs, opt, hr_shift=None):
    """The log-spectral distance of every utterance on its own, differentiable in sr -> float64 device tensor [U]: column 6 of
    ``compute_matrics_many`` bit for bit, from the same operand forms (lists of waveforms, or packed ``(buffer, starts,
    lengths)`` / ``(buffer, starts[, lengths])`` read where they lie), the same ``plan_metrics`` table and the same launches
    (mg_lsd_rows, mg_rows_moments).  The gradient reaches a packed sr buffer that requires grad, or the list entries that do
    (packed then by one differentiable concatenation); it is mg_lsd_rows_backward's: two launches whatever U is, deterministic,
    exactly 0 on frames whose distance is 0 (sr == hr, silence), where autograd through torch.stft has NaN.  hr is a constant:
    a ground truth that requires grad raises NotImplementedError.  Nothing is read back."""
    return _lsd_rows(hrs, srs, opt, hr_shift)


def lsd_loss(sr_audio, hr_audio, opt):
    """The reference's ``lsd`` (util/util.py:171-175: the mean over all frames of a batch of equal-length clips) as a training
    loss -> 0-dim float64 tensor, differentiable in sr_audio.  sr_audio / hr_audio: dense float32 device tensors [B, T], [B, 1,
    T] or [B, 1, 1, T] -- what ``Audio2MDCT.to_audio`` returns -- read in place as a pack with starts b * T (no packing copy).
    Nothing is read back and the row tables of a geometry are uploaded once and kept, so forward + backward capture into a
    graph on one stream after one eager call.  As for any autograd capture: no graph built on another stream from the same
    leaf may still be alive (detach or drop earlier losses), or the engine synchronises the capture with that stream."""
    return _lsd_rows(*_dense_batch(sr_audio, hr_audio, opt)).mean()


def _dense_pack(sr_audio, hr_audio):
    """The operand checks of the dense-batch losses -> (hrs, srs, B, T): both batches as packs read in place."""
    flat = []
    for x, what in ((sr_audio, "sr_audio"), (hr_audio, "hr_audio")):
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() not in (2, 3, 4) \
                or any(n != 1 for n in x.shape[1:-1]):
            raise ValueError("%s is a float32 device tensor [B, T], [B, 1, T] or [B, 1, 1, T]" % what)
        flat.append((x if x.is_contiguous() else x.contiguous()).reshape(-1))
    B, T = int(sr_audio.shape[0]), int(sr_audio.shape[-1])
    if (int(hr_audio.shape[0]), int(hr_audio.shape[-1])) != (B, T):
        raise ValueError("sr_audio holds %d clips of %d samples, hr_audio %d of %d" % (B, T, hr_audio.shape[0], hr_audio.shape[-1]))
    starts, lengths = [b * T for b in range(B)], [T] * B
    return (flat[1], starts, lengths), (flat[0], starts, lengths), B, T


def _dense_batch(sr_audio, hr_audio, opt):
    """lsd_loss's and lsd_loss_term's operand checks -> the arguments of _lsd_operands: both batches as packs read in place."""
    hrs, srs, B, T = _dense_pack(sr_audio, hr_audio)
    key = ("lsd", B, T, int(opt.n_fft), int(opt.hop_length), bool(opt.center), str(sr_audio.device))
    return hrs, srs, opt, None, key


class _LsdMeanLoss(torch.autograd.Function):
    """scale * the mean over all frames of a pack's per-frame LSD, as a node of the training step's loss family (functional._LossFn):
    a float32 [1] loss, the constant factor inside, the upstream gradient read on the device.  Forward: mg_lsd_rows and
    mg_lsd_mean_loss.  Backward: mg_lsd_rows_backward_seeded into an uninitialised buffer of sr's size -- the caller's pack is dense
    (every sample belongs to a live row, and the gather writes every sample of a live row), so there is nothing to zero-fill."""

    @staticmethod
    def forward(ctx, sr, hr, row_t, fs_t, window, geom, scale):
        n_fft, hop, center, total_frames, _ = geom
        lib = _lib.load()
        per_frame = torch.empty(total_frames, dtype=torch.float32, device=sr.device)
        _lib.check(lib.mg_lsd_rows(_lib.ptr(hr), hr.numel(), _lib.ptr(sr), sr.numel(), _lib.ptr(row_t), row_t.shape[0],
                                   _lib.ptr(fs_t), total_frames, None, _lib.ptr(window), n_fft, hop, int(center),
                                   _lib.ptr(per_frame), _lib.stream()), "mg_lsd_rows")
        loss = torch.empty(1, dtype=torch.float32, device=sr.device)
        _lib.check(lib.mg_lsd_mean_loss(_lib.ptr(per_frame), total_frames, scale, _lib.ptr(loss), _lib.stream()), "mg_lsd_mean_loss")
        ctx.save_for_backward(sr, hr, row_t, fs_t, window)
        ctx.geom, ctx.scale = geom, scale
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        sr, hr, row_t, fs_t, window = ctx.saved_tensors
        n_fft, hop, center, total_frames, _ = ctx.geom
        lib = _lib.load()
        go = go.reshape(1).float().contiguous()
        grad_sr = torch.empty_like(sr)
        nbytes = lib.mg_lsd_rows_backward_workspace(total_frames, n_fft)
        ws = _lib.workspace(nbytes, sr.device)
        _lib.check(lib.mg_lsd_rows_backward_seeded(_lib.ptr(hr), hr.numel(), _lib.ptr(sr), sr.numel(), _lib.ptr(row_t),
                                                   row_t.shape[0], _lib.ptr(fs_t), total_frames, None, _lib.ptr(window), n_fft, hop,
                                                   int(center), _lib.ptr(go), ctx.scale, _lib.ptr(grad_sr), _lib.ptr(ws), nbytes,
                                                   _lib.stream()), "mg_lsd_rows_backward_seeded")
        return grad_sr, None, None, None, None, None, None


def lsd_loss_term(sr_audio, hr_audio, opt, scale):
    """``scale * lsd_loss(sr_audio, hr_audio, opt)`` as a term of the training step -> 0-dim float32 tensor, differentiable in
    sr_audio: lsd_loss's operand forms, checks and cached row tables, but one autograd node in the step's loss convention
    (functional._LossFn) instead of a float64 composition.  Forward is mg_lsd_rows plus one reduction launch (the mean over all
    frames: for the equal-length clips of a dense batch, lsd_loss's mean of per-clip means up to float64 rounding); backward is
    mg_lsd_rows_backward_seeded, which forms every clip's upstream gradient on the device from the upstream scalar -- in the
    arithmetic autograd performs for ``scale * lsd_loss``, so a power-of-two scale gives that gradient bit for bit -- and writes
    every sample, so no buffer is zero-filled.  The upstream gradient (the GradScaler's loss scale in a --fp16 step) stays on the
    device and is read when the kernel runs: a captured step follows it.  Capturable after one eager call, like lsd_loss."""
    scale = _finite_scale(scale)
    sr, hr, row_t, fs_t, _, _, window, geom = _lsd_operands(*_dense_batch(sr_audio, hr_audio, opt))
    return _LsdMeanLoss.apply(sr, hr, row_t, fs_t, window, geom, scale)


# ---------------------------------------------------------------------------------------------------------------------
# The losses of several resolutions, two launches each way per resolution, row_out [R, U, 4]: the multi-resolution STFT loss
# (spectral convergence + log-magnitude L1, csrc/stft_loss_rows.hip) and the multi-scale mel-spectrogram L1 loss
# (csrc/mel_loss_rows.hip).  One operand builder, one forward and one backward loop, one pair of autograd nodes and one dense-batch
# wrapper, parameterised by a _RowsLoss; what differs between the two stands in their resolution parsers and in mel's filterbanks.
# ---------------------------------------------------------------------------------------------------------------------
STFT_RESOLUTIONS = ((512, 128), (1024, 256), (2048, 512))       # (n_fft, hop) of the default loss
STFT_CLAMP = 1e-7                                               # m = sqrt(max(re^2 + im^2, STFT_CLAMP))
MEL_RESOLUTIONS = ((512, 128, 40), (1024, 256, 80), (2048, 512, 160))       # (n_fft, hop, n_mels) of the default loss
MEL_FLOOR = 1e-5                                                            # l = ln(max(E, MEL_FLOOR))
MEL_MAX_FILTERS = 256                                                       # the kernels' limit on n_mels

_mel_fbanks = {}            # (sample_rate, n_fft, n_mels, f_min, f_max, device) -> (W, band_k, band_j) on the device


def _hann(n_fft: int, device):
    """The periodic Hann window of n_fft samples, evaluated in float64 and rounded to float32 once."""
    key = ("hann", n_fft, str(device))
    if key not in _windows:
        _windows[key] = torch.hann_window(n_fft, periodic=True, dtype=torch.float64).to(torch.float32).to(device).contiguous()
    return _windows[key]


def _parse_resolutions(resolutions, fields, kernels):
    """-> a tuple of int tuples, one value per field: ("n_fft", "hop") or ("n_fft", "hop", "n_mels"); `kernels` names the loss."""
    shape = "(%s) %s" % (", ".join(fields), "pair" if len(fields) == 2 else "triple")
    try:
        res = tuple(tuple(int(v) for v in r) for r in resolutions)
        if any(len(r) != len(fields) for r in res):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("resolutions: a sequence of %ss" % shape) from None
    if not res:
        raise ValueError("resolutions: at least one %s" % shape)
    for r in res:
        if r[0] not in LSD_ROWS_N_FFT:
            raise NotImplementedError("the %s loss kernels serve n_fft in %s (got %d)" % (kernels, LSD_ROWS_N_FFT, r[0]))
        if r[1] < 1:
            raise ValueError("resolution %s: the hop must be at least 1" % (r,))
        if len(r) == 3 and not 1 <= r[2] <= MEL_MAX_FILTERS:
            raise ValueError("resolution %s: the mel loss kernels serve 1 to %d filters" % (r, MEL_MAX_FILTERS))
    return res


def _resolutions(resolutions):
    return _parse_resolutions(resolutions, ("n_fft", "hop"), "STFT")


def _mel_resolutions(resolutions):
    return _parse_resolutions(resolutions, ("n_fft", "hop", "n_mels"), "mel")


def _plan_resolutions(lengths, res, center):
    plans = []
    for r in res:
        try:
            plans.append(plan_metrics(lengths, r[0], r[1], center))
        except ValueError as e:
            raise ValueError("resolution %s: %s" % (r, e)) from None
    return plans


def plan_mrstft(lengths, resolutions=STFT_RESOLUTIONS, center: bool = True):
    """plan_metrics for every resolution (host only) -> [MetricsPlan]; ValueError naming the utterance AND the resolution where an
    utterance has no frame or (centred) cannot be reflected: len <= n_fft / 2."""
    return _plan_resolutions(lengths, _resolutions(resolutions), center)


def plan_mel(lengths, resolutions=MEL_RESOLUTIONS, center: bool = True):
    """plan_metrics for every resolution (n_fft, hop, n_mels) (host only) -> [MetricsPlan]; ValueError naming the utterance AND the
    resolution where an utterance has no frame or (centred) cannot be reflected: len <= n_fft / 2."""
    return _plan_resolutions(lengths, _mel_resolutions(resolutions), center)


def mel_fbank(sample_rate, n_fft: int, n_mels: int, f_min: float = 0.0, f_max=None):
    """The HTK triangular mel filterbank without area normalisation -> float32 host tensor [n_mels, n_fft / 2 + 1], evaluated in
    float64 and rounded once: mel(f) = 2595 log10(1 + f / 700); n_mels + 2 equally spaced mel points from f_min to f_max (default
    sample_rate / 2) mapped back to Hz, h_0 .. h_{n_mels + 1}; with f_k = k sample_rate / n_fft,
        W[j][k] = max(0, min((f_k - h_j) / (h_{j+1} - h_j), (h_{j+2} - f_k) / (h_{j+2} - h_{j+1})))."""
    n_fft, n_mels = int(n_fft), int(n_mels)
    sample_rate, f_min = float(sample_rate), float(f_min)
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    if n_fft < 2 or n_mels < 1 or not sample_rate > 0.0:
        raise ValueError("mel_fbank: n_fft >= 2, n_mels >= 1 and a positive sample rate")
    if not 0.0 <= f_min < f_max <= sample_rate / 2.0:
        raise ValueError("mel_fbank: 0 <= f_min < f_max <= sample_rate / 2 (got %r, %r)" % (f_min, f_max))
    mel_lo, mel_hi = (2595.0 * np.log10(1.0 + f / 700.0) for f in (f_min, f_max))
    h = 700.0 * (10.0 ** (np.linspace(mel_lo, mel_hi, n_mels + 2, dtype=np.float64) / 2595.0) - 1.0)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * (sample_rate / n_fft)
    up = (f[None, :] - h[:-2, None]) / (h[1:-1] - h[:-2])[:, None]
    down = (h[2:, None] - f[None, :]) / (h[2:] - h[1:-1])[:, None]
    return torch.from_numpy(np.maximum(0.0, np.minimum(up, down)).astype(np.float32))


def mel_band_tables(fbank):
    """The two tables the kernels walk a filterbank with, derived from W [J, K] (host) -> int32 numpy (band_k [J, 2], band_j [K, 2]):
    filter j is non-zero exactly on the bins [band_k[j, 0], band_k[j, 1]), bin k lies exactly in the filters [band_j[k, 0],
    band_j[k, 1]) (a bin in no filter: an empty range).  ValueError for a W that is not a finite float32 matrix of 1 .. 256 rows,
    an empty filter (an all-zero row, named), a support or a bin's set of filters that is not one contiguous run, or tables that
    are not monotone (the ends of the non-empty ranges must not decrease)."""
    W = fbank.detach().cpu().numpy() if torch.is_tensor(fbank) else np.asarray(fbank)
    if W.ndim != 2 or W.dtype != np.float32 or not 1 <= W.shape[0] <= MEL_MAX_FILTERS or not np.all(np.isfinite(W)):
        raise ValueError("a filterbank is a finite float32 matrix [n_mels, bins] with 1 <= n_mels <= %d" % MEL_MAX_FILTERS)
    nz = W != 0.0
    tables = []
    for what, mask in (("filter", nz), ("bin", nz.T)):
        table = np.zeros((mask.shape[0], 2), dtype=np.int32)
        last = (0, 0)
        for i, row in enumerate(mask):
            at = np.flatnonzero(row)
            if at.size == 0:
                if what == "filter":
                    raise ValueError("filter %d is empty (an all-zero row of the filterbank)" % i)
                continue
            lo, hi = int(at[0]), int(at[-1]) + 1
            if hi - lo != at.size:
                raise ValueError("%s %d: its %s are not one contiguous run" % (what, i, "bins" if what == "filter" else "filters"))
            if lo < last[0] or hi < last[1]:
                raise ValueError("%s %d: the band tables are not monotone" % (what, i))
            table[i] = last = (lo, hi)
        tables.append(table)
    return tables[0], tables[1]


def _mel_bank(sample_rate, n_fft, n_mels, f_min, f_max, device=None):
    """mel_fbank and its band tables, checked; device None: the host check alone, else the three tensors on the device (built once
    per (sample_rate, n_fft, n_mels, f_min, f_max, device) and kept).  ValueError naming the filter for an empty one."""
    key = (float(sample_rate), n_fft, n_mels, float(f_min), None if f_max is None else float(f_max))
    bank = _mel_fbanks.get(key + (str(device),))
    if bank is None:
        host = _mel_fbanks.get(key + ("None",))
        if host is None:
            W = mel_fbank(sample_rate, n_fft, n_mels, f_min, f_max)
            host = _mel_fbanks[key + ("None",)] = (W,) + tuple(torch.from_numpy(t) for t in mel_band_tables(W))
        bank = host if device is None else tuple(t.to(device).contiguous() for t in host)
        _mel_fbanks[key + (str(device),)] = bank
    return bank


def _mel_banks(res, sample_rate, f_min, f_max, device=None):
    banks = []
    for n, h, j in res:
        try:
            banks.append(_mel_bank(sample_rate, n, j, f_min, f_max, device))
        except ValueError as e:
            raise ValueError("resolution (%d, %d, %d) at %g Hz: %s" % (n, h, j, float(sample_rate), e)) from None
    return tuple(banks)


@dataclass(frozen=True)
class _RowsLoss:
    """One loss of the family.  what: its name in messages; entry: its forward C entry point -- entry + "_workspace", "_backward",
    "_backward_workspace" and "_backward_seeded" are the others; parse: its resolution parser; extras(res, device, *params): per
    resolution, what its entry points take between `center` and the outputs (device None: the host checks alone, for their
    refusals); sums: whether the backward reads the forward's row_out."""
    what: str
    entry: str
    parse: object
    extras: object
    sums: bool


_MRSTFT = _RowsLoss("MR-STFT loss", "mg_stft_loss_rows", _resolutions, lambda res, device: ((),) * len(res), True)
def _mel_extras(res, device, sample_rate, f_min, f_max):
    """(W, band_k, band_j, n_mels) per resolution.  _rows_loss_operands calls this twice: with device None before anything is packed
    -- _mel_banks then builds and checks the banks on the host, which is where an empty filter is refused -- and with the device."""
    return tuple(bank + (r[2],) for bank, r in zip(_mel_banks(res, sample_rate, f_min, f_max, device), res))


_MEL = _RowsLoss("mel loss", "mg_mel_loss_rows", _mel_resolutions, _mel_extras, False)


def _rows_loss_operands(loss, hrs, srs, resolutions, center, params=(), table_key=None):
    """What every node of the family is applied to -> (loss, sr, hr, row_t, tabs); tabs = (frame_start tables, windows, extras,
    geometries (n_fft, hop, center, total_frames)), one entry per resolution.  params: loss.extras' (mel: sample_rate, f_min,
    f_max).  Every refusal comes before anything is packed or uploaded."""
    res, center = loss.parse(resolutions), bool(center)
    ops_, lengths = _checked_operands(((hrs, "hrs"), (srs, "srs")))
    _hr_is_constant(ops_[0], loss.what)
    plans = _plan_resolutions(lengths, res, center)
    loss.extras(res, None, *params)
    device, (hr, sr), starts = _pack_operands(ops_, True)
    extras = loss.extras(res, device, *params)
    tables = _row_tables(table_key, starts, lengths, lambda: [p.frame_start for p in plans], device)
    geoms = tuple((p.n_fft, p.hop, center, p.total_frames) for p in plans)
    return loss, sr, hr, tables[0], (tuple(tables[1:]), tuple(_hann(r[0], device) for r in res), extras, geoms)


def _ptrs(args):
    return tuple(_lib.ptr(a) if torch.is_tensor(a) else a for a in args)


def _rows_loss_forward(loss, sr, hr, row_t, tabs):
    """loss.entry for every resolution -> row_out float64 [R, U, 4]: {A, B, C, loss} (MR-STFT), {sum, 0, 0, loss} (mel)."""
    lib = _lib.load()
    U = row_t.shape[0]
    row_out = torch.empty(len(tabs[3]), U, 4, dtype=torch.float64, device=sr.device)
    for r, (fs_t, window, extra, (n_fft, hop, center, total_frames)) in enumerate(zip(*tabs)):
        nbytes = getattr(lib, loss.entry + "_workspace")(total_frames)
        ws = _lib.workspace(nbytes, sr.device)
        _lib.check(getattr(lib, loss.entry)(_lib.ptr(hr), hr.numel(), _lib.ptr(sr), sr.numel(), _lib.ptr(row_t), U, _lib.ptr(fs_t),
                                            total_frames, _lib.ptr(window), n_fft, hop, int(center), *_ptrs(extra),
                                            _lib.ptr(row_out[r]), _lib.ptr(ws), nbytes, _lib.stream()), loss.entry)
    return row_out


def _rows_loss_backward(loss, sr, hr, row_t, tabs, row_out, grad_sr, grad_rows=None, go=None, scale=0.0):
    """loss.entry + "_backward" (grad_rows [U]) or its seeded form (go [1], scale) for every resolution, in resolution order: the
    first writes every sample of the live rows of grad_sr, the later ones add to it."""
    lib = _lib.load()
    U, R = row_t.shape[0], len(tabs[3])
    for r, (fs_t, window, extra, (n_fft, hop, center, total_frames)) in enumerate(zip(*tabs)):
        nbytes = getattr(lib, loss.entry + "_backward_workspace")(total_frames, n_fft)
        ws = _lib.workspace(nbytes, sr.device)
        head = (_lib.ptr(hr), hr.numel(), _lib.ptr(sr), sr.numel(), _lib.ptr(row_t), U, _lib.ptr(fs_t), total_frames, _lib.ptr(window),
                n_fft, hop, int(center)) + _ptrs(extra) + ((_lib.ptr(row_out[r]),) if loss.sums else ())
        tail = (int(r > 0), _lib.ptr(grad_sr), _lib.ptr(ws), nbytes, _lib.stream())
        if go is None:
            what = loss.entry + "_backward"
            _lib.check(getattr(lib, what)(*head, _lib.ptr(grad_rows), *tail), what)
        else:
            what = loss.entry + "_backward_seeded"
            _lib.check(getattr(lib, what)(*head, _lib.ptr(go), scale, R, *tail), what)
    return grad_sr


class _RowsLossRows(torch.autograd.Function):
    """Per-utterance loss [U] (float64) of a packed sr buffer against a packed, constant hr buffer: the losses of the resolutions
    added in resolution order and divided by their number.  Backward: into a zero-filled buffer of sr's size."""

    @staticmethod
    def forward(ctx, loss, sr, hr, row_t, tabs):
        row_out = _rows_loss_forward(loss, sr, hr, row_t, tabs)
        ctx.save_for_backward(sr, hr, row_t, row_out)
        ctx.loss, ctx.tabs = loss, tabs
        total = row_out[0, :, 3].clone()
        for r in range(1, row_out.shape[0]):
            total = total + row_out[r, :, 3]
        return total / row_out.shape[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        sr, hr, row_t, row_out = ctx.saved_tensors
        grad_rows = (grad.double() / row_out.shape[0]).float().contiguous()
        return None, _rows_loss_backward(ctx.loss, sr, hr, row_t, ctx.tabs, row_out, torch.zeros_like(sr),
                                         grad_rows=grad_rows), None, None, None


class _RowsLossMean(torch.autograd.Function):
    """scale * the mean over the clips of a loss of the family as a node of the training step's loss family: a float32 [1] loss, the
    constant factor inside, the upstream gradient read on the device.  Forward: loss.entry per resolution and mg_stft_loss_mean
    (row_out has one layout).  Backward: the seeded entry point per resolution into an uninitialised buffer of sr's size -- the
    pack is dense and every row is live at every resolution, so the first resolution writes every sample."""

    @staticmethod
    def forward(ctx, loss, sr, hr, row_t, tabs, scale):
        row_out = _rows_loss_forward(loss, sr, hr, row_t, tabs)
        out = torch.empty(1, dtype=torch.float32, device=sr.device)
        _lib.check(_lib.load().mg_stft_loss_mean(_lib.ptr(row_out), row_out.shape[1], row_out.shape[0], scale, _lib.ptr(out),
                                                 _lib.stream()), "mg_stft_loss_mean")
        ctx.save_for_backward(sr, hr, row_t, row_out)
        ctx.loss, ctx.tabs, ctx.scale = loss, tabs, scale
        return out.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        sr, hr, row_t, row_out = ctx.saved_tensors
        go = go.reshape(1).float().contiguous()
        return None, _rows_loss_backward(ctx.loss, sr, hr, row_t, ctx.tabs, row_out, torch.empty_like(sr), go=go,
                                         scale=ctx.scale), None, None, None, None


def _rows_loss_dense(loss, sr_audio, hr_audio, resolutions, params=()):
    """The dense-batch losses' operands: both batches as packs read in place, the tables kept under the geometry."""
    hrs, srs, B, T = _dense_pack(sr_audio, hr_audio)
    res = loss.parse(resolutions)
    key = (loss.entry, B, T, res) + tuple(None if p is None else float(p) for p in params) + (str(sr_audio.device),)
    return _rows_loss_operands(loss, hrs, srs, res, True, params, key)


def mrstft_many(hrs, srs, resolutions=STFT_RESOLUTIONS, center=True):
    """The multi-resolution STFT loss of every utterance on its own, differentiable in sr -> float64 device tensor [U].  For one
    resolution (n_fft, hop) -- periodic Hann window of n_fft samples, centred frames reflected at the utterance's own ends, K =
    n_fft / 2 + 1 bins, F_u frames, m = sqrt(max(re^2 + im^2, 1e-7)) --
        loss_u = sqrt(sum (m_hr - m_sr)^2 / sum m_hr^2) + sum |ln m_hr - ln m_sr| / (F_u K)
    with the sums over all frames and bins of utterance u, and the result is the mean over the resolutions.  Operand forms as for
    ``lsd_many``: lists of waveforms, or packed ``(buffer, starts, lengths)`` / ``(buffer, starts[, lengths])`` read where they
    lie.  Two library launches per resolution forward and two backward, whatever U is (csrc/stft_loss_rows.hip), plus the
    element-wise launches on [U] that join the resolutions (a copy, R - 1 adds, a divide; backward: a divide, a cast and the zero
    fill); deterministic; nothing is read back.  The gradient is exactly 0 where autograd through torch.stft has NaN or Inf: sr == hr, silence, clamped bins.  hr
    is a constant: a ground truth that requires grad raises NotImplementedError.  ValueError (naming utterance and resolution)
    for an utterance that cannot be reflected at a resolution, len <= n_fft / 2."""
    return _RowsLossRows.apply(*_rows_loss_operands(_MRSTFT, hrs, srs, resolutions, center))


def mrstft_loss(sr_audio, hr_audio, resolutions=STFT_RESOLUTIONS):
    """``mrstft_many`` of a dense batch as a training loss -> 0-dim float64 tensor, the mean over the clips, differentiable in
    sr_audio.  sr_audio / hr_audio: float32 device tensors [B, T], [B, 1, T] or [B, 1, 1, T], read in place (no packing copy).
    The tables of a geometry are uploaded once and kept, so forward + backward capture into a graph on one stream after one
    eager call (lsd_loss's note on live graphs from other streams applies)."""
    return _RowsLossRows.apply(*_rows_loss_dense(_MRSTFT, sr_audio, hr_audio, resolutions)).mean()


def mrstft_loss_term(sr_audio, hr_audio, scale, resolutions=STFT_RESOLUTIONS):
    """``scale * mrstft_loss(sr_audio, hr_audio, resolutions)`` as a term of the training step -> 0-dim float32 tensor,
    differentiable in sr_audio: mrstft_loss's operand forms, checks and cached tables, but one autograd node in the step's loss
    convention (functional._LossFn).  Forward is mg_stft_loss_rows per resolution plus one reduction launch; backward is
    mg_stft_loss_rows_backward_seeded per resolution, which forms every clip's upstream gradient in the kernel, in double, from the
    upstream scalar -- the GradScaler's loss scale in a --fp16 step stays on the device and is read when the kernel runs, so a
    captured step follows it -- and writes every sample, so no buffer is zero-filled.  Capturable after one eager call."""
    scale = _finite_scale(scale)
    return _RowsLossMean.apply(*_rows_loss_dense(_MRSTFT, sr_audio, hr_audio, resolutions), scale)


def mel_many(hrs, srs, sample_rate, resolutions=MEL_RESOLUTIONS, center=True, f_min=0.0, f_max=None):
    """The multi-scale mel-spectrogram L1 loss of every utterance on its own, differentiable in sr -> float64 device tensor [U].
    For one resolution (n_fft, hop, n_mels) -- periodic Hann window of n_fft samples, centred frames reflected at the utterance's
    own ends, K = n_fft / 2 + 1 bins, F_u frames, m = sqrt(max(re^2 + im^2, 1e-7)) as for ``mrstft_many``, W = mel_fbank(sample_rate,
    n_fft, n_mels, f_min, f_max) --
        E_j = sum_k W[j][k] m_k,   loss_u = sum_{f,j} |ln max(E_hr, 1e-5) - ln max(E_sr, 1e-5)| / (F_u n_mels)
    and the result is the mean over the resolutions.  Operand forms as for ``lsd_many``: lists of waveforms, or packed ``(buffer,
    starts, lengths)`` / ``(buffer, starts[, lengths])`` read where they lie.  Two library launches per resolution forward and two
    backward, whatever U is (csrc/mel_loss_rows.hip), plus the element-wise launches on [U] that join the resolutions;
    deterministic; nothing is read back.  The filterbanks and their band tables are built once per (sample_rate, n_fft, n_mels,
    f_min, f_max, device) and kept on the device.  The gradient is exactly 0 where autograd through torch.stft has NaN or Inf: sr ==
    hr, silence, clamped bins, filters under the floor.  hr is a constant: a ground truth that requires grad raises
    NotImplementedError.  ValueError (naming utterance and resolution) for an utterance that cannot be reflected at a resolution,
    len <= n_fft / 2, and (naming resolution and filter) for a filterbank with an empty filter."""
    return _RowsLossRows.apply(*_rows_loss_operands(_MEL, hrs, srs, resolutions, center, (sample_rate, f_min, f_max)))


def mel_loss(sr_audio, hr_audio, sample_rate, resolutions=MEL_RESOLUTIONS):
    """``mel_many`` of a dense batch as a training loss -> 0-dim float64 tensor, the mean over the clips, differentiable in
    sr_audio.  sr_audio / hr_audio: float32 device tensors [B, T], [B, 1, T] or [B, 1, 1, T], read in place (no packing copy).
    The tables of a geometry are uploaded once and kept, so forward + backward capture into a graph on one stream after one
    eager call (lsd_loss's note on live graphs from other streams applies)."""
    return _RowsLossRows.apply(*_rows_loss_dense(_MEL, sr_audio, hr_audio, resolutions, (sample_rate, 0.0, None))).mean()


def mel_loss_term(sr_audio, hr_audio, sample_rate, scale, resolutions=MEL_RESOLUTIONS):
    """``scale * mel_loss(sr_audio, hr_audio, sample_rate, resolutions)`` as a term of the training step -> 0-dim float32 tensor,
    differentiable in sr_audio: mel_loss's operand forms, checks and cached tables, but one autograd node in the step's loss
    convention (functional._LossFn).  Forward is mg_mel_loss_rows per resolution plus one reduction launch; backward is
    mg_mel_loss_rows_backward_seeded per resolution, which forms every clip's upstream gradient in the kernel from the upstream
    scalar -- in the arithmetic autograd performs for ``scale * mel_loss``, so a power-of-two scale gives that gradient bit for bit;
    the GradScaler's loss scale in a --fp16 step stays on the device and is read when the kernel runs, so a captured step follows
    it -- and writes every sample, so no buffer is zero-filled.  Capturable after one eager call."""
    scale = _finite_scale(scale)
    return _RowsLossMean.apply(*_rows_loss_dense(_MEL, sr_audio, hr_audio, resolutions, (sample_rate, 0.0, None)), scale)


def eval_model(model, eval_batches, opt, eval_path=None):
    """train.py:104-134: run ``model.inference`` over the evaluation batches (dicts with ``LR_audio`` / ``HR_audio`` like the
    reference's dataloader items, or ``(lr, hr)`` pairs), score every batch with ``compute_matrics`` and average -- the
    same five columns, appended to ``eval_path`` as a CSV row when given.  Everything up to the per-batch Python floats
    stays on the device; the model is put in eval mode for the loop (BatchNorm running statistics of the attention
    blocks) and back in train mode afterwards, like the reference."""
    import csv
    import numpy as np
    err, snr, snr_seg, pesq, lsd = [], [], [], [], []
    was_training = model.training
    dev = getattr(model, "device", "cuda")
    try:
        for j, item in enumerate(eval_batches):
            model.eval()
            lr_audio, hr_audio = (item["LR_audio"], item["HR_audio"]) if isinstance(item, dict) else item
            lr_audio, hr_audio = lr_audio.to(dev), hr_audio.to(dev)
            with torch.no_grad():
                _, sr_audio, _, _, _ = model.inference(lr_audio)
                _mse, _snr_sr, _snr_lr, _ssnr_sr, _ssnr_lr, _pesq, _lsd = compute_matrics(
                    hr_audio.squeeze(), lr_audio.squeeze(), sr_audio.squeeze(), opt)
            err.append(_mse)
            snr.append((_snr_lr, _snr_sr))
            snr_seg.append((_ssnr_lr, _ssnr_sr))
            pesq.append(_pesq)
            lsd.append(_lsd)
            if j >= opt.eval_size:
                break
    finally:
        model.train(was_training)
    result = {"err": float(np.mean(err)), "snr": float(np.mean(snr)), "snr_seg": float(np.mean(snr_seg)),
              "pesq": float(np.mean(pesq)), "lsd": float(np.mean(lsd))}
    if eval_path:
        with open(eval_path, "a") as f:
            writer = csv.DictWriter(f, fieldnames=result.keys())
            if f.tell() == 0:
                writer.writeheader()
            writer.writerow(result)
    return result
