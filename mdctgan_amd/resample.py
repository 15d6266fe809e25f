"""``torchaudio.functional.resample`` for the data path of the reference (data/audio_dataset.py:66-71, 171-177) on the
device: same signature and defaults (sinc_interp_hann, lowpass_filter_width=6, rolloff=0.99), the polyphase filter bank
built once per rate pair exactly as torchaudio's ``_get_sinc_resample_kernel`` does (float64, stored as float32), the
convolution as one HIP launch (``mg_resample``).  torchaudio itself is not a dependency.

Many utterances (``plan_front_end``, ``front_end_many``): AudioTestDataset.read_audio + post_processing (:141-186) for a whole
test set in shared launches.  Every utterance sits at an aligned start of one packed buffer per resampling step, device row
tables (``mg_resample_row``, ``mg_seg_row``) say where each row reads and writes, and the launch count -- one packing copy, one
table copy, the DC mean (``mg_rows_moments``), one ``mg_resample_rows`` per distinct rate pair and step, and under ``--add_noise``
two more moment passes and ``mg_add_noise_rows`` -- does not depend on the number of utterances.  Nothing is read back.  The final
buffer has ``packed.pack_waves``' layout, so ``generate_many``'s gather and decode tables apply to it unchanged.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import List

import numpy as np
import torch

from . import _lib
from .packed import (PackedLayout, add_noise_packed, add_noise_rows, aligned_layout, check_table, noise_buffer,  # noqa: F401
                     pack_waves, rows_moments, upload_tables, window_table)

_kernels = {}


def _sinc_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int, rolloff: float, device):
    key = (int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), str(device))
    hit = _kernels.get(key)
    if hit is not None:
        return hit
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base_freq = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base_freq)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1)[:, None, None] / new + idx          # int64 / int -> float32, then float64
    t = t * base_freq
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    scale = base_freq / orig
    kern = torch.where(t == 0, torch.tensor(1.0, dtype=t.dtype), t.sin() / t)
    kern = (kern * window * scale).to(torch.float32).reshape(new, 2 * width + orig).contiguous().to(device)
    _kernels[key] = (kern, width, orig, new)
    return _kernels[key]


def filter_bank(orig_freq: int, new_freq: int, device, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(kern [new, 2 * width + orig] float32 on `device`, width, orig, new) of one resampling step, on the gcd-reduced rates and
    cached for the life of the process; equal rates: the one-tap identity bank (ones [1, 1], 0, 1, 1), a copy."""
    if int(orig_freq) != int(new_freq):
        return _sinc_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff, device)
    key = ("identity", str(device))
    if key not in _kernels:
        _kernels[key] = (torch.ones(1, 1, dtype=torch.float32, device=device), 0, 1, 1)
    return _kernels[key]


def resample_length(length: int, orig_freq: int, new_freq: int) -> int:
    """mg_resample_length on the gcd-reduced rates, on the host: ceil(new * L / orig), the length aF.resample returns."""
    if int(length) <= 0 or int(orig_freq) <= 0 or int(new_freq) <= 0:
        raise ValueError("lengths and sampling rates must be positive")
    g = math.gcd(int(orig_freq), int(new_freq))
    return -(-(int(new_freq) // g) * int(length) // (int(orig_freq) // g))


def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6,
             rolloff: float = 0.99, resampling_method: str = "sinc_interp_hann") -> torch.Tensor:
    """waveform [..., L] (device) -> [..., ceil(new_freq * L / orig_freq)]."""
    if resampling_method != "sinc_interp_hann":
        raise NotImplementedError("resampling_method %r (the reference uses the default sinc_interp_hann)" % resampling_method)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("Original frequency and desired frequency should be positive")
    if int(orig_freq) == int(new_freq):
        return waveform
    lib = _lib.load()
    kern, width, orig, new = filter_bank(orig_freq, new_freq, waveform.device, lowpass_filter_width, rolloff)
    shape = waveform.shape
    x = _lib.f32c(waveform.reshape(-1, shape[-1]))
    n_out = lib.mg_resample_length(shape[-1], orig, new)
    out = torch.empty(x.shape[0], n_out, dtype=torch.float32, device=x.device)
    _lib.check(lib.mg_resample(_lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(kern), orig, new, width, _lib.ptr(out), n_out,
                               _lib.stream()), "mg_resample")
    return out.reshape(shape[:-1] + (n_out,))


def seg_pad_audio(waveform: torch.Tensor, segment_length: int) -> torch.Tensor:
    """AudioDataset.seg_pad_audio (data/audio_dataset.py:102-110) for a batch [B, L]: crop or zero pad to segment_length."""
    L = waveform.shape[-1]
    if L >= segment_length:
        return waveform[..., :segment_length]
    return torch.nn.functional.pad(waveform, (0, segment_length - L))


def make_training_pair(waveform: torch.Tensor, orig_sample_rate: int, hr_sampling_rate: int, lr_sampling_rate: int,
                       segment_length: int, add_noise: bool = False, snr: float = 55.0, noise=None, generator=None,
                       lowpass_sos=None):
    """AudioDataset.__getitem__ (data/audio_dataset.py:66-82): HR = resample to hr_rate; LR = resample to lr_rate and back up to
    hr_rate, plus the noise of :72-78 under add_noise (on the full resampled waveform, before the crop; see add_noise); both
    cropped / padded to segment_length.  [B, L] -> (lr, hr).  The random file offset of readaudio (:43-48) and whole batches cut
    from a corpus in HBM in shared launches: train_data.draw_windows / training_batch_many.
    lowpass_sos (not in the reference; [n <= 6, 6] second-order sections at orig_sample_rate, lowpass.lowpass_sos): the LR leg
    reads lowpass.lowpass_waveform(waveform, lowpass_sos), the zero-phase IIR low-pass of the waveform; HR is unchanged."""
    hr = resample(waveform, orig_sample_rate, hr_sampling_rate)
    src = waveform
    if lowpass_sos is not None:
        from .lowpass import lowpass_waveform
        src = lowpass_waveform(waveform, lowpass_sos)
    lr = resample(resample(src, orig_sample_rate, lr_sampling_rate), lr_sampling_rate, hr_sampling_rate)
    if add_noise:
        lr = add_noise_rows_of(lr, snr, segment_length, noise, generator, in_place=lr.data_ptr() != waveform.data_ptr())
    return seg_pad_audio(lr, segment_length), seg_pad_audio(hr, segment_length)


def make_test_segments(raw_audio: torch.Tensor, in_sampling_rate: int, hr_sampling_rate: int, lr_sampling_rate: int,
                       segment_length: int, gen_overlap: int = 0, is_lr_input: bool = False, add_noise: bool = False,
                       snr: float = 55.0, noise=None, generator=None):
    """AudioTestDataset (data/audio_dataset.py:141-186) for one waveform [1, L] in HBM: the DC shift of
    read_audio (``raw += 1e-4 - mean(raw)``), then the low-rate input of the model -- a file that already IS low-rate
    (``--is_lr_input``) is only brought up to hr_rate, anything else goes down to lr_rate and back up -- plus the noise of
    :178-184 under add_noise (see add_noise_rows_of), cut into segments
    by seg_pad_audio (generate_audio.segment_audio).  -> (lr_audio [1, L'], segments [n_seg, segment_length]).
    front_end_many does this for any number of waveforms in shared launches."""
    from .generate_audio import segment_audio
    raw = raw_audio.to(torch.float32)
    raw = raw + (1e-4 - raw.mean())
    if is_lr_input:
        lr_audio = resample(raw, in_sampling_rate, hr_sampling_rate)
    else:
        lr_audio = resample(resample(raw, in_sampling_rate, lr_sampling_rate), lr_sampling_rate, hr_sampling_rate)
    if add_noise:
        lr_audio = add_noise_rows_of(lr_audio, snr, segment_length, noise, generator, in_place=True)
    return lr_audio, segment_audio(lr_audio, segment_length, gen_overlap)


# ---------------------------------------------------------------------------------------------------------------------
# Row-table kernels: many utterances in shared launches
# ---------------------------------------------------------------------------------------------------------------------
def resample_rows(x: torch.Tensor, table: torch.Tensor, max_out_len: int, orig_freq: int, new_freq: int, out: torch.Tensor,
                  shift=None, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """mg_resample_rows: row u of `table` (int64 [n, 4] = in_pos, in_len, out_pos, out_len, on the device) reads its window of the
    packed float32 buffer `x` and writes resample()'s result for it into its window of `out`; shift [n] float32 enters row u's
    samples as x + shift[u].  Equal rates copy (a one-tap bank)."""
    lib = _lib.load()
    n = check_table(table, 4, "resample_rows").shape[0]
    if x.dtype != torch.float32 or out.dtype != torch.float32 or not x.is_contiguous() or not out.is_contiguous():
        raise ValueError("resample_rows: x and out are contiguous float32 buffers")
    if shift is not None and (shift.dtype != torch.float32 or shift.numel() != n or not shift.is_contiguous()):
        raise ValueError("resample_rows: shift is a contiguous float32 [%d] tensor" % n)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("Original frequency and desired frequency should be positive")
    kern, width, orig, new = filter_bank(orig_freq, new_freq, x.device, lowpass_filter_width, rolloff)
    _lib.check(lib.mg_resample_rows(_lib.ptr(x), x.numel(), _lib.ptr(table), n, int(max_out_len), _lib.ptr(shift), _lib.ptr(kern),
                                    orig, new, width, _lib.ptr(out), out.numel(), _lib.stream()), "mg_resample_rows")
    return out


def add_noise_rows_of(waveform: torch.Tensor, snr: float, segment_length: int, noise=None, generator=None,
                      in_place: bool = False) -> torch.Tensor:
    """data/audio_dataset.py:73-78 / :179-184 for every row of a [..., L] waveform on the device: ``noise = randn(size); noise -=
    noise.mean(); lr + sqrt(sum(lr^2) / segment_length / 10^(snr / 10)) / noise.std() * noise`` (mean, power and standard
    deviation per row, as the reference sees one file at a time).  noise: the caller's samples (same shape) instead of
    torch.randn(..., generator=generator) on the device -- the CPU stream of the reference cannot be matched there."""
    shape = waveform.shape
    L = int(shape[-1])
    if L < 2:
        raise ValueError("add_noise: a waveform of %d sample(s) has no standard deviation" % L)
    x = _lib.f32c(waveform.reshape(-1, L))
    if not in_place and x.data_ptr() == waveform.data_ptr():
        x = x.clone()
    B = x.shape[0]
    if noise is None:
        z = torch.randn(B, L, dtype=torch.float32, device=x.device, generator=generator)
    else:
        if noise.numel() != x.numel():
            raise ValueError("add_noise: noise has the waveform's shape %s (got %s)" % (tuple(shape), tuple(noise.shape)))
        z = noise.to(device=x.device, dtype=torch.float32).reshape(B, L).contiguous()
    table, = upload_tables([window_table(np.arange(B, dtype=np.int64) * L, [L] * B)], x.device)
    add_noise_packed(x.view(-1), table, L, snr, segment_length, z.view(-1))
    return x.reshape(shape)


@dataclass
class ResampleGroup:
    """The rows of one mg_resample_rows launch: utterances `index` (in table order) share the rate pair orig_freq -> new_freq."""
    orig_freq: int
    new_freq: int
    index: List[int]
    rows: np.ndarray            # int64 [n, 4] = in_pos, in_len, out_pos, out_len
    max_out_len: int


@dataclass
class FrontEndPlan:
    """plan_front_end's result.  `lengths[s]` / `starts[s]` / `totals[s]`: per-utterance lengths, aligned starts and the size of
    the packed buffer before step s (s = 0: the raw waveforms) and after the last one (s = len(steps): the low-rate input at
    hr_rate).  `steps[s]`: the ResampleGroups of step s, one per distinct rate pair.  `order`: the utterances in the order of the
    first step's groups -- the row order of the DC-mean table, so that every group's shifts are contiguous.  `utterances`:
    generate_audio.plan_utterances over the final lengths; its in_layout IS starts[-1] / lengths[-1] / totals[-1].  `raw`: None, or
    under front_end_many(keep_raw=True) a namespace of the packed raw buffer (`buffer`, float32 [totals[0]]; utterance u at
    starts[0][u], lengths[0][u] samples) and the DC shift per utterance (`shift`, float32 [U] on the device, in UTTERANCE order):
    raw + shift is read_audio's waveform, the ground truth of metrics.compute_matrics_many."""
    rates: List[int]
    lengths: List[List[int]]
    starts: List[List[int]]
    totals: List[int]
    steps: List[List[ResampleGroup]]
    order: List[int]
    utterances: object
    raw: object = None

    @property
    def final_lengths(self):
        return self.lengths[-1]

    @property
    def in_rows(self):
        return self.utterances.in_rows

    @property
    def out_rows(self):
        return self.utterances.out_rows

    @property
    def n_launches(self) -> int:
        """mg_resample_rows launches: one per distinct rate pair and step."""
        return sum(len(step) for step in self.steps)


def plan_front_end(lengths, rates, hr_rate: int, lr_rate: int, is_lr_input: bool, segment_length: int, gen_overlap: int,
                   batch_size: int, out_segment_length=None, align: int = 64) -> FrontEndPlan:
    """Where every utterance reads and writes in every step of AudioTestDataset.post_processing (host only: no device call).
    Utterance u of lengths[u] samples at rates[u] Hz goes to hr_rate (is_lr_input) or down to lr_rate and back up to hr_rate;
    each step's lengths are resample_length of the step before.  Every packed buffer has packed.aligned_layout's layout
    (starts rounded up to `align` samples), the last one exactly the one plan_utterances(final lengths, segment_length,
    out_segment_length (default: segment_length), gen_overlap, batch_size) describes."""
    from .generate_audio import plan_utterances
    lengths, rates = [int(n) for n in lengths], [int(r) for r in rates]
    if not lengths or len(lengths) != len(rates):
        raise ValueError("plan_front_end needs one sampling rate per utterance, and at least one utterance")
    if min(lengths) <= 0 or min(rates) <= 0 or int(hr_rate) <= 0 or int(lr_rate) <= 0:
        raise ValueError("lengths and sampling rates must be positive")
    targets = [int(hr_rate)] if is_lr_input else [int(lr_rate), int(hr_rate)]
    layouts, steps, now = [aligned_layout(lengths, align)], [], rates
    for target in targets:
        src_len, src_start = layouts[-1].lengths, layouts[-1].starts
        dst_len = [resample_length(n, r, target) for n, r in zip(src_len, now)]
        layouts.append(aligned_layout(dst_len, align))
        dst_start = layouts[-1].starts
        members = {}
        for u, r in enumerate(now):
            members.setdefault(r, []).append(u)
        steps.append([ResampleGroup(r, target, idx,
                                    np.asarray([(src_start[u], src_len[u], dst_start[u], dst_len[u]) for u in idx],
                                               dtype=np.int64).reshape(-1, 4), max(dst_len[u] for u in idx))
                      for r, idx in members.items()])
        now = [target] * len(lengths)
    L = int(segment_length)
    utt = plan_utterances(layouts[-1].lengths, L, L if out_segment_length is None else int(out_segment_length), gen_overlap,
                          batch_size, align)
    assert utt.in_layout == layouts[-1]                         # (both come from aligned_layout)
    return FrontEndPlan(rates, [p.lengths for p in layouts], [p.starts for p in layouts], [p.total for p in layouts], steps,
                        [u for g in steps[0] for u in g.index], utt)


def data_options(opt) -> dict:
    """lr_sampling_rate, hr_sampling_rate and segment_length are required; is_lr_input / add_noise default to off, snr to 55,
    gen_overlap to 0, batch_size to 64, out_segment_length to segment_length; lowpass_aug (a comma list of filter kinds, or a
    sequence of them; empty: off) with lowpass_order / lowpass_ripple / lowpass_cutoff becomes `lowpass`, a lowpass.LowpassSpec or
    None.  `opt`: an options namespace or a dict."""
    get = (lambda k, d=None: opt.get(k, d)) if isinstance(opt, dict) else (lambda k, d=None: getattr(opt, k, d))
    o = dict(lr_sampling_rate=get("lr_sampling_rate"), hr_sampling_rate=get("hr_sampling_rate"),
             segment_length=get("segment_length"), is_lr_input=bool(get("is_lr_input", False)),
             add_noise=bool(get("add_noise", False)), snr=float(get("snr", 55.0)), gen_overlap=int(get("gen_overlap", 0) or 0),
             batch_size=int(get("batch_size", 64) or 64), out_segment_length=get("out_segment_length"))
    for k in ("lr_sampling_rate", "hr_sampling_rate", "segment_length"):
        if o[k] is None:
            raise ValueError("front_end_many needs %s" % k)
    o["lowpass"] = None
    if get("lowpass_aug", ""):
        from .lowpass import spec_from_options
        o["lowpass"] = spec_from_options(get("lowpass_aug"), get("lowpass_order", (2, 10)), get("lowpass_ripple", (0.01, 1.0)),
                                         get("lowpass_cutoff", (0.9, 1.0)))
    return o


def _prepacked(raws):
    """front_end_many's `raws` when they are packed already -- a wavio.WavPack (anything with buffer / starts / lengths) or a
    (buffer, starts, lengths) triple -> (float32 device buffer, starts, lengths); None for a list of waveforms."""
    if all(hasattr(raws, a) for a in ("buffer", "starts", "lengths")):
        raws = (raws.buffer, raws.starts, raws.lengths)
    elif not (isinstance(raws, tuple) and len(raws) == 3 and torch.is_tensor(raws[0]) and not torch.is_tensor(raws[1])):
        return None
    buf, starts, lengths = raws
    if buf.dtype != torch.float32 or not buf.is_cuda or not buf.is_contiguous() or buf.dim() != 1:
        raise ValueError("front_end_many: a packed raw buffer is a contiguous float32 [total] device tensor")
    return buf, [int(s) for s in starts], [int(n) for n in lengths]


def front_end_many(raws, rates, opt_or_kwargs, noise=None, generator=None, device=None, keep_raw=False, raw_moments=None):
    """AudioTestDataset.read_audio + post_processing (data/audio_dataset.py:141-186) for a list of raw waveforms ([T_u] or
    [1, T_u], on the host or the device) at sampling rates `rates` -> (packed, views, plan): the packed low-rate buffer at
    hr_sampling_rate (float32 [plan.totals[-1]], packed.pack_waves' layout, zeros in the gaps), one [1, T'_u] view of it
    per utterance, and the FrontEndPlan (plan.utterances: the UtterancePlan generate_many's tables come from).
    opt_or_kwargs: an options namespace or a dict (see data_options).  Under add_noise, `noise` is a list of per-utterance
    waveforms of the final lengths (for tests: the reference draws from the CPU stream, which a device cannot reproduce);
    otherwise torch.randn(..., generator=generator) on the device.
    Launches: one packing copy, one table copy, mg_rows_moments, a handful of element-wise launches over [U] for the shift, one
    mg_resample_rows per distinct rate pair and step, and under add_noise two more mg_rows_moments and mg_add_noise_rows --
    whatever the number of utterances.  No host read-back.
    keep_raw: plan.raw keeps the packed raw buffer and the shift in utterance order (see FrontEndPlan; one more element-wise launch
    when the rates differ); nothing else changes.
    raws may also be packed already: a wavio.WavPack (rates=None: its own) or a (buffer, starts, lengths) triple over a float32
    device buffer in packed.aligned_layout's layout -- then there is no packing copy, the buffer is read where it is.
    raw_moments: float64 [U, 2] on the device, {sum x, sum x^2} of every raw waveform in UTTERANCE order with packed.rows_moments'
    bits (wavio.read_wav_many(with_moments=True) has them from its decode pass) -- in place of the mg_rows_moments launch.  With a
    list of waveforms and no raw_moments the launches are what they were."""
    o = data_options(opt_or_kwargs)
    prepacked = _prepacked(raws)
    if prepacked is not None:
        raw_buf, raw_starts, lengths = prepacked
        if rates is None:
            rates = getattr(raws, "rates", None)
        raws = []
    else:
        raws = list(raws)
        lengths = [w.numel() for w in raws]
    if len(lengths) == 0:
        raise ValueError("no waveforms")
    if min(lengths) == 0:
        raise ValueError("an empty waveform cannot be resampled")
    plan = plan_front_end(lengths, rates, o["hr_sampling_rate"], o["lr_sampling_rate"], o["is_lr_input"],
                          o["segment_length"], o["gen_overlap"], o["batch_size"], o["out_segment_length"])
    if prepacked is not None:
        if raw_starts != plan.starts[0] or raw_buf.numel() < plan.totals[0]:
            raise ValueError("front_end_many: a packed raw buffer has packed.aligned_layout's layout over its lengths")
        if device is None:
            device = raw_buf.device
        want = torch.device(device)
        if want.type != "cuda" or (want.index is not None and want.index != raw_buf.device.index):
            raise ValueError("front_end_many: the packed raw buffer is on %s, not on %s" % (raw_buf.device, device))
        device = raw_buf.device
    U = len(lengths)
    if raw_moments is not None and (raw_moments.dtype != torch.float64 or tuple(raw_moments.shape) != (U, 2)
                                    or not raw_moments.is_cuda):
        raise ValueError("front_end_many: raw_moments is a float64 [%d, 2] device tensor, one row per utterance" % U)
    final = plan.final_lengths
    if o["add_noise"]:
        if min(final) < 2:
            raise ValueError("add_noise: an utterance of fewer than 2 samples has no standard deviation")
        if noise is not None and [z.numel() for z in noise] != final:
            raise ValueError("add_noise: noise holds one waveform per utterance, of the lengths %s" % final)
    if device is None:
        device = next((w.device for w in raws if w.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())

    # every table in one copy: the raw windows in group order, the final windows, each group's rows, then where utterance u sits in
    # plan.order
    shuffled = plan.order != list(range(U))
    reorder = keep_raw and shuffled
    pick = raw_moments is not None and shuffled                     # (the moments arrive in utterance order)
    raw_win, lr_win, *group_rows = upload_tables(
        [window_table(plan.starts[0], plan.lengths[0], plan.order), window_table(plan.starts[-1], final)]
        + [g.rows for step in plan.steps for g in step]
        + ([np.argsort(np.asarray(plan.order, dtype=np.int64), kind="stable")] if reorder else [])
        + ([np.asarray(plan.order, dtype=np.int64)] if pick else []), device)
    order_t = group_rows.pop() if pick else None
    place = group_rows.pop() if reorder else None

    if prepacked is not None:
        buf = raw_buf[:plan.totals[0]]
    else:
        buf = pack_waves(raws, PackedLayout(plan.starts[0], plan.lengths[0], plan.totals[0]), device)
    if raw_moments is not None:
        mom = raw_moments[order_t] if pick else raw_moments
    else:
        mom = rows_moments(buf, raw_win, max(plan.lengths[0]))
    shift = (1e-4 - mom[:, 0] / (raw_win[:, 2] - raw_win[:, 1]).double()).float()     # raw += 1e-4 - mean(raw), per utterance
    if keep_raw:
        plan.raw = SimpleNamespace(buffer=buf, shift=shift[place].contiguous() if reorder else shift,
                                   starts=plan.starts[0], lengths=plan.lengths[0])
    tables = iter(group_rows)
    for s, step in enumerate(plan.steps):
        out = torch.zeros(plan.totals[s + 1], dtype=torch.float32, device=device)
        row = 0
        for g in step:
            n = len(g.index)
            resample_rows(buf, next(tables), g.max_out_len, g.orig_freq, g.new_freq, out,
                          shift=shift[row:row + n] if s == 0 else None)
            row += n
        buf = out
    if o["add_noise"]:
        z = noise_buffer(noise, plan.utterances.in_layout, device, generator)
        add_noise_packed(buf, lr_win, max(final), o["snr"], o["segment_length"], z)
    return buf, [buf[s0:s0 + n].view(1, -1) for s0, n in zip(plan.starts[-1], final)], plan
