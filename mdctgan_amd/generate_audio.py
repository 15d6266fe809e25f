"""Whole-utterance inference: the device-side part of generate_audio.py:22-53.

The reference script walks the dataset loader, calls ``model.inference`` per batch, copies every ``sr_audio`` to the
host and concatenates (or cross-fades with ``F.fold`` when ``--gen_overlap > 0``).  Here the waveform is built in HBM by
the decoder itself: batches of low-rate segments go through ``model.inference`` and K2's overlap-add store writes each
segment at its place in the stitched waveform, cross-fade included (``mg_imdct4_stitched``, ``mg_imdct4_pow2_stitched`` at
n_fft 256 / 1024 / 2048); codec geometries neither covers decode per batch and one gather kernel (``mg_stitch_segments``) stitches.  Dataset loading, resampling and the
metrics of ``util.compute_matrics`` are outside the hot path.

Many short utterances (``generate_many``, ``make_graphed_generate_many``): the segments of any number of waveforms share the
generator's batches.  Every waveform sits at an aligned start of one packed input buffer and one packed output buffer, and two
device row tables (``mg_seg_row``: position, window) say where each batch row reads and writes: one gather launch per batch cuts
the segments (``mg_segments_gather``), and the row-table decode (``mg_imdct4_stitched_rows``, ``mg_imdct4_pow2_stitched_rows``)
stitches every utterance in its own window.  The launch topology does not depend on the mix of lengths, so one captured graph
serves them all.  ``super_resolve_many`` starts one step earlier, from raw files at their own sampling rates: the packed
front end of ``resample.front_end_many`` leaves the packed input buffer that these batches read.  ``super_resolve_files``,
``evaluate_files`` and the command line (``python -m mdctgan_amd.generate_audio``) start and end at WAV files: ``wavio`` decodes
all of them in one launch in front of that, and encodes all outputs in one launch behind it.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from . import _lib
from . import functional as Fh
from . import ops
from .packed import PackedLayout, aligned_layout, pack_waves


def segment_audio(audio: torch.Tensor, segment_length: int, gen_overlap: int = 0) -> torch.Tensor:
    """AudioTestDataset.seg_pad_audio (data/audio_dataset.py:153-167): [T] or [1, T] waveform -> [n_seg, segment_length].
    A waveform of at least one segment is zero padded by ``gen_overlap`` in front and up to ``ceil(T / L) * L +
    gen_overlap`` behind, then unfolded at stride ``L - gen_overlap``; a shorter one is padded to a single segment."""
    x = audio.reshape(-1)
    length = x.numel()
    if gen_overlap < 0 or gen_overlap >= segment_length:
        raise ValueError("gen_overlap must be in [0, segment_length)")
    if length >= segment_length:
        num_segments = -(-length // segment_length)
        x = torch.nn.functional.pad(x, (gen_overlap, segment_length * num_segments - length + gen_overlap))
        return x.unfold(0, segment_length, segment_length - gen_overlap).contiguous()
    return torch.nn.functional.pad(x, (0, segment_length - length)).unsqueeze(0)


def generate(model, lr_segments: torch.Tensor, batch_size: int = 64, gen_overlap: int = 0) -> torch.Tensor:
    """lr_segments [n_seg, T] (device) -> stitched super-resolved waveform [1, total] (generate_audio.py:28-53)."""
    if lr_segments.dim() != 2:
        raise ValueError("lr_segments must be [n_seg, T]")
    outs = []
    # A codec geometry with a stitched decoder (K2 at n_fft 512, K2' at 256 / 1024 / 2048): the overlap-add store writes every
    # batch's segments straight into the stitched waveform
    # (mg_imdct4_stitched: the halving, F.fold and the crop of generate_audio.py:43-50 -- or the torch.cat of :52 -- happen in
    # the store; no list of segments, no concatenation, no stitching launch).  Other geometries decode per batch and stitch after.
    pre = model.preprocess
    fused = bool(getattr(pre, "has_stitched_decoder", False)) and os.environ.get("MG_NO_STITCHED_K2") != "1"
    out = None
    if fused:
        n_seg, T = lr_segments.shape
        seg_len = (_lib.load().mg_mdct4_num_frames(T, pre.n_fft) - 1) * (pre.n_fft // 2)
        total = _lib.load().mg_stitch_length(n_seg, seg_len, gen_overlap)
        if total <= 0:
            raise ValueError("invalid stitching geometry: n_seg=%d segment_length=%d gen_overlap=%d" % (n_seg, seg_len, gen_overlap))
        out = torch.empty(total, dtype=torch.float32, device=lr_segments.device)
    # generate_audio.py:27 calls model.eval() first: the BatchNorm2d layers of the bottleneck-attention blocks must use
    # their running statistics (and must not update them) during inference
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for i in range(0, lr_segments.shape[0], batch_size):
                if fused:
                    model.inference(lr_segments[i:i + batch_size], stitch=(out, gen_overlap, i, seg_len))
                else:
                    _, sr_audio, _, _, _ = model.inference(lr_segments[i:i + batch_size])
                    outs.append(sr_audio)
    finally:
        model.train(was_training)
    if fused:
        return out.view(1, -1)
    audio = torch.cat(outs, dim=0)                      # [n_seg, 1, 1, T]
    return ops.stitch_segments(audio, audio.shape[-1], gen_overlap)


def make_graphed_generate(model, lr_segments: torch.Tensor, batch_size: int = 64, gen_overlap: int = 0, warmup: int = 2):
    """Capture generate() for a fixed segment count into one hipGraph (K1, ~120 generator launches and the stitching K2
    per batch) and return run(lr_segments) -> stitched waveform (a buffer that the next replay overwrites).  The
    generator weights must not change between capture and replay without re-capturing: the Winograd layers read the
    transformed-weight images cached by the warm-up calls."""
    static_in = lr_segments.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(warmup, 1)):
            generate(model, static_in, batch_size, gen_overlap)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = generate(model, static_in, batch_size, gen_overlap)

    # The captured launches hold raw pointers to the transformed-weight images the warm-up cached on the parameters
    # (weight._mg_u_cache).  Pin those tensors for the graph's lifetime -- an eager inference after an optimiser step
    # would replace the cache entries and free them -- and refuse to replay once the weights have moved.
    params = list(model.netG.parameters())
    pinned = [getattr(p, "_mg_u_cache", None) for p in params]
    stamp = (Fh.WEIGHT_EPOCH[0], tuple(p._version for p in params), tuple(p.data_ptr() for p in params))

    def run(lr=None):
        now = (Fh.WEIGHT_EPOCH[0], tuple(p._version for p in params), tuple(p.data_ptr() for p in params))
        if now != stamp:
            raise RuntimeError("the generator's weights changed after make_graphed_generate() captured them "
                               "(optimizer step / load_state_dict): capture again")
        if lr is not None:
            static_in.copy_(lr, non_blocking=True)
        graph.replay()
        return out
    run.graph, run.pinned = graph, pinned
    return run


# ---------------------------------------------------------------------------------------------------------------------
# Many utterances of different lengths in shared batches
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class UtterancePlan:
    """plan_utterances' result.  Per utterance: `segments` (segment_audio's count), `in_start` / `out_start` (first sample in the
    packed input / output buffer) and `out_length` (mg_stitch_length of its segments).  `in_rows` / `out_rows`: the mg_seg_row
    tables (int64 [n_rows, 3] = pos, lo, hi) in batch order -- utterance after utterance, segment after segment, then the dead
    rows (lo == hi) that fill the last batch.  `in_total` / `out_total`: samples of the packed buffers."""
    segment_length: int
    out_segment_length: int
    gen_overlap: int
    batch_size: int
    lengths: List[int]
    segments: List[int]
    in_start: List[int]
    out_start: List[int]
    out_length: List[int]
    in_rows: np.ndarray
    out_rows: np.ndarray
    in_total: int
    out_total: int
    n_live: int

    @property
    def in_layout(self) -> PackedLayout:
        """The packed input buffer, as packed.pack_waves lays it out."""
        return PackedLayout(self.in_start, self.lengths, self.in_total)

    @property
    def n_batches(self) -> int:
        return self.in_rows.shape[0] // self.batch_size

    @property
    def live_fraction(self) -> float:
        return self.n_live / float(self.in_rows.shape[0])


def stitch_length(n_seg: int, seg_len: int, overlap: int) -> int:
    """mg_stitch_length on the host (generate_audio.py:40-53: concatenation, or fold at stride seg_len - overlap and the crop)."""
    if n_seg <= 0 or seg_len <= 0 or overlap < 0 or 2 * overlap >= seg_len:
        return -1
    return n_seg * seg_len if overlap == 0 else (n_seg - 1) * (seg_len - overlap) + seg_len - 2 * overlap


def plan_utterances(lengths, segment_length: int, out_segment_length: int, gen_overlap: int, batch_size: int,
                    align: int = 64) -> UtterancePlan:
    """Where every segment of every utterance reads and writes (host only: no device call).

    An utterance of `length` samples has segment_audio's segments: ceil(length / L) * L samples plus gen_overlap zeros on both
    sides, cut at stride L - gen_overlap (segment k starts at k (L - gen_overlap) - gen_overlap of the waveform), or the single
    segment [0, L) when it is shorter than L.  Its stitched output has mg_stitch_length(segments, out_segment_length, gen_overlap)
    samples; segment k starts at k (L_out - gen_overlap) - gen_overlap of it.  Starts in both packed buffers are rounded up to
    `align` samples, so a row's position keeps the alignment it has for a single utterance (the 16-byte paths of the kernels)."""
    L, Lo, ov, bs = int(segment_length), int(out_segment_length), int(gen_overlap), int(batch_size)
    lengths = [int(n) for n in lengths]
    if L <= 0 or Lo <= 0 or bs <= 0 or align <= 0:
        raise ValueError("segment_length, out_segment_length, batch_size and align must be positive")
    if ov < 0 or ov >= L or 2 * ov >= Lo:
        raise ValueError("gen_overlap must be in [0, segment_length) and below half a decoded segment")
    if not lengths or min(lengths) <= 0:
        raise ValueError("plan_utterances needs at least one utterance, each of at least one sample")
    segments, out_length = [], []
    for n in lengths:
        n_seg = (-(-n // L) * L + 2 * ov - L) // (L - ov) + 1 if n >= L else 1
        segments.append(n_seg)
        out_length.append(stitch_length(n_seg, Lo, ov))
    ins, outs = aligned_layout(lengths, align), aligned_layout(out_length, align)
    in_rows, out_rows = [], []
    for n, n_seg, total, in_pos, out_pos in zip(lengths, segments, out_length, ins.starts, outs.starts):
        front = ov if n >= L else 0             # (the short waveform is padded behind only)
        for k in range(n_seg):
            in_rows.append((in_pos + k * (L - ov) - front, in_pos, in_pos + n))
            out_rows.append((out_pos + k * (Lo - ov) - ov, out_pos, out_pos + total))
    n_live = len(in_rows)
    dead = -n_live % bs
    in_rows += [(0, 0, 0)] * dead
    out_rows += [(0, 0, 0)] * dead
    return UtterancePlan(L, Lo, ov, bs, lengths, segments, ins.starts, outs.starts, out_length,
                         np.asarray(in_rows, dtype=np.int64).reshape(-1, 3), np.asarray(out_rows, dtype=np.int64).reshape(-1, 3),
                         ins.total, outs.total, n_live)


def check_capacity(plan: UtterancePlan, max_segments: int, max_samples: int) -> None:
    """What make_graphed_generate_many's run() asks before it copies anything: the mix fits the captured batches
    (ceil(max_segments / batch_size) of them) and its waveforms the packed input buffer (max_samples in all)."""
    cap = -(-int(max_segments) // plan.batch_size)
    if plan.n_batches > cap:
        raise ValueError("%d segments (%d batches of %d) do not fit the %d captured batches (max_segments=%d)"
                         % (plan.n_live, plan.n_batches, plan.batch_size, cap, max_segments))
    if sum(plan.lengths) > int(max_samples):
        raise ValueError("%d samples do not fit the packed input buffer (max_samples=%d)" % (sum(plan.lengths), max_samples))


def _decoded_segment_length(pre, segment_length: int) -> int:
    hop = pre.n_fft // 2
    return -(-segment_length // hop) * hop          # (mg_mdct4_num_frames(T, n_fft) - 1) * hop


def _fused_many(model) -> bool:
    return bool(getattr(model.preprocess, "has_stitched_decoder", False)) and os.environ.get("MG_NO_STITCHED_K2") != "1"


def _plan_for(model, waves, batch_size, gen_overlap, segment_length):
    if len(waves) == 0:
        raise ValueError("no waveforms")
    L = int(segment_length if segment_length is not None else model.opt.segment_length)
    if any(w.numel() == 0 for w in waves):
        raise ValueError("an empty waveform has no segments")
    return plan_utterances([w.numel() for w in waves], L, _decoded_segment_length(model.preprocess, L), gen_overlap, batch_size)


def _views(out, plan: UtterancePlan):
    return [out[s:s + n].view(1, -1) for s, n in zip(plan.out_start, plan.out_length)]


def _run_packed(model, packed, plan: UtterancePlan, pad_batches: bool = False, with_buffer: bool = False):
    """generate_many's batches over a packed input buffer and its plan: per batch one gather launch, model.inference and the
    row-table decode -> list of stitched waveforms [1, total_u].  with_buffer: -> (list, packed output buffer of which the
    waveforms are views at plan.out_start, or None without a stitched decoder)."""
    from .mdct import seg_row_table, segments_gather
    dev = packed.device
    gen_overlap = plan.gen_overlap
    tables = seg_row_table(np.stack([plan.in_rows, plan.out_rows]), dev).view(2, -1, 3)
    fused = _fused_many(model)
    # (zeros: the cross-fade zones are added into the buffer, and the alignment gaps between utterances are never written)
    out = torch.zeros(plan.out_total, dtype=torch.float32, device=dev) if fused else None
    outs = []
    bs = plan.batch_size
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for r0 in range(0, plan.n_live, bs):
                nb = bs if pad_batches else min(bs, plan.n_live - r0)
                segs = segments_gather(packed, tables[0, r0:r0 + nb], plan.segment_length)
                if fused:
                    model.inference(segs, rows=(out, gen_overlap, tables[1, r0:r0 + nb], plan.out_segment_length, False))
                else:
                    outs.append(model.inference(segs)[1][:min(bs, plan.n_live - r0)])
    finally:
        model.train(was_training)
    if fused:
        return (_views(out, plan), out) if with_buffer else _views(out, plan)
    audio = torch.cat(outs, dim=0)                      # [n_live, 1, 1, T]
    first = np.concatenate([[0], np.cumsum(plan.segments)])
    waves = [ops.stitch_segments(audio[first[u]:first[u + 1]], audio.shape[-1], gen_overlap) for u in range(len(plan.lengths))]
    return (waves, None) if with_buffer else waves


def generate_many(model, waves, batch_size: int = 64, gen_overlap: int = 0, pad_batches: bool = False, segment_length=None):
    """Whole-utterance inference over a list of low-rate waveforms ([T_u] or [1, T_u]) of any lengths, their segments sharing the
    generator's batches -> list of stitched super-resolved waveforms [1, total_u] (views of one packed buffer), each what
    generate(model, segment_audio(wave_u, ...), ...) stitches from the same generator outputs.  Per batch: one gather launch
    (mg_segments_gather), model.inference, and its row-table decode that writes every utterance's window of the packed output.
    pad_batches: every batch runs at the full batch_size (dead rows are zero segments and write nothing); otherwise the last batch
    runs at its live size.  Codec geometries without a stitched decoder (or MG_NO_STITCHED_K2=1) decode per batch and stitch every
    utterance with ops.stitch_segments.  segment_length: the model's --segment_length by default.
    The factored n_fft-512 decode addresses its output with 32 bits: a packed output of 2^30 - 2^14 samples or more (about six
    hours at 48 kHz; plan.out_total) still decodes correctly, but on the slower generic kernel (mg_mdct_last_kernel(1) names it)
    -- split a larger corpus into several calls."""
    plan = _plan_for(model, waves, batch_size, gen_overlap, segment_length)
    dev = next(model.netG.parameters()).device
    return _run_packed(model, pack_waves(waves, plan.in_layout, dev), plan, pad_batches)


def super_resolve_many(model, raws, rates, batch_size: int = 64, gen_overlap=None, noise=None, generator=None,
                       raw_moments=None):
    """From raw files to super-resolved waveforms for a whole test set: resample.front_end_many (AudioTestDataset.read_audio +
    post_processing, data/audio_dataset.py:141-186, for all utterances in shared launches) followed by generate_many's batches
    over the packed buffer it leaves -- no per-utterance launch, no repacking.  raws: waveforms [T_u] or [1, T_u] (host or device)
    at sampling rates `rates`.  lr_sampling_rate, hr_sampling_rate, is_lr_input, add_noise, snr, segment_length and (unless given)
    gen_overlap come from model.opt.  noise / generator: see front_end_many.  -> list of stitched waveforms [1, total_u], views
    of one packed buffer, bit for bit generate_many(model, front_end_many(...)'s views).  raws may be packed already (a
    wavio.WavPack or a triple) and raw_moments given: see front_end_many."""
    from .resample import front_end_many
    dev = next(model.netG.parameters()).device
    packed, _, plan = front_end_many(raws, rates, _front_end_kwargs(model, batch_size, gen_overlap), noise=noise,
                                     generator=generator, device=dev, raw_moments=raw_moments)
    return _run_packed(model, packed, plan.utterances)


def _front_end_kwargs(model, batch_size, gen_overlap) -> dict:
    opt = model.opt
    L = int(opt.segment_length)
    ov = int(getattr(opt, "gen_overlap", 0) or 0) if gen_overlap is None else int(gen_overlap)
    return dict(lr_sampling_rate=opt.lr_sampling_rate, hr_sampling_rate=opt.hr_sampling_rate,
                is_lr_input=bool(getattr(opt, "is_lr_input", False)), add_noise=bool(getattr(opt, "add_noise", False)),
                snr=float(getattr(opt, "snr", 55.0)), segment_length=L, gen_overlap=ov, batch_size=batch_size,
                out_segment_length=_decoded_segment_length(model.preprocess, L))


def evaluate_many(model, raws, rates, batch_size: int = 64, gen_overlap=None, noise=None, generator=None, metric_path=None,
                  raw_moments=None):
    """generate_audio.py:22-88 for a whole test set of files at hr_sampling_rate: super_resolve_many, then every utterance scored
    against its own ground truth by metrics.compute_matrics_many -- front end, generator batches and metrics over the same packed
    buffers, the host never waiting.  The ground truth is read_audio's waveform, the packed raw buffer plus the per-utterance DC
    shift (added inside the metric kernels, never materialised); the low-rate and the stitched waveform are cropped to its length
    (`lr_audio[..., :audio_len]`, :58-59).  Every rates[u] must be opt.hr_sampling_rate (ValueError): the reference compares
    raw_audio with the model's output sample by sample, which means something only then.
    -> (waveforms, scores): super_resolve_many's list, and a float64 device tensor [U, 7] = (mse, snr_sr, snr_lr, 0, 0, 0, lsd) per
    utterance.  metric_path: one `MSE,SNR_SR,LSD` line per utterance is appended (:86-88) -- the only read-back, after everything
    is queued.  raws may be packed already and raw_moments given: see front_end_many."""
    from .metrics import compute_matrics_many
    from .resample import front_end_many
    opt = model.opt
    rates = [int(r) for r in rates]
    for u, r in enumerate(rates):
        if r != int(opt.hr_sampling_rate):
            raise ValueError("utterance %d: %d Hz is not hr_sampling_rate (%d Hz): it cannot be scored against its own file"
                             % (u, r, int(opt.hr_sampling_rate)))
    dev = next(model.netG.parameters()).device
    packed, _, plan = front_end_many(raws, rates, _front_end_kwargs(model, batch_size, gen_overlap), noise=noise,
                                     generator=generator, device=dev, keep_raw=True, raw_moments=raw_moments)
    utt = plan.utterances
    waves, out = _run_packed(model, packed, utt, with_buffer=True)
    srs = (out, utt.out_start, utt.out_length) if out is not None else waves
    scores = compute_matrics_many((plan.raw.buffer, plan.raw.starts, plan.raw.lengths), (packed, utt.in_start, utt.lengths), srs,
                                  opt, hr_shift=plan.raw.shift)
    if metric_path:
        with open(metric_path, "a") as f:
            for mse, snr_sr, _, _, _, _, lsd in scores.tolist():
                f.write("%f,%f,%f\n" % (mse, snr_sr, lsd))
    return waves, scores


def make_graphed_generate_many(model, max_segments: int, max_samples: int, batch_size: int = 64, gen_overlap: int = 0,
                               warmup: int = 2, segment_length=None):
    """Capture generate_many(pad_batches=True) for ANY mix of utterances of at most max_segments segments and max_samples samples
    in all into one hipGraph -- ceil(max_segments / batch_size) iterations of gather, generator and row-table decode in one linear
    chain, over static packed buffers and static row tables -- and return run(waves) -> list of [1, total_u] views of the static
    output (the next replay overwrites them; run.last keeps the latest list).  run copies the packed samples and the new tables and replays; batches past the mix
    run on dead rows.  A mix that does not fit raises ValueError before anything is copied.  The weights must not change between
    capture and replay (see make_graphed_generate: the guard and the pinned Winograd images are the same)."""
    from .mdct import seg_row_table, segments_gather
    pre = model.preprocess
    if not _fused_many(model):
        raise NotImplementedError("make_graphed_generate_many needs a codec geometry with a stitched decoder")
    L = int(segment_length if segment_length is not None else model.opt.segment_length)
    Lo, bs, align = _decoded_segment_length(pre, L), int(batch_size), 64
    plan_utterances([L], L, Lo, gen_overlap, bs, align)                 # (validates the geometry)
    n_batches = -(-int(max_segments) // bs)
    if n_batches <= 0 or max_samples <= 0:
        raise ValueError("max_segments and max_samples must be positive")
    n_rows = n_batches * bs
    dev = next(model.netG.parameters()).device
    # every utterance has at least one segment and wastes less than `align` samples in front of the next start
    static_in = torch.zeros(int(max_samples) + n_rows * align, dtype=torch.float32, device=dev)
    static_out = torch.zeros(n_rows * (Lo + align), dtype=torch.float32, device=dev)
    static_rows = torch.zeros(2, n_rows, 3, dtype=torch.int64, device=dev)          # all dead
    static_segs = torch.empty(bs, L, dtype=torch.float32, device=dev)

    def body():
        for b in range(n_batches):
            segments_gather(static_in, static_rows[0, b * bs:(b + 1) * bs], L, out=static_segs)
            # (the first batch clears the whole output when the cross-fade zones are added into it)
            model.inference(static_segs, rows=(static_out, gen_overlap, static_rows[1, b * bs:(b + 1) * bs], Lo,
                                               b == 0 and gen_overlap > 0))

    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(max(warmup, 1)):
                    body()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                body()
    finally:
        model.train(was_training)

    # as in make_graphed_generate: pin the transformed-weight images the captured launches point at, refuse to replay once the
    # weights have moved
    params = list(model.netG.parameters())
    pinned = [getattr(p, "_mg_u_cache", None) for p in params]
    stamp = (Fh.WEIGHT_EPOCH[0], tuple(p._version for p in params), tuple(p.data_ptr() for p in params))

    def run(waves):
        now = (Fh.WEIGHT_EPOCH[0], tuple(p._version for p in params), tuple(p.data_ptr() for p in params))
        if now != stamp:
            raise RuntimeError("the generator's weights changed after make_graphed_generate_many() captured them "
                               "(optimizer step / load_state_dict): capture again")
        plan = _plan_for(model, waves, bs, gen_overlap, L)
        check_capacity(plan, max_segments, max_samples)
        rows = np.zeros((2, n_rows, 3), dtype=np.int64)
        rows[0, :plan.in_rows.shape[0]], rows[1, :plan.out_rows.shape[0]] = plan.in_rows, plan.out_rows
        pack_waves(waves, plan.in_layout, dev, out=static_in)
        static_rows.copy_(seg_row_table(rows).view(2, n_rows, 3), non_blocking=True)
        graph.replay()
        run.last = _views(static_out, plan)
        return run.last
    run.graph, run.pinned, run.last = graph, pinned, None
    return run


# ---------------------------------------------------------------------------------------------------------------------
# Files in, files out
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class FilesResult:
    """super_resolve_files' result.  `waves[r]`: the super-resolved waveform [1, T'_r] of row r of `pack` (wavio.WavPack: channel
    pack.channel[r] of pack.paths[pack.file[r]]), cropped to the row's final front-end length.  `out_paths[f]`: the file written
    for input f (None without out_dir).  `clipped[r]`: the samples of row r that the encoder clamped or found NaN (None without
    out_dir)."""
    waves: list
    pack: object
    out_paths: object = None
    clipped: object = None


def _output_paths(paths, out_dir):
    stems = [os.path.splitext(os.path.basename(os.fspath(p)))[0] for p in paths]
    seen = {}
    for p, s in zip(paths, stems):
        if s in seen:
            raise ValueError("%s and %s would both be written to %s.wav" % (seen[s], p, s))
        seen[s] = p
    return [os.path.join(os.fspath(out_dir), s + ".wav") for s in stems]


def _write_cropped(out_paths, waves, out, utt, lengths, groups, rate, encoding):
    """wavio.write_wav_many over the stitched waveforms cropped to `lengths`: straight from the packed output buffer when the
    decoder left one."""
    from .wavio import write_wav_many
    os.makedirs(os.path.dirname(out_paths[0]) or ".", exist_ok=True)
    rows = (out, utt.out_start, lengths) if out is not None else [w[..., :n] for w, n in zip(waves, lengths)]
    return write_wav_many(out_paths, rows, rate, encoding, groups)


def super_resolve_files(model, paths, out_dir=None, channels: str = "all", encoding: str = "PCM_F32", batch_size: int = 64,
                        gen_overlap=None, noise=None, generator=None) -> FilesResult:
    """From WAV files to WAV files: wavio.read_wav_many (one decode launch, the DC moments from the same pass), super_resolve_many's
    front end and generator batches over the packed buffer it leaves, and wavio.write_wav_many (one encode launch) -- no
    per-file launch anywhere.  channels "all": every channel of a file is a row of its own and all of them end up in ONE output
    file; "first": channel 0 only (what the reference's datasets keep).  Every output is cropped to the row's final front-end
    length (its length at hr_sampling_rate) and written to <out_dir>/<stem>.wav at hr_sampling_rate as `encoding` ("PCM_F32",
    "PCM_S16", "PCM_S24": see write_wav_many); two inputs with one stem are a ValueError.  out_dir None: nothing is written."""
    from .resample import front_end_many
    from .wavio import read_wav_many
    paths = [os.fspath(p) for p in paths]
    out_paths = _output_paths(paths, out_dir) if out_dir is not None else None
    dev = next(model.netG.parameters()).device
    pack = read_wav_many(paths, dev, channels, with_moments=True)
    packed, _, plan = front_end_many(pack, pack.rates, _front_end_kwargs(model, batch_size, gen_overlap), noise=noise,
                                     generator=generator, device=dev, raw_moments=pack.moments)
    utt = plan.utterances
    waves, out = _run_packed(model, packed, utt, with_buffer=True)
    lengths = [min(n, t) for n, t in zip(plan.final_lengths, utt.out_length)]
    res = FilesResult([w[..., :n] for w, n in zip(waves, lengths)], pack)
    if out_paths is not None:
        groups = [[] for _ in paths]
        for r, f in enumerate(pack.file):
            groups[f].append(r)
        res.out_paths = out_paths
        res.clipped = _write_cropped(out_paths, waves, out, utt, lengths, groups, int(model.opt.hr_sampling_rate), encoding)
    return res


def evaluate_files(model, paths, metric_path=None, batch_size: int = 64, gen_overlap=None, noise=None, generator=None,
                   out_dir=None, encoding: str = "PCM_F32"):
    """evaluate_many over WAV files: channel 0 of every file (read_audio's waveform), each of which must be at hr_sampling_rate
    (evaluate_many's rule).  -> (waveforms, scores) as evaluate_many; metric_path: its `MSE,SNR_SR,LSD` lines.  out_dir: the
    waveforms are written as well, as super_resolve_files(channels="first") writes them."""
    from .wavio import read_wav_many
    paths = [os.fspath(p) for p in paths]
    out_paths = _output_paths(paths, out_dir) if out_dir is not None else None
    pack = read_wav_many(paths, next(model.netG.parameters()).device, "first", with_moments=True)
    waves, scores = evaluate_many(model, pack, pack.rates, batch_size, gen_overlap, noise, generator, metric_path,
                                  raw_moments=pack.moments)
    if out_paths is not None:
        # (every file is at hr_sampling_rate: the final front-end length is the file's own)
        lengths = [min(n, w.shape[-1]) for n, w in zip(pack.lengths, waves)]
        clipped = _write_cropped(out_paths, waves, None, None, lengths, None, int(model.opt.hr_sampling_rate), encoding)
        return waves, scores, clipped
    return waves, scores


def input_files(path) -> List[str]:
    """AudioDataset.get_files (data/audio_dataset.py:84-100): a directory is walked for .wav files (the reference's test admits
    every name; .mp3 and .flac are out of scope here), a .wav file is itself, anything else is a CSV whose entries are paths
    relative to its own directory."""
    import csv
    path = os.fspath(path)
    if os.path.isdir(path):
        files = []
        for root, _, names in os.walk(path, topdown=False):
            files += [os.path.join(root, n) for n in sorted(names) if os.path.splitext(n)[1].lower() == ".wav"]
        return files
    if os.path.splitext(path)[1].lower() == ".wav":
        return [path]
    root = os.path.split(path)[0]
    with open(path, "r") as f:
        return [os.path.join(root, item) for row in csv.reader(f) for item in row]


def main(argv=None) -> int:
    """python -m mdctgan_amd.generate_audio --input FILE|DIR|CSV --output_dir DIR [--channels first|all]
    [--out_encoding PCM_F32|PCM_S16|PCM_S24] [--metrics] plus the model's flags (the checkpoint: --load_pretrain DIR
    --which_epoch LABEL, through load_network).  --metrics scores channel 0 of every file against the file itself and writes
    <output_dir>/metric.txt."""
    from .options import TrainOptions
    from .pix2pixHD_model import create_model
    options = TrainOptions()
    opt = options.parse(argv)
    if not opt.input or not opt.output_dir:
        options.parser.error("--input and --output_dir are required")
    files = input_files(opt.input)
    if not files:
        options.parser.error("no .wav file under %s" % opt.input)
    model = create_model(opt)
    if opt.metrics:
        os.makedirs(opt.output_dir, exist_ok=True)
        metric_path = os.path.join(opt.output_dir, "metric.txt")
        with open(metric_path, "w") as f:
            f.write("MSE,SNR_SR,LSD\n")
        _, _, clipped = evaluate_files(model, files, metric_path, batch_size=opt.batchSize, out_dir=opt.output_dir,
                                       encoding=opt.out_encoding)
        by_file = clipped
    else:
        res = super_resolve_files(model, files, opt.output_dir, opt.channels, opt.out_encoding, batch_size=opt.batchSize)
        by_file = [0] * len(files)
        for r, f in enumerate(res.pack.file):
            by_file[f] += res.clipped[r]
    for path, n in zip(files, by_file):
        if n:
            print("%s: %d samples clipped" % (path, n))
    print("%d files written to %s" % (len(files), opt.output_dir))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
