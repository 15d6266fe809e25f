"""MDCT4 / IMDCT4 with the reference's call signatures (models/mdct.py:359-489), executed by the
gfx950 kernels K1 / K2 in csrc/mdct.hip through the C ABI (include/mdctgan_hip.h).

Differences from the reference, all deliberate and documented in DESIGN.md:

* arithmetic is float32 end to end (the DCT-IV runs on the f32 MFMA pipe); the reference promotes to
  complex128 after its float32 window multiply.  Tolerances: tests/test_mdct_gpu.py.
* the returned spectrogram / waveform dtype is float32 unless ``dtype=torch.float64`` is requested
  (then the float32 result is widened, for code that relies on the reference's float64 outputs).
* frame padding follows the signal length T (the reference uses ``len(signal)`` == batch size for
  2-D input, SURVEY A2'); identical for every legal segment length (T % hop == 0).
* geometry: win_length == n_fft == 2 * hop_length == 512 (the hot path) runs the fused kernels K1 / K2 (csrc/mdct.hip:
  TDAC fold + 256-point DCT-IV); every other legal geometry of the reference (win_length <= n_fft, hop_length <=
  win_length, e.g. the class default n_fft = 2048) runs the generic path of csrc/codec_generic.hip: framing + window, the
  [frames, win] x [win, n_fft/2] cosine contraction as a dense exact-float32 MFMA GEMM (the 1x1 case of mg_conv_fwd),
  window + overlap-add.  There is no eager / CPU fallback.
* the other Princen-Bradley power-of-two geometries (win_length == n_fft == 2 * hop_length, centre padding, n_fft in 256 /
  1024 / 2048, e.g. the class default) run the fused kernels K1' / K2' of csrc/mdct_pow2.hip (TDAC fold + DCT-IV as an
  n_fft/4-point FFT in LDS) -- the ``.fast`` attribute; ``.fused`` keeps naming the 512 kernels only.  MG_MDCT_POW2=0 (read at call
  time) sends them back to the generic path.

Layout: the leaf launchers (one per kernel: mdct4_codec / imdct4_codec = K1 / K2, mdct4_pow2 / imdct4_pow2 = K1' / K2', mdct4_generic /
imdct4_generic, codec_forward / codec_inverse / codec_backward) make the ABI calls; which of them serves a request is decided in one place,
``Transform.route_analysis`` / ``Transform.route_synthesis`` (pure host functions), and ``Transform.analysis`` / ``synthesis`` / ``*_backward``
run the route.  MDCT4, IMDCT4 and Audio2MDCT are shells around one Transform.  The codec's constants travel as one ``Codec`` record, a
stitched decode's destination as one ``Stitch`` / ``Rows`` record.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple, Optional

import torch

from . import _lib

_FUSABLE = (_lib.MG_CODEC_RAW, _lib.MG_CODEC_ARCSINH, _lib.MG_CODEC_RANGE)        # the codecs K1 / K2 / K1' / K2' carry inside


class Codec(NamedTuple):
    """The codec block of the C ABI: the mode (MG_CODEC_*) and its constants.  ``codec._replace(src_range=...)`` for a per-call range."""
    mode: int = _lib.MG_CODEC_RAW
    gain: float = 1.0
    alpha: float = 0.6
    min_value: float = 1e-7
    norm_range: tuple = (0.0, 1.0)
    src_range: tuple = (0.0, 1.0)

    def kw(self, full=False):
        """The record as the leaf launchers' keywords (full: with the dB codec's alpha / min_value, for codec_forward / codec_inverse)."""
        kw = dict(codec=self.mode, gain=self.gain, norm_range=self.norm_range, src_range=self.src_range)
        return dict(kw, alpha=self.alpha, min_value=self.min_value) if full else kw


RAW = Codec()


def _per_clip(min_b, max_b, n):
    """Per-clip (min, max) of a decode as flat contiguous float32 [n] tensors (None, None: the codec's fixed src_range)."""
    if min_b is None:
        return None, None
    min_b, max_b = _lib.f32c(min_b.reshape(-1)), _lib.f32c(max_b.reshape(-1))
    assert min_b.numel() == n and max_b.numel() == n
    return min_b, max_b


class Stitch(NamedTuple):
    """Destination of a stitched decode: the clips are segments first_seg.. of ONE waveform `out` [mg_stitch_length(n_seg, T_out,
    overlap)].  segment_length: what `out` was sized for (checked).  zero_out: clear `out` first when overlap > 0 (None: first_seg == 0)."""
    out: torch.Tensor
    overlap: int
    first_seg: int
    segment_length: Optional[int] = None
    zero_out: Optional[bool] = None


class Rows(NamedTuple):
    """Destination of a row-table decode: the clips are the rows of a device row table (seg_row_table: one (pos, lo, hi) per clip) of the
    packed buffer `out`, which holds any number of stitched waveforms.  zero_out clears the whole of `out` first."""
    out: torch.Tensor
    overlap: int
    table: torch.Tensor
    segment_length: Optional[int] = None
    zero_out: bool = False


def _destination(stitch, rows, B, t_out, out_dtype, want_frames, what):
    """The validated destination of a stitched decode (a Stitch, a Rows, or None for a plain decode); `what` names the kernel."""
    if stitch is None and rows is None:
        return None
    if stitch is not None and rows is not None:
        raise ValueError("stitched %s: either stitch or rows" % what)
    dest = Stitch(*stitch) if rows is None else Rows(*rows)
    if rows is not None:
        _check_table(dest.table, B, what)
    if dest.segment_length is not None and int(dest.segment_length) != t_out:
        # the caller sized `out` for segments of another length than the spectrogram decodes to: the store's bounds check would
        # drop samples or leave part of `out` unwritten without a word
        raise ValueError("stitched %s: the output was sized for %d-sample segments, the spectrogram decodes to %d"
                         % (what, int(dest.segment_length), t_out))
    if want_frames or dest.out.dtype != out_dtype or not dest.out.is_contiguous():
        raise ValueError("stitched %s: contiguous output of the requested dtype, no synthesis frames" % what)
    return dest


def _check_table(table, B, what):
    if table.dtype != torch.int64 or tuple(table.shape) != (B, 3) or not table.is_contiguous():
        raise ValueError("stitched %s: the row table is a contiguous int64 [%d, 3] tensor (pos, lo, hi), got %s %s"
                         % (what, B, table.dtype, tuple(table.shape)))


def kbdwin(N: int, beta: float = 12.0, device="cpu") -> torch.Tensor:
    """Kaiser-Bessel-derived window (reference: util/util.py:179-186).  Host-side table: built with the
    same float32 op chain on the CPU so it is bit-identical to the reference's, then moved."""
    assert N % 2 == 0, "N must be even"
    w = torch.kaiser_window(window_length=N // 2 + 1, beta=beta * torch.pi, periodic=False, dtype=torch.float32)
    half = torch.sqrt(torch.cumsum(w, dim=0) / w.sum())[:-1]
    return torch.cat((half, half.flip(dims=(0,))), dim=0).to(device)


_dct4_cache = {}


def dct4_table(m: int, device) -> torch.Tensor:
    """D4[n, k] = cos(pi/M (n + 1/2)(k + 1/2)) evaluated in float64 on the host, rounded once to float32 -- followed, in the
    same buffer, by the stage-matrix image the factored kernels load (mg_dct4_image, mg_dct4_image_floats(2 m) floats; include/mdctgan_hip.h: the `dct4_image` argument of
    mg_mdct4_forward / mg_imdct4_forward).  Returns the flat tensor; ``dct4_table(m, dev)[:m * m].view(m, m)`` is the table
    itself, ``dct4_image(t, m)`` the image part (None for geometries without fused kernels)."""
    key = (m, str(device))
    t = _dct4_cache.get(key)
    if t is None:
        n = torch.arange(m, dtype=torch.float64) + 0.5
        tab = torch.cos((math.pi / m) * torch.outer(n, n)).to(torch.float32)
        lib = _lib.load() if m == 256 else None          # the fused n_fft = 512 kernels are the only users of the images
        extra = int(lib.mg_dct4_image_floats(2 * m)) if lib is not None else 0
        t = torch.zeros(m * m + extra, dtype=torch.float32, device=device)
        t[:m * m] = tab.reshape(-1).to(device)
        if extra:
            _lib.check(lib.mg_dct4_image(_lib.ptr(t), t.data_ptr() + 4 * m * m, _lib.stream()), "mg_dct4_image")
        _dct4_cache[key] = t
    return t


def dct4_image(table: torch.Tensor, m: int):
    """The image part of a dct4_table() buffer as a raw pointer argument (None: no image behind the table)."""
    return (table.data_ptr() + 4 * m * m) if table.numel() > m * m else None


def _make_window(window, win_length, device):
    if window is None:
        window = torch.ones
    if callable(window):
        win_length = int(win_length)
        w = window(win_length)
    else:
        w = window
        win_length = len(window)
    return w.to(device=device, dtype=torch.float32).contiguous(), win_length


def _check_geometry(n_fft, hop_length, win_length):
    """True: the fused n_fft = 512 kernels apply; False: the generic path."""
    assert win_length <= n_fft, "Window lenth %d should be no more than fft length %d" % (win_length, n_fft)
    assert hop_length <= win_length, "You hopped more than one frame"
    if n_fft % 2 or n_fft < 4:
        raise NotImplementedError("n_fft must be even")
    return n_fft == 512 and win_length == n_fft and hop_length * 2 == n_fft


_mdct_tab_cache = {}


def mdct_table(n_fft: int, win_length: int, device, transposed: bool) -> torch.Tensor:
    """C[n, k] = cos(2 pi / N (n + 1/2 + N/4)(k + 1/2)), n < win_length, k < N/2 (float64 on the host, rounded once).
    transposed: [N/2][win] (rows are the k-contiguous weight rows of the forward GEMM); else [win][N/2] (inverse)."""
    key = (n_fft, win_length, str(device), transposed)
    t = _mdct_tab_cache.get(key)
    if t is None:
        n = torch.arange(win_length, dtype=torch.float64)[:, None] + 0.5 + n_fft / 4.0
        k = torch.arange(n_fft // 2, dtype=torch.float64)[None, :] + 0.5
        c = torch.cos((2.0 * math.pi / n_fft) * n * k)
        t = (c.t() if transposed else c).contiguous().to(torch.float32).to(device)
        _mdct_tab_cache[key] = t
    return t


def num_frames(T: int, win_length: int, hop_length: int, center: bool = True) -> int:
    """Frames MDCT4.forward produces for a T-sample signal (mdct.py:393-407 with the T-based tail padding, SURVEY A2')."""
    start = hop_length if center else 0
    end = start + (hop_length - T % hop_length if T % hop_length else 0)
    return (T + start + end - win_length) // hop_length + 1


def _dense(a2d: torch.Tensor, w2d: torch.Tensor) -> torch.Tensor:
    """[R, K] x [N, K]^T on the exact-float32 MFMA GEMM (a 1x1 convolution over R 'pixels')."""
    from . import ops
    R, K = a2d.shape
    g = ops.conv_geom(1, 1, R, K, w2d.shape[0], 1, 1, 1, 0, False)
    return ops.conv_fwd(g, a2d.view(1, 1, R, K), w2d.view(w2d.shape[0], 1, 1, K)).view(R, w2d.shape[0])


def mdct4_generic(audio, window, n_fft, hop_length, center=True, want_frames=False):
    """MDCT4.forward for any legal geometry: audio [B, T] -> (raw coefficients [B, F, n_fft/2], frames [B, F, win] | None)."""
    lib = _lib.load()
    audio = _lib.f32c(audio)
    B, T = audio.shape
    win = window.numel()
    F = num_frames(T, win, hop_length, center)
    if F <= 0:
        raise ValueError("signal of %d samples is too short for win_length=%d" % (T, win))
    frames = torch.empty(B, F, win, dtype=torch.float32, device=audio.device)
    _lib.check(lib.mg_frames_window(_lib.ptr(audio), B, T, win, hop_length, hop_length if center else 0, F,
                                    _lib.ptr(window), _lib.ptr(frames), _lib.stream()), "mg_frames_window")
    spec = _dense(frames.view(B * F, win), mdct_table(n_fft, win, audio.device, True)).view(B, F, n_fft // 2)
    return spec, (frames if want_frames else None)


def imdct4_generic(spec, window, n_fft, hop_length, center=True, out_length=None, out_dtype=torch.float32,
                   want_frames=False):
    """IMDCT4.forward for any legal geometry: raw coefficients [B, F, n_fft/2] -> (audio [B, T_out], frames | None)."""
    lib = _lib.load()
    spec = _lib.f32c(spec)
    B, F, M = spec.shape
    win = window.numel()
    y = _dense(spec.view(B * F, M), mdct_table(n_fft, win, spec.device, False)).view(B, F, win)
    full = (F - 1) * hop_length + win
    crop = win // 2 if center else 0
    t_out = full - crop - ((win + 1) // 2 if center else 0)          # signal[win//2 : -win//2]  (mdct.py:484-486)
    if out_length is not None:
        t_out = min(t_out, int(out_length))
    audio = torch.empty(B, t_out, dtype=out_dtype, device=spec.device)
    _lib.check(lib.mg_overlap_add(_lib.ptr(y), B, F, win, hop_length, n_fft, _lib.ptr(window), crop, _lib.ptr(audio), t_out,
                                  int(out_dtype == torch.float64), _lib.stream()), "mg_overlap_add")
    frames = None
    if want_frames:
        frames = y * window
    return audio, frames


def codec_forward(raw, *, codec, gain=1.0, alpha=0.6, min_value=1e-7, norm_range=(0.0, 1.0), src_range=(0.0, 1.0),
                  per_sample=False, want_pair=False, want_stats=False):
    """Audio2MDCT.normalize on raw coefficients [B, F, M] (any codec, csrc/codec_generic.hip) -> dict like mdct4_codec,
    spec [B, C, F, M] with C = 2 for the explicit encoding."""
    lib = _lib.load()
    raw = _lib.f32c(raw)
    B, F, M = raw.shape
    C = 2 if codec == _lib.MG_CODEC_EXPLICIT else 1
    dev = raw.device
    spec = torch.empty(B, C, F, M, dtype=torch.float32, device=dev)
    pair = torch.empty(B, F, M, 2, dtype=torch.float32, device=dev) if (want_pair and C == 1) else None
    stats = torch.empty(2, dtype=torch.float64, device=dev) if want_stats else None
    mn = mx = scratch = None
    if per_sample:
        mn = torch.empty(B * C, dtype=torch.float32, device=dev)
        mx = torch.empty(B * C, dtype=torch.float32, device=dev)
        scratch = torch.empty(2 * B * C, dtype=torch.int32, device=dev)
    _lib.check(lib.mg_codec_forward(_lib.ptr(raw), B, F * M, codec, gain, alpha, min_value, norm_range[0], norm_range[1],
                                    src_range[0], src_range[1], int(per_sample), _lib.ptr(spec), _lib.ptr(pair), _lib.ptr(mn),
                                    _lib.ptr(mx), _lib.ptr(scratch), _lib.ptr(stats), _lib.stream()), "mg_codec_forward")
    return {"spec4": spec, "spec": spec[:, 0] if C == 1 else None, "pair": pair, "frames": None,
            "min": mn.view(B, C) if per_sample else None, "max": mx.view(B, C) if per_sample else None, "stats": stats}


def codec_inverse(spec4, *, codec, gain=1.0, alpha=0.6, min_value=1e-7, norm_range=(0.0, 1.0), src_range=(0.0, 1.0),
                  min_b=None, max_b=None):
    """Audio2MDCT.denormalize (+ the explicit-encoding channel combination of to_audio): [B, C, F, M] -> raw [B, F, M]."""
    lib = _lib.load()
    spec4 = _lib.f32c(spec4)
    B, C, F, M = spec4.shape
    assert C == (2 if codec == _lib.MG_CODEC_EXPLICIT else 1)
    raw = torch.empty(B, F, M, dtype=torch.float32, device=spec4.device)
    min_b, max_b = _per_clip(min_b, max_b, B * C)
    _lib.check(lib.mg_codec_inverse(_lib.ptr(spec4), B, F * M, codec, gain, alpha, min_value, norm_range[0], norm_range[1],
                                    src_range[0], src_range[1], _lib.ptr(min_b), _lib.ptr(max_b), _lib.ptr(raw),
                                    _lib.stream()), "mg_codec_inverse")
    return raw


def mdct4_codec(audio, window, dct4, n_fft, *, codec=_lib.MG_CODEC_RAW, gain=1.0, norm_range=(0.0, 1.0),
                src_range=(0.0, 1.0), per_sample=False, want_pair=False, want_frames=False, want_stats=False):
    """K1 launcher.  audio [B, T] (device, float32) -> dict(spec [B,F,M], pair [B,F,M,2]|None, frames|None,
    min/max [B]|None, stats double[2]|None)."""
    lib = _lib.load()
    audio = _lib.f32c(audio)
    B, T = audio.shape
    M = n_fft // 2
    F = lib.mg_mdct4_num_frames(T, n_fft)
    dev = audio.device
    pair = torch.empty(B, F, M, 2, dtype=torch.float32, device=dev) if want_pair else None
    image = dct4_image(dct4, M)
    # with the pair the spectrogram is its channel 0 (a strided view): K1 then writes 393 216 B per clip instead of 526 848
    legacy = os.environ.get("MG_MDCT_CT") == "0" or "MG_MDCT_FT" in os.environ      # (the generic kernels, forced)
    pair_only = (want_pair and image is not None and not per_sample and not want_frames and codec == _lib.MG_CODEC_ARCSINH
                 and T % 4 == 0 and audio.data_ptr() % 16 == 0 and window.data_ptr() % 16 == 0 and not legacy
                 # the factored kernels address through 32-bit buffer offsets (csrc/mdct.hip: the same guards decide there);
                 # beyond them the dense-table kernel runs and needs a real spectrogram buffer
                 and B * F * M * 8 < (1 << 32) - (1 << 18) and B * T * 4 < (1 << 32))
    spec = pair[..., 0] if pair_only else torch.empty(B, F, M, dtype=torch.float32, device=dev)
    frames = torch.empty(B, F, n_fft, dtype=torch.float32, device=dev) if want_frames else None
    stats = torch.empty(2, dtype=torch.float64, device=dev) if want_stats else None
    mn = mx = scratch = None
    if per_sample:
        mn = torch.empty(B, dtype=torch.float32, device=dev)
        mx = torch.empty(B, dtype=torch.float32, device=dev)
        scratch = torch.empty(2 * B, dtype=torch.int32, device=dev)
    rc = lib.mg_mdct4_forward(_lib.ptr(audio), B, T, n_fft, _lib.ptr(window), _lib.ptr(dct4), image, codec, gain,
                              norm_range[0], norm_range[1], src_range[0], src_range[1], int(per_sample),
                              None if pair_only else _lib.ptr(spec), _lib.ptr(pair), _lib.ptr(frames), _lib.ptr(mn), _lib.ptr(mx),
                              _lib.ptr(stats), _lib.ptr(scratch), _lib.stream())
    _lib.check(rc, "mg_mdct4_forward")
    return {"spec": spec, "pair": pair, "frames": frames, "min": mn, "max": mx, "stats": stats}


def imdct4_codec(spec, window, dct4, n_fft, *, codec=_lib.MG_CODEC_RAW, gain=1.0, norm_range=(0.0, 1.0),
                 src_range=(0.0, 1.0), min_b=None, max_b=None, out_length=None, out_dtype=torch.float32,
                 want_frames=False, stitch=None, rows=None):
    """K2 launcher.  spec [B, F, M] (device) -> (audio [B, T_out], frames|None).
    stitch (a Stitch or its tuple): K2's overlap-add store writes the clips straight into the stitched waveform, with
    generate_audio.py:40-53's cross-fade (mg_imdct4_stitched); rows (a Rows or its tuple): into the packed buffer of any number of
    stitched waveforms (mg_imdct4_stitched_rows).  Both return (out, None)."""
    lib = _lib.load()
    spec = _lib.f32c(spec)
    B, F, M = spec.shape
    t_out = (F - 1) * M
    if out_length is not None:
        t_out = min(t_out, int(out_length))
    dest = _destination(stitch, rows, B, t_out, out_dtype, want_frames, "K2")
    min_b, max_b = _per_clip(min_b, max_b, B)
    head = (_lib.ptr(spec), B, F, n_fft, _lib.ptr(window), _lib.ptr(dct4), dct4_image(dct4, M), codec, gain, norm_range[0], norm_range[1],
            src_range[0], src_range[1], _lib.ptr(min_b), _lib.ptr(max_b))
    f64 = int(out_dtype == torch.float64)
    if dest is not None:
        name = "mg_imdct4_stitched_rows" if rows is not None else "mg_imdct4_stitched"
        _lib.check(getattr(lib, name)(*head, *_destination_args(dest, t_out, f64)), name)
        return dest.out, None
    audio = torch.empty(B, t_out, dtype=out_dtype, device=spec.device)
    frames = torch.empty(B, F, n_fft, dtype=torch.float32, device=spec.device) if want_frames else None
    _lib.check(lib.mg_imdct4_forward(*head, _lib.ptr(audio), t_out, f64, _lib.ptr(frames), _lib.stream()), "mg_imdct4_forward")
    return audio, frames


def _destination_args(dest, t_out, f64):
    """The arguments of mg_imdct4[_pow2]_stitched[_rows] that follow the codec block."""
    if isinstance(dest, Rows):
        where, zero = _lib.ptr(dest.table), dest.zero_out
    else:
        where, zero = int(dest.first_seg), (dest.first_seg == 0 if dest.zero_out is None else dest.zero_out)
    return _lib.ptr(dest.out), dest.out.numel(), t_out, int(dest.overlap), where, int(bool(zero)), f64, _lib.stream()


def seg_row_table(rows, device=None) -> torch.Tensor:
    """mg_seg_row array from a sequence of (pos, lo, hi): an int64 [n, 3] tensor (on `device` when given)."""
    t = torch.as_tensor(rows, dtype=torch.int64).reshape(-1, 3).contiguous()
    return t if device is None else t.to(device)


def segments_gather(wave, table, segment_length: int, out=None):
    """mg_segments_gather: packed waveform [total] + row table [n, 3] -> [n, segment_length] (zeros outside each row's window)."""
    lib = _lib.load()
    wave = _lib.f32c(wave).reshape(-1)
    n = table.shape[0]
    _check_table(table, n, "gather")
    if out is None:
        out = torch.empty(n, segment_length, dtype=torch.float32, device=wave.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, segment_length) or not out.is_contiguous():
        raise ValueError("segments_gather: out is a contiguous float32 [%d, %d] tensor" % (n, segment_length))
    _lib.check(lib.mg_segments_gather(_lib.ptr(wave), wave.numel(), _lib.ptr(table), n, int(segment_length), _lib.ptr(out),
                                      _lib.stream()), "mg_segments_gather")
    return out


_UNSUPPORTED = -2       # MG_ERR_UNSUPPORTED: the fused backward's guards failed, the generic composition runs


def pow2_enabled() -> bool:
    """The MG_MDCT_POW2 switch, read at call time (0: every route of K1' / K2' goes back to the generic composition)."""
    return os.environ.get("MG_MDCT_POW2", "1") != "0"


def pow2_geometry(n_fft, hop_length, win_length, center=True) -> bool:
    """mg_mdct_pow2_supported: a geometry of the fused K1' / K2' kernels (csrc/mdct_pow2.hip); a pure host query."""
    return bool(_lib.load().mg_mdct_pow2_supported(int(n_fft), int(hop_length), int(win_length), int(bool(center))))


def pow2_radices(n_fft: int):
    """Stage radices of the n_fft/4-point Stockham FFT inside K1' / K2' (csrc/mdct_pow2.hip pw_dct4): radix 8, after one radix-2 /
    radix-4 stage when log2 is not a multiple of 3."""
    bits = (n_fft // 4).bit_length() - 1
    return ([1 << (bits % 3)] if bits % 3 else []) + [8] * (bits // 3)


def pow2_twiddles_host(n_fft: int, dtype=torch.float32) -> torch.Tensor:
    """mg_mdct_pow2_twiddles on the host: [3, n_fft/4, 2] = (pre, post, root) as (re, im); float64: before the rounding."""
    lib = _lib.load()
    n = int(lib.mg_mdct_pow2_twiddle_floats(n_fft))
    if n <= 0:
        raise NotImplementedError("no K1' / K2' kernels for n_fft = %d" % n_fft)
    t = torch.empty(n, dtype=dtype)
    _lib.check(lib.mg_mdct_pow2_twiddles(n_fft, t.data_ptr(), int(dtype == torch.float64)), "mg_mdct_pow2_twiddles")
    return t.view(3, n_fft // 4, 2)


_pow2_tw_cache = {}


def pow2_twiddles(n_fft: int, device) -> torch.Tensor:
    """The device copy of the twiddle buffer, built on the first (eager) call per geometry and device."""
    key = (n_fft, str(device))
    t = _pow2_tw_cache.get(key)
    if t is None:
        t = pow2_twiddles_host(n_fft).reshape(-1).to(device)
        _pow2_tw_cache[key] = t
    return t


def mdct4_pow2(audio, window, n_fft, F=None, *, codec=_lib.MG_CODEC_RAW, gain=1.0, norm_range=(0.0, 1.0), src_range=(0.0, 1.0),
               want_stats=False):
    """K1' launcher.  audio [B, T] -> dict like mdct4_codec (spec [B, F, n_fft/2], stats), F frames (default: num_frames(T));
    None where the kernel's guards refuse (MG_ERR_UNSUPPORTED): the caller runs the composition."""
    lib = _lib.load()
    audio = _lib.f32c(audio)
    B, T = audio.shape
    M = n_fft // 2
    if F is None:
        F = num_frames(T, n_fft, M, True)
    if F <= 0:
        raise ValueError("signal of %d samples is too short for win_length=%d" % (T, n_fft))
    dev = audio.device
    tw = pow2_twiddles(n_fft, dev)
    spec = torch.empty(B, F, M, dtype=torch.float32, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev) if want_stats else None
    rc = lib.mg_mdct4_pow2_forward(_lib.ptr(audio), B, T, F, n_fft, _lib.ptr(window), _lib.ptr(tw), codec, gain, norm_range[0],
                                   norm_range[1], src_range[0], src_range[1], 0, _lib.ptr(spec), None, _lib.ptr(stats),
                                   _lib.stream())
    if rc == _UNSUPPORTED:
        return None
    _lib.check(rc, "mg_mdct4_pow2_forward")
    return {"spec": spec, "pair": None, "frames": None, "min": None, "max": None, "stats": stats}


def imdct4_pow2(spec, window, n_fft, *, codec=_lib.MG_CODEC_RAW, gain=1.0, norm_range=(0.0, 1.0), src_range=(0.0, 1.0),
                min_b=None, max_b=None, out_length=None, scale=None, stitch=None, rows=None):
    """K2' launcher.  spec [B, F, n_fft/2] -> audio [B, T_out] (scale: in place of the transform's 4 / n_fft), or the destination of
    stitch / rows as in imdct4_codec (mg_imdct4_pow2_stitched, mg_imdct4_pow2_stitched_rows); None where the kernel's guards
    refuse a plain decode and nothing has been written."""
    lib = _lib.load()
    spec = _lib.f32c(spec)
    B, F, M = spec.shape
    t_out = (F - 1) * M
    if out_length is not None:
        t_out = min(t_out, int(out_length))
    tw = pow2_twiddles(n_fft, spec.device)
    dest = _destination(stitch, rows, B, t_out, torch.float32, False, "K2'")
    min_b, max_b = _per_clip(min_b, max_b, B)
    head = (_lib.ptr(spec), B, F, n_fft, _lib.ptr(window), _lib.ptr(tw), codec, gain, norm_range[0], norm_range[1], src_range[0],
            src_range[1], _lib.ptr(min_b), _lib.ptr(max_b))
    if dest is not None:
        name = "mg_imdct4_pow2_stitched_rows" if rows is not None else "mg_imdct4_pow2_stitched"
        _lib.check(getattr(lib, name)(*head, *_destination_args(dest, t_out, 0)), name)
        return dest.out
    audio = torch.empty(B, t_out, dtype=torch.float32, device=spec.device)
    rc = lib.mg_imdct4_pow2_forward(*head, _lib.ptr(audio), t_out, 0, 4.0 / n_fft if scale is None else float(scale), _lib.stream())
    if rc == _UNSUPPORTED:
        return None
    _lib.check(rc, "mg_imdct4_pow2_forward")
    return audio


def codec_backward(grad, spec, *, codec, to_spectro, scale=1.0, gain=1.0, norm_range=(0.0, 1.0), src_range=(0.0, 1.0),
                   min_b=None, max_b=None):
    """mg_codec_backward on [B, F, M]: scale * grad * dX/ds(spec) (to_spectro=False) or scale * grad / dX/ds(spec)."""
    lib = _lib.load()
    grad = _lib.f32c(grad)
    B = grad.shape[0]
    spec = _lib.f32c(spec) if spec is not None else None
    min_b, max_b = _per_clip(min_b, max_b, B)
    out = torch.empty_like(grad)
    _lib.check(lib.mg_codec_backward(_lib.ptr(grad), _lib.ptr(spec), B, grad.numel() // B, codec, int(to_spectro), scale, gain,
                                     norm_range[0], norm_range[1], src_range[0], src_range[1], _lib.ptr(min_b), _lib.ptr(max_b),
                                     _lib.ptr(out), _lib.stream()), "mg_codec_backward")
    return out


class Route(NamedTuple):
    """What serves one request.  kernel: "k512" (K1 / K2 and their backward kernels), "pow2" (K1' / K2') or "generic" (framing / GEMM /
    overlap-add).  codec_inside: no mg_codec_* launch accompanies the transform (else the transform runs in RAW mode beside one).
    fallback: where the kernel answers MG_ERR_UNSUPPORTED the generic composition serves this call (else that raises)."""
    kernel: str
    codec_inside: bool
    fallback: bool


class Transform:
    """One transform geometry: its float32 window, its tables and the ONE decision which kernel family serves a request on it --
    "k512": n_fft == win == 2 hop == 512 with centre padding; "pow2": mg_mdct_pow2_supported; "generic": the rest."""

    def __init__(self, n_fft, hop_length, win_length, window, center=True, device="cpu", allow=("k512", "pow2")) -> None:
        self.window, self.win_length = _make_window(window, win_length, device)
        self.n_fft, self.hop_length, self.center = n_fft, hop_length, center
        self.fused = _check_geometry(n_fft, hop_length, self.win_length) and bool(center)
        self._family = "k512" if self.fused else "pow2" if pow2_geometry(n_fft, hop_length, self.win_length, center) else "generic"
        if self._family not in allow:           # (the fused= / fast= switches of mdct4_backward / imdct4_backward)
            self._family = "generic"

    @property
    def family(self) -> str:
        """The family at this call: MG_MDCT_POW2=0 (pow2_enabled, read here and nowhere else) turns "pow2" into "generic"."""
        return "generic" if (self._family == "pow2" and not pow2_enabled()) else self._family

    @property
    def fast(self) -> bool:
        return self.family == "pow2"

    def window_on(self, device) -> torch.Tensor:
        if self.window.device != device:
            self.window = self.window.to(device)
        return self.window

    def dct4(self, device) -> torch.Tensor:
        return dct4_table(self.n_fft // 2, device)

    def covered(self, F, T) -> int:
        """Samples of a T-sample signal that its F analysis frames reach (the rest gets no gradient)."""
        return min(T, (F - 1) * self.hop_length + self.win_length - (self.hop_length if self.center else 0))

    # -- routes: pure host functions, no launch, no allocation ------------------------------------
    def route_analysis(self, codec=RAW, *, per_sample=False, want_pair=False, want_frames=False, backward=False, F=0, T=0) -> Route:
        """The MDCT (+ encode) of a request; backward: its gradient with respect to the audio, from F frames back to T samples."""
        fam = self.family
        if backward:        # K2-shaped: mg_mdct4_backward, or K2' in RAW mode (scale 1) after mg_codec_backward
            if fam == "pow2" and not (F > 1 and self.covered(F, T) <= (F - 1) * self.hop_length):
                fam = "generic"
            return Route(fam, fam == "k512", fam != "generic")
        raw = codec.mode == _lib.MG_CODEC_RAW
        if fam == "k512":
            return Route(fam, codec.mode in _FUSABLE, False)
        if fam == "pow2" and not want_frames:       # (K1' returns no frames)
            return Route(fam, raw or (codec.mode in _FUSABLE and not per_sample and not want_pair), True)
        return Route("generic", raw, False)

    def route_synthesis(self, codec=RAW, *, F=2, out_dtype=torch.float32, want_frames=False, dest=False, backward=False) -> Route:
        """The (decode +) IMDCT of an F-frame request (dest: into a Stitch / Rows destination); backward: its gradient with respect
        to the spectrogram."""
        fam = self.family
        if backward:        # K1-shaped: mg_imdct4_backward, or K1' in RAW mode before mg_codec_backward; float64 came from the generic kernels
            fam = fam if out_dtype == torch.float32 else "generic"
            return Route(fam, fam == "k512", fam != "generic")
        if fam == "pow2" and (want_frames or out_dtype != torch.float32 or F <= 1):       # (what K2' does not serve)
            fam = "generic"
        if dest and (fam == "generic" or codec.mode not in (_lib.MG_CODEC_ARCSINH, _lib.MG_CODEC_RANGE)):
            raise NotImplementedError("stitched decode needs the fused 512 / 256 geometry")
        if fam == "generic":
            return Route(fam, codec.mode == _lib.MG_CODEC_RAW, False)
        return Route(fam, codec.mode in _FUSABLE, fam == "pow2" and not dest)

    # -- the operations ---------------------------------------------------------------------------
    def analysis(self, audio, codec=RAW, *, per_sample=False, want_pair=False, want_stats=False, want_frames=False):
        """audio [..., T] -> the launcher dict: spec [B, F, M], spec4 [B, C, F, M], pair, frames, min / max, stats, and raw (the
        coefficients, where mg_codec_forward ran beside the transform)."""
        r = self.route_analysis(codec, per_sample=per_sample, want_pair=want_pair, want_frames=want_frames)
        a = audio if audio.dim() == 2 else audio.reshape(-1, audio.shape[-1])
        window = self.window_on(a.device)
        opts = dict(per_sample=per_sample, want_pair=want_pair, want_stats=want_stats)
        inside = r.codec_inside
        out = None
        if r.kernel == "k512":
            out = mdct4_codec(a, window, self.dct4(a.device), self.n_fft, want_frames=want_frames,
                              **(dict(codec.kw(), **opts) if inside else {}))
        elif r.kernel == "pow2":
            out = mdct4_pow2(a, window, self.n_fft, **(dict(codec.kw(), want_stats=want_stats) if inside else {}))
        if out is None:             # the generic family, a guard, or K1' refused
            raw, frames = mdct4_generic(a, window, self.n_fft, self.hop_length, self.center, want_frames)
            out = {"spec": raw, "pair": None, "frames": frames, "min": None, "max": None, "stats": None}
            inside = codec.mode == _lib.MG_CODEC_RAW
        if inside:
            out["spec4"], out["raw"] = out["spec"][:, None], None
            return out
        raw, frames = out["spec"], out["frames"]
        out = codec_forward(raw, **codec.kw(full=True), **opts)
        out["frames"], out["raw"] = frames, raw
        return out

    def synthesis(self, spec, codec=RAW, *, min_b=None, max_b=None, out_length=None, out_dtype=torch.float32, want_frames=False,
                  stitch=None, rows=None):
        """spec [B, F, M] or [B, C, F, M] -> (audio [B, T_out], frames | None), or (the destination's `out`, None)."""
        r = self.route_synthesis(codec, F=spec.shape[-2], out_dtype=out_dtype, want_frames=want_frames,
                                 dest=stitch is not None or rows is not None)
        window = self.window_on(spec.device)

        def raw_of(s):
            return codec_inverse(s if s.dim() == 4 else s[:, None], min_b=min_b, max_b=max_b, **codec.kw(full=True))
        clip = dict(min_b=min_b, max_b=max_b)
        if not r.codec_inside:
            spec, codec, clip = raw_of(spec), RAW, {}
        elif spec.dim() == 4:
            spec = spec.squeeze(1)
        if r.kernel == "k512":
            return imdct4_codec(spec, window, self.dct4(spec.device), self.n_fft, out_length=out_length, out_dtype=out_dtype,
                                want_frames=want_frames, stitch=stitch, rows=rows, **codec.kw(), **clip)
        if r.kernel == "pow2":
            audio = imdct4_pow2(spec, window, self.n_fft, out_length=out_length, stitch=stitch, rows=rows, **codec.kw(), **clip)
            if audio is not None:
                return audio, None
            if codec.mode != _lib.MG_CODEC_RAW:             # refused with the codec inside
                spec = raw_of(spec)
        return imdct4_generic(spec, window, self.n_fft, self.hop_length, self.center, out_length, out_dtype, want_frames)

    def synthesis_backward(self, grad_audio, spec, codec=RAW, *, F, min_b=None, max_b=None, out_dtype=torch.float32):
        """Gradient of synthesis() with respect to its spectrogram: grad_audio [B, T_out] -> grad_spec [B, F, n_fft/2].  The K1-shaped
        kernel (mg_imdct4_backward) where its guards hold; else frames of grad_audio with the IMDCT's crop as start padding, window,
        [frames, win] x [win, n_fft/2] on the exact-f32 GEMM -- or K1' in RAW mode with the forward's F (the adjoint of K2' is 4/N K1')
        -- then dX/ds and the 4/N scale (mg_codec_backward)."""
        lib = _lib.load()
        r = self.route_synthesis(codec, out_dtype=out_dtype, backward=True)
        gy = _lib.f32c(grad_audio)
        B, t_out = gy.shape
        dev = gy.device
        window, n_fft, win = self.window_on(dev), self.n_fft, self.win_length
        min_b, max_b = _per_clip(min_b, max_b, B)
        spec = _lib.f32c(spec) if (spec is not None and codec.mode != _lib.MG_CODEC_RAW) else None
        M = n_fft // 2
        if r.kernel == "k512":
            gs = torch.empty(B, F, M, dtype=torch.float32, device=dev)
            rc = lib.mg_imdct4_backward(_lib.ptr(gy), B, t_out, F, n_fft, _lib.ptr(window), dct4_image(self.dct4(dev), M), codec.mode,
                                        codec.gain, *codec.norm_range, *codec.src_range, _lib.ptr(min_b), _lib.ptr(max_b),
                                        _lib.ptr(spec), _lib.ptr(gs), _lib.stream())
            if rc != _UNSUPPORTED:
                _lib.check(rc, "mg_imdct4_backward")
                return gs
        out = mdct4_pow2(gy, window, n_fft, F) if r.kernel == "pow2" else None
        if out is not None:
            g = out["spec"]
        else:
            frames = torch.empty(B, F, win, dtype=torch.float32, device=dev)
            _lib.check(lib.mg_frames_window(_lib.ptr(gy), B, t_out, win, self.hop_length, win // 2 if self.center else 0, F,
                                            _lib.ptr(window), _lib.ptr(frames), _lib.stream()), "mg_frames_window")
            g = _dense(frames.view(B * F, win), mdct_table(n_fft, win, dev, True)).view(B, F, M)
        return codec_backward(g, spec, to_spectro=False, scale=4.0 / n_fft, min_b=min_b, max_b=max_b, **codec.kw())

    def analysis_backward(self, grad_spec, spec, codec=RAW, *, T):
        """Gradient of analysis() (fixed-range encode) with respect to the audio: grad_spec [B, F, n_fft/2] (gradient of the normalised
        spec) -> grad_audio [B, T].  The K2-shaped kernel (mg_mdct4_backward) where its guards hold; else ds/dX (mg_codec_backward),
        then [F, n_fft/2] x [n_fft/2, win] on the exact-f32 GEMM, window and overlap-add with the MDCT's start padding as crop
        (mg_overlap_add with n_fft = 4: scale 1) -- or K2' in RAW mode with output scale 1 (the adjoint of K1')."""
        lib = _lib.load()
        g = _lib.f32c(grad_spec)
        B, F, M = g.shape
        r = self.route_analysis(codec, backward=True, F=F, T=T)
        dev = g.device
        window, n_fft, win = self.window_on(dev), self.n_fft, self.win_length
        spec = _lib.f32c(spec) if (spec is not None and codec.mode != _lib.MG_CODEC_RAW) else None
        if r.kernel == "k512":
            ga = torch.empty(B, T, dtype=torch.float32, device=dev)
            rc = lib.mg_mdct4_backward(_lib.ptr(g), _lib.ptr(spec), B, T, n_fft, _lib.ptr(window), dct4_image(self.dct4(dev), M),
                                       codec.mode, codec.gain, *codec.norm_range, *codec.src_range, _lib.ptr(ga), _lib.stream())
            if rc != _UNSUPPORTED:
                _lib.check(rc, "mg_mdct4_backward")
                return ga
        if codec.mode != _lib.MG_CODEC_RAW:
            g = codec_backward(g, spec, to_spectro=True, **codec.kw())
        covered = self.covered(F, T)
        ga = imdct4_pow2(g, window, n_fft, out_length=covered, scale=1.0) if r.kernel == "pow2" else None
        if ga is None:
            z = _dense(g.view(B * F, M), mdct_table(n_fft, win, dev, False)).view(B, F, win)
            ga = torch.empty(B, covered, dtype=torch.float32, device=dev)
            # mg_overlap_add scales by 4 / n_fft: n_fft = 4 makes it 1
            _lib.check(lib.mg_overlap_add(_lib.ptr(z), B, F, win, self.hop_length, 4, _lib.ptr(window), self.hop_length if self.center else 0,
                                          _lib.ptr(ga), covered, 0, _lib.stream()), "mg_overlap_add")
        if covered < T:
            ga = torch.cat((ga, ga.new_zeros(B, T - covered)), dim=1)
        return ga


def _legacy_transform(window, n_fft, hop_length, center, fused, fast):
    return Transform(n_fft, hop_length, None, window, center, window.device,
                     allow=tuple(name for name, on in (("k512", fused), ("pow2", fast)) if on))


def imdct4_backward(grad_audio, spec, window, n_fft, hop_length, F, center=True, *, codec=_lib.MG_CODEC_RAW, gain=1.0,
                    norm_range=(0.0, 1.0), src_range=(0.0, 1.0), min_b=None, max_b=None, fused=True, fast=False):
    """Transform.synthesis_backward for callers that hold a window (fused / fast: the 512 / the K1' kernels may run)."""
    return _legacy_transform(window, n_fft, hop_length, center, fused, fast).synthesis_backward(
        grad_audio, spec, Codec(codec, gain, norm_range=norm_range, src_range=src_range), F=F, min_b=min_b, max_b=max_b)


def mdct4_backward(grad_spec, spec, window, n_fft, hop_length, T, center=True, *, codec=_lib.MG_CODEC_RAW, gain=1.0,
                   norm_range=(0.0, 1.0), src_range=(0.0, 1.0), fused=True, fast=False):
    """Transform.analysis_backward for callers that hold a window (fused / fast: the 512 / the K2' kernels may run)."""
    return _legacy_transform(window, n_fft, hop_length, center, fused, fast).analysis_backward(
        grad_spec, spec, Codec(codec, gain, norm_range=norm_range, src_range=src_range), T=T)


class CodecGrad(torch.autograd.Function):
    """y = fwd(x) with the gradient bwd(grad_y, x, y).  fwd is today's launcher chain, unchanged (same kernels, same bits); the
    extra tensor inputs are constants of the forward (norm_param's min / max): a gradient asked of them is not built."""

    @staticmethod
    def forward(ctx, fwd, bwd, x, *consts):
        y = fwd(x)
        ctx.bwd = bwd
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        if any(ctx.needs_input_grad[3:]):
            raise NotImplementedError("the gradient with respect to norm_param tensors (min / max) is not built")
        x, y = ctx.saved_tensors
        gx = ctx.bwd(grad_y, x, y) if ctx.needs_input_grad[2] else None
        return (None, None, gx) + (None,) * (len(ctx.needs_input_grad) - 3)


def wants_grad(*tensors) -> bool:
    """The autograd Functions are entered only here: grad mode on and some input requiring grad (else today's path, no grad_fn)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class _Shell(torch.nn.Module):
    """What MDCT4 and IMDCT4 share: the reference's attributes over one Transform."""

    def __init__(self, n_fft, hop_length, win_length, window, center, pad_mode, device, dtype) -> None:
        super().__init__()
        self.n_fft, self.pad_mode, self.device, self.hop_length, self.center = n_fft, pad_mode, device, hop_length, center
        self.transform = Transform(n_fft, hop_length, win_length, window, center, device)
        self.win_length, self.fused, self.out_dtype = self.transform.win_length, self.transform.fused, dtype

    window = property(lambda self: self.transform.window)
    fast = property(lambda self: self.transform.fast, doc="K1' / K2' (csrc/mdct_pow2.hip) run this geometry (MG_MDCT_POW2=0 says no)")

    def _differentiable(self, run, bwd, x):
        """run(x) -> (y, frames), through CodecGrad where a gradient is wanted."""
        if not wants_grad(x):
            return run(x)
        held = {}

        def fwd(a):
            y, held["frames"] = run(a)
            return y
        return CodecGrad.apply(fwd, bwd, x), held["frames"]


class MDCT4(_Shell):
    """models/mdct.py:359-425.  forward(signal, return_frames=False) -> (spec [..., F, n_fft/2], frames)."""

    def __init__(self, n_fft=2048, hop_length=None, win_length=None, window=None, center=True,
                 pad_mode="constant", device="cuda", dtype=torch.float32) -> None:
        super().__init__(n_fft, hop_length, win_length, window, center, pad_mode, device, dtype)
        if pad_mode != "constant":
            raise NotImplementedError("HIP MDCT4 implements zero ('constant') padding")

    def forward(self, signal, return_frames: bool = False):
        lead = signal.shape[:-1]
        x = signal.reshape(-1, signal.shape[-1])

        def run(a):
            r = self.transform.analysis(a, want_frames=return_frames)
            return r["spec"], r["frames"]
        sp, fr = self._differentiable(run, lambda g, a, _: self.transform.analysis_backward(g, None, T=a.shape[-1]), x)
        spec = sp.reshape(*lead, *sp.shape[1:]).to(self.out_dtype)
        frames = fr.reshape(*lead, *fr.shape[1:]) if return_frames else torch.empty(1)
        return spec, frames


class IMDCT4(_Shell):
    """models/mdct.py:428-489.  forward(spec [B, F, n_fft/2], return_frames=False) -> (audio [B,1,1,T], frames)."""

    def __init__(self, n_fft=2048, hop_length=None, win_length=None, window=None, center=True,
                 pad_mode="constant", out_length=None, device="cuda", dtype=torch.float32) -> None:
        super().__init__(n_fft, hop_length, win_length, window, center, pad_mode, device, dtype)
        self.out_length = out_length

    def forward(self, signal, return_frames: bool = False):
        assert signal.dim() == 3, "Only tensors shaped in BHW are supported, got tensor of shape %s" % (
            str(signal.size()))
        assert signal.size()[-1] == self.n_fft // 2, \
            "The last dim of input tensor should match the n_fft. Expected %d ,got %d" % (self.n_fft, signal.size()[-1])
        audio, frames = self._differentiable(
            lambda spec: self.transform.synthesis(spec, out_length=self.out_length, out_dtype=self.out_dtype, want_frames=return_frames),
            lambda g, spec, _: self.transform.synthesis_backward(g, None, F=spec.shape[1], out_dtype=self.out_dtype), signal)
        return audio[:, None, None, :], (frames if return_frames else torch.zeros(1))
