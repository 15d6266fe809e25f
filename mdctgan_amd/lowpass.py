"""Filter-diverse low-rate inputs: a different IIR low-pass per training example before the rate change (not in the reference).

Every low-rate input of the reference's data path comes from one filter, the Hann-windowed sinc of the resampler; a model trained
on it learns that filter's transition band.  Here a Butterworth or Chebyshev-I low-pass of random order, ripple and cutoff is
drawn per batch row (``LowpassSpec``, ``draw_lowpass``), designed on the host in float64 without SciPy (``lowpass_sos``: closed-form
analog prototype poles, pre-warped bilinear transform, one second-order section per conjugate pair) and applied on the device,
forward and backward from a zero state (zero phase: the low band keeps its alignment with the HR target), by ``mg_sos_rows``
(csrc/sos_rows.hip): ``sos_rows`` over a packed buffer and a row table, ``lowpass_waveform`` for one waveform.  The recursion is
double precision, the result sosfilt(sos, sosfilt(sos, x)[::-1])[::-1] in float64 rounded to float32 once; a row has the same bits
alone as in any pack.  ``resample.make_training_pair(lowpass_sos=)`` and ``train_data.training_batch_many(lowpass=)`` put it in
front of the low-rate leg.
"""
from __future__ import annotations

import cmath
import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from . import _lib
from .packed import check_table, upload_tables

__all__ = ["MG_SOS_MAX_SECTIONS", "MG_SOS_CHUNK", "KINDS", "LowpassSpec", "lowpass_sos", "identity_sos", "pad_sos", "check_sos",
           "spec_from_options", "draw_lowpass", "sos_rows", "lowpass_waveform"]

MG_SOS_MAX_SECTIONS = 6         # include/mdctgan_hip.h
MG_SOS_CHUNK = 256
MAX_ORDER = 2 * MG_SOS_MAX_SECTIONS
KINDS = ("butter", "cheby1")
SOS_ROW_COLS = 3                # mg_sos_row: in_pos, len, out_pos


def lowpass_sos(kind: str, order: int, cutoff_hz: float, fs: float, ripple_db=None) -> np.ndarray:
    """A digital low-pass of `order` (1 .. 12) with its edge at cutoff_hz (0 < cutoff_hz < fs / 2) -> float64 [ceil(order / 2), 6]
    rows of b0 b1 b2 1 a1 a2.  kind "butter" (edge: -3 dB) or "cheby1" (edge: -ripple_db, ripple_db > 0 required).
    The analog prototype's poles in closed form, frequency pre-warped, bilinear transform (all zeros at z = -1), one section per
    conjugate pair; an odd order has one first-order section (b2 = a2 = 0), which comes first.  The sections follow in the order
    of their poles' distance from the unit circle, the sharpest last.  Every section has gain 1 at DC and the first carries the
    filter's: |H(0)| = 1, or 10^(-ripple_db / 20) for an even-order Chebyshev (SciPy's convention) -- so no intermediate of the
    cascade leaves the signal's range."""
    if kind not in KINDS:
        raise ValueError("lowpass_sos: kind is one of %s, got %r" % (KINDS, kind))
    if isinstance(order, bool) or int(order) != order or not 1 <= int(order) <= MAX_ORDER:
        raise ValueError("lowpass_sos: order is an integer from 1 to %d, got %r" % (MAX_ORDER, order))
    N, fs, fc = int(order), float(fs), float(cutoff_hz)
    if not (math.isfinite(fs) and math.isfinite(fc) and fs > 0 and 0 < fc < fs / 2):
        raise ValueError("lowpass_sos: 0 < cutoff_hz < fs / 2 (got %r at fs %r)" % (cutoff_hz, fs))
    gain = 1.0
    if kind == "butter":
        if ripple_db is not None:
            raise ValueError("lowpass_sos: ripple_db is for cheby1")
        mu = None
    else:
        if ripple_db is None or not (math.isfinite(float(ripple_db)) and float(ripple_db) > 0):
            raise ValueError("lowpass_sos: cheby1 needs ripple_db > 0, got %r" % (ripple_db,))
        eps = math.sqrt(10.0 ** (0.1 * float(ripple_db)) - 1.0)
        mu = math.asinh(1.0 / eps) / N
        if N % 2 == 0:
            gain = 10.0 ** (-float(ripple_db) / 20.0)
    warped = 4.0 * math.tan(math.pi * fc / fs)                    # bilinear at a sampling rate of 2: s = 4 (z - 1) / (z + 1)
    first, pairs = [], []
    for m in range(-N + 1, N, 2):                                  # the poles of the upper half plane, and the real one (m == 0)
        if m < 0:
            continue
        theta = math.pi * m / (2 * N)
        p = -complex(math.cos(theta), math.sin(theta)) if mu is None else -cmath.sinh(complex(mu, theta))
        p = complex(p) * warped
        z = (4.0 + p) / (4.0 - p)
        one_minus_z = -2.0 * p / (4.0 - p)                         # 1 - z without the cancellation of a pole close to z = 1
        if m == 0:
            first.append([one_minus_z.real / 2, one_minus_z.real / 2, 0.0, 1.0, -z.real, 0.0])
        else:
            g = abs(one_minus_z) ** 2 / 4
            pairs.append((abs(z), [g, 2 * g, g, 1.0, -2 * z.real, abs(z) ** 2]))
    sos = np.asarray(first + [s for _, s in sorted(pairs, key=lambda t: t[0])], dtype=np.float64)
    sos[0, :3] *= gain
    return sos


def identity_sos(n: int = MG_SOS_MAX_SECTIONS) -> np.ndarray:
    out = np.zeros((n, 6), dtype=np.float64)
    out[:, 0] = out[:, 3] = 1.0
    return out


def pad_sos(sos) -> np.ndarray:
    """float64 [n, 6] sections (n <= 6) -> [MG_SOS_MAX_SECTIONS, 6], the unused sections the identity (b0 = a0 = 1, the rest 0)."""
    sos = np.asarray(sos.cpu() if torch.is_tensor(sos) else sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or not 1 <= sos.shape[0] <= MG_SOS_MAX_SECTIONS:
        raise ValueError("second-order sections are a [n <= %d, 6] array, got %s" % (MG_SOS_MAX_SECTIONS, sos.shape))
    out = identity_sos()
    out[:sos.shape[0]] = sos
    return out


def check_sos(table) -> np.ndarray:
    """The host-side refusal of a coefficient table [rows, 6, 6] (or [6, 6]) before any launch: every number finite, a0 == 1 and
    every section stable -- |a2| < 1 and |a1| < 1 + a2, the stability triangle.  -> the table as float64 [rows, 6, 6]."""
    t = np.asarray(table.cpu() if torch.is_tensor(table) else table, dtype=np.float64)
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3 or t.shape[1:] != (MG_SOS_MAX_SECTIONS, 6) or t.shape[0] == 0:
        raise ValueError("a coefficient table is float64 [rows, %d, 6], got %s" % (MG_SOS_MAX_SECTIONS, t.shape))
    if not np.isfinite(t).all():
        raise ValueError("non-finite filter coefficients")
    if not (t[:, :, 3] == 1.0).all():
        raise ValueError("sections are normalised to a0 == 1")
    a1, a2 = t[:, :, 4], t[:, :, 5]
    if not ((np.abs(a2) < 1.0) & (np.abs(a1) < 1.0 + a2)).all():
        raise ValueError("unstable section: |a2| < 1 and |a1| < 1 + a2 must hold")
    return np.ascontiguousarray(t)


@dataclass(frozen=True)
class LowpassSpec:
    """What draw_lowpass draws from, per batch row: a kind out of `kinds`, an order out of the inclusive range `order`, for a
    Chebyshev the pass-band ripple in dB out of `ripple`, and the edge as a fraction `cutoff` of lr_sampling_rate / 2."""
    kinds: Tuple[str, ...] = KINDS
    order: Tuple[int, int] = (2, 10)
    ripple: Tuple[float, float] = (0.01, 1.0)
    cutoff: Tuple[float, float] = (0.9, 1.0)

    def __post_init__(self):
        kinds = tuple(self.kinds)
        object.__setattr__(self, "kinds", kinds)
        if not kinds or any(k not in KINDS for k in kinds):
            raise ValueError("LowpassSpec: kinds out of %s, got %r" % (KINDS, kinds))
        lo, hi = (int(v) for v in self.order)
        if not 1 <= lo <= hi <= MAX_ORDER:
            raise ValueError("LowpassSpec: 1 <= order range <= %d, got %r" % (MAX_ORDER, self.order))
        object.__setattr__(self, "order", (lo, hi))
        r0, r1 = (float(v) for v in self.ripple)
        if not 0 < r0 <= r1 < math.inf:
            raise ValueError("LowpassSpec: 0 < ripple range in dB, got %r" % (self.ripple,))
        object.__setattr__(self, "ripple", (r0, r1))
        c0, c1 = (float(v) for v in self.cutoff)
        if not 0 < c0 <= c1 < math.inf:
            raise ValueError("LowpassSpec: 0 < cutoff range (a fraction of lr_sampling_rate / 2), got %r" % (self.cutoff,))
        object.__setattr__(self, "cutoff", (c0, c1))


def spec_from_options(kinds, order=(2, 10), ripple=(0.01, 1.0), cutoff=(0.9, 1.0)):
    """--lowpass_aug / --lowpass_order / --lowpass_ripple / --lowpass_cutoff -> a LowpassSpec, or None when the comma list of kinds
    is empty (the feature is off)."""
    if isinstance(kinds, str):
        kinds = [k.strip() for k in kinds.split(",") if k.strip()]
    if not kinds:
        return None
    return LowpassSpec(tuple(kinds), tuple(order), tuple(ripple), tuple(cutoff))


def draw_lowpass(file_rates, lr_rate: int, spec: LowpassSpec, generator=None) -> np.ndarray:
    """One filter per batch row -> the coefficient table float64 [rows, MG_SOS_MAX_SECTIONS, 6], unused sections the identity.
    Per row, in row order, four draws from the global CPU stream or the CPU `generator`: kind, order (torch.randint), ripple and
    cutoff fraction (torch.rand, uniform over their ranges; the ripple is drawn for a Butterworth too, so that a row's draws do not
    depend on its kind).  The filter is designed at the row's FILE rate with its edge at fraction * lr_rate / 2; a row whose edge
    would reach file_rate / 2 has nothing to remove and gets identity sections."""
    rates = [int(r) for r in file_rates]
    if not rates or min(rates) <= 0 or int(lr_rate) <= 0:
        raise ValueError("draw_lowpass needs positive sampling rates, one per row")
    out = np.empty((len(rates), MG_SOS_MAX_SECTIONS, 6), dtype=np.float64)
    for b, fs in enumerate(rates):
        kind = spec.kinds[int(torch.randint(0, len(spec.kinds), (1,), generator=generator).item())]
        order = int(torch.randint(spec.order[0], spec.order[1] + 1, (1,), generator=generator).item())
        u = torch.rand(2, dtype=torch.float64, generator=generator).tolist()
        ripple = spec.ripple[0] + (spec.ripple[1] - spec.ripple[0]) * u[0]
        edge = (spec.cutoff[0] + (spec.cutoff[1] - spec.cutoff[0]) * u[1]) * int(lr_rate) / 2
        if edge >= fs / 2:
            out[b] = identity_sos()
        else:
            out[b] = pad_sos(lowpass_sos(kind, order, edge, fs, ripple if kind == "cheby1" else None))
    return check_sos(out)


def sos_table_bits(table: np.ndarray) -> np.ndarray:
    """A float64 coefficient table as the int64 words upload_tables carries (the device side views them as float64 again)."""
    return np.ascontiguousarray(table, dtype=np.float64).view(np.int64)


def sos_rows(buf: torch.Tensor, table, sos, out=None, zero_phase: bool = True, max_len=None, workspace=None) -> torch.Tensor:
    """mg_sos_rows: row u of `table` (int64 [n, 3] = in_pos, len, out_pos; len == 0: a dead row) reads its window of the packed
    float32 buffer `buf`, runs the cascade sos[u] over it from a zero state in double -- with zero_phase again over the reversed
    result -- and writes the float32 result to out[out_pos : out_pos + len] (out: default a zero buffer of buf's size; it may not
    overlap buf).  -> out.
    table and sos on the HOST (arrays or CPU tensors; sos float64 [n, 6, 6] or one [6, 6] for every row): the sections are checked
    (check_sos: unstable or non-finite ones raise ValueError before any launch) and both travel in one copy.  On the DEVICE
    (table int64 [n, 3], sos float64 [n, 6, 6]): the caller has checked them and names max_len, the longest row.
    workspace: a uint8 device buffer of mg_sos_rows_workspace(n, max_len) bytes instead of the stream's scratch (a capture)."""
    lib = _lib.load()
    if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.dim() != 1:
        raise ValueError("sos_rows: buf is a contiguous float32 buffer")
    on_device = torch.is_tensor(table) and table.is_cuda
    if on_device:
        if not (torch.is_tensor(sos) and sos.is_cuda and sos.dtype == torch.float64 and sos.is_contiguous()
                and tuple(sos.shape) == (table.shape[0], MG_SOS_MAX_SECTIONS, 6)):
            raise ValueError("sos_rows: with a device table, sos is a contiguous float64 [n, %d, 6] device tensor"
                             % MG_SOS_MAX_SECTIONS)
        if max_len is None:
            raise ValueError("sos_rows: a device table needs max_len, the longest row")
        n = check_table(table, SOS_ROW_COLS, "sos_rows").shape[0]
    else:
        rows = np.asarray(table.cpu() if torch.is_tensor(table) else table, dtype=np.int64)
        if rows.ndim != 2 or rows.shape[1] != SOS_ROW_COLS or rows.shape[0] == 0:
            raise ValueError("sos_rows: the row table is int64 [n, 3] = in_pos, len, out_pos")
        n = rows.shape[0]
        coef = check_sos(sos)
        if coef.shape[0] == 1 and n > 1:
            coef = np.ascontiguousarray(np.broadcast_to(coef, (n, MG_SOS_MAX_SECTIONS, 6)))
        if coef.shape[0] != n:
            raise ValueError("sos_rows: one [%d, 6] set of sections per row (%d rows, %d sets)" % (MG_SOS_MAX_SECTIONS, n, coef.shape[0]))
        if max_len is None:
            max_len = max(int(rows[:, 1].max()), 1)
        table, bits = upload_tables([rows, sos_table_bits(coef)], buf.device)
        sos = bits.view(torch.float64)
    if out is None:
        out = torch.zeros(buf.numel(), dtype=torch.float32, device=buf.device)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 1:
        raise ValueError("sos_rows: out is a contiguous float32 buffer")
    nbytes = lib.mg_sos_rows_workspace(n, int(max_len))
    if nbytes == 0:
        raise ValueError("sos_rows: 0 < max_len <= 2^30 (got %r)" % (max_len,))
    ws = _lib.workspace(nbytes, buf.device) if workspace is None else workspace
    if not (torch.is_tensor(ws) and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nbytes):
        raise ValueError("sos_rows: workspace is a contiguous uint8 buffer of at least %d bytes" % nbytes)
    for t, name in ((table, "table"), (sos, "sos"), (out, "out"), (ws, "workspace")):
        if t.device != buf.device:
            raise ValueError("sos_rows: %s lives on %s, buf on %s" % (name, t.device, buf.device))
    _lib.check(lib.mg_sos_rows(_lib.ptr(buf), buf.numel(), _lib.ptr(table), _lib.ptr(sos), n, int(max_len), int(bool(zero_phase)),
                               _lib.ptr(out), out.numel(), _lib.ptr(ws), ws.numel(), _lib.stream()), "mg_sos_rows")
    return out


def lowpass_waveform(x: torch.Tensor, sos, zero_phase: bool = True) -> torch.Tensor:
    """The one-waveform form: x [..., L] float32 on the device -> the same shape, every row of it filtered by `sos` ([n <= 6, 6])
    from a zero state, with zero_phase forward and backward."""
    shape = x.shape
    L = int(shape[-1])
    if L <= 0:
        raise ValueError("lowpass_waveform: an empty waveform")
    flat = _lib.f32c(x.reshape(-1, L))
    B = flat.shape[0]
    pos = np.arange(B, dtype=np.int64) * L
    rows = np.stack([pos, np.full(B, L, dtype=np.int64), pos], axis=1)
    out = torch.empty(B * L, dtype=torch.float32, device=x.device)
    return sos_rows(flat.view(-1), rows, pad_sos(sos), out=out, zero_phase=zero_phase, max_len=L).view(shape)
