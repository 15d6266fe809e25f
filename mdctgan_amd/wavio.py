"""WAV files in, WAV files out: ``torchaudio.info`` / ``torchaudio.load`` (data/audio_dataset.py:37-51, :143) and ``torchaudio.save``
(generate_audio.py:89-96) for MANY files at once.

The host parses and writes RIFF/WAVE headers (``wav_info``, ``wav_header``) and moves payload bytes; every sample is converted on
the device (csrc/pcm_rows.hip).  ``read_wav_many``: the payloads of all files in one pinned byte buffer (each at a 16-byte aligned
offset), one copy to the device, one table copy and ONE decode launch into a packed float32 buffer of ``packed.aligned_layout``'s
layout -- optionally with the {sum x, sum x^2} moments ``resample.front_end_many`` starts with, from the same pass.
``write_wav_many``: one encode launch over the rows of any number of files, one copy back, then headers and payloads to disk.
Integer PCM of 8 (unsigned), 16, 24 and 32 bits and IEEE float of 32 and 64 bits are read; float32, 16- and 24-bit PCM are written.
Parity with torchaudio itself is unpinned (it is not installed where this project is tested): the arithmetic is the documented
one of ``torchaudio.load(normalize=True)``, checked against a numpy restatement.  Imports only ``_lib`` and ``packed``.
"""
from __future__ import annotations

import os
import struct
from dataclasses import dataclass
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .packed import PackedLayout, aligned_layout, check_table, pack_waves, upload_tables

MG_PCM_U8, MG_PCM_S16, MG_PCM_S24, MG_PCM_S32, MG_PCM_F32, MG_PCM_F64 = range(6)          # include/mdctgan_hip.h
SAMPLE_BYTES = {MG_PCM_U8: 1, MG_PCM_S16: 2, MG_PCM_S24: 3, MG_PCM_S32: 4, MG_PCM_F32: 4, MG_PCM_F64: 8}
ENCODINGS = {"PCM_F32": MG_PCM_F32, "PCM_S16": MG_PCM_S16, "PCM_S24": MG_PCM_S24}         # what write_wav_many writes
_BY_TAG_BITS = {(1, 8): MG_PCM_U8, (1, 16): MG_PCM_S16, (1, 24): MG_PCM_S24, (1, 32): MG_PCM_S32, (3, 32): MG_PCM_F32,
                (3, 64): MG_PCM_F64}
_COMPRESSED = {2: "MS ADPCM", 6: "A-law", 7: "mu-law", 0x11: "IMA ADPCM", 0x31: "GSM 6.10", 0x50: "MPEG", 0x55: "MPEG layer 3"}
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")           # KSDATAFORMAT_SUBTYPE_*: the tag, then these 14 bytes
PAYLOAD_ALIGN = 16


class WavInfo(NamedTuple):
    """wav_info's result.  `fmt`: the format tag that describes the samples, 1 (integer PCM) or 3 (IEEE float) -- an extensible
    header's SubFormat.  The payload is bytes [data_offset, data_offset + data_bytes) of the file: num_frames whole frames."""
    sample_rate: int
    num_frames: int
    num_channels: int
    bits: int
    fmt: int
    data_offset: int
    data_bytes: int

    @property
    def format(self) -> int:
        """The MG_PCM_* code of mg_pcm_row.format."""
        return _BY_TAG_BITS[(self.fmt, self.bits)]


def wav_info(path) -> WavInfo:
    """The header of a RIFF/WAVE file (the payload is not read).  Chunks in any order, unknown chunks and pad bytes are skipped; a
    data size of 0 or 0xFFFFFFFF, or one that runs past the end of the file, means "to the end of the file, whole frames only".
    ValueError (naming the file and the reason): anything this project does not read."""
    path = os.fspath(path)

    def bad(why):
        return ValueError("%s: %s" % (path, why))
    ext = os.path.splitext(path)[1].lower()
    if ext in (".mp3", ".flac"):
        raise bad("%s files are out of scope: only RIFF/WAVE is read" % ext)
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        head = f.read(12)
        if head[:4] in (b"RIFX", b"RF64"):
            raise bad("%s files (%s) are out of scope" % (head[:4].decode(),
                                                         "big-endian" if head[:4] == b"RIFX" else "64-bit RIFF"))
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise bad("not RIFF/WAVE")
        fmt, data, pos = None, None, 12
        while pos + 8 <= size:
            f.seek(pos)
            cid, n = struct.unpack("<4sI", f.read(8))
            body = pos + 8
            if cid == b"fmt " and fmt is None:
                fmt = f.read(min(n, 40))
            elif cid == b"data" and data is None:
                open_ended = n in (0, 0xFFFFFFFF) or body + n > size
                data = (body, size - body if open_ended else n)
                if open_ended:
                    break                                   # (nothing can follow a payload that runs to the end of the file)
            if fmt is not None and data is not None:
                break
            pos = body + n + (n & 1)
    if fmt is None:
        raise bad("no 'fmt ' chunk")
    if data is None:
        raise bad("no 'data' chunk")
    if len(fmt) < 16:
        raise bad("a 'fmt ' chunk of %d bytes" % len(fmt))
    tag, channels, rate, _, block_align, bits = struct.unpack("<HHIIHH", fmt[:16])
    valid = bits
    if tag == 0xFFFE:
        if len(fmt) < 40:
            raise bad("an extensible 'fmt ' chunk of %d bytes" % len(fmt))
        valid, = struct.unpack("<H", fmt[18:20])
        tag, = struct.unpack("<H", fmt[24:26])
    if tag not in (1, 3):
        raise bad("format tag 0x%04x (%s) is compressed or unknown: only integer PCM (1) and IEEE float (3) are read"
                  % (tag, _COMPRESSED.get(tag, "?")))
    if channels == 0:
        raise bad("0 channels")
    if (tag, bits) not in _BY_TAG_BITS:
        raise bad("%d-bit %s samples are not read" % (bits, "integer" if tag == 1 else "float"))
    if valid != bits:
        raise bad("%d valid bits in a %d-bit container are not read" % (valid, bits))
    if block_align != channels * bits // 8:
        raise bad("block_align %d is not channels * bits / 8 = %d" % (block_align, channels * bits // 8))
    if rate == 0:
        raise bad("a sampling rate of 0")
    frames = data[1] // block_align
    if frames == 0:
        raise bad("zero frames")
    return WavInfo(rate, frames, channels, bits, tag, data[0], frames * block_align)


def wav_header(sample_rate: int, num_channels: int, fmt_code: int, num_frames: int) -> bytes:
    """Everything of a WAV file in front of its payload: format tag 1 / 3 for at most 2 channels and extensible above, a `fact`
    chunk in a float file, all sizes correct (the caller appends the payload and, where that is odd, one pad byte)."""
    if fmt_code not in SAMPLE_BYTES:
        raise ValueError("unknown sample format %r" % (fmt_code,))
    nb = SAMPLE_BYTES[fmt_code]
    tag = 3 if fmt_code in (MG_PCM_F32, MG_PCM_F64) else 1
    block = num_channels * nb
    payload = num_frames * block
    if not (0 < num_channels <= 65535 and 0 < sample_rate < 1 << 32 and num_frames > 0 and block <= 65535):
        raise ValueError("a WAV file needs 1 .. 65535 channels, a positive sampling rate and at least one frame")
    base = struct.pack("<HHIIHH", 0xFFFE if num_channels > 2 else tag, num_channels, sample_rate, sample_rate * block, block, 8 * nb)
    if num_channels > 2:
        fmt = base + struct.pack("<HHI", 22, 8 * nb, 0) + struct.pack("<H", tag) + _GUID_TAIL
    elif tag == 3:
        fmt = base + struct.pack("<H", 0)
    else:
        fmt = base
    fact = struct.pack("<4sII", b"fact", 4, num_frames) if tag == 3 else b""
    riff = 4 + 8 + len(fmt) + len(fact) + 8 + payload + (payload & 1)
    if riff >= 1 << 32:
        raise ValueError("%d bytes do not fit a RIFF file (RF64 is out of scope)" % payload)
    return (struct.pack("<4sI4s", b"RIFF", riff, b"WAVE") + struct.pack("<4sI", b"fmt ", len(fmt)) + fmt + fact
            + struct.pack("<4sI", b"data", payload))


# ---------------------------------------------------------------------------------------------------------------------
# The two launches
# ---------------------------------------------------------------------------------------------------------------------
def _check_rows(what, rows, bytes_total, samples_total, byte_col, sample_col, formats):
    """The host's validation of an mg_pcm_row table (int64 [n, 6] = src_pos, frames, channels, channel, format, dst_pos) against
    the byte buffer and the float32 buffer; the kernels' own clamping is the second line of defence."""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    if rows.ndim != 2 or rows.shape[1] != 6 or rows.shape[0] == 0:
        raise ValueError("%s: the row table is int64 [n, 6] with at least one row" % what)
    frames, ch, c, fm = rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4]
    if (fm < 0).any() or (fm > MG_PCM_F64).any():
        raise ValueError("%s: an unknown sample format" % what)
    if not np.isin(fm, formats).all():
        raise NotImplementedError("%s: only the sample formats %s (MG_ERR_UNSUPPORTED)" % (what, sorted(formats)))
    if (frames <= 0).any() or (ch < 1).any() or (ch > 65535).any() or (c < 0).any() or (c >= ch).any():
        raise ValueError("%s: every row has frames > 0, 1 .. 65535 channels and a channel below that" % what)
    nb = np.asarray([SAMPLE_BYTES[int(v)] for v in fm], dtype=np.int64)
    bp, sp = rows[:, byte_col], rows[:, sample_col]
    if (bp < 0).any() or (frames > (int(bytes_total) - bp) // (ch * nb)).any():
        raise ValueError("%s: a row's frames do not lie inside the byte buffer (%d bytes)" % (what, bytes_total))
    if (sp < 0).any() or (sp + frames > int(samples_total)).any():
        raise ValueError("%s: a row's samples do not lie inside the float32 buffer (%d samples)" % (what, samples_total))
    return rows


def _device_table(what, rows, table, device):
    if table is None:
        table, = upload_tables([rows], device)
    if check_table(table, 6, what).shape[0] != rows.shape[0]:
        raise ValueError("%s: the device table has the host table's rows" % what)
    return table


def pcm_decode_rows(data: torch.Tensor, rows, out: torch.Tensor, with_moments: bool = False, table=None):
    """mg_pcm_decode_rows: `data` (contiguous uint8 device buffer of payload bytes), `rows` (HOST int64 [n, 6] mg_pcm_row table,
    validated here against both buffers; `table`: the same rows already on the device, else they are copied) -> `out` (contiguous
    float32 device buffer, written in place at every row's dst_pos), and with_moments the float64 [n, 2] tensor that
    packed.rows_moments gives over the decoded windows, bit for bit (else None)."""
    lib = _lib.load()
    if data.dtype != torch.uint8 or not data.is_contiguous() or data.dim() != 1:
        raise ValueError("pcm_decode_rows: the payload is a contiguous uint8 buffer")
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("pcm_decode_rows: out is a contiguous float32 buffer")
    rows = _check_rows("pcm_decode_rows", rows, data.numel(), out.numel(), 0, 5, list(range(6)))
    table = _device_table("pcm_decode_rows", rows, table, out.device)
    n, longest = rows.shape[0], int(rows[:, 1].max())
    moments, ws, nbytes = None, None, 0
    if with_moments:
        nbytes = lib.mg_pcm_decode_rows_workspace(n, longest)
        ws = _lib.workspace(nbytes, out.device)
        moments = torch.empty(n, 2, dtype=torch.float64, device=out.device)
    _lib.check(lib.mg_pcm_decode_rows(_lib.ptr(data), data.numel(), _lib.ptr(table), n, longest, _lib.ptr(out), out.numel(),
                                      _lib.ptr(moments), _lib.ptr(ws), nbytes, _lib.stream()), "mg_pcm_decode_rows")
    return out, moments


def pcm_encode_rows(x: torch.Tensor, rows, data: torch.Tensor, table=None, clipped=None) -> torch.Tensor:
    """mg_pcm_encode_rows: the rows of `x` (contiguous float32 device buffer; a row's src_pos is its first sample) -> the bytes of
    `data` (contiguous uint8 device buffer; dst_pos is the byte offset of the file's payload) as MG_PCM_F32, MG_PCM_S16 or
    MG_PCM_S24 (anything else: NotImplementedError).  -> int64 [n] on the device: the samples of every row that were clamped or
    NaN.  `rows`, `table`: see pcm_decode_rows."""
    lib = _lib.load()
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("pcm_encode_rows: x is a contiguous float32 buffer")
    if data.dtype != torch.uint8 or not data.is_contiguous() or data.dim() != 1:
        raise ValueError("pcm_encode_rows: the payload is a contiguous uint8 buffer")
    rows = _check_rows("pcm_encode_rows", rows, data.numel(), x.numel(), 5, 0, sorted(ENCODINGS.values()))
    table = _device_table("pcm_encode_rows", rows, table, x.device)
    n = rows.shape[0]
    if clipped is None:
        clipped = torch.empty(n, dtype=torch.int64, device=x.device)
    elif clipped.dtype != torch.int64 or tuple(clipped.shape) != (n,) or not clipped.is_contiguous():
        raise ValueError("pcm_encode_rows: clipped is a contiguous int64 [%d] tensor" % n)
    _lib.check(lib.mg_pcm_encode_rows(_lib.ptr(x), x.numel(), _lib.ptr(table), n, int(rows[:, 1].max()), _lib.ptr(data),
                                      data.numel(), _lib.ptr(clipped), _lib.stream()), "mg_pcm_encode_rows")
    return clipped


# ---------------------------------------------------------------------------------------------------------------------
# Files
# ---------------------------------------------------------------------------------------------------------------------
def _round_up(n: int, align: int) -> int:
    return -(-n // align) * align


@dataclass
class ReadPlan:
    """plan_read's result (host only).  File f's payload goes to bytes [byte_starts[f], byte_starts[f] + infos[f].data_bytes) of a
    staging buffer of bytes_total bytes, every start a multiple of 16.  Row r is channel `channel[r]` of file `file[r]`; the rows
    (int64 [n, 6] mg_pcm_row) decode into a float32 buffer of `layout` (packed.aligned_layout over the rows' frame counts)."""
    byte_starts: List[int]
    bytes_total: int
    layout: PackedLayout
    rows: np.ndarray
    file: List[int]
    channel: List[int]


def plan_read(infos, channels: str = "first", align: int = 64) -> ReadPlan:
    """channels "first": one row per file, its channel 0 (what seg_pad_audio keeps, data/audio_dataset.py:104).  "all": one row
    per channel, file-major."""
    if channels not in ("first", "all"):
        raise ValueError('channels is "first" or "all" (got %r)' % (channels,))
    infos = list(infos)
    if not infos:
        raise ValueError("no files")
    byte_starts, pos = [], 0
    for i in infos:
        byte_starts.append(pos)
        pos = _round_up(pos + i.data_bytes, PAYLOAD_ALIGN)
    file = [f for f, i in enumerate(infos) for _ in range(i.num_channels if channels == "all" else 1)]
    channel = [c for i in infos for c in range(i.num_channels if channels == "all" else 1)]
    layout = aligned_layout([infos[f].num_frames for f in file], align)
    rows = np.asarray([(byte_starts[f], infos[f].num_frames, infos[f].num_channels, c, infos[f].format, s)
                       for f, c, s in zip(file, channel, layout.starts)], dtype=np.int64).reshape(-1, 6)
    return ReadPlan(byte_starts, pos, layout, rows, file, channel)


@dataclass
class WavPack:
    """read_wav_many's result: row r (channel `channel[r]` of paths[file[r]], at rates[r] Hz) is buffer[starts[r] : starts[r] +
    lengths[r]] of a packed float32 device buffer in packed.aligned_layout's layout, zeros in the gaps.  `moments`: None, or
    float64 [n, 2] = {sum x, sum x^2} per row, packed.rows_moments' bits.  resample.front_end_many takes a WavPack as `raws`."""
    buffer: torch.Tensor
    starts: List[int]
    lengths: List[int]
    rates: List[int]
    file: List[int]
    channel: List[int]
    moments: Optional[torch.Tensor]
    paths: List[str]
    infos: List[WavInfo]

    def __len__(self):
        return len(self.lengths)

    @property
    def views(self):
        return [self.buffer[s:s + n] for s, n in zip(self.starts, self.lengths)]


def stage_payloads(paths, infos, plan: ReadPlan, pin: bool = True) -> torch.Tensor:
    """The payload bytes of every file at plan.byte_starts of one (pinned) uint8 host buffer; the few bytes between payloads are 0."""
    host = torch.zeros(max(plan.bytes_total, 1), dtype=torch.uint8, pin_memory=pin)
    view = memoryview(host.numpy())
    for path, i, s in zip(paths, infos, plan.byte_starts):
        with open(path, "rb") as f:
            f.seek(i.data_offset)
            if f.readinto(view[s:s + i.data_bytes]) != i.data_bytes:
                raise ValueError("%s: the file ends inside its payload" % path)
    return host


def read_wav_many(paths, device=None, channels: str = "first", with_moments: bool = False) -> WavPack:
    """torchaudio.load(normalize=True) for a list of WAV files -> WavPack.  All payloads in one pinned host buffer, one copy to the
    device, one table copy, one mg_pcm_decode_rows launch (two kernels with_moments) -- whatever the number of files and whatever
    their formats, channel counts and sampling rates.  No host read-back."""
    paths = [os.fspath(p) for p in paths]
    infos = [wav_info(p) for p in paths]
    plan = plan_read(infos, channels)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise _lib.HipLibraryError("read_wav_many decodes on the device (got %s); there is no CPU fallback" % device)
    data = stage_payloads(paths, infos, plan).to(device, non_blocking=True)
    table, = upload_tables([plan.rows], device)
    out = torch.zeros(plan.layout.total, dtype=torch.float32, device=device)
    _, moments = pcm_decode_rows(data, plan.rows, out, with_moments, table)
    return WavPack(out, plan.layout.starts, plan.layout.lengths, [infos[f].sample_rate for f in plan.file], plan.file,
                   plan.channel, moments, paths, infos)


def _as_packed(rows, device):
    """A list of waveforms, or a (buffer, starts, lengths) triple -> (float32 device buffer, starts, lengths)."""
    if isinstance(rows, tuple) and len(rows) == 3 and torch.is_tensor(rows[0]) and not torch.is_tensor(rows[1]):
        buf, starts, lengths = rows
        if buf.dtype != torch.float32 or not buf.is_cuda or not buf.is_contiguous():
            raise ValueError("write_wav_many: a packed buffer is a contiguous float32 device tensor")
        return buf.view(-1), [int(s) for s in starts], [int(n) for n in lengths]
    rows = list(rows)
    if not rows:
        raise ValueError("write_wav_many: no waveforms")
    if device is None:
        device = next((w.device for w in rows if w.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    layout = aligned_layout([w.numel() for w in rows])
    return pack_waves(rows, layout, device), layout.starts, layout.lengths


def write_wav_many(paths, rows, rate, encoding: str = "PCM_F32", groups=None, device=None) -> List[int]:
    """torchaudio.save for many files.  rows: a list of waveforms ([T] or [1, T]) or a (buffer, starts, lengths) triple over a
    packed float32 device buffer; groups[f]: the rows that are the channels of paths[f], in channel order (default: row f alone);
    the rows of one file have equal lengths.  rate: one sampling rate, or one per file.  encoding: "PCM_F32" (the default: what
    torchaudio.save writes for a float32 tensor), "PCM_S16" or "PCM_S24" (round half to even, clamped, no dither).
    One mg_pcm_encode_rows launch, one copy back, then headers and payloads on the host.  -> per row, the number of samples that
    were clamped or NaN (a host list: the only read-back, after everything is queued)."""
    if encoding not in ENCODINGS:
        raise ValueError("encoding is one of %s (got %r)" % (sorted(ENCODINGS), encoding))
    code, paths = ENCODINGS[encoding], [os.fspath(p) for p in paths]
    buf, starts, lengths = _as_packed(rows, device)
    groups = [[r] for r in range(len(lengths))] if groups is None else [[int(r) for r in g] for g in groups]
    rates = [int(rate)] * len(paths) if np.ndim(rate) == 0 else [int(r) for r in rate]
    if not paths or len(groups) != len(paths) or len(rates) != len(paths):
        raise ValueError("write_wav_many needs one group of rows and one sampling rate per file, and at least one file")
    nb = SAMPLE_BYTES[code]
    table, byte_starts, pos, headers = [], [], 0, []
    for path, g, r in zip(paths, groups, rates):
        if not g or any(not 0 <= i < len(lengths) for i in g) or len({lengths[i] for i in g}) != 1:
            raise ValueError("%s: the channels of one file are rows of equal lengths (rows %s)" % (path, g))
        frames = lengths[g[0]]
        headers.append(wav_header(r, len(g), code, frames))
        byte_starts.append(pos)
        table += [(starts[i], frames, len(g), c, code, pos) for c, i in enumerate(g)]
        pos = _round_up(pos + frames * len(g) * nb, PAYLOAD_ALIGN)
    table = np.asarray(table, dtype=np.int64).reshape(-1, 6)
    # the payload bytes and, behind them, the int64 counts: one buffer, so ONE copy back
    raw = torch.empty(pos + 8 * table.shape[0], dtype=torch.uint8, device=buf.device)
    clipped = raw[pos:].view(torch.int64)
    pcm_encode_rows(buf, table, raw[:pos], clipped=clipped)
    host = torch.empty(raw.numel(), dtype=torch.uint8, pin_memory=True)
    host.copy_(raw, non_blocking=True)
    torch.cuda.current_stream(buf.device).synchronize()
    payload, counts = memoryview(host.numpy()), host[pos:].view(torch.int64).tolist()
    for path, g, head, s in zip(paths, groups, headers, byte_starts):
        n = lengths[g[0]] * len(g) * nb
        with open(path, "wb") as f:
            f.write(head)
            f.write(payload[s:s + n])
            if n & 1:
                f.write(b"\0")
    by_row = [0] * len(lengths)
    for (i, count) in zip([i for g in groups for i in g], counts):
        by_row[i] = count
    return by_row
