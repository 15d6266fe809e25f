"""mdctgan_amd.wavio on the host: the RIFF/WAVE parser and writer, the staging plan, the host-side refusals, and the numpy
restatement of the sample arithmetic that tests/test_wavio_gpu.py holds the kernels to.  Every WAV file is written here, at run
time, with struct (and stdlib wave where it can); every comparison is exact."""
import os
import struct
import wave

import numpy as np
import pytest
import torch

from mdctgan_amd import wavio
from mdctgan_amd.wavio import MG_PCM_F32, MG_PCM_F64, MG_PCM_S16, MG_PCM_S24, MG_PCM_S32, MG_PCM_U8, SAMPLE_BYTES

FORMATS = [MG_PCM_U8, MG_PCM_S16, MG_PCM_S24, MG_PCM_S32, MG_PCM_F32, MG_PCM_F64]
TAG = {MG_PCM_U8: 1, MG_PCM_S16: 1, MG_PCM_S24: 1, MG_PCM_S32: 1, MG_PCM_F32: 3, MG_PCM_F64: 3}
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


# ---------------------------------------------------------------------------------------------------------------------
# The numpy restatement (torchaudio.load(normalize=True) / torchaudio.save, as the issue states them)
# ---------------------------------------------------------------------------------------------------------------------
def np_decode(payload, code: int, channels: int) -> np.ndarray:
    """payload bytes (whole interleaved frames) -> float32 [channels, frames]."""
    b = np.frombuffer(bytes(payload), dtype=np.uint8)
    if code == MG_PCM_U8:
        x = (b.astype(np.int32) - 128).astype(np.float32) / np.float32(128)
    elif code == MG_PCM_S16:
        x = b.view("<i2").astype(np.float32) / np.float32(32768)
    elif code == MG_PCM_S24:
        t = b.reshape(-1, 3).astype(np.int32)
        v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) / np.float32(8388608)
    elif code == MG_PCM_S32:
        x = b.view("<i4").astype(np.float32) / np.float32(2147483648)
    elif code == MG_PCM_F32:
        x = b.view("<f4")
    else:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            x = b.view("<f8").astype(np.float32)
    return np.ascontiguousarray(x.reshape(-1, channels).T)


def np_quantise(x: np.ndarray, bits: int):
    """float32 -> (integer codes, clamped-or-NaN mask): clamp(rint(x 2^(bits - 1)), -2^(bits - 1), 2^(bits - 1) - 1), NaN -> 0."""
    s = np.float32(1 << (bits - 1))
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.rint(np.asarray(x, dtype=np.float32) * s)              # float32 product (exact), round half to even
    nan = np.isnan(y)
    y = np.where(nan, np.float32(0), y)
    bad = nan | (y > s - 1) | (y < -s)
    return np.clip(y, -s, s - 1).astype(np.int64), bad


def np_encode(x: np.ndarray, code: int):
    """float32 [channels, frames] -> (interleaved payload as uint8 array, clamped-or-NaN count per channel)."""
    x = np.asarray(x, dtype=np.float32)
    if code == MG_PCM_F32:
        return np.ascontiguousarray(x.T).astype("<f4").view(np.uint8).reshape(-1), [0] * x.shape[0]
    bits = 8 * SAMPLE_BYTES[code]
    q, bad = np_quantise(x, bits)
    q = np.ascontiguousarray(q.T).reshape(-1)
    if code == MG_PCM_S16:
        out = q.astype("<i2").view(np.uint8)
    else:
        out = np.stack([q & 0xff, (q >> 8) & 0xff, (q >> 16) & 0xff], axis=1).astype(np.uint8).reshape(-1)
    return out, bad.sum(axis=1).tolist()


def bits_equal(a, b) -> bool:
    """float32 arrays / tensors, NaN payloads included."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def payload_for(code: int, channels: int, frames: int, seed: int = 0) -> bytes:
    """Random frames with the format's extremes (and, for the float formats, NaN / +-inf / subnormal payloads; for S32, values
    that need rounding) in front, as far as they fit."""
    rng = np.random.default_rng(seed + 17 * code + channels)
    n = frames * channels
    if code == MG_PCM_U8:
        v = rng.integers(0, 256, n, dtype=np.uint8)
        v[:min(n, 3)] = np.asarray([0, 255, 128], dtype=np.uint8)[:min(n, 3)]
        return v.tobytes()
    if code == MG_PCM_S16:
        v = rng.integers(-32768, 32768, n).astype("<i2")
        v[:min(n, 4)] = np.asarray([-32768, 32767, 0, -1], dtype="<i2")[:min(n, 4)]
        return v.tobytes()
    if code == MG_PCM_S24:
        v = rng.integers(-(1 << 23), 1 << 23, n)
        v[:min(n, 4)] = np.asarray([-(1 << 23), (1 << 23) - 1, 0, -1])[:min(n, 4)]
        return np.stack([v & 0xff, (v >> 8) & 0xff, (v >> 16) & 0xff], axis=1).astype(np.uint8).tobytes()
    if code == MG_PCM_S32:
        v = rng.integers(-(1 << 31), 1 << 31, n).astype("<i4")
        head = np.asarray([-(1 << 31), (1 << 31) - 1, (1 << 24) + 1, (1 << 24) + 3, -(1 << 25) - 2, (1 << 31) - 65, 0x7fffffc0, 1],
                          dtype="<i4")
        v[:min(n, 8)] = head[:min(n, 8)]
        return v.tobytes()
    if code == MG_PCM_F32:
        v = rng.standard_normal(n).astype("<f4").view(np.uint32)
        head = np.asarray([0x7fc00000, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x80000000, 0x7f7fffff],
                          dtype=np.uint32)
        v[:min(n, 9)] = head[:min(n, 9)]
        return v.astype("<u4").tobytes()
    v = rng.standard_normal(n).astype("<f8")
    head = np.asarray([np.nan, np.inf, -np.inf, 1e-40, -3e-45, 1e-320, 1e39, -1e39, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -0.0,
                       2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149], dtype="<f8")
    v[:min(n, head.size)] = head[:min(n, head.size)]
    return v.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# Writing test files with struct
# ---------------------------------------------------------------------------------------------------------------------
def chunk(cid: bytes, body: bytes, size=None) -> bytes:
    return struct.pack("<4sI", cid, len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def fmt_chunk(code, channels, rate, extensible=False, tag=None, bits=None, valid=None, block_align=None) -> bytes:
    bits = 8 * SAMPLE_BYTES[code] if bits is None else bits
    tag = TAG[code] if tag is None else tag
    block = channels * bits // 8 if block_align is None else block_align
    base = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block, block, bits)
    if extensible:
        base += struct.pack("<HHI", 22, bits if valid is None else valid, 0) + struct.pack("<H", tag) + GUID_TAIL
    elif tag != 1:
        base += struct.pack("<H", 0)
    return chunk(b"fmt ", base)


def write_wav(path, code, channels, rate, payload: bytes, variant="plain", **fmt_kw):
    """The accepted header variants of the issue, by name."""
    fmt = fmt_chunk(code, channels, rate, extensible=(variant == "extensible"), **fmt_kw)
    data = chunk(b"data", payload)
    tail = b""
    if variant in ("plain", "extensible"):
        body = fmt + data
    elif variant == "list_before":
        body = fmt + chunk(b"LIST", b"INFOISFT\x05\0\0\0abcd\0\0") + data
    elif variant == "odd_chunk_pad":
        body = fmt + chunk(b"fact", struct.pack("<I", 1)) + chunk(b"bext", b"odd") + data
    elif variant == "chunks_after":
        body = fmt + data + chunk(b"LIST", b"INFO") + chunk(b"id3 ", b"xyz")
    elif variant == "data_first":
        body = chunk(b"JUNK", b"1234567") + data + chunk(b"fact", struct.pack("<I", 1)) + fmt
    elif variant == "size_zero":
        body = fmt + struct.pack("<4sI", b"data", 0) + payload
    elif variant == "size_ffffffff":
        body = fmt + struct.pack("<4sI", b"data", 0xFFFFFFFF) + payload
    elif variant == "size_past_end":
        body = fmt + struct.pack("<4sI", b"data", len(payload) + 1000) + payload
        tail = b"\x01" * (channels * SAMPLE_BYTES[code] - 1)               # a partial frame: whole frames only
    else:
        raise AssertionError(variant)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sI4s", b"RIFF", 4 + len(body) + len(tail), b"WAVE") + body + tail)
    return path


VARIANTS = ["plain", "extensible", "list_before", "odd_chunk_pad", "chunks_after", "data_first", "size_zero", "size_ffffffff",
            "size_past_end"]


def parse_wav(path):
    """The tests' own reader: (tag, channels, rate, bits, payload bytes, chunk ids) of a well-formed file; every size is checked."""
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8
    pos, found, ids = 12, {}, []
    while pos < len(raw):
        cid, n = struct.unpack("<4sI", raw[pos:pos + 8])
        found[cid] = raw[pos + 8:pos + 8 + n]
        assert len(found[cid]) == n
        ids.append(cid)
        pos += 8 + n + (n & 1)
    assert pos == len(raw)
    fmt = found[b"fmt "]
    tag, channels, rate, byte_rate, block, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE:
        assert len(fmt) == 40 and struct.unpack("<HH", fmt[16:20]) == (22, bits) and fmt[26:40] == GUID_TAIL
        tag, = struct.unpack("<H", fmt[24:26])
    assert block == channels * bits // 8 and byte_rate == rate * block and len(found[b"data"]) % block == 0
    if tag == 3:
        assert struct.unpack("<I", found[b"fact"])[0] == len(found[b"data"]) // block
    return tag, channels, rate, bits, found[b"data"], ids


# ---------------------------------------------------------------------------------------------------------------------
# 1. wav_info
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("code", FORMATS)
def test_wav_info_accepts(tmp_path, code, variant):
    channels, frames, rate = (3 if code == MG_PCM_S24 else 2), 37, 22050
    payload = payload_for(code, channels, frames)
    path = write_wav(str(tmp_path / "a.wav"), code, channels, rate, payload, variant)
    info = wavio.wav_info(path)
    assert info[:5] == (rate, frames, channels, 8 * SAMPLE_BYTES[code], TAG[code]) and info.format == code
    assert info.data_bytes == len(payload)
    assert open(path, "rb").read()[info.data_offset:info.data_offset + info.data_bytes] == payload


@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("channels", [1, 2])
def test_wav_info_agrees_with_stdlib_wave(tmp_path, width, channels):
    path = str(tmp_path / "w.wav")
    code = {1: MG_PCM_U8, 2: MG_PCM_S16, 3: MG_PCM_S24, 4: MG_PCM_S32}[width]
    payload = payload_for(code, channels, 101)
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(16000)
        w.writeframes(payload)
    info = wavio.wav_info(path)
    with wave.open(path, "rb") as w:
        assert (info.sample_rate, info.num_frames, info.num_channels, info.bits) == (w.getframerate(), w.getnframes(),
                                                                                   w.getnchannels(), 8 * w.getsampwidth())
        assert w.readframes(w.getnframes()) == payload
    assert info.fmt == 1 and info.format == code
    # ... and stdlib wave reads what wav_header writes for plain PCM
    with open(path, "wb") as f:
        f.write(wavio.wav_header(16000, channels, code, 101) + payload + (b"\0" if len(payload) & 1 else b""))
    with wave.open(path, "rb") as w:
        assert (w.getframerate(), w.getnframes(), w.getnchannels(), w.getsampwidth()) == (16000, 101, channels, width)
        assert w.readframes(101) == payload


def _riff(body: bytes, magic=b"RIFF", form=b"WAVE") -> bytes:
    return struct.pack("<4sI4s", magic, 4 + len(body), form) + body


REJECTED = {
    "not RIFF/WAVE": lambda: b"OggS" + b"\0" * 40,
    "not RIFF/WAVE ": lambda: _riff(fmt_chunk(MG_PCM_S16, 1, 8000) + chunk(b"data", b"\0\0"), form=b"AVI "),
    "RIFX": lambda: _riff(fmt_chunk(MG_PCM_S16, 1, 8000) + chunk(b"data", b"\0\0"), magic=b"RIFX"),
    "RF64": lambda: _riff(fmt_chunk(MG_PCM_S16, 1, 8000) + chunk(b"data", b"\0\0"), magic=b"RF64"),
    "no 'fmt '": lambda: _riff(chunk(b"LIST", b"INFO") + chunk(b"data", b"\0\0")),
    "no 'data'": lambda: _riff(fmt_chunk(MG_PCM_S16, 1, 8000) + chunk(b"LIST", b"INFO")),
    "A-law": lambda: _riff(fmt_chunk(MG_PCM_U8, 1, 8000, tag=6) + chunk(b"data", b"\0\0")),
    "mu-law": lambda: _riff(fmt_chunk(MG_PCM_U8, 1, 8000, tag=7) + chunk(b"data", b"\0\0")),
    "ADPCM": lambda: _riff(fmt_chunk(MG_PCM_S16, 1, 8000, tag=2) + chunk(b"data", b"\0\0")),
    "MPEG": lambda: _riff(fmt_chunk(MG_PCM_S16, 1, 8000, tag=0x55) + chunk(b"data", b"\0\0")),
    "compressed": lambda: _riff(fmt_chunk(MG_PCM_U8, 1, 8000, tag=7, extensible=True) + chunk(b"data", b"\0\0")),
    "0 channels": lambda: _riff(fmt_chunk(MG_PCM_S16, 0, 8000) + chunk(b"data", b"\0\0")),
    "block_align": lambda: _riff(fmt_chunk(MG_PCM_S16, 2, 8000, block_align=2) + chunk(b"data", b"\0\0\0\0")),
    "20 valid bits": lambda: _riff(fmt_chunk(MG_PCM_S24, 1, 8000, extensible=True, valid=20) + chunk(b"data", b"\0\0\0")),
    "zero frames": lambda: _riff(fmt_chunk(MG_PCM_S16, 2, 8000) + chunk(b"data", b"\0\0")),
    "zero frames ": lambda: _riff(fmt_chunk(MG_PCM_S16, 1, 8000) + struct.pack("<4sI", b"data", 0)),
    "12-bit": lambda: _riff(fmt_chunk(MG_PCM_S16, 1, 8000, bits=12, block_align=1) + chunk(b"data", b"\0\0")),
    "16-bit float": lambda: _riff(fmt_chunk(MG_PCM_S16, 1, 8000, tag=3) + chunk(b"data", b"\0\0")),
}


@pytest.mark.parametrize("reason", sorted(REJECTED))
def test_wav_info_rejects(tmp_path, reason):
    path = str(tmp_path / "bad.wav")
    with open(path, "wb") as f:
        f.write(REJECTED[reason]())
    with pytest.raises(ValueError) as e:
        wavio.wav_info(path)
    assert path in str(e.value)
    want = {"compressed": "compressed", "20 valid bits": "20 valid bits", "12-bit": "12-bit", "16-bit float": "16-bit float",
            "ADPCM": "ADPCM", "MPEG": "MPEG"}.get(reason, reason.strip())
    assert want in str(e.value), str(e.value)


@pytest.mark.parametrize("name", ["a.mp3", "b.FLAC"])
def test_mp3_and_flac_are_out_of_scope(tmp_path, name):
    path = str(tmp_path / name)
    open(path, "wb").write(b"\0" * 64)
    with pytest.raises(ValueError, match="out of scope"):
        wavio.wav_info(path)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the staging plan and the writer
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_read_alignment_and_layout():
    from mdctgan_amd.packed import aligned_layout
    infos = [wavio.WavInfo(48000, 1001, 1, 16, 1, 44, 2002), wavio.WavInfo(44100, 7, 3, 24, 1, 80, 63),
             wavio.WavInfo(8000, 4097, 2, 32, 3, 58, 4097 * 8), wavio.WavInfo(16000, 1, 1, 8, 1, 44, 1)]
    for channels, file, channel in (("first", [0, 1, 2, 3], [0, 0, 0, 0]), ("all", [0, 1, 1, 1, 2, 2, 3], [0, 0, 1, 2, 0, 1, 0])):
        plan = wavio.plan_read(infos, channels)
        assert plan.file == file and plan.channel == channel
        assert all(s % 16 == 0 for s in plan.byte_starts) and plan.bytes_total % 16 == 0
        ends = [s + i.data_bytes for s, i in zip(plan.byte_starts, infos)]
        assert all(e <= s for e, s in zip(ends, plan.byte_starts[1:] + [plan.bytes_total]))
        assert plan.layout == aligned_layout([infos[f].num_frames for f in file])
        want = [(plan.byte_starts[f], infos[f].num_frames, infos[f].num_channels, c, infos[f].format, s)
                for f, c, s in zip(file, channel, plan.layout.starts)]
        assert plan.rows.dtype == np.int64 and plan.rows.tolist() == [list(r) for r in want]
    with pytest.raises(ValueError):
        wavio.plan_read(infos, "mix")
    with pytest.raises(ValueError):
        wavio.plan_read([])


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
@pytest.mark.parametrize("code", FORMATS)
def test_writer_headers_parse_back(tmp_path, code, channels):
    frames, rate = 5, 44100
    payload = payload_for(code, channels, frames)
    head = wavio.wav_header(rate, channels, code, frames)
    path = str(tmp_path / "h.wav")
    with open(path, "wb") as f:
        f.write(head + payload + (b"\0" if len(payload) & 1 else b""))
    info = wavio.wav_info(path)
    assert info == wavio.WavInfo(rate, frames, channels, 8 * SAMPLE_BYTES[code], TAG[code], len(head), len(payload))
    tag, ch, r, bits, data, ids = parse_wav(path)
    assert (tag, ch, r, bits, data) == (TAG[code], channels, rate, 8 * SAMPLE_BYTES[code], payload)
    assert (b"fact" in ids) == (TAG[code] == 3)
    raw_tag, = struct.unpack("<H", head[20:22])
    assert raw_tag == (0xFFFE if channels > 2 else TAG[code])


def test_writer_refuses_nonsense():
    for args in ((0, 1, MG_PCM_S16, 4), (8000, 0, MG_PCM_S16, 4), (8000, 1, MG_PCM_S16, 0), (8000, 1, 9, 4),
                 (8000, 1, MG_PCM_F32, 1 << 30)):
        with pytest.raises(ValueError):
            wavio.wav_header(*args)


def test_row_tables_are_checked_on_the_host():
    ok = np.asarray([(0, 10, 2, 1, MG_PCM_S16, 64)], dtype=np.int64)
    assert wavio._check_rows("t", ok, 40, 74, 0, 5, list(range(6))).shape == (1, 6)
    for bad, exc in (((0, 11, 2, 1, MG_PCM_S16, 64), ValueError),          # 44 bytes of 40
                     ((-2, 10, 2, 1, MG_PCM_S16, 64), ValueError), ((0, 10, 2, 1, MG_PCM_S16, 65), ValueError),
                     ((0, 10, 2, 2, MG_PCM_S16, 64), ValueError), ((0, 10, 0, 0, MG_PCM_S16, 64), ValueError),
                     ((0, 0, 2, 1, MG_PCM_S16, 64), ValueError), ((0, 10, 2, 1, 6, 64), ValueError),
                     ((0, 10, 2, 1, -1, 64), ValueError)):
        with pytest.raises(exc):
            wavio._check_rows("t", np.asarray([bad], dtype=np.int64), 40, 74, 0, 5, list(range(6)))
    with pytest.raises(ValueError):
        wavio._check_rows("t", np.zeros((0, 6), dtype=np.int64), 40, 74, 0, 5, list(range(6)))
    with pytest.raises(ValueError):
        wavio._check_rows("t", np.zeros((1, 5), dtype=np.int64), 40, 74, 0, 5, list(range(6)))
    # the encoder writes F32, S16 and S24 only: MG_ERR_UNSUPPORTED's exception for the rest
    for code in (MG_PCM_U8, MG_PCM_S32, MG_PCM_F64):
        with pytest.raises(NotImplementedError):
            wavio._check_rows("t", np.asarray([(0, 1, 1, 0, code, 0)], dtype=np.int64), 64, 64, 5, 0,
                              sorted(wavio.ENCODINGS.values()))


def test_write_wav_many_refuses_before_any_launch(tmp_path):
    x = [torch.zeros(8), torch.zeros(9)]
    with pytest.raises(ValueError, match="encoding"):
        wavio.write_wav_many([str(tmp_path / "a.wav")], x, 8000, "PCM_S32")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_s16_round_trip_all_codes():
    codes = np.arange(-32768, 32768).astype("<i2")
    x = np_decode(codes.tobytes(), MG_PCM_S16, 1)
    assert np.array_equal(x[0].astype(np.float64) * 32768, codes.astype(np.float64))          # exact
    back, clipped = np_encode(x, MG_PCM_S16)
    assert back.tobytes() == codes.tobytes() and clipped == [0]


def test_restatement_s24_round_trip():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.integers(-(1 << 23), 1 << 23, 1 << 20), [-(1 << 23), (1 << 23) - 1, 0, -1, 1]])
    payload = np.stack([v & 0xff, (v >> 8) & 0xff, (v >> 16) & 0xff], axis=1).astype(np.uint8).tobytes()
    x = np_decode(payload, MG_PCM_S24, 1)
    assert np.array_equal(x[0].astype(np.float64) * 8388608, v.astype(np.float64))            # exact
    back, clipped = np_encode(x, MG_PCM_S24)
    assert back.tobytes() == payload and clipped == [0]


def test_restatement_ties_and_clamps():
    u = np.float32(2.0 ** -15)
    q, bad = np_quantise(np.asarray([0.5, 1.5, 2.5, -0.5, -1.5], dtype=np.float32) * u, 16)
    assert q.tolist() == [0, 2, 2, 0, -2] and not bad.any()
    x = np.asarray([32767.5 / 32768, 1.0, 7.0, np.inf, -32768.5 / 32768, -1.5, -np.inf, 32767.25 / 32768, -1.0, np.nan],
                   dtype=np.float32)
    q, bad = np_quantise(x, 16)
    assert q.tolist() == [32767, 32767, 32767, 32767, -32768, -32768, -32768, 32767, -32768, 0]
    # (-32768.5 ties to the even -32768, which is in range: the value the issue names, and nothing was clamped)
    assert bad.tolist() == [True, True, True, True, False, True, True, False, False, True]
    q, bad = np_quantise(np.asarray([8388607.5 / 8388608, -8388608.5 / 8388608, 8388607 / 8388608], dtype=np.float32), 24)
    assert q.tolist() == [8388607, -8388608, 8388607] and bad.tolist() == [True, False, False]
    # (-8388608.5 is no float32: it is -8388608 before the product, and in range)


def test_restatement_s32_is_one_rounding():
    rng = np.random.default_rng(11)
    v = np.concatenate([rng.integers(-(1 << 31), 1 << 31, 2_000_000), [-(1 << 31), (1 << 31) - 1, (1 << 24) + 1, (1 << 24) + 3]])
    v = v.astype("<i4")
    x = np_decode(v.tobytes(), MG_PCM_S32, 1)[0]
    t = (torch.from_numpy(v.astype(np.int32)).to(torch.float32) / 2147483648).numpy()
    assert np.array_equal(x, t)
    assert np.array_equal(x, (v.astype(np.float64) / 2147483648.0).astype(np.float32))


def test_restatement_other_formats():
    assert np_decode(bytes([0, 128, 255]), MG_PCM_U8, 1)[0].tolist() == [-1.0, 0.0, 127 / 128]
    f = np.asarray([0x7fc00001, 0x00000001, 0xff800000], dtype="<u4")
    assert np_decode(f.tobytes(), MG_PCM_F32, 1).view(np.uint32).tolist() == [f.tolist()]
    d = np.asarray([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e39, 2.0 ** -150, 1.5 * 2.0 ** -149], dtype="<f8")   # ties to even
    assert np_decode(d.tobytes(), MG_PCM_F64, 1)[0].tolist() == [1.0, 1.0 + 2.0 ** -22, np.inf, 0.0, 2.0 ** -148]
    st = np_decode(np.asarray([1, -2, 3, -4], dtype="<i2").tobytes(), MG_PCM_S16, 2)
    assert (st * 32768).tolist() == [[1, 3], [-2, -4]]
    back, _ = np_encode(st, MG_PCM_S16)
    assert back.view("<i2").tolist() == [1, -2, 3, -4]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the host side of the paths over files
# ---------------------------------------------------------------------------------------------------------------------
def test_command_line_flags_and_file_lists(tmp_path):
    from mdctgan_amd import options
    from mdctgan_amd.generate_audio import _output_paths, input_files
    opt = options.make_opt("--gpu_ids", "-1")
    assert (opt.input, opt.output_dir, opt.channels, opt.out_encoding, opt.metrics) == ("", "", "all", "PCM_F32", False)
    opt = options.make_opt("--gpu_ids", "-1", "--input", "x", "--output_dir", "y", "--channels", "first", "--out_encoding",
                           "PCM_S24", "--metrics")
    assert (opt.input, opt.output_dir, opt.channels, opt.out_encoding, opt.metrics) == ("x", "y", "first", "PCM_S24", True)
    with pytest.raises(SystemExit):
        options.make_opt("--out_encoding", "PCM_U8")
    (tmp_path / "d" / "sub").mkdir(parents=True)
    for name in ("d/b.wav", "d/a.WAV", "d/sub/c.wav", "d/skip.mp3", "d/notes.txt"):
        (tmp_path / name).write_bytes(b"")
    got = input_files(tmp_path / "d")
    assert sorted(os.path.relpath(p, tmp_path) for p in got) == ["d/a.WAV", "d/b.wav", "d/sub/c.wav"]
    assert input_files(tmp_path / "d" / "b.wav") == [str(tmp_path / "d" / "b.wav")]
    (tmp_path / "list.csv").write_text("d/b.wav,d/sub/c.wav\nd/a.WAV\n")
    assert input_files(tmp_path / "list.csv") == [str(tmp_path / n) for n in ("d/b.wav", "d/sub/c.wav", "d/a.WAV")]
    assert _output_paths(["x/a.wav", "y/b.wav"], "out") == [os.path.join("out", "a.wav"), os.path.join("out", "b.wav")]
    with pytest.raises(ValueError, match="a.wav"):
        _output_paths(["x/a.wav", "y/a.wav"], "out")


def test_front_end_many_tells_packed_input_from_a_list():
    from mdctgan_amd.resample import _prepacked
    assert _prepacked([torch.zeros(4), torch.zeros(5), torch.zeros(6)]) is None
    assert _prepacked((torch.zeros(4), torch.zeros(5), torch.zeros(6))) is None
    with pytest.raises(ValueError):                                  # a packed buffer lives on the device
        _prepacked((torch.zeros(64), [0], [4]))


def test_scipy_reads_what_the_writer_writes(tmp_path):
    """A second reader, where it is installed."""
    wavfile = pytest.importorskip("scipy.io.wavfile")
    for code, dtype in ((MG_PCM_S16, "<i2"), (MG_PCM_F32, "<f4")):
        payload = np.random.default_rng(code).integers(-3000, 3000, 2 * 50).astype("<i2").astype(dtype).tobytes()
        path = str(tmp_path / ("s%d.wav" % code))
        with open(path, "wb") as f:
            f.write(wavio.wav_header(22050, 2, code, 50) + payload)
        rate, data = wavfile.read(path)
        assert rate == 22050 and data.shape == (50, 2) and data.astype(dtype).tobytes() == payload
