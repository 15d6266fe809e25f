"""WAV files in, WAV files out on the MI355X: mg_pcm_decode_rows, mg_pcm_encode_rows, wavio.read_wav_many / write_wav_many, the packed
front end from a WavPack, pack_corpus_files, super_resolve_files, evaluate_files and the command line.  Expected values are the
numpy restatement of tests/test_wavio_host.py; every comparison is bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_wavio_host import FORMATS, bits_equal, np_decode, np_encode, parse_wav, payload_for, write_wav
from mdctgan_amd.wavio import MG_PCM_F32, MG_PCM_S16, MG_PCM_S24, SAMPLE_BYTES

pytestmark = pytest.mark.gpu

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096                                     # MG_MOMENTS_CHUNK
LENGTHS = [1, 3, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
LAYOUTS = [(1, (0,)), (2, (0, 1)), (3, (0, 2))]  # channels, the rows taken: channel 0 and the last channel
GUARD, SENTINEL = 64, 1234.5


def _lib():
    from mdctgan_amd import _lib as L
    return L


def test_chunk_constant_is_the_header_s():
    text = open(os.path.join(REPO, "include", "mdctgan_hip.h")).read()
    assert "#define MG_MOMENTS_CHUNK %d\n" % CHUNK in text


def stage(payloads, shift=0):
    """Payloads at 16-byte aligned offsets (+ shift) of one byte buffer -> (uint8 array, starts)."""
    starts, pos = [], shift
    for p in payloads:
        starts.append(pos)
        pos = -(-(pos + len(p) - shift) // 16) * 16 + shift
    buf = np.zeros(pos + 16, dtype=np.uint8)
    for p, s in zip(payloads, starts):
        buf[s:s + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return buf, starts


def decode_case(formats=FORMATS, lengths=LENGTHS, shift=0, sample_shift=0, seed=0):
    """Every format x channel layout x length as one table: (bytes, rows int64 [n, 6], expected float32 rows, out_total)."""
    from mdctgan_amd.packed import aligned_layout
    files = [(code, ch, take, n) for code in formats for ch, take in LAYOUTS for n in lengths]
    payloads = [payload_for(code, ch, n, seed) for code, ch, _, n in files]
    data, starts = stage(payloads, shift)
    rows, want = [], []
    for (code, ch, take, n), p, s in zip(files, payloads, starts):
        x = np_decode(p, code, ch)
        for c in take:
            rows.append([s, n, ch, c, code, 0])
            want.append(x[c])
    layout = aligned_layout([r[1] for r in rows])
    for r, s in zip(rows, layout.starts):
        r[5] = s + sample_shift
    return data, np.asarray(rows, dtype=np.int64), want, layout.total + sample_shift


def raw_decode(data_t, rows, out_total, with_moments=True, prefill=0.0):
    """mg_pcm_decode_rows itself, its output, moments and workspace views into buffers with GUARD sentinels behind them."""
    L = _lib()
    lib = L.load()
    n, longest = rows.shape[0], int(rows[:, 1].max())
    big_out = torch.full((out_total + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    out = big_out[:out_total]
    out.fill_(prefill)
    nbytes = lib.mg_pcm_decode_rows_workspace(n, longest)
    assert nbytes == n * (-(-longest // CHUNK)) * 16
    big_ws = torch.full((nbytes // 8 + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    big_m = torch.full((2 * n + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    if prefill != prefill:
        big_ws[:nbytes // 8] = prefill
        big_m[:2 * n] = prefill
    table = torch.from_numpy(rows).to(DEV)
    rc = lib.mg_pcm_decode_rows(L.ptr(data_t), data_t.numel(), L.ptr(table), n, longest, L.ptr(out), out_total,
                                L.ptr(big_m) if with_moments else None, L.ptr(big_ws) if with_moments else None,
                                nbytes if with_moments else 0, L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (big_out[out_total:] == SENTINEL).all() and (big_ws[nbytes // 8:] == SENTINEL).all() and (big_m[2 * n:] == SENTINEL).all()
    if not with_moments:
        assert (big_m == SENTINEL).all() and (big_ws == SENTINEL).all()
    return out, big_m[:2 * n].view(n, 2)


def windows(rows):
    from mdctgan_amd.packed import window_table
    return torch.from_numpy(window_table(rows[:, 5], rows[:, 1])).to(DEV)


def check_rows(out, rows, want):
    got = out.cpu().numpy()
    covered = np.zeros(got.size, dtype=bool)
    for r, w in zip(rows, want):
        assert bits_equal(got[r[5]:r[5] + r[1]], w), r
        covered[r[5]:r[5] + r[1]] = True
    return got, covered


@pytest.fixture(scope="module")
def full_case():
    data, rows, want, total = decode_case()
    return torch.from_numpy(data).to(DEV), rows, want, total


# ---------------------------------------------------------------------------------------------------------------------
# 1. decode
# ---------------------------------------------------------------------------------------------------------------------
def test_decode_every_format_layout_and_length(full_case):
    """Six formats x (mono, stereo, 3 channels; channel 0 and the last) x seven lengths around the chunk, in ONE launch: the
    restatement's bits, zero gaps, rows_moments' bits, nothing written behind any buffer; a second call on NaN-filled outputs
    gives the same bits."""
    from mdctgan_amd.packed import rows_moments
    data, rows, want, total = full_case
    assert rows.shape[0] == 6 * 5 * 7
    out, mom = raw_decode(data, rows, total)
    got, covered = check_rows(out, rows, want)
    assert not got[~covered].any()                                   # the gaps of the packed buffer stay zero
    ref = rows_moments(out, windows(rows), int(rows[:, 1].max()))
    assert torch.equal(mom.view(torch.int64), ref.view(torch.int64))
    finite = torch.isfinite(ref).all(dim=1).cpu().numpy()
    assert finite.sum() > 100                                        # (rows with NaN / inf payloads aside, these are numbers ...)
    with np.errstate(invalid="ignore", over="ignore"):
        sums = np.asarray([[np.sum(w, dtype=np.float64), np.sum(w.astype(np.float64) ** 2)] for w in want])
    np.testing.assert_allclose(mom.cpu().numpy()[finite], sums[finite], rtol=1e-9, atol=1e-9)   # (... the right ones: a sanity check)
    out2, mom2 = raw_decode(data, rows, total, prefill=float("nan"))
    check_rows(out2, rows, want)
    assert torch.equal(mom2.view(torch.int64), mom.view(torch.int64))
    assert torch.isnan(out2[torch.from_numpy(~covered).to(DEV)]).all()       # (and the gaps were not touched)
    out3, _ = raw_decode(data, rows, total, with_moments=False)
    assert torch.equal(out3.view(torch.int32), out.view(torch.int32))


def test_decode_row_alone_has_the_bits_of_the_pack(full_case):
    data, rows, want, total = full_case
    out, mom = raw_decode(data, rows, total)
    host = data.cpu().numpy()
    for i, r in enumerate(rows):
        if r[1] not in (3, CHUNK + 1, 2 * CHUNK + 5):
            continue
        nbytes = int(r[1] * r[2] * SAMPLE_BYTES[int(r[4])])
        alone = torch.from_numpy(host[r[0]:r[0] + nbytes].copy()).to(DEV)
        one = np.asarray([[0, r[1], r[2], r[3], r[4], 0]], dtype=np.int64)
        o, m = raw_decode(alone, one, int(r[1]))
        assert torch.equal(o.view(torch.int32), out[r[5]:r[5] + r[1]].view(torch.int32)), r
        assert torch.equal(m.view(torch.int64), mom[i:i + 1].view(torch.int64)), r


@pytest.mark.parametrize("shift,sample_shift", [(1, 1), (2, 3), (4, 2), (8, 0)])
def test_decode_unaligned_payloads_and_outputs(shift, sample_shift):
    """Payloads that do not start on 16 bytes and rows that do not start on 4 samples take the narrower loads and scalar stores:
    the same bits."""
    from mdctgan_amd.packed import rows_moments
    data, rows, want, total = decode_case(lengths=[3, 1023, CHUNK + 1], shift=shift, sample_shift=sample_shift, seed=shift)
    out, mom = raw_decode(torch.from_numpy(data).to(DEV), rows, total)
    check_rows(out, rows, want)
    ref = rows_moments(out, windows(rows), int(rows[:, 1].max()))
    assert torch.equal(mom.view(torch.int64), ref.view(torch.int64))


def test_decode_wrapper_checks_its_arguments(full_case):
    from mdctgan_amd import wavio
    data, rows, want, total = full_case
    out = torch.zeros(total, device=DEV)
    got, mom = wavio.pcm_decode_rows(data, rows, out, with_moments=True)
    assert got is out and mom.shape == (rows.shape[0], 2)
    check_rows(out, rows, want)
    assert wavio.pcm_decode_rows(data, rows, out)[1] is None
    with pytest.raises(ValueError):
        wavio.pcm_decode_rows(data.float(), rows, out)
    with pytest.raises(ValueError):
        wavio.pcm_decode_rows(data, rows, out.double())
    with pytest.raises(ValueError):
        wavio.pcm_decode_rows(data, rows, out, table=torch.from_numpy(rows[:, :5].copy()).to(DEV))
    with pytest.raises(ValueError):                                  # a row that leaves the float buffer is refused on the host
        wavio.pcm_decode_rows(data, rows, out[:total - 64])


# ---------------------------------------------------------------------------------------------------------------------
# 2. encode
# ---------------------------------------------------------------------------------------------------------------------
ENC_LENGTHS = [1, 3, 1023, CHUNK + 1, 2 * CHUNK + 5]
SPECIAL = np.asarray([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 32767.5 / 32768, 1.0, -32768.5 / 32768,
                      -1.0, 7.0, np.nan, np.inf, -np.inf, 0.5 / 8388608, 1.5 / 8388608, 8388607.5 / 8388608, -0.0, 1e-42],
                     dtype=np.float32)


def encode_case(seed=1):
    from mdctgan_amd.packed import aligned_layout
    rng = np.random.default_rng(seed)
    files = [(code, ch, n) for code in (MG_PCM_F32, MG_PCM_S16, MG_PCM_S24) for ch in (1, 3) for n in ENC_LENGTHS]
    waves, groups = [], []
    for code, ch, n in files:
        x = (0.6 * rng.standard_normal((ch, n))).astype(np.float32)          # (some of it beyond +-1)
        for c in range(ch):
            k = min(n, SPECIAL.size)
            x[c, :k] = np.roll(SPECIAL, c)[:k]
        groups.append(list(range(len(waves), len(waves) + ch)))
        waves += [x[c] for c in range(ch)]
    layout = aligned_layout([w.size for w in waves])
    buf = np.zeros(layout.total, dtype=np.float32)
    for w, s in zip(waves, layout.starts):
        buf[s:s + w.size] = w
    rows, byte_starts, pos = [], [], 0
    for (code, ch, n), g in zip(files, groups):
        byte_starts.append(pos)
        rows += [(layout.starts[i], n, ch, c, code, pos) for c, i in enumerate(g)]
        pos = -(-(pos + n * ch * SAMPLE_BYTES[code]) // 16) * 16
    return files, waves, groups, buf, np.asarray(rows, dtype=np.int64), byte_starts, pos


def test_encode_bytes_and_clipped_counts():
    from mdctgan_amd import wavio
    files, waves, groups, buf, rows, byte_starts, total = encode_case()
    x = torch.from_numpy(buf).to(DEV)
    big = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    clipped = wavio.pcm_encode_rows(x, rows, big[:total])
    torch.cuda.synchronize()
    got, covered = big.cpu().numpy(), np.zeros(total + GUARD, dtype=bool)
    want_clipped = []
    for (code, ch, n), g, s in zip(files, groups, byte_starts):
        want, counts = np_encode(np.stack([waves[i] for i in g]), code)
        assert np.array_equal(got[s:s + want.size], want), (code, ch, n)
        covered[s:s + want.size] = True
        want_clipped += counts
    assert (got[~covered] == 0xA5).all()                             # the bytes between payloads and behind the buffer
    assert clipped.tolist() == want_clipped and sum(want_clipped) > 50
    assert wavio.pcm_encode_rows(x, rows, big[:total]).tolist() == want_clipped          # run to run
    with pytest.raises(NotImplementedError):
        bad = rows.copy()
        bad[0, 4] = wavio.MG_PCM_S32
        wavio.pcm_encode_rows(x, bad, big[:total])
    with pytest.raises(ValueError):
        wavio.pcm_encode_rows(x, rows, big[:total - 16])


@pytest.mark.parametrize("code", [MG_PCM_S16, MG_PCM_S24])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_decode_encode_decode_returns_the_payload(code, channels):
    from mdctgan_amd import wavio
    from mdctgan_amd.packed import aligned_layout
    n = CHUNK + 37
    payload = payload_for(code, channels, n, seed=9)
    data = torch.from_numpy(np.frombuffer(payload, dtype=np.uint8).copy()).to(DEV)
    layout = aligned_layout([n] * channels)
    dec = np.asarray([(0, n, channels, c, code, s) for c, s in enumerate(layout.starts)], dtype=np.int64)
    x = torch.zeros(layout.total, device=DEV)
    wavio.pcm_decode_rows(data, dec, x)
    enc = np.asarray([(s, n, channels, c, code, 0) for c, s in enumerate(layout.starts)], dtype=np.int64)
    back = torch.zeros(len(payload), dtype=torch.uint8, device=DEV)
    clipped = wavio.pcm_encode_rows(x, enc, back)
    assert back.cpu().numpy().tobytes() == payload and clipped.tolist() == [0] * channels
    x2 = torch.zeros_like(x)
    wavio.pcm_decode_rows(back, dec, x2)
    assert torch.equal(x2, x)


# ---------------------------------------------------------------------------------------------------------------------
# 3. files
# ---------------------------------------------------------------------------------------------------------------------
MIXED = [  # name, format, channels, rate, frames, header variant
    ("a.wav", MG_PCM_S16, 1, 48000, 5000, "plain"), ("b.wav", MG_PCM_F32, 2, 16000, 3001, "list_before"),
    ("c.wav", MG_PCM_S24, 1, 44100, 4500, "odd_chunk_pad"), ("d.wav", MG_PCM_S16, 1, 16000, 2000, "size_past_end"),
]


def audio_payload(code, channels, frames, seed):
    """Audio-like content (no NaN): a restatement-decodable payload of moderate level."""
    rng = np.random.default_rng(seed)
    x = (0.1 * rng.standard_normal((channels, frames))).astype(np.float32)
    return np_encode(x, code)[0].tobytes()


def write_mixed(tmp_path, spec=MIXED):
    paths, tensors, rates, file, channel = [], [], [], [], []
    for f, (name, code, ch, rate, n, variant) in enumerate(spec):
        p = audio_payload(code, ch, n, seed=f)
        paths.append(write_wav(str(tmp_path / name), code, ch, rate, p, variant))
        x = np_decode(p, code, ch)
        for c in range(ch):
            tensors.append(torch.from_numpy(x[c].copy()))
            rates.append(rate)
            file.append(f)
            channel.append(c)
    return paths, tensors, rates, file, channel


def test_read_wav_many_equals_host_decoded_pack(tmp_path):
    from mdctgan_amd import wavio
    from mdctgan_amd.packed import aligned_layout, pack_waves, rows_moments, window_table
    paths, tensors, rates, file, channel = write_mixed(tmp_path)
    pack = wavio.read_wav_many(paths, DEV, channels="all", with_moments=True)
    layout = aligned_layout([t.numel() for t in tensors])
    assert (pack.starts, pack.lengths, pack.rates, pack.file, pack.channel) == (layout.starts, layout.lengths, rates, file, channel)
    assert torch.equal(pack.buffer, pack_waves(tensors, layout, DEV))
    win = torch.from_numpy(window_table(layout.starts, layout.lengths)).to(DEV)
    assert torch.equal(pack.moments, rows_moments(pack.buffer, win, max(layout.lengths)))
    first = wavio.read_wav_many(paths, DEV)                          # channels="first", no moments
    keep = [r for r, c in enumerate(channel) if c == 0]
    assert first.moments is None and first.file == [0, 1, 2, 3] and first.rates == [rates[r] for r in keep]
    assert all(torch.equal(v.cpu(), tensors[r]) for v, r in zip(first.views, keep))
    with pytest.raises(_lib().HipLibraryError):
        wavio.read_wav_many(paths, "cpu")


FRONT = dict(lr_sampling_rate=12000, hr_sampling_rate=48000, segment_length=7936, gen_overlap=100, batch_size=4)


def test_front_end_from_a_wavpack_is_the_front_end_from_tensors(tmp_path):
    from mdctgan_amd import wavio
    from mdctgan_amd.resample import front_end_many
    paths, tensors, rates, _, _ = write_mixed(tmp_path)
    pack = wavio.read_wav_many(paths, DEV, channels="all", with_moments=True)
    want_buf, want_views, want_plan = front_end_many(tensors, rates, FRONT, device=DEV, keep_raw=True)
    assert want_plan.order != list(range(len(tensors)))              # (the moments have to be put in group order)
    for raws, r, mom in ((pack, None, pack.moments), (pack, rates, None), ((pack.buffer, pack.starts, pack.lengths), rates, pack.moments)):
        buf, views, plan = front_end_many(raws, r, FRONT, keep_raw=True, raw_moments=mom)
        assert torch.equal(buf, want_buf) and len(views) == len(want_views)
        assert all(torch.equal(a, b) for a, b in zip(views, want_views))
        assert torch.equal(plan.raw.shift, want_plan.raw.shift) and torch.equal(plan.raw.buffer, want_plan.raw.buffer)
        assert plan.starts == want_plan.starts and plan.lengths == want_plan.lengths
    with pytest.raises(ValueError):
        front_end_many(pack, None, FRONT, raw_moments=pack.moments[:2])
    with pytest.raises(ValueError):                                  # not aligned_layout's layout
        front_end_many((pack.buffer, [s + 1 for s in pack.starts], pack.lengths), rates, FRONT)


def test_pack_corpus_files_equals_pack_corpus(tmp_path):
    from mdctgan_amd.train_data import pack_corpus, pack_corpus_files
    paths, tensors, rates, _, channel = write_mixed(tmp_path)
    keep = [r for r, c in enumerate(channel) if c == 0]
    want = pack_corpus([tensors[r] for r in keep], [rates[r] for r in keep], DEV)
    got = pack_corpus_files(paths, DEV)
    assert torch.equal(got.buffer, want.buffer)
    assert (got.starts, got.lengths, got.rates) == (want.starts, want.lengths, want.rates)


def test_write_wav_many_groups_and_round_trip(tmp_path):
    from mdctgan_amd import wavio
    gen = torch.Generator().manual_seed(4)
    rows = [0.4 * torch.randn(n, generator=gen) for n in (700, 700, 1, 4099, 4099, 4099)]
    rows[3][:4] = torch.tensor([2.0, -2.0, float("nan"), 1.0])
    paths = [str(tmp_path / n) for n in ("st.wav", "one.wav", "tri.wav")]
    groups = [[0, 1], [2], [3, 4, 5]]
    for encoding, code in wavio.ENCODINGS.items():
        clipped = wavio.write_wav_many(paths, [r.to(DEV) for r in rows], [8000, 16000, 44100], encoding, groups)
        for path, g, rate in zip(paths, groups, [8000, 16000, 44100]):
            want, counts = np_encode(np.stack([rows[i].numpy() for i in g]), code)
            tag, ch, r, bits, data, _ = parse_wav(path)
            assert (tag, ch, r, bits) == (3 if code == MG_PCM_F32 else 1, len(g), rate, 8 * SAMPLE_BYTES[code])
            assert data == want.tobytes()
            assert [clipped[i] for i in g] == counts
            assert wavio.wav_info(path).num_frames == rows[g[0]].numel()
        back = wavio.read_wav_many(paths, DEV, channels="all")
        if code == MG_PCM_F32:
            assert all(bits_equal(v, r) for v, r in zip(back.views, rows))
    with pytest.raises(ValueError, match="equal lengths"):
        wavio.write_wav_many(paths[:1], [r.to(DEV) for r in rows], 8000, groups=[[0, 2]])


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------------------------------------------------
E2E = [("m48.wav", MG_PCM_S16, 1, 48000, 9001, "plain"), ("m16.wav", MG_PCM_F32, 1, 16000, 3500, "extensible"),
       ("st.wav", MG_PCM_S24, 2, 48000, 8000, "chunks_after")]


@pytest.fixture(scope="module")
def model():
    from test_generate_many_gpu import make_model
    return make_model()


@pytest.fixture(scope="module")
def e2e(model, tmp_path_factory):
    """The three input files, their host-decoded rows, and super_resolve_many's waveforms for them (batches of one segment, so
    that a row's bits do not depend on what shares its batch)."""
    from mdctgan_amd.generate_audio import super_resolve_many
    from mdctgan_amd.resample import resample_length
    tmp = tmp_path_factory.mktemp("e2e")
    paths, tensors, rates, file, channel = write_mixed(tmp, E2E)
    waves = super_resolve_many(model, tensors, rates, batch_size=1)
    final = [resample_length(resample_length(t.numel(), r, 12000), 12000, 48000) for t, r in zip(tensors, rates)]
    want = [w[..., :n].cpu().numpy().reshape(-1) for w, n in zip(waves, final)]
    assert all(w.size == n for w, n in zip(want, final))
    return tmp, paths, tensors, rates, file, want


def test_super_resolve_files_writes_super_resolve_many(model, e2e, tmp_path):
    from mdctgan_amd.generate_audio import super_resolve_files
    tmp, paths, tensors, rates, file, want = e2e
    res = super_resolve_files(model, paths, tmp_path / "out", batch_size=1)
    assert res.out_paths == [str(tmp_path / "out" / n) for n in ("m48.wav", "m16.wav", "st.wav")]
    assert res.pack.file == file and res.clipped == [0, 0, 0, 0]
    assert all(bits_equal(w.reshape(-1), x) for w, x in zip(res.waves, want))
    for f, path in enumerate(res.out_paths):
        rows = [r for r, g in enumerate(file) if g == f]
        tag, ch, rate, bits, data, _ = parse_wav(path)
        assert (tag, ch, rate, bits) == (3, len(rows), 48000, 32)
        assert data == np_encode(np.stack([want[r] for r in rows]), MG_PCM_F32)[0].tobytes()
    # the stereo file's channels are what each gives as a mono file
    left, right = (write_wav(str(tmp_path / n), MG_PCM_F32, 1, 48000, tensors[r].numpy().tobytes())
                   for n, r in (("left.wav", 2), ("right.wav", 3)))
    mono = super_resolve_files(model, [left, right], None, batch_size=1)
    assert mono.out_paths is None and mono.clipped is None
    assert bits_equal(mono.waves[0].reshape(-1), want[2]) and bits_equal(mono.waves[1].reshape(-1), want[3])
    # channels="first" and 16-bit output: the encode restatement of the same waveforms
    res16 = super_resolve_files(model, paths, tmp_path / "out16", channels="first", encoding="PCM_S16", batch_size=1)
    for path, r in zip(res16.out_paths, (0, 1, 2)):
        tag, ch, rate, bits, data, _ = parse_wav(path)
        enc, counts = np_encode(want[r][None], MG_PCM_S16)
        assert (tag, ch, rate, bits) == (1, 1, 48000, 16) and data == enc.tobytes() and res16.clipped[r] == counts[0]
    with pytest.raises(ValueError, match="m48"):
        super_resolve_files(model, [paths[0], str(tmp / "m48.wav")], tmp_path / "dup")


def test_evaluate_files_writes_evaluate_many_s_lines(model, e2e, tmp_path):
    from mdctgan_amd.generate_audio import evaluate_files, evaluate_many
    tmp, paths, tensors, rates, file, want = e2e
    at_hr = [paths[0], str(tmp_path / "second.wav")]
    write_wav(at_hr[1], MG_PCM_S16, 2, 48000, audio_payload(MG_PCM_S16, 2, 8100, seed=8))
    second = torch.from_numpy(np_decode(audio_payload(MG_PCM_S16, 2, 8100, seed=8), MG_PCM_S16, 2)[0].copy())
    w0, s0 = evaluate_many(model, [tensors[0], second], [48000, 48000], batch_size=1, metric_path=str(tmp_path / "many.txt"))
    w1, s1 = evaluate_files(model, at_hr, str(tmp_path / "files.txt"), batch_size=1)
    assert torch.equal(s0, s1) and all(torch.equal(a, b) for a, b in zip(w0, w1))
    lines = open(tmp_path / "files.txt").read()
    assert lines == open(tmp_path / "many.txt").read() and len(lines.splitlines()) == 2
    with pytest.raises(ValueError, match="hr_sampling_rate"):
        evaluate_files(model, [paths[1]])


def test_command_line_in_a_child_process(model, e2e, tmp_path):
    from mdctgan_amd import options
    from mdctgan_amd.generate_audio import super_resolve_files
    tmp, paths, tensors, rates, file, want = e2e
    model.save_dir = str(tmp_path / "ckpt")
    model.save_network(model.netG, "G", "latest")
    flags = [*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4", "--n_blocks_global", "2",
             "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8", "--batchSize", "1", "--bins", "32", "--segment_length", "7936",
             "--n_fft", "512", "--hop_length", "256", "--win_length", "512", "--gpu_ids", "0"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "mdctgan_amd.generate_audio", *flags, "--load_pretrain", model.save_dir,
                          "--input", paths[2], "--output_dir", str(tmp_path / "cli"), "--out_encoding", "PCM_S24"],
                         cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    super_resolve_files(model, [paths[2]], tmp_path / "here", encoding="PCM_S24", batch_size=1)
    assert open(tmp_path / "cli" / "st.wav", "rb").read() == open(tmp_path / "here" / "st.wav", "rb").read()
    tag, ch, rate, bits, data, _ = parse_wav(str(tmp_path / "cli" / "st.wav"))
    assert (tag, ch, rate, bits) == (1, 2, 48000, 24) and data == np_encode(np.stack([want[2], want[3]]), MG_PCM_S24)[0].tobytes()
