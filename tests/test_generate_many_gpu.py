"""Batched inference over utterances of different lengths: mg_segments_gather, the row-table stitched decoders
(mg_imdct4_stitched_rows, mg_imdct4_pow2_stitched_rows), generate_many and the graphed runner.  Every comparison is between two
orders of the same float operations, or against the existing composition: there are no tolerances."""
import numpy as np
import pytest
import torch

from oracle import nets as onets

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEG = 7936
LENGTHS = [3000, SEG, SEG + 1, 20000, 4 * SEG + 123]           # 1 + 1 + 2 + 3 + 5 = 12 segments
OVERLAPS = [0, 1024, 100]
SENTINEL = 1234.5


def _lib():
    from mdctgan_amd import _lib as L
    return L.load()


def _kernel(which=1):
    return _lib().mg_mdct_last_kernel(which).decode()


def make_model(n_fft=512, hop=256, seg=SEG):
    """The toy model of tests/test_nets_gpu.py (and of the pow2 generate test in tests/test_mdct_pow2_gpu.py)."""
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "4",
                           "--n_blocks_global", "2", "--n_blocks_attn_g", "0", "--num_D", "2", "--ndf", "8",
                           "--batchSize", "2", "--bins", "32", "--segment_length", seg, "--n_fft", n_fft, "--hop_length", hop,
                           "--win_length", n_fft, "--gpu_ids", "0")
    model = create_model(opt)
    onets.fill_deterministic(model.netG)
    onets.fill_deterministic(model.netD)
    return model


def _waves(lengths, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [(0.05 * torch.randn(n, generator=gen)).to(DEV) for n in lengths]


def _first(plan):
    return np.concatenate([[0], np.cumsum(plan.segments)])


# ---------------------------------------------------------------------------------------------------------------------
# 1. gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [64, 1])
@pytest.mark.parametrize("overlap", OVERLAPS)
def test_segments_gather_equals_segment_audio(overlap, align):
    """One launch cuts the segments of five utterances (shorter than a segment, exactly one, one sample more, 20000, 4 L + 123)
    as segment_audio cuts each alone; dead rows are zeros; nothing is written behind the last row.  align 1 packs the waveforms
    back to back, so most rows start at positions that are no multiple of 4 (the scalar loads)."""
    from mdctgan_amd.generate_audio import plan_utterances, segment_audio
    from mdctgan_amd.packed import pack_waves
    from mdctgan_amd.mdct import seg_row_table, segments_gather
    waves = _waves(LENGTHS)
    plan = plan_utterances(LENGTHS, SEG, SEG, overlap, 5, align=align)
    assert plan.n_live == 12 and plan.in_rows.shape[0] == 15
    packed = pack_waves(waves, plan.in_layout, DEV)
    assert packed.numel() == plan.in_total
    table = seg_row_table(plan.in_rows, DEV)
    guard = 512
    buf = torch.full((15 * SEG + guard,), SENTINEL, device=DEV)
    out = buf[:15 * SEG].view(15, SEG)
    assert segments_gather(packed, table, SEG, out=out) is out
    want = torch.cat([segment_audio(w, SEG, overlap) for w in waves])
    assert torch.equal(out[:12], want)
    assert not out[12:].any()
    assert (buf[15 * SEG:] == SENTINEL).all()
    # a row table that is not int64 [n, 3] is refused before the launch
    with pytest.raises(ValueError):
        segments_gather(packed, table.int(), SEG)


def test_segments_gather_odd_segment_length_and_negative_positions():
    """A segment length that is no multiple of 4 (the scalar kernel) and rows that start far in front of their window."""
    from mdctgan_amd.mdct import seg_row_table, segments_gather
    wave = torch.arange(1, 1001, dtype=torch.float32, device=DEV)
    rows = [(-50, 0, 1000), (995, 0, 1000), (10, 20, 30), (0, 0, 0), (-5000, 0, 1000)]
    L = 101
    buf = torch.full((5 * L + 64,), SENTINEL, device=DEV)
    out = segments_gather(wave, seg_row_table(rows, DEV), L, out=buf[:5 * L].view(5, L))
    want = torch.zeros(5, L)
    for r, (pos, lo, hi) in enumerate(rows):
        for t in range(L):
            if lo <= pos + t < hi:
                want[r, t] = pos + t + 1
    assert torch.equal(out.cpu(), want)
    assert (buf[5 * L:] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. row-table decode: all three kernels
# ---------------------------------------------------------------------------------------------------------------------
DECODE_CASES = [
    # n_fft, segment, overlap, float64, per-clip ranges, align, kernel
    (512, SEG, 0, False, False, 64, "imdct4_ct_kernel<stitched rows>"),
    (512, SEG, 1024, False, True, 64, "imdct4_ct_kernel<stitched rows>"),
    (512, SEG, 100, False, False, 64, "imdct4_ct_kernel<stitched rows>"),       # (100 is a multiple of 4: the factored kernel)
    (512, SEG, 1024, False, False, 1, "imdct4_ct_kernel<stitched rows>"),       # positions that are no multiple of 4
    (512, SEG, 101, False, True, 64, "imdct4_kernel<stitched rows>"),           # overlap % 4 != 0: the generic kernel
    (512, SEG, 100, True, False, 64, "imdct4_kernel<stitched rows>"),           # float64: the generic kernel
    (512, SEG, 0, True, False, 1, "imdct4_kernel<stitched rows>"),
    (256, 3968, 0, False, False, 64, "imdct4_pow2_kernel<stitched rows>"),
    (256, 3968, 64, False, True, 64, "imdct4_pow2_kernel<stitched rows>"),
    (1024, 7168, 256, False, False, 64, "imdct4_pow2_kernel<stitched rows>"),
    (1024, 7168, 256, False, False, 1, "imdct4_pow2_kernel<stitched rows>"),
    (1024, 7168, 101, False, False, 64, "imdct4_pow2_kernel<stitched rows>"),   # the scalar stores of K2'
]


@pytest.mark.parametrize("n_fft,seg,overlap,f64,per_clip,align,kernel", DECODE_CASES)
def test_row_table_decode_equals_per_utterance_stitched_decode(n_fft, seg, overlap, f64, per_clip, align, kernel):
    """12 live rows of five utterances and 2 dead rows in ONE launch against one mg_imdct4_stitched / mg_imdct4_pow2_stitched
    call per utterance on its rows, into a buffer of its own: the same bits in every window, and not one sample written in the
    gaps between the windows, behind the packed buffer, or by a dead row."""
    from mdctgan_amd import _lib as L
    from mdctgan_amd import mdct
    from mdctgan_amd.generate_audio import plan_utterances
    M = n_fft // 2
    F = seg // M + 1
    lengths = [seg // 3, seg, seg + 1, 2 * seg + 100, 4 * seg + 123]
    plan = plan_utterances(lengths, seg, seg, overlap, 7, align=align)
    assert plan.n_live == 12 and plan.out_rows.shape[0] == 14
    gen = torch.Generator().manual_seed(n_fft + overlap)
    spec = (2 * torch.rand(14, F, M, generator=gen) - 1).to(DEV)
    mn = (-3 - torch.rand(14, generator=gen)).to(DEV) if per_clip else None
    mx = (3 + torch.rand(14, generator=gen)).to(DEV) if per_clip else None
    window = mdct.kbdwin(n_fft).to(DEV)
    dtype = torch.float64 if f64 else torch.float32
    kw = dict(codec=L.MG_CODEC_ARCSINH, gain=1000.0, norm_range=(-1.0, 1.0), src_range=(-3.5, 3.5))

    def decode(s, lo, hi, **how):
        clip = dict(min_b=mn[lo:hi], max_b=mx[lo:hi]) if per_clip else {}
        if n_fft == 512:
            return mdct.imdct4_codec(s, window, mdct.dct4_table(M, DEV), n_fft, out_dtype=dtype, **kw, **clip, **how)[0]
        return mdct.imdct4_pow2(s, window, n_fft, **kw, **clip, **how)

    first = _first(plan)
    want = []
    for u in range(5):
        o = torch.zeros(plan.out_length[u], dtype=dtype, device=DEV)
        decode(spec[first[u]:first[u + 1]], first[u], first[u + 1], stitch=(o, overlap, 0, seg))
        want.append(o)
    assert "rows" not in _kernel(), _kernel()
    per_utt_kernel = _kernel()

    guard = 256
    inside = torch.zeros(plan.out_total + guard, dtype=torch.bool, device=DEV)
    for s, n in zip(plan.out_start, plan.out_length):
        inside[s:s + n] = True
    table = mdct.seg_row_table(plan.out_rows, DEV)
    # (a) into windows the caller cleared, sentinels everywhere else
    buf = torch.where(inside, 0.0, SENTINEL).to(dtype)
    got = decode(spec, 0, 14, rows=(buf[:plan.out_total], overlap, table, seg))
    assert got.data_ptr() == buf.data_ptr()
    assert kernel in _kernel(), _kernel()
    assert _kernel().replace("<stitched rows>", "<stitched>" if "<stitched>" in per_utt_kernel else "") == per_utt_kernel
    for u in range(5):
        s = plan.out_start[u]
        assert torch.equal(buf[s:s + plan.out_length[u]], want[u]), (u, (buf[s:s + plan.out_length[u]] - want[u]).abs().max().item())
    assert (buf[~inside] == SENTINEL).all()
    # (b) zero_out clears the whole packed buffer, and only it, first
    buf2 = torch.full((plan.out_total + guard,), SENTINEL, dtype=dtype, device=DEV)
    decode(spec, 0, 14, rows=(buf2[:plan.out_total], overlap, table, seg, True))
    assert torch.equal(buf2[:plan.out_total], torch.where(inside, buf, 0.0)[:plan.out_total])
    assert (buf2[plan.out_total:] == SENTINEL).all()
    # (c) dead rows alone change nothing
    buf3 = torch.full((plan.out_total + guard,), SENTINEL, dtype=dtype, device=DEV)
    decode(spec[12:], 12, 14, rows=(buf3[:plan.out_total], overlap, table[12:], seg))
    assert (buf3 == SENTINEL).all()
    # a spectrogram that decodes to another segment length than the plan's is refused
    with pytest.raises(ValueError):
        decode(spec, 0, 14, rows=(buf[:plan.out_total], overlap, table, seg - M))


# ---------------------------------------------------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------------------------------------------------
def _check_generate_many(model, seg, lengths, overlap, monkeypatch):
    from mdctgan_amd import ops
    from mdctgan_amd.generate_audio import generate_many, plan_utterances, segment_audio
    waves = _waves(lengths)
    plan = plan_utterances(lengths, seg, seg, overlap, 5)
    assert plan.n_live == 12
    monkeypatch.setenv("MG_NO_STITCHED_K2", "1")
    want = generate_many(model, waves, batch_size=5, gen_overlap=overlap)
    assert "stitched" not in _kernel(), _kernel()
    monkeypatch.delenv("MG_NO_STITCHED_K2")
    got = generate_many(model, waves, batch_size=5, gen_overlap=overlap)
    assert "<stitched rows>" in _kernel(), _kernel()
    assert len(got) == len(want) == len(waves)
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape == (1, _lib().mg_stitch_length(plan.segments[u], seg, overlap))
        assert torch.equal(g, w), (u, overlap, (g - w).abs().max().item())
    # padded batches against the composition by hand: the same zero-padded batches through model.inference, then one
    # ops.stitch_segments per utterance
    padded = generate_many(model, waves, batch_size=5, gen_overlap=overlap, pad_batches=True)
    segs = torch.cat([segment_audio(w, seg, overlap) for w in waves] + [torch.zeros(3, seg, device=DEV)])
    was_training = model.training
    model.eval()
    audio = torch.cat([model.inference(segs[i:i + 5])[1] for i in range(0, 15, 5)])
    model.train(was_training)
    first = _first(plan)
    for u in range(len(waves)):
        hand = ops.stitch_segments(audio[first[u]:first[u + 1]], seg, overlap)
        assert torch.equal(padded[u], hand), (u, overlap, (padded[u] - hand).abs().max().item())
    return got


@pytest.mark.parametrize("overlap", OVERLAPS)
def test_generate_many_equals_decode_then_stitch(overlap, monkeypatch):
    model = make_model()
    was_training = model.training
    got = _check_generate_many(model, SEG, LENGTHS, overlap, monkeypatch)
    assert model.training == was_training          # (generate_many evaluates in eval mode and restores the mode)
    # an utterance alone is what generate() makes of its segments
    from mdctgan_amd.generate_audio import generate, generate_many, segment_audio
    w = _waves(LENGTHS)[3]
    alone = generate_many(model, [w], batch_size=5, gen_overlap=overlap)[0]
    assert torch.equal(alone, generate(model, segment_audio(w, SEG, overlap), batch_size=5, gen_overlap=overlap))
    assert got[3].shape == alone.shape


def test_generate_many_on_a_pow2_geometry(monkeypatch):
    n_fft, hop, seg, ov = 1024, 512, 15872, 128
    model = make_model(n_fft, hop, seg)
    assert model.preprocess.fast and model.preprocess.has_stitched_decoder
    _check_generate_many(model, seg, [6000, seg, seg + 1, 2 * seg + 100, 4 * seg + 123], ov, monkeypatch)
    # without K1' / K2' the geometry has no stitched decoder: the composition serves generate_many, the graphed runner refuses
    from mdctgan_amd.generate_audio import generate_many, make_graphed_generate_many
    monkeypatch.setenv("MG_MDCT_POW2", "0")
    outs = generate_many(model, _waves([6000, seg + 1]), batch_size=2, gen_overlap=ov)
    assert [o.shape[-1] for o in outs] == [seg - 2 * ov, 2 * seg - 3 * ov]
    with pytest.raises(NotImplementedError):
        make_graphed_generate_many(model, 4, 4 * seg, batch_size=2, gen_overlap=ov)


# ---------------------------------------------------------------------------------------------------------------------
# 4. one graph, several mixes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1024])
def test_one_graph_serves_several_mixes(overlap):
    from mdctgan_amd.generate_audio import generate_many, make_graphed_generate_many, plan_utterances
    model = make_model()
    mix_a, mix_b = _waves(LENGTHS, 3), _waves([5000, 2 * SEG + 5, 3 * SEG], 4)
    assert plan_utterances([w.numel() for w in mix_b], SEG, SEG, overlap, 4).n_live == 7
    run = make_graphed_generate_many(model, 12, sum(LENGTHS), batch_size=4, gen_overlap=overlap)
    for mix in (mix_a, mix_b, mix_a):
        got = [g.clone() for g in run(mix)]
        want = generate_many(model, mix, batch_size=4, gen_overlap=overlap, pad_batches=True)
        assert len(got) == len(want)
        for u, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and torch.equal(g, w), (u, (g - w).abs().max().item())
    # a mix that does not fit is refused before anything is copied: the static buffers still hold mix A's result
    before = [g.clone() for g in run(mix_a)]
    with pytest.raises(ValueError):
        run(_waves([3 * SEG] * 5, 5))                    # 15 segments
    with pytest.raises(ValueError):
        run(_waves([sum(LENGTHS) + 1], 5))              # too many samples (and segments)
    with pytest.raises(ValueError):
        run(_waves([SEG - 1] * 12 + [SEG + 12], 5))     # 13 utterances of one segment: segments
    for b, a in zip(before, run.last):
        assert torch.equal(a, b)
    # after an optimiser step the captured weights are stale: run refuses, as make_graphed_generate's does
    lr = torch.stack([mix_a[4][:SEG], mix_a[4][SEG:2 * SEG]])
    model.optimize_parameters(lr, lr.flip(0).contiguous())
    with pytest.raises(RuntimeError):
        run(mix_a)


# ---------------------------------------------------------------------------------------------------------------------
# 5. existing paths are untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_generate_is_untouched_by_generate_many():
    from mdctgan_amd.generate_audio import generate, generate_many, segment_audio
    model = make_model()
    waves = _waves(LENGTHS)
    for overlap, name in ((1024, "imdct4_ct_kernel<stitched> (csrc/mdct_ct.h)"), (0, "imdct4_ct_kernel<stitched> (csrc/mdct_ct.h)")):
        segs = segment_audio(waves[4], SEG, overlap)
        before = generate(model, segs, batch_size=2, gen_overlap=overlap).clone()
        assert _kernel() == name
        generate_many(model, waves, batch_size=5, gen_overlap=overlap)
        assert _kernel() == "imdct4_ct_kernel<stitched rows> (csrc/mdct_ct.h)"
        after = generate(model, segs, batch_size=2, gen_overlap=overlap)
        assert _kernel() == name
        assert torch.equal(before, after)


def test_waveforms_may_live_on_the_host_or_on_both_sides():
    """The packed input is the same whether the list holds device tensors, host tensors or a mix of them."""
    from mdctgan_amd.generate_audio import plan_utterances
    from mdctgan_amd.packed import pack_waves
    waves = _waves(LENGTHS)
    plan = plan_utterances(LENGTHS, SEG, SEG, 100, 5)
    want = pack_waves(waves, plan.in_layout, DEV)
    for u, w in enumerate(waves):
        assert torch.equal(want[plan.in_start[u]:plan.in_start[u] + w.numel()], w)
    assert torch.equal(pack_waves([w.cpu() for w in waves], plan.in_layout, DEV), want)
    assert torch.equal(pack_waves([w.cpu() if u % 2 else w for u, w in enumerate(waves)], plan.in_layout, DEV), want)
    static = torch.full((plan.in_total + 64,), SENTINEL, device=DEV)
    assert pack_waves(waves, plan.in_layout, DEV, out=static).data_ptr() == static.data_ptr()
    assert torch.equal(static[:plan.in_total], want) and (static[plan.in_total:] == SENTINEL).all()
