"""Which kernel family serves a transform request (mdctgan_amd/mdct.py: Transform.route_analysis / route_synthesis), row by row of
the route table, without a GPU: the route functions launch nothing.  A route is (kernel, codec_inside, fallback): the family of
the transform kernel, whether no mg_codec_* launch accompanies it, and whether the generic composition takes over where the
kernel answers MG_ERR_UNSUPPORTED.  The expected values are written out; the GPU tests assert through mg_mdct_last_kernel that
the kernels named here are the ones launched."""
import pytest
import torch

from mdctgan_amd import _lib
from mdctgan_amd.mdct import Codec, Route, Transform, kbdwin

RAW, ARCSINH, RANGE, DB, EXPLICIT = (Codec(m) for m in (_lib.MG_CODEC_RAW, _lib.MG_CODEC_ARCSINH, _lib.MG_CODEC_RANGE,
                                                        _lib.MG_CODEC_DB, _lib.MG_CODEC_EXPLICIT))
F32, F64 = torch.float32, torch.float64

# (n_fft, hop, win, center) -> family with MG_MDCT_POW2 unset, with MG_MDCT_POW2=0
GEOMETRIES = [
    ((512, 256, 512, True), "k512", "k512"),
    ((256, 128, 256, True), "pow2", "generic"),
    ((1024, 512, 1024, True), "pow2", "generic"),
    ((2048, 1024, 2048, True), "pow2", "generic"),
    ((1024, 256, 1024, True), "generic", "generic"),
    ((2048, 1024, 2048, False), "generic", "generic"),
    ((512, 256, 512, False), "generic", "generic"),
]

K512_IN, K512_OUT = ("k512", True, False), ("k512", False, False)
POW2_IN, POW2_OUT = ("pow2", True, True), ("pow2", False, True)
GEN_RAW, GEN_CODEC = ("generic", True, False), ("generic", False, False)

# request -> route per family
ANALYSIS = [
    (RAW, {}, K512_IN, POW2_IN, GEN_RAW),
    (RAW, dict(want_frames=True), K512_IN, GEN_RAW, GEN_RAW),
    (ARCSINH, {}, K512_IN, POW2_IN, GEN_CODEC),
    (RANGE, {}, K512_IN, POW2_IN, GEN_CODEC),
    (ARCSINH, dict(per_sample=True), K512_IN, POW2_OUT, GEN_CODEC),
    (RANGE, dict(want_pair=True), K512_IN, POW2_OUT, GEN_CODEC),
    (ARCSINH, dict(per_sample=True, want_pair=True, want_frames=True), K512_IN, GEN_CODEC, GEN_CODEC),
    (ARCSINH, dict(want_frames=True), K512_IN, GEN_CODEC, GEN_CODEC),
    (DB, {}, K512_OUT, POW2_OUT, GEN_CODEC),
    (EXPLICIT, {}, K512_OUT, POW2_OUT, GEN_CODEC),
    (DB, dict(want_frames=True), K512_OUT, GEN_CODEC, GEN_CODEC),
]
SYNTHESIS = [
    (RAW, {}, K512_IN, POW2_IN, GEN_RAW),
    (ARCSINH, {}, K512_IN, POW2_IN, GEN_CODEC),
    (RANGE, dict(F=64), K512_IN, POW2_IN, GEN_CODEC),
    (DB, {}, K512_OUT, POW2_OUT, GEN_CODEC),
    (EXPLICIT, {}, K512_OUT, POW2_OUT, GEN_CODEC),
    # the guards of K2': synthesis frames, float64 output, a one-frame spectrogram (with the codec inside too)
    (RAW, dict(want_frames=True), K512_IN, GEN_RAW, GEN_RAW),
    (ARCSINH, dict(out_dtype=F64), K512_IN, GEN_CODEC, GEN_CODEC),
    (RAW, dict(F=1), K512_IN, GEN_RAW, GEN_RAW),
    (ARCSINH, dict(F=1), K512_IN, GEN_CODEC, GEN_CODEC),
    (DB, dict(F=1), K512_OUT, GEN_CODEC, GEN_CODEC),
    # a stitch / rows destination: the stitched decoders have no generic stand-in
    (ARCSINH, dict(dest=True), K512_IN, ("pow2", True, False), "stitched decode"),
    (RANGE, dict(dest=True, F=64), K512_IN, ("pow2", True, False), "stitched decode"),
    (RAW, dict(dest=True), "stitched decode", "stitched decode", "stitched decode"),
    (DB, dict(dest=True), "stitched decode", "stitched decode", "stitched decode"),
    (EXPLICIT, dict(dest=True), "stitched decode", "stitched decode", "stitched decode"),
    (ARCSINH, dict(dest=True, out_dtype=F64), K512_IN, "stitched decode", "stitched decode"),
]
K512_BWD, POW2_BWD, GEN_BWD = ("k512", True, True), ("pow2", False, True), ("generic", False, False)
SYNTHESIS_BACKWARD = [
    (dict(out_dtype=F32), K512_BWD, POW2_BWD, GEN_BWD),
    (dict(out_dtype=F64), GEN_BWD, GEN_BWD, GEN_BWD),          # the float64 forward ran on the generic kernels
]
# (frames, samples in hops) of the analysis whose gradient is asked
ANALYSIS_BACKWARD = [
    ((5, 4), K512_BWD, POW2_BWD, GEN_BWD),                     # F = T / hop + 1: every sample inside (F - 1) hop
    ((5, 3.5), K512_BWD, POW2_BWD, GEN_BWD),
    ((1, 1), K512_BWD, GEN_BWD, GEN_BWD),                      # F <= 1
    ((3, 4), K512_BWD, GEN_BWD, GEN_BWD),                      # the frames reach 3 hops, K2' decodes (F - 1) hop = 2
]


def _transform(geom):
    n_fft, hop, win, center = geom
    return Transform(n_fft, hop, win, kbdwin, center, device="cpu")


def _check(route, want, **kw):
    if isinstance(want, str):
        with pytest.raises(NotImplementedError, match=want):
            route(**kw)
    else:
        got = route(**kw)
        assert isinstance(got, Route) and tuple(got) == want, (kw, tuple(got), want)


@pytest.mark.parametrize("switch", [None, "0"])
@pytest.mark.parametrize("geom,family_on,family_off", GEOMETRIES)
def test_route_table(geom, family_on, family_off, switch, monkeypatch):
    monkeypatch.delenv("MG_MDCT_POW2", raising=False)
    t = _transform(geom)
    assert t.family == family_on and t.fused is (family_on == "k512") and t.fast is (family_on == "pow2")
    if switch is not None:
        monkeypatch.setenv("MG_MDCT_POW2", switch)              # read at call time: the same object follows it
    family = family_on if switch is None else family_off
    assert t.family == family and t.fast is (family == "pow2") and t.fused is (family_on == "k512")
    col = {"k512": 0, "pow2": 1, "generic": 2}[family]
    for codec, kw, *want in ANALYSIS:
        _check(lambda **k: t.route_analysis(codec, **k), want[col], **kw)
    for codec, kw, *want in SYNTHESIS:
        _check(lambda **k: t.route_synthesis(codec, **k), want[col], **kw)
    for kw, *want in SYNTHESIS_BACKWARD:
        for codec in (RAW, ARCSINH):
            _check(lambda **k: t.route_synthesis(codec, backward=True, **k), want[col], **kw)
    hop = geom[1]
    for (F, hops), *want in ANALYSIS_BACKWARD:
        for codec in (RAW, RANGE):
            _check(lambda **k: t.route_analysis(codec, backward=True, **k), want[col], F=F, T=int(hops * hop))


def test_routes_make_no_launch_and_no_tensor(monkeypatch):
    """Pure host functions: they run with every launcher and the library loader out of reach."""
    from mdctgan_amd import mdct
    t = _transform((1024, 512, 1024, True))
    for name in ("mdct4_codec", "imdct4_codec", "mdct4_pow2", "imdct4_pow2", "mdct4_generic", "imdct4_generic", "codec_forward",
                 "codec_inverse", "codec_backward", "dct4_table", "pow2_twiddles"):
        monkeypatch.setattr(mdct, name, None)
    monkeypatch.setattr(_lib, "load", None)
    monkeypatch.setattr(torch, "empty", None)
    assert tuple(t.route_analysis(ARCSINH)) == POW2_IN and tuple(t.route_synthesis(ARCSINH, F=8, dest=True)) == ("pow2", True, False)
    assert tuple(t.route_analysis(RAW, backward=True, F=3, T=1024)) == POW2_BWD


def test_stitched_decode_is_refused_where_audio2mdct_has_no_stitched_decoder(monkeypatch):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import Audio2MDCT
    monkeypatch.delenv("MG_MDCT_POW2", raising=False)
    db = [f for f in options.SPECTRAL_FLAGS if f != "--arcsinh_transform"]
    norm = {"min": torch.zeros(1), "max": torch.ones(1)}
    cases = [(512, 256, options.SPECTRAL_FLAGS, True), (1024, 512, options.SPECTRAL_FLAGS, True),
             (1024, 256, options.SPECTRAL_FLAGS, False), (512, 256, db, False), (2048, 1024, db, False)]
    for n_fft, hop, flags, has in cases:
        p = Audio2MDCT(options.make_opt(*flags, "--n_fft", n_fft, "--hop_length", hop, "--win_length", n_fft,
                                        "--lr_sampling_rate", "12000", gpu_ids=[]))
        assert p.has_stitched_decoder is has, (n_fft, hop, p.codec)
        if not has:
            spec = torch.zeros(1, 1, 3, n_fft // 2)
            for dest in (dict(stitch=(torch.zeros(8), 0, 0)), dict(rows=(torch.zeros(8), 0, torch.zeros(1, 3, dtype=torch.int64)))):
                with pytest.raises(NotImplementedError, match="stitched decode"):
                    p.to_audio(spec, norm, None, **dest)
