"""K10 attention on feature maps of 129 to 256 tokens (the attn_wide_* kernels of csrc/bot_attn.hip) without a GPU.

1. Construction: a 256-token BottleStack and the n_fft-1024 generator (128 x 512 spectrogram, 4 downsamplings: 8 x 32 tokens)
   build, with the oracle's state-dict keys.
2. Still rejected, loudly: more than 256 tokens and dim_head > 128 raise NotImplementedError; the C entry points return
   MG_ERR_ARG before any launch (child processes with fake pointers, as in tests/test_bot_attn_host.py).
3. The bar of tests/test_bot_attn_gpu.py has teeth at the new sizes.
"""
import os
import subprocess
import sys

import pytest
import torch

import test_bot_attn_gpu as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MG_ERR_ARG = -1

# (B, fh, fw, heads, d, scale of qkv): the cases of tests/test_bot_attn_wide_gpu.py
WIDE_CASES = [
    (1, 3, 43, 1, 8, 1.0),        # n = 129: first size past the narrow kernels; one key in the third 64-key slot
    (1, 1, 130, 1, 16, 1.0),      # fh = 1: the height table's gradient is analytically zero
    (2, 11, 17, 3, 48, 1.0),      # ragged n = 187, d no multiple of 32
    (2, 11, 17, 3, 48, 6.0),      # logits of several tens
    (1, 7, 29, 1, 5, 1.0),        # n = 203, d = 5: k padding of an MFMA tile; idle threads of the embedding reduction
    (1, 32, 8, 1, 33, 1.0),       # n = 256, fh > fw, odd d
    (2, 8, 32, 2, 128, 1.0),      # both limits: the n_fft-1024 map
    (3, 16, 16, 6, 128, 1.0),     # both limits, square map, six heads: the long-segment map
    (40, 8, 24, 8, 8, 1.0),       # B * heads = 320 > 256
]


# ------------------------------------------------------------------------------------------------------------------
# 1. construction
# ------------------------------------------------------------------------------------------------------------------
def test_256_token_stack_and_n_fft_1024_generator_construct():
    from mdctgan_amd import networks
    from oracle import nets as onets
    stack = networks.BottleStack(dim=16, fmap_size=(8, 32), dim_out=16, num_layers=1, heads=2, dim_head=8, downsample=False)
    assert stack.fmap_size == (8, 32)
    net = networks.define_G(2, 1, 4, "global", 4, 2, n_attn_g=1, input_size=(128, 512))
    ref = onets.build_generator("global", 2, 1, 4, 4, 2, n_attn_g=1, input_size=(128, 512))
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())
    assert any("pos_emb.height" in k for k in net.state_dict())
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items() if "pos_emb" in k}
    assert sorted(s[0] for s in shapes.values()) == [8, 32], shapes


# ------------------------------------------------------------------------------------------------------------------
# 2. still rejected
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmap", [(3, 86), (16, 32)], ids=["tokens258", "tokens512"])
def test_more_than_256_tokens_raise(fmap):
    from mdctgan_amd import networks
    with pytest.raises(NotImplementedError, match="256 tokens"):
        networks.BottleStack(dim=16, fmap_size=fmap, dim_out=16, num_layers=1, heads=2, dim_head=8, downsample=False)


def test_dim_head_129_raises():
    from mdctgan_amd import networks
    with pytest.raises(NotImplementedError, match="dim_head <= 128"):
        networks.BottleStack(dim=16, fmap_size=(8, 32), dim_out=16, num_layers=1, heads=2, dim_head=129, downsample=False)


# (entry point, B, fh, fw, heads, d)
REJECTED = [
    ("fwd", 2, 3, 86, 2, 16),
    ("bwd", 2, 3, 86, 2, 16),
    ("fwd", 2, 8, 32, 2, 129),
    ("bwd", 2, 8, 32, 2, 129),
]

CHILD = """
import sys
sys.path.insert(0, %r)
from mdctgan_amd import _lib
lib = _lib.load()
which, B, fh, fw, heads, d = sys.argv[1], *map(int, sys.argv[2:7])
p = 4096
if which == "fwd":
    rc = lib.mg_attention_fwd(p, p, p, B, fh, fw, heads, d, p, p, None)
else:
    rc = lib.mg_attention_bwd(p, p, p, p, p, B, fh, fw, heads, d, p, p, p, 0, p, 1 << 40, None)
print("rc=%%d" %% rc)
""" % REPO


@pytest.fixture(scope="module")
def children():
    """All child processes at once (each pays the import of torch), results by combination."""
    procs = {c: subprocess.Popen([sys.executable, "-c", CHILD] + [str(v) for v in c], stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True, cwd=REPO) for c in REJECTED}
    return {c: (p,) + p.communicate(timeout=300) for c, p in procs.items()}


@pytest.mark.parametrize("combo", REJECTED, ids=lambda c: "%s_B%d_%dx%d_h%d_d%d" % c)
def test_entry_points_reject_258_tokens_and_d_129(children, combo):
    proc, out, errtxt = children[combo]
    assert proc.returncode == 0, "child exit status %d\n%s" % (proc.returncode, errtxt[-2000:])
    assert out.strip().splitlines()[-1] == "rc=%d" % MG_ERR_ARG


# ------------------------------------------------------------------------------------------------------------------
# 3. the bar at the new sizes
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """float64 and float32 restatements of every case, computed once and shared (never modified)."""
    cache = {}

    def get(case):
        if case not in cache:
            _, _, _, heads, d, _ = case
            qkv, eh, ew, dout = T.attn_inputs(case)
            cache[case] = (T.attn_ref(qkv.double(), eh.double(), ew.double(), dout.double(), heads, d, torch.float64),
                           T.attn_ref(qkv, eh, ew, dout, heads, d, torch.float32))
        return cache[case]
    return get


def _faulty(case, fault):
    _, _, _, heads, d, _ = case
    qkv, eh, ew, dout = T.attn_inputs(case)
    return T.attn_ref(qkv, eh, ew, dout, heads, d, torch.float32, fault)


@pytest.mark.parametrize("case", WIDE_CASES, ids=T.attn_id)
def test_float32_restatement_is_close_at_the_new_sizes(refs, case):
    """Within 2e-5 of float64 on every output (measured: 1.2e-5 on dqkv of the x6 case, at most 1.7e-6 elsewhere)."""
    r64, r32 = refs(case)
    Ne = T.demb_scale(r64)
    for name in ("out", "P", "dqkv", "demb_h", "demb_w"):
        e = T.err(r32[name], r64[name], Ne if name.startswith("demb") else T.scale_of(r64[name]))
        print("K10 yardstick %s | %s | e_f32 %.3e" % (T.attn_id(case), name, e))
        assert e <= 2e-5, (name, e)
        ok, _ = T.passes(r32[name], r32[name], r64[name], Ne if name.startswith("demb") else None)
        assert ok, name


@pytest.mark.parametrize("case", WIDE_CASES, ids=T.attn_id)
def test_bar_rejects_a_softmax_without_its_last_key_at_the_new_sizes(refs, case):
    r64, r32 = refs(case)
    bad = _faulty(case, "drop_key")
    for name in ("out", "P", "dqkv"):
        ok, margin = T.passes(bad[name], r32[name], r64[name])
        print("K10 sanity %s | drop key n-1 | %s | error / bar %.3e" % (T.attn_id(case), name, margin))
        assert not ok and margin > 100, (name, margin)


@pytest.mark.parametrize("case", [c for c in WIDE_CASES if c[1] > 1 and c[2] > 1], ids=T.attn_id)
def test_bar_rejects_a_wrong_row_index_at_the_new_sizes(refs, case):
    """j % fh for the row of token j instead of j / fw."""
    r64, r32 = refs(case)
    bad = _faulty(case, "row_mod")
    Ne = T.demb_scale(r64)
    for name, N in (("out", None), ("P", None), ("dqkv", None), ("demb_h", Ne)):
        ok, margin = T.passes(bad[name], r32[name], r64[name], N)
        print("K10 sanity %s | row j %% fh | %s | error / bar %.3e" % (T.attn_id(case), name, margin))
        assert not ok and margin > 100, (name, margin)
