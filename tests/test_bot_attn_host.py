"""K10 (csrc/bot_attn.hip) without a GPU.

1. The attention entry points reject an empty dimension with MG_ERR_ARG before anything divides by it or launches over it.
   attn_groups(B * heads, n) divides by B * heads: before the check, heads = 0 (forward) or B = 0 (backward) ended the process
   with SIGFPE.  Every rejected combination runs in a fresh child process, so that a signal shows as the child's exit status
   (-8) instead of taking the test run down; the pointers are arbitrary non-null integers, never dereferenced because the call
   returns first.
2. The bar of tests/test_bot_attn_gpu.py has teeth: float32 restatements that are wrong in the ways these kernels could be
   wrong miss it by a wide margin, and the correct float32 restatement passes it.
"""
import os
import subprocess
import sys

import pytest
import torch

import test_bot_attn_gpu as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MG_ERR_ARG = -1

# (entry point, B, fh, fw, heads, d)
REJECTED = [
    ("fwd", 2, 4, 8, 0, 16),
    ("fwd", 2, 4, 8, -1, 16),
    ("bwd", 0, 4, 8, 4, 16),
    ("bwd", -3, 4, 8, 4, 16),
    ("bwd", 2, 4, 8, 0, 16),
    ("bwd", 2, 4, 8, 4, 0),
    ("bwd", 2, 0, 8, 4, 16),
    ("bwd", 2, 4, 0, 4, 16),
    ("bwd", 2, -4, 8, 4, 16),
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
def test_attention_rejects_empty_dimensions(children, combo):
    proc, out, errtxt = children[combo]
    assert proc.returncode == 0, "child exit status %d\n%s" % (proc.returncode, errtxt[-2000:])
    assert out.strip().splitlines()[-1] == "rc=%d" % MG_ERR_ARG


# ------------------------------------------------------------------------------------------------------------------
# the suite's own sanity: what the bar rejects, on the CPU against the reference
# ------------------------------------------------------------------------------------------------------------------
def _attn(case, fault=None):
    B, fh, fw, heads, d, _ = case
    qkv, eh, ew, dout = T.attn_inputs(case)
    r64 = T.attn_ref(qkv.double(), eh.double(), ew.double(), dout.double(), heads, d, torch.float64)
    r32 = T.attn_ref(qkv, eh, ew, dout, heads, d, torch.float32)
    bad = T.attn_ref(qkv, eh, ew, dout, heads, d, torch.float32, fault) if fault else r32
    return r64, r32, bad


@pytest.mark.parametrize("case", [c for c in T.ATTN_CASES if c[1] * c[2] > 1], ids=T.attn_id)
def test_bar_rejects_a_softmax_without_its_last_key(case):
    r64, r32, bad = _attn(case, "drop_key")
    for name in ("out", "P", "dqkv"):
        ok, margin = T.passes(bad[name], r32[name], r64[name])
        print("K10 sanity %s | drop key n-1 | %s | error / bar %.3e" % (T.attn_id(case), name, margin))
        assert not ok and margin > 100, (name, margin)


@pytest.mark.parametrize("case", [c for c in T.ATTN_CASES if c[1] > 1 and c[2] > 1], ids=T.attn_id)
def test_bar_rejects_a_wrong_row_index(case):
    """j % fh for the row of token j instead of j / fw."""
    r64, r32, bad = _attn(case, "row_mod")
    Ne = T.demb_scale(r64)
    for name, N in (("out", None), ("P", None), ("dqkv", None), ("demb_h", Ne)):
        ok, margin = T.passes(bad[name], r32[name], r64[name], N)
        print("K10 sanity %s | row j %% fh | %s | error / bar %.3e" % (T.attn_id(case), name, margin))
        assert not ok and margin > 100, (name, margin)


@pytest.mark.parametrize("case", T.BN_CASES, ids=T.bn_id)
def test_bar_rejects_a_biased_running_var(case):
    t = T.bn_inputs(case)
    for momentum in (0.1, 1.0):
        r64 = T.bn_ref(T.as64(t), T.ACT_NONE, False, momentum, True, torch.float64)
        r32 = T.bn_ref(t, T.ACT_NONE, False, momentum, True, torch.float32)
        bad = (1 - momentum) * t["rv0"] + momentum * t["x"].var(0, unbiased=False)
        ok, margin = T.passes(bad, r32["running_var"], r64["running_var"])
        print("K10 sanity %s m%g | biased running_var | error / bar %.3e" % (T.bn_id(case), momentum, margin))
        assert not ok and margin > 10, margin      # the factor is worth momentum / R: 1e-4 of the buffer at R = 1001, m = 0.1


def test_bar_rejects_syncbn_with_the_local_row_count():
    """The two-part emulation of test_syncbn_without_a_process_group restated in float32 with count = R_local."""
    case = (35, 70, False)
    t = T.bn_inputs(case)
    r64 = T.bn_ref(T.as64(t), T.ACT_NONE, True, 0.1, True, torch.float64)
    r32 = T.bn_ref(t, T.ACT_NONE, True, 0.1, True, torch.float32)
    x = t["x"]
    s1, s2 = x.double().sum(0), (x.double() ** 2).sum(0)        # the two parts' partials, added
    for name, rows in (("part 0", slice(0, T.SYNC_SPLIT[0])), ("part 1", slice(T.SYNC_SPLIT[0], None))):
        for count, wrong in ((x.shape[0], False), (x[rows].shape[0], True)):
            mean = s1 / count
            rstd = ((s2 / count - mean * mean).clamp_min(0) + T.EPS).rsqrt()
            y = (t["gamma"] * ((x[rows] - mean.float()) * rstd.float()) + t["beta"]) + t["res"][rows]
            results = (("y", y, r32["y"][rows], r64["y"][rows], r64["y"].abs().max().item()),
                       ("save_mean", mean.float(), r32["save_mean"], r64["save_mean"], None),
                       ("save_rstd", rstd.float(), r32["save_rstd"], r64["save_rstd"], None))
            for what, got, f32, f64, N in results:
                ok, margin = T.passes(got, f32, f64, N)
                print("K10 sanity syncbn %s count %d | %s | error / bar %.3e" % (name, count, what, margin))
                assert ok != wrong, (name, count, what, margin)
                assert not wrong or margin > 100, (name, count, what, margin)


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=T.attn_id)
def test_float32_restatement_of_attention_is_finite_and_close(case):
    """The yardstick itself: the float32 CPU run stays within 1e-5 of float64 on every output (7e-6 at the amplified logits),
    so the bars of the GPU suite land between 5e-7 and 4e-5."""
    r64, r32, _ = _attn(case)
    Ne = T.demb_scale(r64)
    for name in ("out", "P", "dqkv", "demb_h", "demb_w"):
        e = T.err(r32[name], r64[name], Ne if name.startswith("demb") else T.scale_of(r64[name]))
        print("K10 yardstick %s | %s | e_f32 %.3e" % (T.attn_id(case), name, e))
        assert e <= 1e-5, (name, e)
