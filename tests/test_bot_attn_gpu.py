"""K10 kernels (csrc/bot_attn.hip: BatchNorm2d, multi-head self attention with absolute position embeddings, the
position-embedding gradient reduction) and mg_cat2_* op by op against plain PyTorch float64 CPU references.

Bar (the policy of test_nets_gpu.py without its 5e-4 floor): for every output t, e(t) = max|t - f64| / N with N = max|f64|,
and
    e(HIP)  <=  k * e(torch float32 CPU, the same restatement)  +  4 * 2^-23,      k = 4.
The float64 reference is built from the float32-ROUNDED inputs (x.float().double()), so input rounding is nobody's error.
demb_h / demb_w are normalised by max(max|demb_h|, max|demb_w|, max|dqkv|): a table with one row has an analytically zero
gradient (a shift common to every key of a query leaves the softmax unchanged), a ratio against its own size means nothing.

The reference functions below run without a GPU; tests/test_bot_attn_host.py feeds them deliberately wrong float32
restatements to show that the bar rejects them.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 4.0
ULPS = 4 * 2.0 ** -23
EPS = 1e-5
ACT_NONE, ACT_RELU = 0, 1


# ------------------------------------------------------------------------------------------------------------------
# the bar
# ------------------------------------------------------------------------------------------------------------------
def err(t, f64, N):
    """max|t - f64| / N; NaN (an element nobody wrote) counts as infinite."""
    d = (t.detach().double().cpu() - f64).abs().max().item()
    return float("inf") if d != d else d / max(N, 1e-30)


def scale_of(*f64s):
    return max(t.abs().max().item() for t in f64s)


class Judge:
    """Collects (what, e(HIP), e(float32)) for every output of a case, prints them all, then asserts them all."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def add(self, what, got, f32, f64, N=None, k=K):
        N = scale_of(f64) if N is None else N
        e_hip, e_32 = err(got, f64, N), err(f32, f64, N)
        nrm = max(f64.norm().item(), 1e-30)
        l_hip = (got.detach().double().cpu() - f64).norm().item() / nrm
        l_32 = (f32.detach().double() - f64).norm().item() / nrm
        self.rows.append((what, e_hip, e_32, k * e_32 + ULPS, l_hip, l_32))

    def done(self):
        bad = []
        for what, e_hip, e_32, bar, l_hip, l_32 in self.rows:
            print("K10 %s | %s | e_hip %.3e | e_f32 %.3e | bar %.3e | l2_hip %.3e | l2_f32 %.3e"
                  % (self.case, what, e_hip, e_32, bar, l_hip, l_32))
            if not e_hip <= bar:
                bad.append("%s: e(HIP) %.3e > bar %.3e (e(float32) %.3e)" % (what, e_hip, bar, e_32))
        assert not bad, "%s: %s" % (self.case, "; ".join(bad))


def passes(got, f32, f64, N=None, k=K):
    """The bar as a predicate and its margin e(got) / bar (the host-side sanity test of the suite uses it)."""
    N = scale_of(f64) if N is None else N
    bar = k * err(f32, f64, N) + ULPS
    e = err(got, f64, N)
    return e <= bar, e / bar


# ------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------
# (B, fh, fw, heads, d, scale of qkv)
ATTN_CASES = [
    (2, 1, 1, 1, 1, 1.0),       # n = 1: n / 4 = 0 groups clamps to 1; P is exactly 1
    (1, 1, 3, 2, 5, 1.0),       # n = 3 < 4 waves; d = 5: posemb_grad threads 1020..1023 belong to no group
    (2, 5, 7, 3, 48, 1.0),      # ragged n = 35; 1024 / 48 = 21 groups
    (2, 5, 7, 3, 48, 6.0),      # logits of several tens: softmax stability
    (1, 8, 8, 2, 16, 1.0),      # n = 64: second key slot of every lane masked
    (2, 5, 13, 2, 33, 1.0),     # n = 65: one key in the second slot
    (1, 9, 14, 1, 100, 1.0),    # d > 64, ~101 KB of LDS (raised dynamic-LDS limit), ragged n = 126
    (3, 8, 16, 2, 128, 1.0),    # both limits at once
    (40, 4, 8, 8, 8, 1.0),      # B * heads = 320 > 256: one workgroup per (b, head); the embedding reduction loops over bh
    (1, 16, 8, 1, 8, 1.0),      # fh > fw: j / fw and j % fw swaps
]


def attn_id(c):
    return "B%d_%dx%d_h%d_d%d%s" % (c[0], c[1], c[2], c[3], c[4], "" if c[5] == 1.0 else "_x%g" % c[5])


def attn_inputs(case, seed=10):
    B, fh, fw, heads, d, s = case
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, fh, fw, 3 * heads * d, generator=gen) * s
    eh = torch.randn(fh, d, generator=gen)
    ew = torch.randn(fw, d, generator=gen)
    dout = torch.randn(B, fh, fw, heads * d, generator=gen)
    return qkv, eh, ew, dout


def attn_ref(qkv, eh, ew, dout, heads, d, dtype, fault=None):
    """The header comment of csrc/bot_attn.hip / oracle/nets.py in `dtype` on the CPU; gradients by autograd.
    fault (host-side sanity of the suite only): "drop_key" leaves key n - 1 out of the softmax, "row_mod" takes j % fh
    for the row of token j."""
    B, fh, fw, _ = qkv.shape
    n = fh * fw
    qkv = qkv.to(dtype).clone().requires_grad_()
    eh = eh.to(dtype).clone().requires_grad_()
    ew = ew.to(dtype).clone().requires_grad_()
    q, k, v = qkv.reshape(B, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    if fault == "row_mod":
        j = torch.arange(n)
        E = eh[j % fh] + ew[j % fw]
    else:
        E = (eh[:, None, :] + ew[None, :, :]).reshape(n, d)
    sim = torch.einsum("bhid,bhjd->bhij", q * d ** -0.5, k + E)
    if fault == "drop_key":
        sim = torch.cat((sim[..., :-1], torch.full_like(sim[..., -1:], float("-inf"))), -1)
    P = sim.softmax(dim=-1)
    out = torch.einsum("bhij,bhjd->bhid", P, v).permute(0, 2, 1, 3).reshape(B, fh, fw, heads * d)
    out.backward(dout.to(dtype))
    return dict(out=out.detach(), P=P.detach(), rowsum=P.detach().double().sum(-1), dqkv=qkv.grad, demb_h=eh.grad,
                demb_w=ew.grad)


def demb_scale(r64):
    return scale_of(r64["demb_h"], r64["demb_w"], r64["dqkv"])


def raw_attention(qkv, eh, ew, dout, heads, d, demb_h, demb_w, accumulate):
    """mg_attention_fwd + mg_attention_bwd through the bindings, every buffer (the workspace too) NaN before the call."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    B, fh, fw, _ = qkv.shape
    n = fh * fw
    nan = float("nan")
    out = torch.full((B, fh, fw, heads * d), nan, device=DEV)
    P = torch.full((B, heads, n, n), nan, device=DEV)
    dqkv = torch.full_like(qkv, nan)
    nbytes = lib.mg_attention_bwd_workspace(B, fh, fw, heads, d)
    ws = torch.full(((nbytes + 3) // 4,), nan, device=DEV)
    _lib.check(lib.mg_attention_fwd(_lib.ptr(qkv), _lib.ptr(eh), _lib.ptr(ew), B, fh, fw, heads, d, _lib.ptr(out), _lib.ptr(P),
                                    _lib.stream()), "mg_attention_fwd")
    _lib.check(lib.mg_attention_bwd(_lib.ptr(qkv), _lib.ptr(eh), _lib.ptr(ew), _lib.ptr(dout), _lib.ptr(P), B, fh, fw, heads, d,
                                    _lib.ptr(dqkv), _lib.ptr(demb_h), _lib.ptr(demb_w), int(accumulate), _lib.ptr(ws),
                                    ws.numel() * 4, _lib.stream()), "mg_attention_bwd")
    return out, P, dqkv


@pytest.mark.parametrize("case", ATTN_CASES, ids=attn_id)
def test_attention_fwd_bwd(case):
    """out, P (and its row sums), dqkv, demb_h, demb_w against float64; accumulate = 1 adds the same gradient to what the
    tables held; without tables dqkv keeps its bits; a second call, on NaN-filled buffers, reproduces every bit.

    Measured on an MI355X (e(HIP) / e(float32 CPU), worst over the ten cases): see the per-case lines this test prints."""
    from mdctgan_amd import ops
    B, fh, fw, heads, d, _ = case
    qkv, eh, ew, dout = attn_inputs(case)
    r64 = attn_ref(qkv.double(), eh.double(), ew.double(), dout.double(), heads, d, torch.float64)
    r32 = attn_ref(qkv, eh, ew, dout, heads, d, torch.float32)
    qd, ehd, ewd, dod = (t.to(DEV) for t in (qkv, eh, ew, dout))
    nan = float("nan")
    dh, dw = torch.full((fh, d), nan, device=DEV), torch.full((fw, d), nan, device=DEV)
    out, P = ops.attention_fwd(qd, ehd, ewd, heads, d)
    dqkv = ops.attention_bwd(qd, ehd, ewd, dod, P, heads, d, dh, dw, 0)
    assert out.shape == (B, fh, fw, heads * d) and P.shape == (B, heads, fh * fw, fh * fw)

    j = Judge(attn_id(case))
    j.add("out", out, r32["out"], r64["out"])
    j.add("P", P, r32["P"], r64["P"])
    j.add("P rows sum to 1", P.double().sum(-1), r32["rowsum"], torch.ones_like(r64["rowsum"]), N=1.0)
    j.add("dqkv", dqkv, r32["dqkv"], r64["dqkv"])
    Ne = demb_scale(r64)
    j.add("demb_h", dh, r32["demb_h"], r64["demb_h"], N=Ne)
    j.add("demb_w", dw, r32["demb_w"], r64["demb_w"], N=Ne)

    # accumulate = 1: prefill + gradient (N: the same rule over what the tables now hold)
    gen = torch.Generator().manual_seed(11)
    ph, pw = torch.randn(fh, d, generator=gen), torch.randn(fw, d, generator=gen)
    ah, aw = ph.to(DEV), pw.to(DEV)
    dqkv_acc = ops.attention_bwd(qd, ehd, ewd, dod, P, heads, d, ah, aw, 1)
    wh, ww = ph.double() + r64["demb_h"], pw.double() + r64["demb_w"]
    Na = scale_of(wh, ww, r64["dqkv"])
    j.add("demb_h accumulate", ah, ph + r32["demb_h"], wh, N=Na)
    j.add("demb_w accumulate", aw, pw + r32["demb_w"], ww, N=Na)
    j.done()

    if fh * fw == 1:
        assert torch.equal(P, torch.ones_like(P))
    assert torch.equal(dqkv_acc, dqkv)
    # no tables: the same dqkv bits
    assert torch.equal(ops.attention_bwd(qd, ehd, ewd, dod, P, heads, d, None, None, 0), dqkv)
    # "deterministic": an identical call (on buffers that are NaN wherever nobody writes) agrees on every output
    dh2, dw2 = torch.full_like(dh, nan), torch.full_like(dw, nan)
    out2, P2, dqkv2 = raw_attention(qd, ehd, ewd, dod, heads, d, dh2, dw2, 0)
    for name, a, b in (("out", out, out2), ("P", P, P2), ("dqkv", dqkv, dqkv2), ("demb_h", dh, dh2), ("demb_w", dw, dw2)):
        assert torch.equal(a, b), name


def test_attention_sample_alone_has_the_bits_it_has_in_the_batch():
    """attn_groups: B * heads = 320 launches one workgroup per (b, head), B = 1 (8 heads) launches 8 per (b, head) --
    "every output element is computed by the same instructions: the same bits"."""
    case = (40, 4, 8, 8, 8, 1.0)
    _, _, _, heads, d, _ = case
    qkv, eh, ew, dout = (t.to(DEV) for t in attn_inputs(case))
    nan = float("nan")
    outs = []
    for sl in (slice(None), slice(0, 1)):
        dh, dw = torch.full_like(eh, nan), torch.full_like(ew, nan)
        outs.append(raw_attention(qkv[sl].contiguous(), eh, ew, dout[sl].contiguous(), heads, d, dh, dw, 0))
    for name, whole, alone in zip(("out", "P", "dqkv"), *outs):
        assert alone.shape[0] == 1 and torch.equal(whole[:1], alone), name


def test_attention_table_gradients_stay_inside_their_tables():
    """d = 5: demb_h [1, 5] and demb_w [3, 5] as views into buffers that carry 64 sentinel floats after them."""
    case = (1, 1, 3, 2, 5, 1.0)
    _, fh, fw, heads, d, _ = case
    qkv, eh, ew, dout = (t.to(DEV) for t in attn_inputs(case))
    for accumulate in (0, 1):
        bh, bw = torch.full((fh * d + 64,), 7.25, device=DEV), torch.full((fw * d + 64,), 7.25, device=DEV)
        dh, dw = bh[:fh * d].view(fh, d), bw[:fw * d].view(fw, d)
        dh.fill_(0.5)
        dw.fill_(0.5)
        raw_attention(qkv, eh, ew, dout, heads, d, dh, dw, accumulate)
        assert torch.isfinite(dh).all() and torch.isfinite(dw).all()
        assert not torch.equal(dw, torch.full_like(dw, 0.5))
        assert (bh[fh * d:] == 7.25).all() and (bw[fw * d:] == 7.25).all()


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm2d
# ------------------------------------------------------------------------------------------------------------------
# (R, C, offset): x = randn, or 100 + 0.01 randn (cancellation in E[x^2] - mean^2: why the partials are double)
BN_CASES = [
    (3, 1, False),          # most row slices empty
    (8, 64, False),         # exactly one row per slice
    (35, 70, False),        # ragged second channel block
    (64, 512, False),       # the configs[2] layer at batch 2
    (1001, 65, False),      # ragged rows, a one-channel tail block
    (1001, 65, True),
]
MAX_FLIPS = 2


def bn_id(c):
    return "R%d_C%d%s" % (c[0], c[1], "_offset" if c[2] else "")


def bn_inputs(case, seed=20):
    R, C, offset = case
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(R, C, generator=gen)
    x = 100 + 0.01 * x if offset else x
    t = dict(x=x,
             res=torch.randn(R, C, generator=gen),
             dy=torch.randn(R, C, generator=gen),
             gamma=1 + 0.5 * torch.randn(C, generator=gen),
             beta=0.5 * torch.randn(C, generator=gen),
             rm0=torch.randn(C, generator=gen),
             rv0=0.5 + torch.rand(C, generator=gen))
    if offset:      # eval mode normalises with these: keep them near the data
        t["rm0"] = 100 + 0.01 * t["rm0"]
        t["rv0"] = 1e-4 * t["rv0"]
    return t


def bn_ref(t, act, use_res, momentum, training, dtype, mask=None):
    """nn.BatchNorm2d (+ residual, + ReLU) in `dtype` on the CPU, gradients by autograd.  mask: the ReLU decisions to take
    (None: the reference's own, z > 0); z is the value the ReLU sees."""
    R, C = t["x"].shape
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=momentum).to(dtype)
    with torch.no_grad():
        bn.weight.copy_(t["gamma"])
        bn.bias.copy_(t["beta"])
        bn.running_mean.copy_(t["rm0"])
        bn.running_var.copy_(t["rv0"])
    bn.train(bool(training))
    x = t["x"].to(dtype).clone().requires_grad_()
    res = t["res"].to(dtype).clone().requires_grad_()
    z = bn(x.reshape(R, C, 1, 1)).reshape(R, C)
    if use_res:
        z = z + res
    y = z
    if act == ACT_RELU:
        m = (z.detach() > 0) if mask is None else mask
        y = torch.where(m, z, torch.zeros_like(z))
    y.backward(t["dy"].to(dtype))
    xs = x.detach()
    if training:
        mean = xs.mean(0)
        rstd = (xs.var(0, unbiased=False) + EPS).rsqrt()
    else:
        mean = t["rm0"].to(dtype)
        rstd = (t["rv0"].to(dtype) + EPS).rsqrt()
    return dict(y=y.detach(), z=z.detach(), save_mean=mean, save_rstd=rstd, dx=x.grad, dgamma=bn.weight.grad,
                dbeta=bn.bias.grad, running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone())


def as64(t):
    return {k: v.double() for k, v in t.items()}


def check_relu_decisions(mask_hip, z64, what):
    """Every ReLU decision that differs from the float64 reference's own sits at |z| <= 1e-6 max|z|; at most MAX_FLIPS do."""
    diff = mask_hip != (z64 > 0)
    n = int(diff.sum())
    worst = z64[diff].abs().max().item() if n else 0.0
    print("K10 %s | ReLU decisions differing %d | worst |z| / max|z| %.3e" % (what, n, worst / z64.abs().max().item()))
    assert n <= MAX_FLIPS, "%s: %d ReLU decisions differ from float64" % (what, n)
    assert worst <= 1e-6 * z64.abs().max().item(), "%s: a ReLU decision differs at |z| = %.3e" % (what, worst)


def run_bn(case, act, use_res, momentum, accumulate, training):
    from mdctgan_amd import ops
    R, C, _ = case
    t = bn_inputs(case)
    d = {k: v.to(DEV) for k, v in t.items()}
    what = "%s act%d res%d m%g acc%d %s" % (bn_id(case), act, use_res, momentum, accumulate, "train" if training else "eval")
    rm, rv = d["rm0"].clone(), d["rv0"].clone()
    y, mean, rstd = ops.batchnorm_fwd(d["x"].view(1, R, 1, C), d["gamma"], d["beta"], rm, rv, EPS, momentum, training,
                                      d["res"].view(1, R, 1, C) if use_res else None, act)
    y = y.view(R, C)
    mask = (y > 0).cpu() if act == ACT_RELU else None
    r64 = bn_ref(as64(t), act, use_res, momentum, training, torch.float64, mask)
    r32 = bn_ref(t, act, use_res, momentum, training, torch.float32, mask)
    if act == ACT_RELU:
        check_relu_decisions(mask, r64["z"], what)

    nan = float("nan")
    gen = torch.Generator().manual_seed(21)
    pg, pb = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    dgamma = pg.to(DEV) if accumulate else torch.full((C,), nan, device=DEV)
    dbeta = pb.to(DEV) if accumulate else torch.full((C,), nan, device=DEV)
    dx, dres = ops.batchnorm_bwd(d["dy"].view(1, R, 1, C), d["x"].view(1, R, 1, C), y.view(1, R, 1, C), d["gamma"], mean, rstd,
                                 act, training, dgamma, dbeta, accumulate, True)
    j = Judge(what)
    for name, got in (("y", y), ("save_mean", mean), ("save_rstd", rstd), ("dx", dx.view(R, C)), ("running_mean", rm),
                      ("running_var", rv)):
        j.add(name, got, r32[name], r64[name])
    for name, got, pre in (("dgamma", dgamma, pg), ("dbeta", dbeta, pb)):
        if accumulate:
            j.add(name + " accumulate", got, pre + r32[name], pre.double() + r64[name])
        else:
            j.add(name, got, r32[name], r64[name])
    j.done()
    want_dres = torch.where(y > 0, d["dy"], torch.zeros_like(y)) if act == ACT_RELU else d["dy"]
    assert torch.equal(dres.view(R, C), want_dres)
    if not training:
        assert torch.equal(mean, d["rm0"]) and torch.equal(rm, d["rm0"]) and torch.equal(rv, d["rv0"])


@pytest.mark.parametrize("use_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("case", BN_CASES, ids=bn_id)
def test_batchnorm_training(case, act, use_res):
    """y, save_mean, save_rstd, dx, dgamma, dbeta and the running buffers (nn.BatchNorm2d in float64 from the same starting
    buffers: the unbiased count / (count - 1) factor) over momentum x accumulate; dresidual is dy under HIP's own ReLU mask,
    bit for bit."""
    for momentum in (0.1, 1.0):
        for accumulate in (0, 1):
            run_bn(case, act, use_res, momentum, accumulate, True)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("case", BN_CASES, ids=bn_id)
def test_batchnorm_eval(case, act):
    """training = 0: forward from the running buffers (left untouched), save_* equal to them, dx = rstd gamma g, dgamma and
    dbeta from the same sums."""
    for accumulate in (0, 1):
        run_bn(case, act, True, 0.1, accumulate, False)


def raw_bn_sums(x):
    from mdctgan_amd import _lib
    lib = _lib.load()
    R, C = x.shape
    part = torch.full((lib.mg_batchnorm_slices(), 2, C), float("nan"), dtype=torch.float64, device=DEV)
    assert part.numel() * 8 == lib.mg_batchnorm_workspace(C)
    _lib.check(lib.mg_batchnorm_sums(_lib.ptr(x), R, C, _lib.ptr(part), _lib.stream()), "mg_batchnorm_sums")
    return part


def raw_bn_fwd(x, gamma, beta, rm, rv, res, act, momentum, part, count, y, mean, rstd):
    from mdctgan_amd import _lib
    R, C = x.shape
    _lib.check(_lib.load().mg_batchnorm_fwd(_lib.ptr(x), R, C, EPS, momentum, 1, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(rm),
                                            _lib.ptr(rv), _lib.ptr(res), act, _lib.ptr(y), _lib.ptr(mean), _lib.ptr(rstd),
                                            _lib.ptr(part), float(count), _lib.stream()), "mg_batchnorm_fwd")


def raw_bn_bwd_sums(dy, x, y, mean, rstd, act):
    from mdctgan_amd import _lib
    lib = _lib.load()
    R, C = x.shape
    part = torch.full((lib.mg_batchnorm_slices(), 2, C), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(lib.mg_batchnorm_bwd_sums(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(y), R, C, _lib.ptr(mean), _lib.ptr(rstd), act,
                                         _lib.ptr(part), _lib.stream()), "mg_batchnorm_bwd_sums")
    return part


def raw_bn_bwd(dy, x, y, gamma, mean, rstd, act, dx, dres, dgamma, dbeta, accumulate, lpart, gpart, count):
    from mdctgan_amd import _lib
    R, C = x.shape
    _lib.check(_lib.load().mg_batchnorm_bwd(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(y), R, C, _lib.ptr(gamma), _lib.ptr(mean),
                                            _lib.ptr(rstd), act, 1, _lib.ptr(dx), _lib.ptr(dres), _lib.ptr(dgamma),
                                            _lib.ptr(dbeta), int(accumulate), _lib.ptr(lpart), _lib.ptr(gpart), float(count),
                                            _lib.stream()), "mg_batchnorm_bwd")


SYNC_SPLIT = (13, 22)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU], ids=["none", "relu"])
def test_syncbn_without_a_process_group(act):
    """count != R: (35, 70) as 13 + 22 rows, the partial sums of the two parts added on the device between the sums and the
    apply launches.  Concatenated y and dx, every part's save_* and running buffers, and the summed dgamma / dbeta equal the
    full-batch float64 result."""
    case = (35, 70, False)
    R, C, _ = case
    momentum = 0.1
    t = bn_inputs(case)
    d = {k: v.to(DEV) for k, v in t.items()}
    nan = float("nan")
    rows = (slice(0, SYNC_SPLIT[0]), slice(SYNC_SPLIT[0], R))
    xs = [d["x"][s].contiguous() for s in rows]
    parts = [raw_bn_sums(x) for x in xs]
    tot = parts[0] + parts[1]
    fw = []
    for s, x in zip(rows, xs):
        o = dict(y=torch.full_like(x, nan), save_mean=torch.full((C,), nan, device=DEV), save_rstd=torch.full((C,), nan, device=DEV),
                 running_mean=d["rm0"].clone(), running_var=d["rv0"].clone())
        raw_bn_fwd(x, d["gamma"], d["beta"], o["running_mean"], o["running_var"], d["res"][s].contiguous(), act, momentum, tot, R,
                   o["y"], o["save_mean"], o["save_rstd"])
        fw.append(o)
    y = torch.cat([o["y"] for o in fw])
    mask = (y > 0).cpu() if act == ACT_RELU else None
    r64 = bn_ref(as64(t), act, True, momentum, True, torch.float64, mask)
    r32 = bn_ref(t, act, True, momentum, True, torch.float32, mask)
    if act == ACT_RELU:
        check_relu_decisions(mask, r64["z"], "syncbn act%d" % act)
    j = Judge("syncbn 13+22 act%d" % act)
    j.add("y", y, r32["y"], r64["y"])
    for i, o in enumerate(fw):
        for name in ("save_mean", "save_rstd", "running_mean", "running_var"):
            j.add("%s part %d" % (name, i), o[name], r32[name], r64[name])
    for name in ("save_mean", "save_rstd", "running_mean", "running_var"):
        assert torch.equal(fw[0][name], fw[1][name]), name

    lparts = [raw_bn_bwd_sums(d["dy"][s].contiguous(), x, o["y"], o["save_mean"], o["save_rstd"], act)
              for s, x, o in zip(rows, xs, fw)]
    gtot = lparts[0] + lparts[1]
    bw = []
    for s, x, o, lp in zip(rows, xs, fw, lparts):
        g = dict(dx=torch.full_like(x, nan), dres=torch.full_like(x, nan), dgamma=torch.full((C,), nan, device=DEV),
                 dbeta=torch.full((C,), nan, device=DEV))
        raw_bn_bwd(d["dy"][s].contiguous(), x, o["y"], d["gamma"], o["save_mean"], o["save_rstd"], act, g["dx"], g["dres"],
                   g["dgamma"], g["dbeta"], 0, lp, gtot, R)
        bw.append(g)
    j.add("dx", torch.cat([g["dx"] for g in bw]), r32["dx"], r64["dx"])
    j.add("dgamma 1 + 2", bw[0]["dgamma"] + bw[1]["dgamma"], r32["dgamma"], r64["dgamma"])
    j.add("dbeta 1 + 2", bw[0]["dbeta"] + bw[1]["dbeta"], r32["dbeta"], r64["dbeta"])
    j.done()
    dres = torch.cat([g["dres"] for g in bw])
    assert torch.equal(dres, torch.where(y > 0, d["dy"], torch.zeros_like(y)) if act == ACT_RELU else d["dy"])


def test_batchnorm_channel_vectors_stay_inside_their_buffers():
    """C = 70 (a ragged second channel block): save_mean, save_rstd, running_*, dgamma, dbeta as views into buffers that carry
    64 sentinel floats after them."""
    case = (35, 70, False)
    R, C, _ = case
    d = {k: v.to(DEV) for k, v in bn_inputs(case).items()}
    names = ("save_mean", "save_rstd", "running_mean", "running_var", "dgamma", "dbeta")
    buf = {k: torch.full((C + 64,), 7.25, device=DEV) for k in names}
    v = {k: b[:C] for k, b in buf.items()}
    for k in ("save_mean", "save_rstd", "dgamma", "dbeta"):
        v[k].fill_(float("nan"))
    v["running_mean"].copy_(d["rm0"])
    v["running_var"].copy_(d["rv0"])
    y, dx = torch.full_like(d["x"], float("nan")), torch.full_like(d["x"], float("nan"))
    part = raw_bn_sums(d["x"])
    raw_bn_fwd(d["x"], d["gamma"], d["beta"], v["running_mean"], v["running_var"], None, ACT_RELU, 0.1, part, R, y, v["save_mean"],
               v["save_rstd"])
    lpart = raw_bn_bwd_sums(d["dy"], d["x"], y, v["save_mean"], v["save_rstd"], ACT_RELU)
    raw_bn_bwd(d["dy"], d["x"], y, d["gamma"], v["save_mean"], v["save_rstd"], ACT_RELU, dx, None, v["dgamma"], v["dbeta"], 0,
               lpart, lpart, R)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    for k in names:
        assert torch.isfinite(v[k]).all(), k
        assert (buf[k][C:] == 7.25).all(), k
    assert not torch.equal(v["running_mean"], d["rm0"]) and not torch.equal(v["running_var"], d["rv0"])


# ------------------------------------------------------------------------------------------------------------------
# mg_cat2_fwd / mg_cat2_bwd (csrc/elementwise.hip): torch.cat((a, b), -1) of NHWC tensors and its split
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 1, 2), (1000, 3, 5), (33, 64, 1)], ids=lambda s: "n%d_%d+%d" % s)
def test_cat2_fwd_bwd(shape):
    from mdctgan_amd import _lib
    lib = _lib.load()
    n, Ca, Cb = shape
    gen = torch.Generator().manual_seed(30)
    a, b = torch.randn(n, Ca, generator=gen).to(DEV), torch.randn(n, Cb, generator=gen).to(DEV)
    g = torch.randn(n, Ca + Cb, generator=gen).to(DEV)
    nan = float("nan")
    out = torch.full((n, Ca + Cb), nan, device=DEV)
    _lib.check(lib.mg_cat2_fwd(_lib.ptr(a), Ca, _lib.ptr(b), Cb, n, _lib.ptr(out), _lib.stream()), "mg_cat2_fwd")
    assert torch.equal(out, torch.cat((a, b), -1))
    for want_a, want_b in ((True, True), (True, False), (False, True)):
        ga, gb = torch.full((n, Ca), nan, device=DEV), torch.full((n, Cb), nan, device=DEV)
        _lib.check(lib.mg_cat2_bwd(_lib.ptr(g), Ca, Cb, n, _lib.ptr(ga) if want_a else None, _lib.ptr(gb) if want_b else None,
                                   _lib.stream()), "mg_cat2_bwd")
        assert torch.equal(ga, g[:, :Ca]) if want_a else torch.isnan(ga).all()
        assert torch.equal(gb, g[:, Ca:]) if want_b else torch.isnan(gb).all()
