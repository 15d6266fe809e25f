"""Call-trace recorder for the autograd plumbing (mdctgan_amd/functional.py, optim.py): what the Python side asks of the launchers,
in order, without looking at a single tensor value or address.  scripts/gen_functional_calls_golden.py writes the trace of the five
tiny SCENARIOS below to tests/golden/functional_calls.json; tests/test_functional_calls_gpu.py replays them and compares.

A trace is a list of records:
    ["op", name, {parameter: value}]   a call of a public launcher of mdctgan_amd.ops, its arguments bound to the signature (so a
                                       default, a positional and a keyword spelling of the same value are the same record);
    ["ready", parameter name]          the grad-ready hook (functional.register_grad_ready_hook), in call order;
    ["state", {parameter name: [_mg_fresh, _mg_inf_checked, _mg_known_zero, _mg_g16 is set]}]   after each step (absent: null).
Values: a geometry struct as its field list, a tensor as [shape, dtype], None / bool / int / float / str as themselves, lists and
tuples element by element, a device as its type, anything else as its type's name.
"""
import inspect
import json
import os

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "functional_calls.json")
DEV = "cuda"

# the pure queries of ops.py: they neither launch nor allocate, and how often the host asks them is not behaviour
QUERIES = frozenset((
    "conv_geom", "plan_name", "plan_flops", "conv_flops", "wino_weights_bytes", "traits", "tiles_are_casts", "precast_ok",
    "wino_vnext_ok", "wino_images_half", "wino_vnext_positions", "wino_md_from_norm_ok", "wgrad_checks_finite", "wgrad_h16_ok",
    "wgrad_adam_ok", "weights_are_casts"))


def _enc(a):
    from mdctgan_amd import _lib
    if a is None or isinstance(a, (bool, int, float, str)):
        return a
    if isinstance(a, torch.Tensor):
        return [list(a.shape), str(a.dtype)]
    if isinstance(a, _lib.ConvGeom):
        return [getattr(a, n) for n, _ in a._fields_]
    if isinstance(a, (list, tuple)):
        return [_enc(v) for v in a]
    if isinstance(a, torch.device):
        return a.type
    return type(a).__name__


class Recorder:
    """with Recorder(names) as rec: ...; rec.log.  names: {parameter name: parameter} (the hook and state records speak of these)."""

    def __init__(self, names):
        self.log = []
        self.names = dict(names)
        self._by_id = {id(p): k for k, p in self.names.items()}

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapped(*args, **kwargs):
            b = sig.bind(*args, **kwargs)
            b.apply_defaults()
            self.log.append(["op", name, {k: _enc(v) for k, v in b.arguments.items()}])
            return fn(*args, **kwargs)
        return wrapped

    def _ready(self, p):
        self.log.append(["ready", self._by_id.get(id(p), "?")])

    def state(self):
        self.log.append(["state", {k: [getattr(p, "_mg_fresh", None), getattr(p, "_mg_inf_checked", None),
                                        getattr(p, "_mg_known_zero", None), getattr(p, "_mg_g16", None) is not None]
                                   for k, p in self.names.items()}])

    def __enter__(self):
        from mdctgan_amd import functional as Fh
        from mdctgan_amd import ops
        self._orig = {k: f for k, f in vars(ops).items()
                      if inspect.isfunction(f) and f.__module__ == ops.__name__ and not k.startswith("_") and k not in QUERIES}
        for k, f in self._orig.items():
            setattr(ops, k, self._wrap(k, f))
        Fh.register_grad_ready_hook(self._ready)
        return self

    def __exit__(self, *exc):
        from mdctgan_amd import functional as Fh
        from mdctgan_amd import ops
        Fh.remove_grad_ready_hook(self._ready)
        for k, f in self._orig.items():
            setattr(ops, k, f)
        return False


def _model(*flags):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    from oracle import nets as onets
    m = create_model(options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", *flags, "--n_blocks_attn_g", "0",
                                      "--num_D", "2", "--gpu_ids", "0"))
    onets.fill_deterministic(m.netG)
    onets.fill_deterministic(m.netD)
    names = {"G." + k: p for k, p in m.netG.named_parameters()}
    names.update(("D." + k, p) for k, p in m.netD.named_parameters())
    return m, names


def _steps(m, rec, lr, hr, n=3):
    for _ in range(n):
        m.optimize_parameters(lr, hr)
        rec.state()


def run_float32():
    """The model of test_next_layer_winograd_image_is_bit_identical: step 0 on the separate kernels, steps 1 and 2 on the fused-Adam
    path and the persistent U, then two inference passes (one weight-image cache fill, one hit)."""
    import numpy as np
    g = np.load(os.path.join(REPO, "tests", "golden", "g6_step_global.npz"), allow_pickle=False)
    lr, hr = torch.from_numpy(g["lr"]).to(DEV), torch.from_numpy(g["hr"]).to(DEV)
    m, names = _model("--netG", "global", "--ngf", "8", "--n_blocks_global", "3", "--ndf", "8", "--batchSize", "2", "--bins", "32",
                      "--segment_length", "7936")
    with Recorder(names) as rec:
        _steps(m, rec, lr, hr)
        with torch.no_grad():
            m.inference(lr)
            m.inference(lr)
    torch.cuda.synchronize()
    return rec.log


def run_fp16():
    """The model and inputs of test_producer_written_float16_copies_change_nothing: float16-stored gradients, both hand-over
    directions, the row-sliced "G" pass, the producer flags."""
    torch.manual_seed(5)
    m, names = _model("--netG", "local", "--ngf", "32", "--n_downsample_global", "2", "--n_blocks_global", "2", "--n_blocks_local", "2",
                      "--ndf", "64", "--batchSize", "2", "--bins", "64", "--segment_length", "16128", "--fp16")
    gen = torch.Generator().manual_seed(11)
    hr = (0.1 * torch.randn(2, 16128, generator=gen)).to(DEV)
    lr = (0.1 * torch.randn(2, 16128, generator=gen)).to(DEV)
    m.scaler.state[0] = 64.0
    with Recorder(names) as rec:
        _steps(m, rec, lr, hr)
    torch.cuda.synchronize()
    return rec.log


def run_fp16_checked():
    """The model and inputs of test_producer_side_inf_check_changes_nothing (a wider trunk under --fp16): weight-gradient kernels
    that run the GradScaler's check on their own results, and whatever gradients that trunk stores as float16."""
    torch.manual_seed(5)
    m, names = _model("--netG", "global", "--ngf", "16", "--n_blocks_global", "2", "--ndf", "8", "--batchSize", "2", "--bins", "32",
                      "--segment_length", "7936", "--fp16")
    gen = torch.Generator().manual_seed(11)
    hr = (0.1 * torch.randn(2, 7936, generator=gen)).to(DEV)
    lr = (0.1 * torch.randn(2, 7936, generator=gen)).to(DEV)
    m.scaler.state[0] = 64.0
    with Recorder(names) as rec:
        _steps(m, rec, lr, hr, n=2)
    torch.cuda.synchronize()
    return rec.log


def run_bare():
    """The three public wrappers without a model or an optimiser: B 2, 8x8, 8 -> 16 channels, float32, every weight and bias
    requiring gradient."""
    from mdctgan_amd import functional as Fh
    CL = torch.channels_last
    gen = torch.Generator().manual_seed(0)

    def param(*shape):
        t = (0.1 * torch.randn(*shape, generator=gen)).to(DEV)
        return torch.nn.Parameter(t.contiguous(memory_format=CL) if t.dim() == 4 else t)

    def bwd(y):
        y.backward(torch.ones_like(y))
        rec.state()

    x = torch.randn(2, 8, 8, 8, generator=gen).to(DEV).contiguous(memory_format=CL).requires_grad_()
    p = dict(w=param(16, 8, 3, 3), b=param(16), wt=param(8, 16, 3, 3), bt=param(16), w1=param(16, 8, 3, 3), b1=param(16),
             w2=param(8, 16, 3, 3), b2=param(8))
    with Recorder(p) as rec:
        # overwrite, accumulate; then a bias without a buffer beside a weight with one: two accumulate flags, the separate colsum
        for it in range(3):
            if it == 2:
                p["b"].grad = None
            bwd(Fh.conv2d(x, p["w"], p["b"], stride=1, padding=1, act=Fh.ACT_LRELU02))
        # the transposed weight-gradient tail and its colsum over Ci
        bwd(Fh.conv_transpose2d(x, p["wt"], p["bt"], stride=2, padding=1))
        # a ResnetBlock by hand: the skip connection's gradient travels in a SkipGrad from the second node to the first
        skip = Fh.SkipGrad()
        h = Fh.conv_instnorm(x, p["w1"], p["b1"], 1, True, Fh.ACT_RELU, None, 1e-5, True, ("take", skip), next_reflect=True)
        bwd(Fh.conv_instnorm(h, p["w2"], p["b2"], 1, True, Fh.ACT_NONE, x, 1e-5, True, ("give", skip)))
    torch.cuda.synchronize()
    return rec.log


def run_fused_tail():
    """The fused-Adam tail of _conv_backward itself: a trunk-sized 3x3 layer (the float32 model's geometry) called through plain
    conv2d with a separate InstanceNorm behind, so that the InstanceNorm-to-image fast path of conv_instnorm is not there to take
    it; under fused_adam_scope the weight gradient, Adam and the next transform are one call and only the bias is announced.
    Three steps: the optimiser's arenas exist from the first zero_grad() on."""
    from mdctgan_amd import functional as Fh
    from mdctgan_amd.optim import FusedAdam
    CL = torch.channels_last
    gen = torch.Generator().manual_seed(0)
    w = torch.nn.Parameter((0.05 * torch.randn(128, 128, 3, 3, generator=gen)).to(DEV).contiguous(memory_format=CL))
    b = torch.nn.Parameter((0.05 * torch.randn(128, generator=gen)).to(DEV))
    Fh.mark_bias_feeds_norm(b)
    x = torch.randn(2, 128, 2, 16, generator=gen).to(DEV).contiguous(memory_format=CL).requires_grad_()
    opt = FusedAdam([w, b], lr=1e-3, betas=(0.5, 0.999))
    with Recorder(dict(w=w, b=b)) as rec:
        for _ in range(3):
            opt.zero_grad()
            with Fh.fused_adam_scope(opt):
                y = Fh.instance_norm_act(Fh.conv2d(x, w, b, stride=1, padding=1, reflect=True), Fh.ACT_RELU)
                y.backward(torch.ones_like(y))
            opt.step()
            rec.state()
    torch.cuda.synchronize()
    return rec.log


SCENARIOS = {"float32": run_float32, "fp16": run_fp16, "fp16_checked": run_fp16_checked, "bare": run_bare,
             "fused_tail": run_fused_tail}


def normal(log):
    """A trace as the JSON file gives it back (tuples are lists there)."""
    return json.loads(json.dumps(log))


def pack(traces):
    """{scenario: trace} -> the file's content: every distinct record once, the traces as indices into that table (steps 1 and 2 of
    a model repeat each other record for record)."""
    table, index, out = [], {}, {}
    for name, log in traces.items():
        seq = out[name] = []
        for r in log:
            key = json.dumps(r, sort_keys=True)
            if key not in index:
                index[key] = len(table)
                table.append(r)
            seq.append(index[key])
    return {"records": table, "scenarios": out}


def unpack(doc):
    return {name: [doc["records"][i] for i in seq] for name, seq in doc["scenarios"].items()}
