"""Times mg_attention_fwd and mg_attention_bwd (K10, csrc/bot_attn.hip) with device events at B = 8, heads = 6, d = 128:
8 x 16 = 128 tokens (the narrow kernels: the baseline) and 8 x 32 = 256 tokens (the wide, MFMA-tiled family).  The work grows
4x from 128 to 256 tokens; the statement to check is  t(256) <= 4 t(128),  forward and backward separately.

Every buffer is allocated once; after a warm-up of each shape the two shapes alternate, `--reps` windows of `--inner`
back-to-back calls each, one event pair per window; the figure is the median window over its calls (min and max printed).

With --model-share it also builds the n_fft-1024 toy model whose generator carries a 256-token map (the model of
tests/test_bot_attn_wide_gpu.py), counts the attention calls of one optimisation step, times the step and those calls at
the model's shape and reports their share of the step.

    python scripts/ubench/attn_bench.py [--reps 15] [--inner 20] [--model-share]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from mdctgan_amd import _lib  # noqa: E402

DEV = "cuda"


class Shape:
    def __init__(self, B, fh, fw, heads, d, seed=1):
        lib = _lib.load()
        self.dims = (B, fh, fw, heads, d)
        n = fh * fw
        gen = torch.Generator().manual_seed(seed)
        self.qkv = torch.randn(B, fh, fw, 3 * heads * d, generator=gen).to(DEV)
        self.eh = torch.randn(fh, d, generator=gen).to(DEV)
        self.ew = torch.randn(fw, d, generator=gen).to(DEV)
        self.dout = torch.randn(B, fh, fw, heads * d, generator=gen).to(DEV)
        self.out = torch.empty(B, fh, fw, heads * d, device=DEV)
        self.P = torch.empty(B, heads, n, n, device=DEV)
        self.dqkv = torch.empty_like(self.qkv)
        self.dh, self.dw = torch.empty_like(self.eh), torch.empty_like(self.ew)
        self.ws_bytes = lib.mg_attention_bwd_workspace(B, fh, fw, heads, d)
        self.ws = torch.empty((self.ws_bytes + 3) // 4, device=DEV)
        self.lib = lib

    def fwd(self):
        B, fh, fw, heads, d = self.dims
        _lib.check(self.lib.mg_attention_fwd(_lib.ptr(self.qkv), _lib.ptr(self.eh), _lib.ptr(self.ew), B, fh, fw, heads, d,
                                             _lib.ptr(self.out), _lib.ptr(self.P), _lib.stream()), "mg_attention_fwd")

    def bwd(self):
        B, fh, fw, heads, d = self.dims
        _lib.check(self.lib.mg_attention_bwd(_lib.ptr(self.qkv), _lib.ptr(self.eh), _lib.ptr(self.ew), _lib.ptr(self.dout),
                                             _lib.ptr(self.P), B, fh, fw, heads, d, _lib.ptr(self.dqkv), _lib.ptr(self.dh),
                                             _lib.ptr(self.dw), 0, _lib.ptr(self.ws), self.ws.numel() * 4, _lib.stream()),
                   "mg_attention_bwd")


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def measure(shapes, reps, inner):
    """{(name, pass): [us per call, one per window]}, the shapes alternating."""
    for s in shapes.values():
        for _ in range(3):
            s.fwd()
            s.bwd()
    torch.cuda.synchronize()
    t = {(k, p): [] for k in shapes for p in ("fwd", "bwd")}
    for _ in range(reps):
        for k, s in shapes.items():
            t[(k, "fwd")].append(window(s.fwd, inner))
            t[(k, "bwd")].append(window(s.bwd, inner))
    return t


def model_share(reps, inner):
    from mdctgan_amd import ops, options
    from mdctgan_amd.pix2pixHD_model import create_model
    seg = 65024
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--n_fft", "1024", "--hop_length", "512",
                           "--win_length", "1024", "--bins", "128", "--segment_length", seg, "--netG", "global", "--ngf", "4",
                           "--n_downsample_global", "4", "--n_blocks_global", "2", "--n_blocks_attn_g", "1", "--heads_g", "2",
                           "--dim_head_g", "8", "--num_D", "2", "--ndf", "8", "--batchSize", "2", "--gpu_ids", "0")
    model = create_model(opt)
    g = torch.Generator().manual_seed(3)
    hr, lr = (0.05 * torch.randn(2, seg, generator=g)).to(DEV), (0.05 * torch.randn(2, seg, generator=g)).to(DEV)
    for _ in range(3):
        model.optimize_parameters(lr, hr)
    calls = {"fwd": [], "bwd": []}
    f0, b0 = ops.attention_fwd, ops.attention_bwd

    def cf(qkv, eh, ew, heads, d):
        calls["fwd"].append(tuple(qkv.shape[:3]) + (heads, d))
        return f0(qkv, eh, ew, heads, d)

    def cb(qkv, *a):
        calls["bwd"].append(tuple(qkv.shape[:3]) + (a[4], a[5]))
        return b0(qkv, *a)
    ops.attention_fwd, ops.attention_bwd = cf, cb
    try:
        model.optimize_parameters(lr, hr)
    finally:
        ops.attention_fwd, ops.attention_bwd = f0, b0
    torch.cuda.synchronize()
    step = statistics.median(window(lambda: model.optimize_parameters(lr, hr), 5) for _ in range(reps))
    dims = set(calls["fwd"]) | set(calls["bwd"])
    assert len(dims) == 1, dims
    s = Shape(*dims.pop())
    t = measure({"model": s}, reps, inner)
    tf, tb = statistics.median(t[("model", "fwd")]), statistics.median(t[("model", "bwd")])
    att = len(calls["fwd"]) * tf + len(calls["bwd"]) * tb
    return {"shape": list(s.dims), "fwd_calls": len(calls["fwd"]), "bwd_calls": len(calls["bwd"]), "fwd_us": round(tf, 1),
            "bwd_us": round(tb, 1), "step_us": round(step, 1), "attention_share_of_step": round(att / step, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--model-share", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_bench.py needs a GPU: nothing is timed without one")
    shapes = {"8x16": Shape(8, 8, 16, 6, 128), "8x32": Shape(8, 8, 32, 6, 128)}
    t = measure(shapes, a.reps, a.inner)
    res = {"B": 8, "heads": 6, "d": 128, "reps": a.reps, "inner": a.inner}
    for (k, p), v in t.items():
        res["%s_%s_us" % (k, p)] = round(statistics.median(v), 1)
        print("%-5s %s  median %8.1f us  min %8.1f  max %8.1f" % (k, p, statistics.median(v), min(v), max(v)))
    for p in ("fwd", "bwd"):
        r = statistics.median(t[("8x32", p)]) / statistics.median(t[("8x16", p)])
        res["%s_ratio_256_over_128" % p] = round(r, 3)
        print("%s: t(256 tokens) / t(128 tokens) = %.2f (target <= 4)" % (p, r))
    if a.model_share:
        res["model"] = model_share(a.reps, a.inner)
        print(res["model"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
