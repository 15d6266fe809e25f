"""The log-spectral distance as a loss: mg_lsd_rows (forward), mg_lsd_rows_backward (the two launches of csrc/lsd_rows_grad.hip) and
what a user writes without them -- forward plus backward through torch.stft with autograd on the same device.

    python scripts/ubench/lsd_loss_bench.py              # both workloads, one JSON line

Workload 1, the corpus of generate_many_bench.py: 512 seeded utterances, lengths uniform in 3-6 s at 48 kHz, packed; a 1024-point
transform at hop 512.  The torch composition has no packed form: it runs utterance by utterance (hr's spectrum is recomputed every
pass, as the kernels do).  Workload 2, a training batch: 64 segments of 32512 samples, dense; torch.stft takes it as one [64, T]
batch.  Per workload three rows, alternating in one process, each window timed with device events over --calls back-to-back
repetitions after a warm-up pass; the medians over --rounds windows are reported:
  mg_lsd_rows            the forward launch alone
  mg_lsd_rows_backward   the frame-gradient launch and the gather
  torch_stft_autograd    sqrt(mean((log10(|stft hr|^2 + 1e-6) - log10(|stft sr|^2 + 1e-6))^2)).mean() and .backward()
`grad_rel_diff` is max|HIP - torch| / max|torch| of the gradient per utterance, worst utterance (float32 against float32).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from front_end_bench import timed_calls                      # noqa: E402
from generate_many_bench import corpus                       # noqa: E402  (the same seeded corpus)


def torch_lsd(hr, sr, window, n_fft, hop):
    """util/util.py:171-175 on [T] or [B, T]"""
    def power(a):
        return torch.stft(a, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, pad_mode="reflect",
                          return_complex=True).abs().pow(2)
    d = torch.log10(power(hr) + 1e-6) - torch.log10(power(sr) + 1e-6)
    return torch.sqrt(torch.mean(d ** 2, dim=-2)).mean(-1)


def workload(name, hrs, srs, dense, n_fft, hop, rounds, calls, torch_calls, dev):
    from mdctgan_amd import _lib
    from mdctgan_amd.mdct import kbdwin
    from mdctgan_amd.metrics import plan_metrics
    from mdctgan_amd.packed import aligned_layout, pack_waves
    lib = _lib.load()
    lengths = [h.numel() for h in hrs]
    U = len(lengths)
    layout = aligned_layout(lengths, 64)
    hr, sr = pack_waves(hrs, layout, dev), pack_waves(srs, layout, dev)
    plan = plan_metrics(lengths, n_fft, hop, True)
    window = kbdwin(n_fft).to(device=dev, dtype=torch.float32)
    table = torch.tensor([(s, 0, s, n) for s, n in zip(layout.starts, lengths)], dtype=torch.int64, device=dev)
    fs = torch.tensor(plan.frame_start, dtype=torch.int64, device=dev)
    per_frame = torch.empty(plan.total_frames, device=dev)
    upstream = torch.tensor([1.0 / f for f in plan.frames], dtype=torch.float32, device=dev)
    grad = torch.zeros_like(sr)
    nbytes = lib.mg_lsd_rows_backward_workspace(plan.total_frames, n_fft)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def forward():
        _lib.check(lib.mg_lsd_rows(_lib.ptr(hr), hr.numel(), _lib.ptr(sr), sr.numel(), _lib.ptr(table), U, _lib.ptr(fs),
                                   plan.total_frames, None, _lib.ptr(window), n_fft, hop, 1, _lib.ptr(per_frame), _lib.stream()),
                   "mg_lsd_rows")

    def backward():
        _lib.check(lib.mg_lsd_rows_backward(_lib.ptr(hr), hr.numel(), _lib.ptr(sr), sr.numel(), _lib.ptr(table), U, _lib.ptr(fs),
                                            plan.total_frames, None, _lib.ptr(window), n_fft, hop, 1, _lib.ptr(upstream),
                                            _lib.ptr(grad), _lib.ptr(ws), nbytes, _lib.stream()), "mg_lsd_rows_backward")

    leaves = [torch.stack(srs).requires_grad_()] if dense else [s.clone().requires_grad_() for s in srs]
    consts = [torch.stack(hrs)] if dense else hrs

    def composed():
        for h, s in zip(consts, leaves):
            s.grad = None
            torch_lsd(h, s, window, n_fft, hop).sum().backward()

    rows = [("mg_lsd_rows", forward, calls), ("mg_lsd_rows_backward", backward, calls), ("torch_stft_autograd", composed, torch_calls)]
    for _, fn, _ in rows:
        fn()
    torch.cuda.synchronize()
    tg = leaves[0].grad if dense else None
    worst = 0.0
    for u in range(U):
        want = tg[u] if dense else leaves[u].grad
        got = grad[layout.starts[u]:layout.starts[u] + lengths[u]]
        worst = max(worst, float((got - want).abs().max() / want.abs().max()))
    times = {n: [] for n, _, _ in rows}
    for _ in range(rounds):
        for n, fn, c in rows:
            times[n].append(timed_calls(fn, c))
    out = {"utterances": U, "samples": sum(lengths), "frames": plan.total_frames, "n_fft": n_fft, "hop": hop,
           "workspace_MiB": round(nbytes / 2 ** 20, 1), "grad_rel_diff": worst}
    for n, _, _ in rows:
        out[n] = {"median_us": round(statistics.median(times[n]) * 1e6, 1), "windows_us": [round(t * 1e6, 1) for t in times[n]]}
    out["backward_over_forward"] = round(out["mg_lsd_rows_backward"]["median_us"] / out["mg_lsd_rows"]["median_us"], 2)
    out["torch_over_forward_plus_backward"] = round(out["torch_stft_autograd"]["median_us"] /
                                                    (out["mg_lsd_rows"]["median_us"] + out["mg_lsd_rows_backward"]["median_us"]), 2)
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per row (the rows alternate)")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back repetitions per window of the library rows")
    ap.add_argument("--torch-calls", type=int, default=2, help="the same for the torch composition")
    args = ap.parse_args()
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0)}
    hrs = corpus(args.utterances, args.seed, dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    srs = [h + 0.005 * torch.randn(h.numel(), device=dev, generator=gen) for h in hrs]
    name, out = workload("corpus_3_to_6_s", hrs, srs, False, 1024, 512, args.rounds, args.calls, args.torch_calls, dev)
    result[name] = out
    del hrs, srs
    torch.cuda.empty_cache()
    g = torch.Generator().manual_seed(args.seed)
    hrs = [(0.05 * torch.randn(32512, generator=g)).to(dev) for _ in range(64)]
    srs = [h + 0.005 * torch.randn(h.numel(), device=dev, generator=gen) for h in hrs]
    name, out = workload("segments_64_x_32512", hrs, srs, True, 1024, 512, args.rounds, 10 * args.calls, 10 * args.torch_calls, dev)
    result[name] = out
    print(json.dumps(result))


if __name__ == "__main__":
    main()
