"""The multi-resolution STFT loss (metrics.mrstft_loss_term, csrc/stft_loss_rows.hip) against what a user writes without it -- the
same loss composed from torch.stft with autograd on the same device -- and what --lambda_mrstft costs in the training step.

    python scripts/ubench/mrstft_loss_bench.py                # node against composition: times and launches, one JSON line
    python scripts/ubench/mrstft_loss_bench.py --step         # the captured configs[1] step with --lambda_mrstft 1 against 0

Default: bench.py's batch shape, B = 8 clips of 32512 samples, the default resolutions (512, 128), (1024, 256), (2048, 512).  Two
rows, forward plus backward from a float32 device seed, alternating in one process; each window is --calls back-to-back
repetitions between device events after a warm-up pass, and the medians over --rounds windows are reported with every window.
  mrstft_loss_term     the node: per resolution two launches forward and two backward, plus one reduction
  torch_stft_autograd  mean over clips and resolutions of sqrt(sum (m_hr - m_sr)^2 / sum m_hr^2) + mean |ln m_hr - ln m_sr| with
                       m = sqrt(clamp(re^2 + im^2, 1e-7)), periodic Hann windows, reflect padding; hr's spectra recomputed every
                       pass, as the kernels do
`launches` are the device activities torch.profiler records for one pass of either row (kernels, fills and copies alike);
`grad_rel_diff` is max|node - torch| / max|torch| of the gradient (float32 against float32), `loss_rel_diff` the same for the value.

--step: lambda_lsd_bench.py's measurement with --lambda_mrstft: both models from one seed, captured with make_graphed_step, the
replays alternating.  With 0 the step is the one without the option, launch for launch.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from bench import T_SEG, synth_batch                         # noqa: E402  (the flagship workload's batch)
from front_end_bench import timed_calls                      # noqa: E402
from lambda_lsd_bench import device_launches                 # noqa: E402


def torch_mrstft(hr, sr, resolutions, windows):
    """the definition on [B, T] -> 0-dim float32"""
    total = 0.0
    for (n_fft, hop), w in zip(resolutions, windows):
        def mag(a):
            s = torch.stft(a, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect", return_complex=True)
            return torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=1e-7))
        mh, ms = mag(hr), mag(sr)
        sc = torch.sqrt(((mh - ms) ** 2).sum((-2, -1)) / (mh ** 2).sum((-2, -1)))
        total = total + (sc + (torch.log(mh) - torch.log(ms)).abs().mean((-2, -1))).mean()
    return total / len(resolutions)


def build(lam, batch, dev):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    torch.manual_seed(42)
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "64",
                           "--n_downsample_global", "4", "--n_blocks_global", "9", "--n_blocks_attn_g", "0", "--num_D", "2",
                           "--batchSize", str(batch), "--gpu_ids", str(torch.device(dev).index), "--lambda_mrstft", str(lam))
    return create_model(opt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per row (the rows alternate)")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back repetitions per window")
    ap.add_argument("--step", action="store_true", help="time the captured training step with and without the term instead")
    args = ap.parse_args()
    dev = "cuda:0"
    lr, hr = synth_batch(args.batch, 42, dev)
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "samples": T_SEG}
    if args.step:
        steps = {name: build(lam, args.batch, dev).make_graphed_step(lr, hr, warmup=3)
                 for name, lam in (("lambda_0", 0.0), ("lambda_1", 1.0))}
        for run in steps.values():
            for _ in range(5):
                run()
        times = {name: [] for name in steps}
        for _ in range(args.rounds):
            for name, run in steps.items():
                times[name].append(timed_calls(run, args.calls))
        for name in steps:
            result[name] = {"median_us": round(statistics.median(times[name]) * 1e6, 1),
                            "windows_us": [round(t * 1e6, 1) for t in times[name]]}
        result["term_us"] = round(result["lambda_1"]["median_us"] - result["lambda_0"]["median_us"], 1)
        result["G_mrstft"] = float(steps["lambda_1"]()["G_mrstft"].item())
        print(json.dumps(result))
        return

    from mdctgan_amd.metrics import STFT_RESOLUTIONS, mrstft_loss_term
    hr = hr.reshape(args.batch, -1).contiguous()
    x = (hr + 0.005 * torch.randn_like(hr)).requires_grad_()
    seed = torch.ones((), device=dev)
    windows = [torch.hann_window(n, periodic=True, dtype=torch.float64).float().to(dev) for n, _ in STFT_RESOLUTIONS]
    out = {}

    def node():
        loss = mrstft_loss_term(x, hr, 1.0)
        out["node"] = (loss.detach(), torch.autograd.grad(loss, x, grad_outputs=seed)[0])

    def composition():
        loss = torch_mrstft(hr, x, STFT_RESOLUTIONS, windows)
        out["torch"] = (loss.detach(), torch.autograd.grad(loss, x, grad_outputs=seed)[0])
    rows = [("mrstft_loss_term", node), ("torch_stft_autograd", composition)]
    result["launches"] = {}
    for name, fn in rows:
        result["launches"][name], _ = device_launches(fn)
    (ln, gn), (lt, gt) = out["node"], out["torch"]
    result["loss"] = float(ln)
    result["loss_rel_diff"] = float((ln - lt).abs() / lt.abs())
    result["grad_rel_diff"] = float((gn - gt).abs().max() / gt.abs().max())
    times = {name: [] for name, _ in rows}
    for _ in range(args.rounds):
        for name, fn in rows:
            times[name].append(timed_calls(fn, args.calls))
    for name, _ in rows:
        result[name] = {"median_us": round(statistics.median(times[name]) * 1e6, 1),
                        "windows_us": [round(t * 1e6, 1) for t in times[name]]}
    result["torch_over_node"] = round(result["torch_stft_autograd"]["median_us"] / result["mrstft_loss_term"]["median_us"], 2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
