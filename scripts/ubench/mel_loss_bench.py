"""The multi-scale mel-spectrogram L1 loss (metrics.mel_loss_term, csrc/mel_loss_rows.hip) against what a user writes without it --
the same loss composed from torch.stft, a matmul and log with autograd on the same device -- and what --lambda_mel costs in the
training step.

    python scripts/ubench/mel_loss_bench.py                # node against composition: times and launches, one JSON line
    python scripts/ubench/mel_loss_bench.py --step         # the captured configs[1] step with --lambda_mel 1 against 0

Default: bench.py's batch shape, B = 8 clips of 32512 samples at 48 kHz, the default resolutions (512, 128, 40), (1024, 256, 80),
(2048, 512, 160).  Two rows, forward plus backward from a float32 device seed, alternating in one process; each window is --calls
back-to-back repetitions between device events after a warm-up pass, and the medians over --rounds windows are reported with
every window.
  mel_loss_term        the node: per resolution two launches forward and two backward, plus one reduction
  torch_stft_autograd  mean over clips and resolutions of mean |ln max(W m_hr, 1e-5) - ln max(W m_sr, 1e-5)| with m =
                       sqrt(clamp(re^2 + im^2, 1e-7)), periodic Hann windows, reflect padding, W = metrics.mel_fbank; hr's
                       spectra recomputed every pass, as the kernels do
`launches` are the device activities torch.profiler records for one pass of either row (kernels, fills and copies alike);
`grad_rel_diff` is max|node - torch| / max|torch| of the gradient (float32 against float32), `loss_rel_diff` the same for the value.

--step: lambda_lsd_bench.py's measurement with --lambda_mel: both models from one seed, captured with make_graphed_step, the
replays alternating window by window.  With 0 the step is the one without the option -- the parent commit's -- launch for launch.
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


def torch_mel(hr, sr, resolutions, windows, fbanks):
    """the definition on [B, T] -> 0-dim float32"""
    total = 0.0
    for (n_fft, hop, _), w, fb in zip(resolutions, windows, fbanks):
        def logmel(a):
            s = torch.stft(a, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect", return_complex=True)
            return torch.log(torch.clamp(fb @ torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=1e-7)), min=1e-5))
        total = total + (logmel(hr) - logmel(sr)).abs().mean()
    return total / len(resolutions)


def build(lam, batch, dev):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    torch.manual_seed(42)
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "64",
                           "--n_downsample_global", "4", "--n_blocks_global", "9", "--n_blocks_attn_g", "0", "--num_D", "2",
                           "--batchSize", str(batch), "--gpu_ids", str(torch.device(dev).index), "--lambda_mel", str(lam))
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
        result["G_mel"] = float(steps["lambda_1"]()["G_mel"].item())
        print(json.dumps(result))
        return

    from mdctgan_amd.metrics import MEL_RESOLUTIONS, mel_fbank, mel_loss_term
    from mdctgan_amd.options import HR_SAMPLE_RATE as rate
    hr = hr.reshape(args.batch, -1).contiguous()
    x = (hr + 0.005 * torch.randn_like(hr)).requires_grad_()
    seed = torch.ones((), device=dev)
    windows = [torch.hann_window(n, periodic=True, dtype=torch.float64).float().to(dev) for n, _, _ in MEL_RESOLUTIONS]
    fbanks = [mel_fbank(rate, n, j).to(dev) for n, _, j in MEL_RESOLUTIONS]
    out = {}

    def node():
        loss = mel_loss_term(x, hr, rate, 1.0)
        out["node"] = (loss.detach(), torch.autograd.grad(loss, x, grad_outputs=seed)[0])

    def composition():
        loss = torch_mel(hr, x, MEL_RESOLUTIONS, windows, fbanks)
        out["torch"] = (loss.detach(), torch.autograd.grad(loss, x, grad_outputs=seed)[0])
    rows = [("mel_loss_term", node), ("torch_stft_autograd", composition)]
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
    result["torch_over_node"] = round(result["torch_stft_autograd"]["median_us"] / result["mel_loss_term"]["median_us"], 2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
