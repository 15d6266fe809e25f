"""What --lambda_lsd costs in the training step: the captured configs[1] step (bench.py's flagship workload: netG=global, ngf 64, 9
blocks, num_D 2, batch 8 x 32512 samples, float32) with --lambda_lsd 1 against the same step with 0.

    python scripts/ubench/lambda_lsd_bench.py                 # step times, one JSON line
    python scripts/ubench/lambda_lsd_bench.py --launches      # device launches of one eager step instead (torch.profiler)

Times: both models are built from the same seed and captured with make_graphed_step; the two replays alternate in one process,
each window is --calls back-to-back replays between device events, and the medians over --rounds windows are reported with every
window.  `term_us` is the difference of the medians: to_audio, mg_lsd_rows, mg_lsd_mean_loss and one add forward;
mg_lsd_rows_backward_seeded (two launches), to_audio's backward and the gradient join backward.

Launches (--launches): the device activities torch.profiler records (kernels, fills and copies alike) for one eager
optimize_parameters() of either model -- their difference is what the term adds to a step -- and, on one [8, 32512] batch, for
forward plus backward of the node (lsd_loss_term) and of the composition it replaces, (lambda * lsd_loss(...)).float(), both
started from a float32 device seed as the step starts its backward pass.
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


def build(lam, batch, dev):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    torch.manual_seed(42)
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "12000", "--netG", "global", "--ngf", "64",
                           "--n_downsample_global", "4", "--n_blocks_global", "9", "--n_blocks_attn_g", "0", "--num_D", "2",
                           "--batchSize", str(batch), "--gpu_ids", str(torch.device(dev).index), "--lambda_lsd", str(lam))
    return create_model(opt)


def device_launches(fn):
    """-> (count, {name: count}) of the device activities of one fn()"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {}
    for e in prof.events():
        if e.device_type == DeviceType.CUDA:
            names[e.name] = names.get(e.name, 0) + 1
    return sum(names.values()), names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per model (the two alternate)")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back replays per window")
    ap.add_argument("--launches", action="store_true", help="count the device launches of an eager step instead of timing replays")
    args = ap.parse_args()
    dev = "cuda:0"
    lr, hr = synth_batch(args.batch, 42, dev)
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "samples": T_SEG}
    models = {"lambda_0": build(0.0, args.batch, dev), "lambda_1": build(1.0, args.batch, dev)}
    if args.launches:
        from mdctgan_amd.metrics import lsd_loss, lsd_loss_term
        counts = {}
        for name, m in models.items():
            for _ in range(3):
                m.optimize_parameters(lr, hr)
            counts[name], _ = device_launches(lambda: m.optimize_parameters(lr, hr))
        opt = models["lambda_1"].opt
        x = (hr + 0.005 * torch.randn_like(hr)).requires_grad_()
        seed = torch.ones((), device=dev)

        def node():
            torch.autograd.grad(lsd_loss_term(x, hr, opt, 1.0), x, grad_outputs=seed)

        def composition():
            torch.autograd.grad((1.0 * lsd_loss(x, hr, opt)).float(), x, grad_outputs=seed)
        n_node, node_names = device_launches(node)
        n_comp, comp_names = device_launches(composition)
        result["launches"] = {"eager_step": counts, "term_adds_to_the_step": counts["lambda_1"] - counts["lambda_0"],
                              "node_forward_backward": n_node, "composition_forward_backward": n_comp,
                              "node": node_names, "composition": comp_names}
        print(json.dumps(result))
        return
    steps = {name: m.make_graphed_step(lr, hr, warmup=3) for name, m in models.items()}
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
    result["G_lsd"] = float(steps["lambda_1"]()["G_lsd"].item())
    print(json.dumps(result))


if __name__ == "__main__":
    main()
