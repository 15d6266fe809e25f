"""Inference throughput on many short utterances (configs[4]'s generator, 8k -> 48k, segments of 32512 samples).

    python scripts/ubench/generate_many_bench.py                 # the four variants, one JSON line
    python scripts/ubench/generate_many_bench.py --decode-only   # the two stitched decodes at B = 64, for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python scripts/ubench/generate_many_bench.py --decode-only

Corpus: a seeded set of utterances with lengths uniform in 3-6 s at 48 kHz.  Variants, alternating in one process, each timed
with device events over windows of at least one second after every shape has been warmed up:
  (a) generate() per utterance                 -- batch = the utterance's own 5-9 segments
  (b) generate_many, eager                     -- shared batches of 64, the last one at its live size
  (c) make_graphed_generate_many               -- one hipGraph over padded batches, replayed for the whole corpus
  (d) make_graphed_generate on ONE 64-segment utterance -- the ceiling the project quotes
The unit is audio-s/s over real samples (the utterances' own lengths: padding does not count).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

RATE = 48000
BATCH = 64


def make_model(dev):
    from mdctgan_amd import options
    from mdctgan_amd.pix2pixHD_model import create_model
    torch.manual_seed(42)
    opt = options.make_opt(*options.SPECTRAL_FLAGS, "--lr_sampling_rate", "8000", "--netG", "global", "--ngf", "64",
                           "--n_downsample_global", "4", "--n_blocks_global", "9", "--n_blocks_attn_g", "0", "--num_D", "2",
                           "--batchSize", str(BATCH), "--gpu_ids", str(torch.device(dev).index or 0))
    return create_model(opt)


def corpus(n, seed, dev):
    rng = np.random.RandomState(seed)
    lengths = rng.randint(3 * RATE, 6 * RATE + 1, size=n)
    gen = torch.Generator().manual_seed(seed)
    return [(0.05 * torch.randn(int(k), generator=gen)).to(dev) for k in lengths]


def timed(fn, min_seconds):
    """Device-event time of one call of fn, repeated until the window is at least min_seconds long -> seconds per call."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    start.record()
    while True:
        fn()
        reps += 1
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= min_seconds:
            break
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps, reps


def decode_only(dev, iters):
    """The plain stitched decode (64 segments of one utterance) and the row-table decode (64 rows of eight utterances) on the same
    spectrograms, `iters` launches each: for a kernel trace."""
    from mdctgan_amd import _lib, mdct
    from mdctgan_amd.generate_audio import plan_utterances
    L, M = 32512, 256
    F = L // M + 1
    gen = torch.Generator().manual_seed(1)
    spec = (2 * torch.rand(BATCH, F, M, generator=gen) - 1).to(dev)
    window, d4 = mdct.kbdwin(512).to(dev), mdct.dct4_table(M, dev)
    kw = dict(codec=_lib.MG_CODEC_ARCSINH, gain=1000.0, norm_range=(-1.0, 1.0), src_range=(-5.0, 5.0))
    plan = plan_utterances([7 * L + 100] * 7 + [8 * L - 5], L, L, 0, BATCH)
    assert plan.n_live == BATCH
    table = mdct.seg_row_table(plan.out_rows, dev)
    one = torch.zeros(BATCH * L, device=dev)
    packed = torch.zeros(plan.out_total, device=dev)
    names = []
    for _ in range(iters):
        mdct.imdct4_codec(spec, window, d4, 512, stitch=(one, 0, 0, L), **kw)
    names.append(_lib.load().mg_mdct_last_kernel(1).decode())
    for _ in range(iters):
        mdct.imdct4_codec(spec, window, d4, 512, rows=(packed, 0, table, L), **kw)
    names.append(_lib.load().mg_mdct_last_kernel(1).decode())
    torch.cuda.synchronize()
    print(json.dumps({"decode_only": names, "launches_each": iters}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="timed windows per variant (the variants alternate)")
    ap.add_argument("--window", type=float, default=1.0, help="minimum seconds per timed window")
    ap.add_argument("--decode-only", action="store_true")
    ap.add_argument("--decode-iters", type=int, default=200)
    args = ap.parse_args()
    dev = "cuda:0"
    if args.decode_only:
        return decode_only(dev, args.decode_iters)

    from mdctgan_amd.generate_audio import (generate, generate_many, make_graphed_generate, make_graphed_generate_many,
                                            plan_utterances, segment_audio)
    model = make_model(dev)
    L = model.opt.segment_length
    waves = corpus(args.utterances, args.seed, dev)
    real_seconds = sum(w.numel() for w in waves) / RATE
    plan = plan_utterances([w.numel() for w in waves], L, L, 0, BATCH)
    segs = [segment_audio(w, L, 0) for w in waves]
    ceiling_in = torch.cat(segs)[:BATCH].contiguous()
    if ceiling_in.shape[0] < BATCH:
        ceiling_in = ceiling_in.repeat(-(-BATCH // ceiling_in.shape[0]), 1)[:BATCH].contiguous()

    def variant_a():
        for s in segs:
            generate(model, s, batch_size=BATCH, gen_overlap=0)

    def variant_b():
        generate_many(model, waves, batch_size=BATCH, gen_overlap=0)

    graphed_many = make_graphed_generate_many(model, plan.n_live, sum(plan.lengths), batch_size=BATCH, gen_overlap=0)
    graphed_one = make_graphed_generate(model, ceiling_in, batch_size=BATCH, gen_overlap=0)
    variants = [("a_generate_loop", variant_a, real_seconds), ("b_generate_many", variant_b, real_seconds),
                ("c_graphed_many", lambda: graphed_many(waves), real_seconds),
                ("d_graphed_one_utterance", lambda: graphed_one(), BATCH * L / RATE)]
    # warm-up: every shape of every variant once (variant (a) meets every segment count of the corpus)
    for _, fn, _ in variants:
        fn()
    torch.cuda.synchronize()
    per_call = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, fn, _ in variants:
            per_call[name].append(timed(fn, args.window))
    result = {"utterances": len(waves), "real_audio_s": round(real_seconds, 1), "segments": plan.n_live,
              "batches": plan.n_batches, "live_row_fraction": round(plan.live_fraction, 4),
              "segments_per_utterance": [min(plan.segments), max(plan.segments)], "device": torch.cuda.get_device_name(0)}
    for name, _, audio_s in variants:
        best = min(t for t, _ in per_call[name])
        result[name] = {"audio_s_per_s": round(audio_s / best, 1), "seconds_per_pass": [round(t, 4) for t, _ in per_call[name]],
                        "passes": [r for _, r in per_call[name]]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
