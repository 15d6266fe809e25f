"""The data path in front of the training step: one (LR_audio, HR_audio) batch cut from a corpus that sits in HBM,
AudioDataset.readaudio + __getitem__ (data/audio_dataset.py:34-82) per item against the packed training batch.

    python scripts/ubench/train_batch_bench.py                 # B = 8 and 64, 48 -> 8 -> 48 kHz and 48 -> 12 -> 48 kHz, one JSON line
    python scripts/ubench/train_batch_bench.py --add-noise     # with the noise of --add_noise (no captured variant)

The corpus of generate_many_bench.py (seeded utterances, lengths uniform in 3-6 s, 48 kHz files), segments of 32512 samples, the
crop windows drawn once per batch size by draw_windows and cycled.  Three variants alternating in one process, each timed with device
events over windows of at least --window seconds after every shape has been warmed up; median and min-max over --rounds windows:
  (a) make_training_pair per item on its window of the corpus, copied into the batch tensors  -- what the parent of the packed
      path could do: two mg_resample launches for the low-rate leg (the 48 kHz high-rate leg is a copy), B times
  (b) training_batch_many(out=...)       -- the host plan, one table copy, mg_train_pair_rows
  (c) make_graphed_training_batch's run  -- the host plan, one table copy, one graph replay
`library_launches` counts the calls into libmdctgan_hip.so per batch (the element-wise torch launches around them -- the pads
and copies of (a) -- are not in it).  `share_of_step`: the median over the 10.9 ms captured training step of configs[1].
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import front_end_bench                                        # noqa: E402  (its launch counter)
from generate_many_bench import RATE, corpus, timed          # noqa: E402  (the same seeded corpus and the same timer)

SEG, STEP_MS = 32512, 10.9
front_end_bench.COUNTED = front_end_bench.COUNTED + ("mg_train_pair_rows",)


def spread(ts):
    ms = [t * 1e3 for t, _ in ts]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "share_of_step": round(statistics.median(ms) / STEP_MS, 4), "passes": [r for _, r in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--lr-rates", type=int, nargs="+", default=[8000, 12000])
    ap.add_argument("--tables", type=int, default=16, help="different crop-window tables cycled through")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per variant (the variants alternate)")
    ap.add_argument("--window", type=float, default=0.5, help="minimum seconds per timed window")
    ap.add_argument("--add-noise", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    from mdctgan_amd.resample import make_training_pair
    from mdctgan_amd.train_data import draw_windows, make_graphed_training_batch, pack_corpus, training_batch_many

    waves = corpus(args.files, args.seed, dev)
    packed = pack_corpus(waves, [RATE] * len(waves), dev)
    result = {"files": len(waves), "corpus_MB": round(packed.buffer.numel() * 4 / 2 ** 20, 1), "segment_length": SEG,
              "add_noise": args.add_noise, "device": torch.cuda.get_device_name(0), "cases": {}}
    noise_gen = torch.Generator(device=dev).manual_seed(args.seed)
    for lr_rate in args.lr_rates:
        for B in args.batches:
            opt = dict(lr_sampling_rate=lr_rate, hr_sampling_rate=RATE, segment_length=SEG, add_noise=args.add_noise, snr=55.0)
            pick = torch.Generator().manual_seed(args.seed + B)
            tables = []
            for _ in range(args.tables):
                idx = torch.randint(0, len(waves), (B,), generator=pick).tolist()
                off, ln = draw_windows(packed, idx, SEG, RATE, generator=pick)
                tables.append((idx, off.tolist(), ln.tolist()))
            lr_b, hr_b = (torch.empty(B, SEG, device=dev) for _ in range(2))
            turn = {"n": 0}

            def table():
                turn["n"] += 1
                return tables[turn["n"] % len(tables)]

            def per_item():
                idx, off, ln = table()
                for b, (f, o, n) in enumerate(zip(idx, off, ln)):
                    s0 = packed.starts[f] + o
                    lr, hr = make_training_pair(packed.buffer[s0:s0 + n].view(1, -1), RATE, RATE, lr_rate, SEG,
                                                add_noise=args.add_noise, generator=noise_gen)
                    lr_b[b].copy_(lr[0])
                    hr_b[b].copy_(hr[0])

            def packed_batch():
                idx, off, _ = table()
                training_batch_many(packed, idx, opt, offsets=off, out=(lr_b, hr_b), noise_generator=noise_gen)

            variants = [("a_per_item_loop", per_item), ("b_training_batch_many", packed_batch)]
            if not args.add_noise:
                run = make_graphed_training_batch(packed, B, opt)

                def replay():
                    idx, off, _ = table()
                    run(idx, offsets=off)
                variants.append(("c_graph_replay", replay))
            for _, fn in variants:
                fn()
            torch.cuda.synchronize()
            if not args.add_noise:                               # the three variants give the same batch
                idx, off, _ = tables[0]
                turn["n"] = -1
                per_item()
                want = (lr_b.clone(), hr_b.clone())
                got = training_batch_many(packed, idx, opt, offsets=off)
                rep = run(idx, offsets=off)
                assert all(torch.equal(w, g) and torch.equal(w, r) for w, g, r in zip(want, got, rep))
            launches = {name: front_end_bench.count_library_launches(fn) for name, fn in variants}
            times = {name: [] for name, _ in variants}
            for _ in range(args.rounds):
                for name, fn in variants:
                    times[name].append(timed(fn, args.window))
            case = {name: dict(spread(times[name]), library_launches=launches[name]) for name, _ in variants}
            result["cases"]["lr%d_B%d" % (lr_rate, B)] = case
    print(json.dumps(result))


if __name__ == "__main__":
    main()
