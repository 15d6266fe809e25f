"""The zero-phase IIR low-pass in front of the low-rate leg (mdctgan_amd/lowpass.py, csrc/sos_rows.hip): what it costs alone and
inside a training batch.

    python scripts/ubench/lowpass_rows_bench.py                 # B = 8 and 64, one JSON line

The corpus of generate_many_bench.py (seeded utterances of 3-6 s at 48 kHz), windows of 32512 samples drawn once per batch size and
cycled, 48 -> 8 -> 48 kHz, one order-10 Chebyshev-I filter (0.5 dB, edge 3.8 kHz) per row, forward and backward.  The variants
alternate in one process, each timed with device events around whole calls over windows of at least --window seconds after every
shape has been warmed up; median and min-max over --rounds windows:
  (a) sos_rows alone                          -- tables and coefficients already on the device: the six launches of mg_sos_rows
  (b) training_batch_many(out=...)            -- without the feature: the host plan, one table copy, mg_train_pair_rows
  (c) training_batch_many(lowpass=table)      -- the same with the filter: mg_sos_rows, mg_train_hr_rows, mg_train_lr_rows
  (d) make_graphed_training_batch's run       -- without the feature: one graph replay
  (e) ... with lowpass=spec                   -- the host draws and designs B filters, one copy, one replay of the longer chain
`share_of_step`: the median over the 10.9 ms captured training step of configs[1].  The parent commit's training_batch_many is
train_batch_bench.py run from the parent's tree in the same session, alternating with this one.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from generate_many_bench import RATE, corpus, timed          # noqa: E402  (the same seeded corpus and the same timer)

SEG, STEP_MS, LR_RATE = 32512, 10.9, 8000


def spread(ts):
    ms = [t * 1e3 for t, _ in ts]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "share_of_step": round(statistics.median(ms) / STEP_MS, 4), "passes": [r for _, r in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--tables", type=int, default=16, help="different crop-window tables cycled through")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per variant (the variants alternate)")
    ap.add_argument("--window", type=float, default=0.5, help="minimum seconds per timed window")
    args = ap.parse_args()
    dev = "cuda:0"
    from mdctgan_amd.lowpass import LowpassSpec, lowpass_sos, pad_sos, sos_rows, sos_table_bits
    from mdctgan_amd.packed import aligned_layout, upload_tables
    from mdctgan_amd.train_data import draw_windows, make_graphed_training_batch, pack_corpus, training_batch_many

    waves = corpus(args.files, args.seed, dev)
    packed = pack_corpus(waves, [RATE] * len(waves), dev)
    one = pad_sos(lowpass_sos("cheby1", 10, 3800.0, RATE, 0.5))
    spec = LowpassSpec(("cheby1",), (10, 10), (0.5, 0.5), (0.95, 0.95))
    result = {"files": len(waves), "segment_length": SEG, "filter": "cheby1 order 10, 0.5 dB, 3.8 kHz at 48 kHz, zero phase",
              "device": torch.cuda.get_device_name(0), "cases": {}}
    opt = dict(lr_sampling_rate=LR_RATE, hr_sampling_rate=RATE, segment_length=SEG)
    for B in args.batches:
        pick = torch.Generator().manual_seed(args.seed + B)
        tables = []
        for _ in range(args.tables):
            idx = torch.randint(0, len(waves), (B,), generator=pick).tolist()
            off, ln = draw_windows(packed, idx, SEG, RATE, generator=pick)
            tables.append((idx, off.tolist(), ln.tolist()))
        coef = np.stack([one] * B)
        lr_b, hr_b = (torch.empty(B, SEG, device=dev) for _ in range(2))
        # (a): the filter's own tables, uploaded once per window table
        lay = aligned_layout([SEG] * B)
        scratch = torch.empty(lay.total, dtype=torch.float32, device=dev)
        on_dev = []
        for idx, off, ln in tables:
            rows = np.asarray([(packed.starts[f] + o, n, s) for f, o, n, s in zip(idx, off, ln, lay.starts)], dtype=np.int64)
            t, c = upload_tables([rows, sos_table_bits(coef)], dev)
            on_dev.append((t, c.view(torch.float64)))
        turn = {"n": 0}

        def nxt(seq):
            turn["n"] += 1
            return seq[turn["n"] % len(seq)]

        def filter_alone():
            t, c = nxt(on_dev)
            sos_rows(packed.buffer, t, c, out=scratch, max_len=SEG)

        def batch_plain():
            idx, off, _ = nxt(tables)
            training_batch_many(packed, idx, opt, offsets=off, out=(lr_b, hr_b))

        def batch_lowpass():
            idx, off, _ = nxt(tables)
            training_batch_many(packed, idx, opt, offsets=off, out=(lr_b, hr_b), lowpass=coef)

        run_plain = make_graphed_training_batch(packed, B, opt)
        run_lowpass = make_graphed_training_batch(packed, B, opt, lowpass=spec)

        def replay_plain():
            idx, off, _ = nxt(tables)
            run_plain(idx, offsets=off)

        def replay_lowpass():
            idx, off, _ = nxt(tables)
            run_lowpass(idx, offsets=off)

        variants = [("a_sos_rows_alone", filter_alone), ("b_training_batch_many", batch_plain),
                    ("c_training_batch_many_lowpass", batch_lowpass), ("d_graph_replay", replay_plain),
                    ("e_graph_replay_lowpass", replay_lowpass)]
        for _, fn in variants:
            fn()
        torch.cuda.synchronize()
        # the eager and the captured filter give the same batch
        idx, off, _ = tables[0]
        want = training_batch_many(packed, idx, opt, offsets=off, lowpass=coef)
        got = run_lowpass(idx, offsets=off, lowpass=coef)
        assert all(torch.equal(w, g) for w, g in zip(want, got))
        times = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                times[name].append(timed(fn, args.window))
        result["cases"]["B%d" % B] = {name: spread(times[name]) for name, _ in variants}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
