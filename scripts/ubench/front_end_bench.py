"""The data path in front of the generator on many short utterances: AudioTestDataset.read_audio + post_processing + seg_pad_audio
(data/audio_dataset.py:141-186) per utterance against the packed front end.

    python scripts/ubench/front_end_bench.py                 # both parts, one JSON line
    python scripts/ubench/front_end_bench.py --add-noise     # with the noise of --add_noise in both variants

Part 1, the corpus of generate_many_bench.py (512 seeded utterances, lengths uniform in 3-6 s, 48 kHz files, 8 kHz -> 48 kHz,
segments of 32512 samples), two variants alternating in one process, each timed with device events over windows of at least
--window seconds after every shape has been warmed up:
  (a) make_test_segments per utterance       -- mean, shift, two mg_resample launches and the pad + unfold, 512 times
  (b) front_end_many + one mg_segments_gather over the plan's row table  -- a constant handful of launches
`library_launches` counts the calls into libmdctgan_hip.so per pass (the element-wise torch launches around them -- mean, add,
pad, unfold in (a); the shift arithmetic over [U] and the zero fills in (b) -- are not in it).
Part 2, one long regular row (2^22 samples): mg_resample_rows on a one-row table against mg_resample on the same data, per rate
pair, alternating, --row-calls back-to-back launches per window.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from generate_many_bench import RATE, corpus, timed          # noqa: E402  (the same seeded corpus and the same timer)

LR, SEG, BATCH = 8000, 32512, 64
COUNTED = ("mg_resample", "mg_resample_rows", "mg_rows_moments", "mg_add_noise_rows", "mg_segments_gather")


def count_library_launches(fn):
    """Calls into the library during one fn(), by entry point (mg_rows_moments is two kernel launches per call)."""
    from mdctgan_amd import _lib
    lib = _lib.load()
    counts, saved = {}, {name: getattr(lib, name) for name in COUNTED}

    def counting(name, f):
        def call(*args):
            counts[name] = counts.get(name, 0) + 1
            return f(*args)
        return call
    try:
        for name, f in saved.items():
            setattr(lib, name, counting(name, f))
        fn()
    finally:
        for name, f in saved.items():
            setattr(lib, name, f)
    torch.cuda.synchronize()
    return counts


def timed_calls(fn, calls):
    """Device-event time of `calls` back-to-back launches (no synchronisation between them) -> seconds per call."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e-3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per variant (the variants alternate)")
    ap.add_argument("--window", type=float, default=1.0, help="minimum seconds per timed window")
    ap.add_argument("--add-noise", action="store_true")
    ap.add_argument("--row-samples", type=int, default=1 << 22)
    ap.add_argument("--row-calls", type=int, default=500, help="back-to-back launches per timed window of part 2")
    args = ap.parse_args()
    dev = "cuda:0"
    from mdctgan_amd.mdct import seg_row_table, segments_gather
    from mdctgan_amd.resample import front_end_many, make_test_segments, resample, resample_length, resample_rows

    waves = corpus(args.utterances, args.seed, dev)
    real_seconds = sum(w.numel() for w in waves) / RATE
    rates = [RATE] * len(waves)
    opt = dict(lr_sampling_rate=LR, hr_sampling_rate=RATE, segment_length=SEG, gen_overlap=0, batch_size=BATCH,
               add_noise=args.add_noise, snr=55.0)
    noise_gen = torch.Generator(device=dev).manual_seed(args.seed)

    def per_utterance():
        for w in waves:
            make_test_segments(w.view(1, -1), RATE, RATE, LR, SEG, 0, add_noise=args.add_noise, generator=noise_gen)

    def packed():
        buf, _, plan = front_end_many(waves, rates, opt, generator=noise_gen)
        segments_gather(buf, seg_row_table(plan.in_rows, dev), SEG)

    variants = [("a_per_utterance_loop", per_utterance), ("b_front_end_many", packed)]
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    launches = {name: count_library_launches(fn) for name, fn in variants}
    times = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            times[name].append(timed(fn, args.window))
    result = {"utterances": len(waves), "real_audio_s": round(real_seconds, 1), "add_noise": args.add_noise,
              "device": torch.cuda.get_device_name(0)}
    for name, _ in variants:
        result[name] = {"ms_per_pass": [round(t * 1e3, 3) for t, _ in times[name]], "passes": [r for _, r in times[name]],
                        "library_launches": launches[name], "library_launches_total": sum(launches[name].values())}

    # part 2: one long regular row
    n = args.row_samples
    x = (0.05 * torch.randn(n, generator=torch.Generator().manual_seed(args.seed))).to(dev)
    rows = {}
    for orig, new in ((RATE, LR), (LR, RATE)):
        m = resample_length(n, orig, new)
        table = torch.tensor([(0, n, 0, m)], dtype=torch.int64, device=dev)
        out = torch.empty(m, device=dev)
        pair = [("mg_resample", lambda: resample(x.view(1, -1), orig, new)),
                ("mg_resample_rows", lambda: resample_rows(x, table, m, orig, new, out))]
        assert torch.equal(pair[0][1]().view(-1), pair[1][1]())
        got = {name: [] for name, _ in pair}
        for _ in range(args.rounds):
            for name, fn in pair:
                got[name].append(timed_calls(fn, args.row_calls))
        rows["%d_to_%d" % (orig, new)] = {name: [round(t * 1e6, 1) for t in ts] for name, ts in got.items()}
    result["one_row_us_per_call"] = {"samples": n, **rows}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
