"""The metrics behind the generator on many short utterances: compute_matrics per utterance (generate_audio.py:57-67, one file at
a time) against the packed metrics.compute_matrics_many.

    python scripts/ubench/metrics_many_bench.py              # both parts, one JSON line

Part 1, the corpus of generate_many_bench.py (512 seeded utterances, lengths uniform in 3-6 s at 48 kHz; n_fft 512, i.e. a
1024-point STFT at hop 512), three variants alternating in one process, each timed with device events over windows of at least
--window seconds after a warm-up pass:
  (a) compute_matrics per utterance      -- mg_metrics_rows, 2 x (mg_stft_frames + the dense DFT GEMM), mg_lsd_frames and four
                                            .item() read-backs, 512 times
  (b) compute_matrics_many, packed       -- on (buffer, starts, lengths) operands, as evaluate_many calls it: one table copy,
                                            mg_metrics_rows_packed, mg_lsd_rows, mg_rows_moments, nothing read back
  (c) compute_matrics_many, lists        -- the same from three lists of waveforms: three packing copies more
`library_launches` counts the calls into libmdctgan_hip.so per pass (the element-wise torch launches around them are not in it).
Part 2, one long regular row (2^22 samples): mg_lsd_rows against power_spectra x 2 + mg_lsd_frames on the same data,
alternating, --row-calls back-to-back repetitions per window, for every transform size mg_lsd_rows serves.
"""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from front_end_bench import timed_calls                      # noqa: E402
from generate_many_bench import RATE, corpus, timed          # noqa: E402  (the same seeded corpus and the same timers)

COUNTED = ("mg_metrics_rows", "mg_stft_frames", "mg_conv_fwd_w", "mg_lsd_frames", "mg_metrics_rows_packed", "mg_lsd_rows",
           "mg_rows_moments")


def count_library_launches(fn):
    """Calls into the library during one fn(), by entry point (mg_rows_moments and mg_metrics_rows_packed are two kernel launches
    per call)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per variant (the variants alternate)")
    ap.add_argument("--window", type=float, default=1.0, help="minimum seconds per timed window")
    ap.add_argument("--row-samples", type=int, default=1 << 22)
    ap.add_argument("--row-calls", type=int, default=50, help="back-to-back repetitions per timed window of part 2")
    args = ap.parse_args()
    dev = "cuda:0"
    from mdctgan_amd import _lib
    from mdctgan_amd.mdct import kbdwin
    from mdctgan_amd.metrics import compute_matrics, compute_matrics_many, plan_metrics, power_spectra
    from mdctgan_amd.packed import aligned_layout, pack_waves

    opt = types.SimpleNamespace(n_fft=512, hop_length=256, win_length=512, center=True)
    hrs = corpus(args.utterances, args.seed, dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    srs = [h + 0.005 * torch.randn(h.numel(), device=dev, generator=gen) for h in hrs]
    lrs = [h + 0.015 * torch.randn(h.numel(), device=dev, generator=gen) for h in hrs]
    lengths = [h.numel() for h in hrs]
    real_seconds = sum(lengths) / RATE
    layout = aligned_layout(lengths, 64)
    packed = [(pack_waves(ws, layout, dev), layout.starts, lengths) for ws in (hrs, lrs, srs)]

    def per_utterance():
        return [compute_matrics(h, l, s, opt) for h, l, s in zip(hrs, lrs, srs)]

    def many_packed():
        return compute_matrics_many(packed[0], packed[1], packed[2], opt)

    def many_lists():
        return compute_matrics_many(hrs, lrs, srs, opt)

    variants = [("a_per_utterance_loop", per_utterance), ("b_compute_matrics_many_packed", many_packed),
                ("c_compute_matrics_many_lists", many_lists)]
    outs = [fn() for _, fn in variants]
    torch.cuda.synchronize()
    # the three agree (the packed pass has compute_matrics' bounds: tests/test_metrics_many_gpu.py)
    loop = torch.tensor(outs[0], dtype=torch.float64)
    assert torch.equal(outs[1], outs[2])
    worst_lsd = float(((outs[1][:, 6].cpu() - loop[:, 6]).abs() / loop[:, 6]).max())
    worst_snr = float((outs[1][:, 1].cpu() - loop[:, 1]).abs().max())
    launches = {name: count_library_launches(fn) for name, fn in variants}
    times = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            times[name].append(timed(fn, args.window))
    result = {"utterances": len(hrs), "real_audio_s": round(real_seconds, 1), "n_fft": 2 * opt.n_fft, "hop": 2 * opt.hop_length,
              "device": torch.cuda.get_device_name(0), "many_vs_loop": {"lsd_rel": worst_lsd, "snr_sr_db": worst_snr}}
    for name, _ in variants:
        result[name] = {"ms_per_pass": [round(t * 1e3, 3) for t, _ in times[name]], "passes": [r for _, r in times[name]],
                        "library_launches": launches[name], "library_launches_total": sum(launches[name].values())}
    del hrs, lrs, srs, packed, outs
    torch.cuda.empty_cache()

    # part 2: one long regular row
    lib = _lib.load()
    n = args.row_samples
    g = torch.Generator().manual_seed(args.seed)
    x = (0.05 * torch.randn(n, generator=g)).to(dev)
    y = x + (0.005 * torch.randn(n, generator=g)).to(dev)
    rows = {}
    for n_fft in (512, 1024, 2048):
        hop = n_fft // 2
        window = kbdwin(n_fft).to(dev)
        plan = plan_metrics([n], n_fft, hop, True)
        table = torch.tensor([(0, 0, 0, n)], dtype=torch.int64, device=dev)
        fs = torch.tensor(plan.frame_start, dtype=torch.int64, device=dev)
        fused_out = torch.empty(plan.total_frames, device=dev)
        chain_out = torch.empty(plan.total_frames, device=dev)

        def fused():
            _lib.check(lib.mg_lsd_rows(_lib.ptr(x), n, _lib.ptr(y), n, _lib.ptr(table), 1, _lib.ptr(fs), plan.total_frames, None,
                                       _lib.ptr(window), n_fft, hop, 1, _lib.ptr(fused_out), _lib.stream()), "mg_lsd_rows")

        def chain():
            sa, _ = power_spectra(x.view(1, -1), n_fft, hop, window, True)
            sb, _ = power_spectra(y.view(1, -1), n_fft, hop, window, True)
            _lib.check(lib.mg_lsd_frames(_lib.ptr(sa), _lib.ptr(sb), sa.shape[0], n_fft // 2 + 1, _lib.ptr(chain_out),
                                         _lib.stream()), "mg_lsd_frames")

        pair = [("power_spectra_x2_lsd_frames", chain), ("mg_lsd_rows", fused)]
        for _, fn in pair:
            fn()
        torch.cuda.synchronize()
        rel = float(((fused_out - chain_out).abs() / chain_out).max())
        got = {name: [] for name, _ in pair}
        for _ in range(args.rounds):
            for name, fn in pair:
                got[name].append(timed_calls(fn, args.row_calls))
        rows["n_fft_%d" % n_fft] = {"frames": plan.total_frames, "per_frame_rel_diff": rel,
                                    **{name: [round(t * 1e6, 1) for t in ts] for name, ts in got.items()}}
    result["one_row_us_per_call"] = {"samples": n, **rows}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
