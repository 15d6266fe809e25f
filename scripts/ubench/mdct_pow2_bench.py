"""Times K1' / K2' / the stitched K2' (csrc/mdct_pow2.hip; to_spectro / to_audio, arcsinh, --abs_norm) against the generic
composition on the same build (MG_MDCT_POW2=0: mg_frames_window + dense GEMM + mg_codec_* + mg_overlap_add [+ mg_stitch_segments])
for n_fft 256 / 1024 / 2048 at 8, 64 and 4096 clips of 32512 samples, with K1 / K2 at n_fft 512 as the yardstick.  Device-event
timings; the two routes alternate window by window in one process; per point: median window, spread of the windows, algorithmic
bytes B (T + F M) 4 and GB/s against the 6.3 TB/s the part delivers.

    python scripts/ubench/mdct_pow2_bench.py [--clips 8 64 4096] [--n_fft 256 1024 2048] [--windows 4]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from mdctgan_amd import _lib, options, ops  # noqa: E402
from mdctgan_amd.pix2pixHD_model import Audio2MDCT  # noqa: E402

DELIVERED = 6.3e12


def window_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(fn, routes, iters, windows):
    """{route: [us per window]}: warm-up per route, then the routes take turns, one window each."""
    times = {r: [] for r in routes}
    for r in routes:
        os.environ["MG_MDCT_POW2"] = r
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(windows):
        for r in routes:
            os.environ["MG_MDCT_POW2"] = r
            times[r].append(window_us(fn, iters))
    os.environ.pop("MG_MDCT_POW2", None)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[8, 64, 4096])
    ap.add_argument("--n_fft", type=int, nargs="+", default=[256, 1024, 2048, 512])
    ap.add_argument("--samples", type=int, default=32512)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--overlap", type=int, default=1024)
    a = ap.parse_args()
    lib = _lib.load()
    rows = []
    for n_fft in a.n_fft:
        hop = n_fft // 2
        pre = Audio2MDCT(options.make_opt(*options.SPECTRAL_FLAGS, "--n_fft", n_fft, "--hop_length", hop, "--win_length", n_fft,
                                          "--lr_sampling_rate", "12000", "--gpu_ids", "0"))
        routes = ["1", "0"] if pre.fast else ["1"]               # n_fft 512: K1 / K2, one route
        for B in a.clips:
            T = a.samples
            iters = 50 if B >= 1024 else 200                      # >= 200 launches per point, windows well above a millisecond
            x = 0.05 * torch.randn(B, T, device="cuda")
            with torch.no_grad():
                s, _, norm = pre.to_spectro(x)
                F = s.shape[2]
                seg = (F - 1) * hop
                total = lib.mg_stitch_length(B, seg, a.overlap)
                out = torch.empty(total, device="cuda")

                def stitched():
                    if pre.has_stitched_decoder:
                        return pre.to_audio(s, norm, stitch=(out, a.overlap, 0, seg))
                    return ops.stitch_segments(pre.to_audio(s, norm), seg, a.overlap)
                enc_b, dec_b = B * (T + F * hop) * 4, B * (F * hop + seg) * 4
                for what, fn, nbytes in (("encode", lambda: pre.encode(x), enc_b), ("decode", lambda: pre.to_audio(s, norm), dec_b),
                                         ("stitched", stitched, B * F * hop * 4 + total * 4)):
                    t = alternate(fn, routes, iters, a.windows)
                    new = statistics.median(t["1"])
                    kern = lib.mg_mdct_last_kernel(0 if what == "encode" else 1).decode()
                    row = {"n_fft": n_fft, "clips": B, "op": what, "kernel": kern, "new_us": round(new, 1),
                           "new_spread": round((max(t["1"]) - min(t["1"])) / new, 3), "GB": round(nbytes / 1e9, 4),
                           "GB/s": round(nbytes / new / 1e3, 1), "of_6.3TB/s": round(nbytes / (new * 1e-6) / DELIVERED, 3)}
                    if "0" in t:
                        comp = statistics.median(t["0"])
                        row.update(comp_us=round(comp, 1), comp_spread=round((max(t["0"]) - min(t["0"])) / comp, 3),
                                   speedup=round(comp / new, 2))
                    rows.append(row)
                    print("n_fft %4d  %4d clips  %-8s  new %9.1f us (+-%4.1f %%)  composition %10s us  x%-6s %8.1f GB/s  %5.1f %% of 6.3 TB/s"
                          % (n_fft, B, what, new, 100 * row["new_spread"], row.get("comp_us", "-"), row.get("speedup", "-"), row["GB/s"],
                             100 * row["of_6.3TB/s"]), flush=True)
            del x, s, out
            torch.cuda.empty_cache()
    print(json.dumps({"samples": a.samples, "rows": rows}))


if __name__ == "__main__":
    main()
