"""Times K1 / K2 (to_spectro / to_audio forward, arcsinh, --abs_norm) and their backward kernels (mg_mdct4_backward,
mg_imdct4_backward) at 4096 clips x 32512 samples with torch events; reports us per call and GB/s against the 8 TB/s HBM peak.
Kernel-level times: run it under `rocprofv3 --kernel-trace --stats -- python scripts/ubench/codec_grad_bench.py`.

    python scripts/ubench/codec_grad_bench.py [--clips 4096] [--iters 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from mdctgan_amd import _lib  # noqa: E402
from mdctgan_amd.mdct import dct4_image, dct4_table, imdct4_backward, imdct4_codec, kbdwin, mdct4_backward, mdct4_codec  # noqa: E402

PEAK = 8.0e12


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=32512)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    B, T = a.clips, a.samples
    dev = "cuda"
    w = kbdwin(512).to(dev)
    d4 = dct4_table(256, dev)
    assert dct4_image(d4, 256) is not None
    codec = dict(codec=_lib.MG_CODEC_ARCSINH, gain=1000.0, norm_range=(-1.0, 1.0), src_range=(-5.0, 5.0))
    x = 0.05 * torch.randn(B, T, device=dev)
    s = mdct4_codec(x, w, d4, 512, **codec)["spec"]
    F = s.shape[1]
    gy = torch.randn(B, T, device=dev)
    gs = torch.randn(B, F, 256, device=dev)
    spec_b, audio_b = B * F * 256 * 4, B * T * 4
    rows = [
        ("K1 mdct4_ct_kernel (to_spectro)", lambda: mdct4_codec(x, w, d4, 512, **codec), audio_b + spec_b),
        ("K2 imdct4_ct_kernel (to_audio)", lambda: imdct4_codec(s, w, d4, 512, **codec), spec_b + audio_b),
        ("imdct4_ct_bwd_kernel (to_audio backward)",
         lambda: imdct4_backward(gy, s, w, 512, 256, F, codec=codec["codec"], gain=1000.0, norm_range=(-1.0, 1.0),
                                 src_range=(-5.0, 5.0)), audio_b + 2 * spec_b),
        ("mdct4_ct_bwd_kernel (to_spectro backward)",
         lambda: mdct4_backward(gs, s, w, 512, 256, T, codec=codec["codec"], gain=1000.0, norm_range=(-1.0, 1.0),
                                src_range=(-5.0, 5.0)), 2 * spec_b + audio_b),
    ]
    out = []
    for name, fn, nbytes in rows:
        us = timed(fn, a.iters)
        out.append({"kernel": name, "us": round(us, 1), "GB": round(nbytes / 1e9, 3), "GB/s": round(nbytes / us / 1e3, 1),
                    "of_peak": round(nbytes / (us * 1e-6) / PEAK, 3)})
        print("%-44s %9.1f us  %6.3f GB  %7.1f GB/s  %5.1f %% of 8 TB/s" % (name, us, nbytes / 1e9, nbytes / us / 1e3,
                                                                           100 * nbytes / (us * 1e-6) / PEAK))
    print(json.dumps({"clips": B, "samples": T, "rows": out}))


if __name__ == "__main__":
    main()
