"""Write tests/golden/lowpass_scipy.npz: what SciPy says about the filters of mdctgan_amd/lowpass.py.  Run once, by hand, where
SciPy is installed; the tests read the file and need no SciPy.

Per case k (both kinds; orders 1, 2, 3, 7, 8, 11, 12; edges of 1, 4 and 6 kHz at 48 kHz and 4 kHz at 16 kHz):
    kind_k, order_k, cutoff_k, fs_k, ripple_k (NaN for a Butterworth)
    sos_k        SciPy's second-order sections [ceil(order / 2), 6]
    h_sos_k      H(e^jw) at the 257 frequencies w = linspace(0, pi, 257) from the sections (sosfreqz)
    h_zpk_k      ... and from the zeros, poles and gain (freqz_zpk): a second float64 route to the same filter
    x_k          a seeded float32 input of 1200 samples
    y1_k         sosfilt(sos, x) in float64
    y2_k         sosfilt(sos, sosfilt(sos, x)[::-1])[::-1] in float64: forward and backward, both from a zero state
"""
import os

import numpy as np
from scipy import signal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (1, 2, 3, 7, 8, 11, 12)
EDGES = ((1000.0, 48000.0), (4000.0, 48000.0), (6000.0, 48000.0), (4000.0, 16000.0))
RIPPLES = (0.01, 0.1, 0.5, 1.0)
N_FREQ, N_SAMPLES = 257, 1200


def cases():
    out = []
    for kind in ("butter", "cheby1"):
        for i, order in enumerate(ORDERS):
            fc, fs = EDGES[i % len(EDGES)]
            out.append((kind, order, fc, fs, RIPPLES[i % len(RIPPLES)] if kind == "cheby1" else float("nan")))
    # the sharpest filters of the menu: the highest orders at the lowest edge (the poles closest to z = 1)
    out += [("butter", 12, 1000.0, 48000.0, float("nan")), ("cheby1", 11, 1000.0, 48000.0, 1.0), ("cheby1", 12, 1000.0, 48000.0, 1.0)]
    return out


def main():
    w = np.linspace(0.0, np.pi, N_FREQ)
    data = {"w": w}
    all_cases = cases()
    for k, (kind, order, fc, fs, rp) in enumerate(all_cases):
        design = (lambda out: signal.butter(order, fc, fs=fs, output=out)) if kind == "butter" else \
                 (lambda out: signal.cheby1(order, rp, fc, fs=fs, output=out))
        sos = design("sos")
        z, p, g = design("zpk")
        x = (0.5 * np.random.default_rng(1000 + k).standard_normal(N_SAMPLES)).astype(np.float32)
        y1 = signal.sosfilt(sos, x.astype(np.float64))
        y2 = signal.sosfilt(sos, y1[::-1])[::-1]
        data.update({"sos_%d" % k: sos, "h_sos_%d" % k: signal.sosfreqz(sos, worN=w)[1],
                     "h_zpk_%d" % k: signal.freqz_zpk(z, p, g, worN=w)[1], "x_%d" % k: x, "y1_%d" % k: y1,
                     "y2_%d" % k: np.ascontiguousarray(y2)})
    data["kind"] = np.asarray([c[0] for c in all_cases])
    data["order"] = np.asarray([c[1] for c in all_cases], dtype=np.int64)
    data["cutoff"] = np.asarray([c[2] for c in all_cases], dtype=np.float64)
    data["fs"] = np.asarray([c[3] for c in all_cases], dtype=np.float64)
    data["ripple"] = np.asarray([c[4] for c in all_cases], dtype=np.float64)
    path = os.path.join(REPO, "tests", "golden", "lowpass_scipy.npz")
    np.savez_compressed(path, **data)
    print("%s: %d cases, %d bytes" % (path, len(all_cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
