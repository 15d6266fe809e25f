"""From WAV payload bytes in host memory to the packed low-rate buffer, and the PCM kernels alone.

    python scripts/ubench/wavio_bench.py                     # one JSON line

Part 1, the corpus of generate_many_bench.py as 16-bit mono files (512 seeded clips of 3-6 s at 48 kHz, 8 kHz -> 48 kHz), the payloads
held in host memory so that no disk read is timed.  Two variants alternate in one process; each pass is timed on the host clock
from the first byte touched to a device synchronisation (the host conversion of (a) is what is being compared, so device events
alone would not see it):
  (a) numpy int16 -> float32 / 32768 per file, torch.from_numpy, front_end_many(list)        -- the only route without wavio
  (b) the payloads copied into one pinned staging buffer, one H2D copy, mg_pcm_decode_rows with moments,
      front_end_many(packed triple, raw_moments=...)                                           -- wavio.read_wav_many's steps
`library_launches` counts the calls into libmdctgan_hip.so per pass.
Part 2, the kernels alone on the same rows, back-to-back launches between device events: decode (with and without moments) and
encode (16-bit and float32), beside the bytes each must move and the fraction of 6.3 TB/s (the delivered HBM bandwidth DESIGN.md
records) that makes.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from front_end_bench import count_library_launches, timed_calls          # noqa: E402
from generate_many_bench import RATE                                       # noqa: E402
import front_end_bench                                                     # noqa: E402

LR, SEG, BATCH, HBM = 8000, 32512, 64, 6.3e12
front_end_bench.COUNTED = front_end_bench.COUNTED + ("mg_pcm_decode_rows", "mg_pcm_encode_rows")


def host_timed(fn, passes):
    out = []
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5, help="passes per round and variant")
    ap.add_argument("--kernel-calls", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    from mdctgan_amd import wavio
    from mdctgan_amd.resample import front_end_many

    rng = np.random.RandomState(args.seed)
    lengths = rng.randint(3 * RATE, 6 * RATE + 1, size=args.clips)
    payloads = [np.clip(np.rint(0.05 * 32768 * rng.standard_normal(int(n))), -32768, 32767).astype("<i2").tobytes() for n in lengths]
    infos = [wavio.WavInfo(RATE, int(n), 1, 16, 1, 44, 2 * int(n)) for n in lengths]
    rates = [RATE] * args.clips
    opt = dict(lr_sampling_rate=LR, hr_sampling_rate=RATE, segment_length=SEG, gen_overlap=0, batch_size=BATCH)
    plan = wavio.plan_read(infos, "first")
    keep = {}

    def numpy_route():
        waves = [torch.from_numpy(np.frombuffer(p, dtype="<i2").astype(np.float32) / np.float32(32768)) for p in payloads]
        keep["a"] = front_end_many(waves, rates, opt, device=dev)[0]

    def device_route():
        host = torch.empty(plan.bytes_total, dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        for p, s in zip(payloads, plan.byte_starts):
            view[s:s + len(p)] = np.frombuffer(p, dtype=np.uint8)
        data = host.to(dev, non_blocking=True)
        out = torch.zeros(plan.layout.total, dtype=torch.float32, device=dev)
        _, mom = wavio.pcm_decode_rows(data, plan.rows, out, with_moments=True)
        keep["b"] = front_end_many((out, plan.layout.starts, plan.layout.lengths), rates, opt, raw_moments=mom)[0]

    variants = [("a_numpy_per_file", numpy_route), ("b_device_decode", device_route)]
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    assert torch.equal(keep["a"], keep["b"])
    launches = {name: count_library_launches(fn) for name, fn in variants}
    times = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            times[name] += host_timed(fn, args.passes)
    samples = int(lengths.sum())
    result = {"clips": args.clips, "samples": samples, "real_audio_s": round(samples / RATE, 1),
              "device": torch.cuda.get_device_name(0)}
    for name, _ in variants:
        result[name] = {"ms_per_pass_median": round(statistics.median(times[name]) * 1e3, 3),
                        "ms_per_pass_min": round(min(times[name]) * 1e3, 3), "ms_per_pass_max": round(max(times[name]) * 1e3, 3),
                        "passes": len(times[name]), "library_launches": launches[name],
                        "library_launches_total": sum(launches[name].values())}

    # part 2: the kernels alone
    view = np.zeros(plan.bytes_total, dtype=np.uint8)
    for p, s in zip(payloads, plan.byte_starts):
        view[s:s + len(p)] = np.frombuffer(p, dtype=np.uint8)
    data = torch.from_numpy(view).to(dev)
    table, = wavio.upload_tables([plan.rows], dev)
    out = torch.zeros(plan.layout.total, dtype=torch.float32, device=dev)
    kernels = {}

    def report(name, fn, bytes_moved):
        fn()
        ts = [timed_calls(fn, args.kernel_calls) for _ in range(args.rounds)]
        t = statistics.median(ts)
        kernels[name] = {"us_per_call": [round(x * 1e6, 1) for x in ts], "bytes": bytes_moved,
                         "fraction_of_6.3TBps": round(bytes_moved / t / HBM, 3)}

    report("decode_s16", lambda: wavio.pcm_decode_rows(data, plan.rows, out, False, table), 6 * samples)
    report("decode_s16_with_moments", lambda: wavio.pcm_decode_rows(data, plan.rows, out, True, table), 6 * samples)
    for code, nb in ((wavio.MG_PCM_S16, 2), (wavio.MG_PCM_F32, 4)):
        rows = plan.rows.copy()
        rows[:, 0], rows[:, 5], rows[:, 4] = plan.rows[:, 5], plan.rows[:, 0] * (nb // 2), code
        raw = torch.empty(plan.bytes_total * (nb // 2), dtype=torch.uint8, device=dev)
        enc_table, = wavio.upload_tables([rows], dev)
        clipped = torch.empty(rows.shape[0], dtype=torch.int64, device=dev)
        report("encode_%s" % ("s16" if nb == 2 else "f32"),
               lambda rows=rows, raw=raw, t=enc_table, c=clipped: wavio.pcm_encode_rows(out, rows, raw, t, c), (4 + nb) * samples)
    result["kernels"] = kernels
    print(json.dumps(result))


if __name__ == "__main__":
    main()
