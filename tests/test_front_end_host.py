"""The packed front end without a GPU.

1. plan_front_end is host arithmetic: its lengths are the lengths oracle.resample.inference_segments produces, every packed
   buffer starts its utterances at multiples of 64, and the embedded plan is plan_utterances over the final lengths.
2. Every new entry point rejects null pointers, an empty table and non-positive rates or lengths with MG_ERR_ARG before any
   launch.  The calls run in child processes (one per entry point), so that a signal shows as the child's exit status; the
   pointers are arbitrary non-null integers, never dereferenced because the call returns first.
3. The noise bar of tests/test_front_end_gpu.py has teeth: the reference's own five lines on torch CPU float32 pass it; the same
   lines with the signal power divided by the waveform's length instead of segment_length, or with the biased standard deviation,
   miss it on 3000-sample rows.  (The biased deviation is worth a factor 1 + 1 / 2N on the noise: at --snr 55 the noise itself is
   1e-3 of the signal, the fault 2e-7 of it -- below the float32 rounding of lr + noise that the bar allows.  It shows at --snr
   10, where the noise is a fifth of the signal.)
The resampler's parity with torchaudio is unpinned (oracle/resample.py), the noise's beyond the restatement in the GPU file.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_front_end_gpu as T
from oracle import resample as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MG_ERR_ARG = -1
SEG = 4096
LENGTHS = [1, 5, 4095, 4096, 4097, 20000]
RATES = [48000, 44100, 16000, 8000]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the plan
# ---------------------------------------------------------------------------------------------------------------------
_oracle_lengths = {}


def oracle_length(n, fs, lr_rate, is_lr_input):
    """Length of R.inference_segments' lr_audio for a waveform of n samples at fs Hz (computed once per case)."""
    key = (n, fs, lr_rate, is_lr_input)
    if key not in _oracle_lengths:
        raw = np.linspace(-0.5, 0.5, n, dtype=np.float32)[None]
        _oracle_lengths[key] = R.inference_segments(raw, fs, 48000, lr_rate, SEG, 0, is_lr_input)[0].shape[1]
    return _oracle_lengths[key]


@pytest.mark.parametrize("is_lr_input", [False, True])
@pytest.mark.parametrize("lr_rate", [8000, 12000])
def test_plan_lengths_are_the_oracles(lr_rate, is_lr_input):
    from mdctgan_amd.generate_audio import plan_utterances
    from mdctgan_amd.resample import plan_front_end
    cases = [(n, fs) for fs in RATES for n in LENGTHS]
    lengths, rates = [n for n, _ in cases], [fs for _, fs in cases]
    for overlap, bs in ((0, 5), (1024, 64)):
        plan = plan_front_end(lengths, rates, 48000, lr_rate, is_lr_input, SEG, overlap, bs)
        assert plan.lengths[0] == lengths and len(plan.lengths) == len(plan.steps) + 1 == (2 if is_lr_input else 3)
        assert plan.final_lengths == [oracle_length(n, fs, lr_rate, is_lr_input) for n, fs in cases]
        for s, (lens, starts, total) in enumerate(zip(plan.lengths, plan.starts, plan.totals)):
            assert all(p % 64 == 0 for p in starts) and total % 64 == 0
            assert all(a + n <= b for a, n, b in zip(starts, lens, starts[1:] + [total]))        # no overlap, in order
        want = plan_utterances(plan.final_lengths, SEG, SEG, overlap, bs)
        got = plan.utterances
        assert (got.in_start, got.out_start, got.segments, got.out_length, got.in_total, got.out_total, got.n_live) == \
            (want.in_start, want.out_start, want.segments, want.out_length, want.in_total, want.out_total, want.n_live)
        assert np.array_equal(plan.in_rows, want.in_rows) and np.array_equal(plan.out_rows, want.out_rows)
        assert got.in_start == plan.starts[-1] and got.in_total == plan.totals[-1]
        # every utterance is in exactly one group of every step; a group's rows chain the buffers of its step
        for s, step in enumerate(plan.steps):
            assert sorted(u for g in step for u in g.index) == list(range(len(cases)))
            assert len({(g.orig_freq, g.new_freq) for g in step}) == len(step)
            for g in step:
                assert g.rows.dtype == np.int64 and g.rows.shape == (len(g.index), 4)
                for (a, n, b, m), u in zip(g.rows.tolist(), g.index):
                    assert (a, n, b, m) == (plan.starts[s][u], plan.lengths[s][u], plan.starts[s + 1][u], plan.lengths[s + 1][u])
                    assert m == -(-n * g.new_freq // g.orig_freq)
                assert g.max_out_len == g.rows[:, 3].max()
        assert plan.n_launches == len(RATES) + (0 if is_lr_input else 1)
        assert plan.order == [u for g in plan.steps[0] for u in g.index]


def test_plan_refuses_what_it_cannot_place():
    from mdctgan_amd.resample import plan_front_end
    for lengths, rates in (([], []), ([100], [48000, 16000]), ([0], [48000]), ([100], [0]), ([100], [-8000])):
        with pytest.raises(ValueError):
            plan_front_end(lengths, rates, 48000, 8000, False, SEG, 0, 8)
    with pytest.raises(ValueError):
        plan_front_end([100], [48000], 48000, 0, False, SEG, 0, 8)
    with pytest.raises(ValueError):
        plan_front_end([100], [48000], 48000, 8000, False, SEG, SEG, 8)          # gen_overlap: plan_utterances' rule


# ---------------------------------------------------------------------------------------------------------------------
# 2. the C ABI rejects bad arguments before any launch
# ---------------------------------------------------------------------------------------------------------------------
P = 4096                         # a non-null "pointer"
NAN = float("nan")
# good argument lists (never called as they stand), then (position, bad value) pairs
GOOD = {
    # x, x_total, rows, n_rows, max_out_len, shift, kern, orig, new_, width, out, out_total, stream
    "mg_resample_rows": [P, 1000, P, 3, 100, None, P, 6, 1, 37, P, 1000, None],
    # x, total, rows, n_rows, max_len, out, workspace, workspace_bytes, stream
    "mg_rows_moments": [P, 1000, P, 3, 5000, P, P, 1 << 20, None],
    # lr, noise, total, rows, n_rows, max_len, lr_moments, noise_moments, snr, segment_length, stream
    "mg_add_noise_rows": [P, P, 1000, P, 3, 500, P, P, 55.0, 7936, None],
}
BAD = {
    "mg_resample_rows": [(0, None), (2, None), (6, None), (10, None), (3, 0), (3, -1), (1, 0), (1, -5), (11, 0), (11, -5), (4, 0),
                         (7, 0), (7, -6), (8, 0), (8, -1), (9, -1)],
    "mg_rows_moments": [(0, None), (2, None), (5, None), (6, None), (3, 0), (3, -2), (1, 0), (1, -1), (4, 0), (4, -4096),
                        (7, 3 * 2 * 2 * 8 - 1)],
    "mg_add_noise_rows": [(0, None), (1, None), (3, None), (6, None), (7, None), (4, 0), (4, -1), (2, 0), (2, -1), (5, 0), (5, -3),
                          (9, 0), (9, -7936), (8, NAN)],
}
CASES = [(name, pos, bad) for name in GOOD for pos, bad in BAD[name]]

CHILD = """
import json, sys
sys.path.insert(0, %r)
from mdctgan_amd import _lib
lib = _lib.load()
name, good, bad = json.loads(sys.argv[1])
for pos, value in bad:
    args = list(good)
    args[pos] = float("nan") if value == "nan" else value
    print("rc %%d %%d" %% (pos, getattr(lib, name)(*args)), flush=True)
print("ws %%d %%d %%d" %% (lib.mg_rows_moments_workspace(0, 100), lib.mg_rows_moments_workspace(3, 0), lib.mg_rows_moments_workspace(3, 5000)))
""" % REPO


@pytest.fixture(scope="module")
def children():
    """One child per entry point (each pays the import of torch), all started at once -> name: (exit status, stdout, stderr)."""
    import json
    procs = {}
    for name in GOOD:
        bad = [(pos, "nan" if value != value else value) for pos, value in BAD[name]]
        procs[name] = subprocess.Popen([sys.executable, "-c", CHILD, json.dumps([name, GOOD[name], bad])], stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True, cwd=REPO)
    return {name: (p,) + p.communicate(timeout=300) for name, p in procs.items()}


@pytest.mark.parametrize("name,pos,bad", CASES, ids=lambda v: "nan" if v != v else str(v))
def test_entry_points_reject_bad_arguments(children, name, pos, bad):
    proc, out, errtxt = children[name]
    assert proc.returncode == 0, "child exit status %d\n%s" % (proc.returncode, errtxt[-2000:])
    lines = [ln.split() for ln in out.splitlines() if ln.startswith("rc ")]
    assert len(lines) == len(BAD[name])
    assert lines[[q for q, _ in BAD[name]].index(pos) if bad != bad else BAD[name].index((pos, bad))] == ["rc", str(pos), str(MG_ERR_ARG)]


def test_moments_workspace_query(children):
    _, out, _ = children["mg_rows_moments"]
    ws = [ln.split() for ln in out.splitlines() if ln.startswith("ws ")]
    assert ws == [["ws", "0", "0", str(3 * 2 * 2 * 8)]]                # 3 rows x ceil(5000 / 4096) chunks x {sum, sum sq} doubles


# ---------------------------------------------------------------------------------------------------------------------
# 3. the noise bar has teeth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snr", T.SNRS)
@pytest.mark.parametrize("n", T.NOISE_LENGTHS)
def test_float32_restatement_passes_the_noise_bar(n, snr):
    lr, noise = T.noise_inputs(n)
    f64, f32 = T.noise_ref64(lr, noise, snr, T.SEG), T.noise_ref32(lr, noise, snr, T.SEG)
    ok, margin = T.noise_passes(f32, f32, f64)
    assert ok and margin <= 0.25 + 1e-12
    # and float64 itself realises the requested SNR with the reference's divisor
    added = f64 - lr.numpy().astype(np.float64)
    assert abs(10 * np.log10((np.sum(lr.numpy().astype(np.float64) ** 2) / T.SEG) / added.var(ddof=1)) - snr) <= 1e-9
    assert abs(added.mean()) <= 1e-12 * added.std(ddof=1)


@pytest.mark.parametrize("snr", T.SNRS)
def test_bar_rejects_the_waveform_length_as_divisor(snr):
    n = 3000
    lr, noise = T.noise_inputs(n)
    f64, f32 = T.noise_ref64(lr, noise, snr, T.SEG), T.noise_ref32(lr, noise, snr, T.SEG)
    ok, margin = T.noise_passes(T.noise_ref32(lr, noise, snr, T.SEG, "length"), f32, f64)
    print("noise bar | / N instead of / segment_length | n=%d snr=%g | error / bar %.3e" % (n, snr, margin))
    assert not ok and margin > 100, margin


def test_bar_rejects_the_biased_standard_deviation():
    n, snr = 3000, 10.0
    lr, noise = T.noise_inputs(n)
    f64, f32 = T.noise_ref64(lr, noise, snr, T.SEG), T.noise_ref32(lr, noise, snr, T.SEG)
    ok, margin = T.noise_passes(T.noise_ref32(lr, noise, snr, T.SEG, "biased"), f32, f64)
    print("noise bar | biased std | n=%d snr=%g | error / bar %.3e" % (n, snr, margin))
    assert not ok and margin > 10, margin
