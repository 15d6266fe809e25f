"""Low-pass rows without a GPU: the host side of mdctgan_amd/lowpass.py, and the reference every GPU comparison of
tests/test_lowpass_gpu.py uses.

1. Filter design against tests/golden/lowpass_scipy.npz (scripts/gen_lowpass_golden.py; SciPy is not needed here).  The yardstick
   is what the fixture says about SciPy itself: how far its `sos` and `zpk` evaluations of one filter sit apart.  The bar is 10 x
   that, per case.
   Measured, max |H_ours - H_scipy| / max |H| over the 17 cases, against the sos and the zpk route: 2.3e-16 to 2.2e-13 (the
   largest: cheby1 order 12 at 1 kHz / 48 kHz, 2.19e-13 and 2.16e-13 where SciPy's two routes differ by 1.07e-13); the ratio to
   the yardstick lies between 0.90 and 2.21 (test_design_matches_scipy prints every figure).
2. `sos_cascade` / `sos_zero_phase`: a plain sequential restatement of the cascade, a numpy loop, pinned to the fixture's float64
   outputs at 1e-13 of the row's peak.
3. The GPU bar (|y - ref| <= 2^-23 max |ref| per row) has teeth: the same restatement in float32 misses it on the order-11 / 12
   Chebyshev cases, by the factors printed (measured: 68 x at 4 kHz / 48 kHz to 1244 x at 1 kHz / 48 kHz).
4. Draws, refusals, options.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mdctgan_amd import lowpass
from mdctgan_amd.lowpass import LowpassSpec, check_sos, draw_lowpass, identity_sos, lowpass_sos, pad_sos

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_BAR = 2.0 ** -23            # of the row's peak: twice the rounding bound of the float32 output
MG_ERR_ARG = -1


# ------------------------------------------------------------------------------------------------------------------
# the fixture and the reference
# ------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, g, k):
        self.k = k
        self.kind, self.order = str(g["kind"][k]), int(g["order"][k])
        self.cutoff, self.fs, self.ripple = float(g["cutoff"][k]), float(g["fs"][k]), float(g["ripple"][k])
        self.sos, self.h_sos, self.h_zpk = g["sos_%d" % k], g["h_sos_%d" % k], g["h_zpk_%d" % k]
        self.x, self.y1, self.y2 = g["x_%d" % k], g["y1_%d" % k], g["y2_%d" % k]
        self.id = "%s_n%d_%gk_%gk" % (self.kind, self.order, self.cutoff / 1e3, self.fs / 1e3)

    @property
    def sharp_cheby(self):
        return self.kind == "cheby1" and self.order >= 11


def load_cases():
    g = np.load(os.path.join(REPO, "tests", "golden", "lowpass_scipy.npz"), allow_pickle=False)
    return g["w"], [Case(g, k) for k in range(len(g["kind"]))]


W, CASES = load_cases()


def sos_cascade(sos, x, dtype=np.float64):
    """The cascade over x from a zero state, one sample after the other, in `dtype`: per section (transposed direct form II)
    y = b0 x + s1; s1 = b1 x - a1 y + s2; s2 = b2 x - a2 y."""
    sos = np.asarray(sos, dtype=dtype)
    y = np.asarray(x, dtype=dtype).copy()
    for b0, b1, b2, _, a1, a2 in sos:
        s1 = s2 = dtype(0)
        for n in range(y.shape[0]):
            xn = y[n]
            yn = b0 * xn + s1
            s1 = b1 * xn - a1 * yn + s2
            s2 = b2 * xn - a2 * yn
            y[n] = yn
    return y


def sos_zero_phase(sos, x, dtype=np.float64, forward=None):
    """sos_cascade forward, then again from a zero state over the reversed result: sosfilt(sos, sosfilt(sos, x)[::-1])[::-1].
    forward: sos_cascade(sos, x) where the caller has it (the cascade is causal: a prefix of it is the prefix's result)."""
    f = sos_cascade(sos, x, dtype) if forward is None else forward
    return sos_cascade(sos, f[::-1], dtype)[::-1]


_forward = {}


def reference(case, n, zero_phase):
    """The float64 reference of the first n samples of the case's input (computed once, shared, never modified)."""
    if case.k not in _forward:
        _forward[case.k] = sos_cascade(case.sos, case.x)
        _forward[case.k].setflags(write=False)
    key = (case.k, n, bool(zero_phase))
    if key not in _forward:
        f = _forward[case.k][:n]
        _forward[key] = sos_zero_phase(case.sos, None, forward=f) if zero_phase else f
        _forward[key].setflags(write=False)
    return _forward[key]


# ------------------------------------------------------------------------------------------------------------------
# 1. design
# ------------------------------------------------------------------------------------------------------------------
def freq_response(sos, w):
    z = np.exp(-1j * w)
    h = np.ones_like(z)
    for b0, b1, b2, a0, a1, a2 in np.asarray(sos, dtype=np.float64):
        h = h * (b0 + b1 * z + b2 * z * z) / (a0 + a1 * z + a2 * z * z)
    return h


def design_of(case):
    return lowpass_sos(case.kind, case.order, case.cutoff, case.fs, case.ripple if case.kind == "cheby1" else None)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_design_matches_scipy(case):
    sos = design_of(case)
    assert sos.dtype == np.float64 and sos.shape == ((case.order + 1) // 2, 6)
    assert (sos[:, 3] == 1.0).all()
    if case.order % 2:
        assert sos[0, 2] == 0.0 and sos[0, 5] == 0.0                       # one first-order section
    check_sos(pad_sos(sos))
    h = freq_response(sos, W)
    peak = np.abs(case.h_sos).max()
    yard = np.abs(case.h_sos - case.h_zpk).max() / peak
    e_sos, e_zpk = np.abs(h - case.h_sos).max() / peak, np.abs(h - case.h_zpk).max() / peak
    print("lowpass design %s | sos-zpk yardstick %.3e | ours-sos %.3e | ours-zpk %.3e | worst / yardstick %.2f"
          % (case.id, yard, e_sos, e_zpk, max(e_sos, e_zpk) / yard))
    assert max(e_sos, e_zpk) <= 10 * yard
    # the gain convention: |H(0)| = 1, or 10^(-rp / 20) for an even-order Chebyshev
    dc = 10 ** (-case.ripple / 20) if case.kind == "cheby1" and case.order % 2 == 0 else 1.0
    assert abs(abs(h[0]) - dc) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------
# 2. the reference is SciPy's
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_restatement_is_pinned_to_the_fixture(case):
    y1, y2 = reference(case, len(case.x), False), reference(case, len(case.x), True)
    for name, ours, ref in (("one pass", y1, case.y1), ("zero phase", y2, case.y2)):
        e = np.abs(ours - ref).max() / np.abs(ref).max()
        print("lowpass restatement %s | %s | %.3e of the peak" % (case.id, name, e))
        assert e <= 1e-13


def test_a_prefix_of_the_forward_pass_is_the_prefix_of_the_result():
    case = CASES[-1]
    np.testing.assert_array_equal(reference(case, 257, False), sos_cascade(case.sos, case.x[:257]))
    np.testing.assert_array_equal(reference(case, 257, True), sos_zero_phase(case.sos, case.x[:257]))


# ------------------------------------------------------------------------------------------------------------------
# 3. the bar has teeth
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c.sharp_cheby], ids=lambda c: c.id)
def test_float32_recursion_misses_the_gpu_bar(case):
    n = len(case.x)
    for zero_phase in (False, True):
        ref = reference(case, n, zero_phase)
        y32 = sos_zero_phase(case.sos, case.x, np.float32) if zero_phase else sos_cascade(case.sos, case.x, np.float32)
        e = np.abs(y32.astype(np.float64) - ref).max() / np.abs(ref).max()
        print("lowpass float32 recursion %s | zero_phase %d | %.3e of the peak = %.1f x the bar" % (case.id, zero_phase, e, e / GPU_BAR))
        assert e > GPU_BAR
        # ... and the float64 reference, rounded once, passes it
        assert np.abs(ref.astype(np.float32).astype(np.float64) - ref).max() <= GPU_BAR * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------------------------
# 4. draws, refusals, options
# ------------------------------------------------------------------------------------------------------------------
def test_draw_lowpass_repeats_under_a_seed_and_follows_the_spec():
    spec = LowpassSpec(("butter", "cheby1"), (1, 12), (0.01, 1.0), (0.5, 1.0))
    rates = [48000, 16000, 44100, 48000, 22050, 48000, 48000, 16000]
    a = draw_lowpass(rates, 8000, spec, torch.Generator().manual_seed(7))
    b = draw_lowpass(rates, 8000, spec, torch.Generator().manual_seed(7))
    c = draw_lowpass(rates, 8000, spec, torch.Generator().manual_seed(8))
    assert a.dtype == np.float64 and a.shape == (8, lowpass.MG_SOS_MAX_SECTIONS, 6)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, c)
    check_sos(a)
    ident = identity_sos()
    for row in a:
        used = [k for k in range(6) if not np.array_equal(row[k], ident[k])]
        assert used == list(range(len(used))) and 1 <= len(used) <= 6       # the unused sections are the identity, at the end
    # the global CPU stream when no generator is given
    torch.manual_seed(3)
    d = draw_lowpass(rates, 8000, spec)
    torch.manual_seed(3)
    np.testing.assert_array_equal(d, draw_lowpass(rates, 8000, spec))
    # a row's filter depends on the rows before it only through the stream: the same prefix of rows draws the same filters
    np.testing.assert_array_equal(draw_lowpass(rates[:3], 8000, spec, torch.Generator().manual_seed(7)), a[:3])


def test_a_row_whose_cutoff_reaches_its_nyquist_gets_identity_sections():
    spec = LowpassSpec(("cheby1",), (4, 4), (0.1, 0.1), (1.0, 1.0))            # the edge is lr_rate / 2 = 4 kHz exactly
    t = draw_lowpass([8000, 7000, 48000], 8000, spec, torch.Generator().manual_seed(0))
    np.testing.assert_array_equal(t[0], identity_sos())                        # 4 kHz is the Nyquist frequency of 8 kHz
    np.testing.assert_array_equal(t[1], identity_sos())
    np.testing.assert_array_equal(t[2], pad_sos(lowpass_sos("cheby1", 4, 4000.0, 48000, 0.1)))


def test_window_draws_do_not_move_when_the_feature_is_on():
    """The filters are drawn after the windows: draw_windows yields the offsets it yields without the feature.  The order is
    training_batch_many's own: its host half, _windows followed by _lowpass_table on one generator, gives these offsets and the
    filters draw_lowpass gives behind them.  (The whole call is compared in tests/test_lowpass_gpu.py: a == b == c.)"""
    from mdctgan_amd.train_data import TrainingCorpus, draw_windows
    corpus = TrainingCorpus(torch.zeros(1), [0, 4096, 8192, 16384], [3000, 3100, 5000, 9000], [48000, 16000, 48000, 16000])
    idx = [0, 1, 2, 3, 2, 0]
    off_a, len_a = draw_windows(corpus, idx, 1024, 48000, torch.Generator().manual_seed(11))
    g = torch.Generator().manual_seed(11)
    off_b, len_b = draw_windows(corpus, idx, 1024, 48000, g)
    draw_lowpass([corpus.rates[i] for i in idx], 8000, LowpassSpec(), g)
    assert torch.equal(off_a, off_b) and torch.equal(len_a, len_b)
    from mdctgan_amd import train_data
    from mdctgan_amd.resample import data_options
    o = data_options(dict(lr_sampling_rate=8000, hr_sampling_rate=48000, segment_length=1024, lowpass_aug="butter,cheby1"))
    g = torch.Generator().manual_seed(11)
    off_c, len_c = train_data._windows(corpus, idx, o, None, None, g)
    coef_c = train_data._lowpass_table(o["lowpass"], corpus, idx, 8000, g)
    assert torch.equal(off_a, off_c) and torch.equal(len_a, len_c)
    g = torch.Generator().manual_seed(11)
    draw_windows(corpus, idx, 1024, 48000, g)
    np.testing.assert_array_equal(coef_c, draw_lowpass([corpus.rates[i] for i in idx], 8000, LowpassSpec(), g))
    # ... and in training_batch_many's order the next batch's windows move only by the filter draws, never the other way round
    assert off_a.tolist() != [0] * 6


def test_unstable_and_non_finite_sections_are_refused():
    good = pad_sos(lowpass_sos("butter", 4, 4000.0, 48000))
    check_sos(good)
    for k, v in ((5, 1.0), (5, -1.0), (5, 1.5), (4, 2.5), (4, -2.5), (0, float("nan")), (1, float("inf")), (3, 2.0)):
        bad = good.copy()
        bad[1, k] = v
        with pytest.raises(ValueError):
            check_sos(bad)
    edge = good.copy()
    edge[0, 4], edge[0, 5] = 1.5, 0.5                                       # |a1| == 1 + a2: a pole on the unit circle
    with pytest.raises(ValueError):
        check_sos(edge)
    with pytest.raises(ValueError):
        check_sos(np.zeros((2, 5, 6)))
    with pytest.raises(ValueError):
        pad_sos(np.zeros((7, 6)))
    # the wrapper refuses on the host, before it looks at the device at all
    bad = good.copy()
    bad[2, 5] = 1.0
    with pytest.raises(ValueError, match="unstable"):
        lowpass.sos_rows(torch.zeros(64), np.asarray([[0, 64, 0]]), bad)
    with pytest.raises(ValueError, match="unstable"):
        lowpass.lowpass_waveform(torch.zeros(1, 64), bad)


@pytest.mark.parametrize("args", [
    ("bessel", 4, 4000.0, 48000, None), ("ellip", 4, 4000.0, 48000, 1.0), ("butter", 0, 4000.0, 48000, None),
    ("butter", 13, 4000.0, 48000, None), ("butter", 2.5, 4000.0, 48000, None), ("butter", 4, 0.0, 48000, None),
    ("butter", 4, -1.0, 48000, None), ("butter", 4, 24000.0, 48000, None), ("butter", 4, 30000.0, 48000, None),
    ("butter", 4, float("nan"), 48000, None), ("butter", 4, 4000.0, 0, None), ("cheby1", 4, 4000.0, 48000, None),
    ("cheby1", 4, 4000.0, 48000, 0.0), ("cheby1", 4, 4000.0, 48000, -1.0), ("butter", 4, 4000.0, 48000, 1.0),
], ids=str)
def test_bad_kind_order_cutoff_or_ripple_raise(args):
    with pytest.raises(ValueError):
        lowpass_sos(*args)


def test_bad_specs_raise():
    for kw in (dict(kinds=()), dict(kinds=("bessel",)), dict(order=(0, 4)), dict(order=(5, 4)), dict(order=(2, 13)),
               dict(ripple=(0.0, 1.0)), dict(ripple=(2.0, 1.0)), dict(cutoff=(0.0, 1.0)), dict(cutoff=(1.0, 0.5))):
        with pytest.raises(ValueError):
            LowpassSpec(**kw)


def test_flags_parse_and_the_defaults_leave_the_feature_off():
    from mdctgan_amd.options import make_opt
    from mdctgan_amd.resample import data_options
    opt = make_opt()
    assert opt.lowpass_aug == "" and tuple(opt.lowpass_order) == (2, 10)
    assert tuple(opt.lowpass_ripple) == (0.01, 1.0) and tuple(opt.lowpass_cutoff) == (0.9, 1.0)
    assert data_options(opt)["lowpass"] is None
    assert data_options(dict(lr_sampling_rate=8000, hr_sampling_rate=48000, segment_length=1024))["lowpass"] is None
    opt = make_opt("--lowpass_aug", "butter,cheby1", "--lowpass_order", "3", "7", "--lowpass_ripple", "0.1", "0.5",
                   "--lowpass_cutoff", "0.8", "0.95")
    spec = data_options(opt)["lowpass"]
    assert spec == LowpassSpec(("butter", "cheby1"), (3, 7), (0.1, 0.5), (0.8, 0.95))
    assert data_options(make_opt("--lowpass_aug", "cheby1"))["lowpass"] == LowpassSpec(("cheby1",))
    with pytest.raises(ValueError):
        data_options(make_opt("--lowpass_aug", "elliptic"))


# ------------------------------------------------------------------------------------------------------------------
# 5. the entry points refuse bad arguments before any launch (child processes with fake pointers, as in
#    tests/test_bot_attn_wide_host.py)
# ------------------------------------------------------------------------------------------------------------------
CHILD = """
import ctypes, sys
sys.path.insert(0, %r)
from mdctgan_amd import _lib
lib = _lib.load()
p, big = 4096, 1 << 40
bank = _lib.ResampleBank(None, 1, 1, 0)
need = lib.mg_sos_rows_workspace(4, 1200)
assert need > 0 and lib.mg_sos_rows_workspace(0, 1200) == 0 and lib.mg_sos_rows_workspace(4, 0) == 0
assert lib.mg_sos_rows_workspace(4, (1 << 30) + 1) == 0
calls = {
    "sos_null_x": lambda: lib.mg_sos_rows(None, 100, p, p, 4, 1200, 1, 1 << 20, 100, 1 << 24, need, None),
    "sos_null_rows": lambda: lib.mg_sos_rows(p, 100, None, p, 4, 1200, 1, 1 << 20, 100, 1 << 24, need, None),
    "sos_null_sos": lambda: lib.mg_sos_rows(p, 100, p, None, 4, 1200, 1, 1 << 20, 100, 1 << 24, need, None),
    "sos_null_out": lambda: lib.mg_sos_rows(p, 100, p, p, 4, 1200, 1, None, 100, 1 << 24, need, None),
    "sos_null_workspace": lambda: lib.mg_sos_rows(p, 100, p, p, 4, 1200, 1, 1 << 20, 100, None, need, None),
    "sos_no_rows": lambda: lib.mg_sos_rows(p, 100, p, p, 0, 1200, 1, 1 << 20, 100, 1 << 24, need, None),
    "sos_short_workspace": lambda: lib.mg_sos_rows(p, 100, p, p, 4, 1200, 1, 1 << 20, 100, 1 << 24, need - 1, None),
    "sos_out_is_x": lambda: lib.mg_sos_rows(p, 100, p, p, 4, 1200, 1, p, 100, 1 << 24, need, None),
    "sos_out_overlaps_x": lambda: lib.mg_sos_rows(p, 100, p, p, 4, 1200, 1, p + 4 * 99, 100, 1 << 24, need, None),
    "sos_no_length": lambda: lib.mg_sos_rows(p, 100, p, p, 4, 0, 1, 1 << 20, 100, 1 << 24, need, None),
    "lr_null_buffer": lambda: lib.mg_train_lr_rows(None, 100, p, 4, 64, bank, bank, p, 4, None, 0, 0, None),
    "lr_null_rows": lambda: lib.mg_train_lr_rows(p, 100, None, 4, 64, bank, bank, p, 4, None, 0, 0, None),
    "lr_null_lr": lambda: lib.mg_train_lr_rows(p, 100, p, 4, 64, bank, bank, None, 4, None, 0, 0, None),
    "lr_no_rows": lambda: lib.mg_train_lr_rows(p, 100, p, 0, 64, bank, bank, p, 4, None, 0, 0, None),
    "lr_null_bank": lambda: lib.mg_train_lr_rows(p, 100, p, 4, 64, None, bank, p, 4, None, 0, 0, None),
    "lr_full_without_length": lambda: lib.mg_train_lr_rows(p, 100, p, 4, 64, bank, bank, None, 4, p, 100, 0, None),
    "hr_null_hr": lambda: lib.mg_train_hr_rows(p, 100, p, 4, 64, bank, None, 4, None),
    "hr_no_segment": lambda: lib.mg_train_hr_rows(p, 100, p, 4, 0, bank, p, 4, None),
}
for name in sys.argv[1:]:
    print("%%s rc=%%d" %% (name, calls[name]()))
""" % REPO

REFUSED = ["sos_null_x", "sos_null_rows", "sos_null_sos", "sos_null_out", "sos_null_workspace", "sos_no_rows",
           "sos_short_workspace", "sos_out_is_x", "sos_out_overlaps_x", "sos_no_length", "lr_null_buffer", "lr_null_rows",
           "lr_null_lr", "lr_no_rows", "lr_null_bank", "lr_full_without_length", "hr_null_hr", "hr_no_segment"]


@pytest.fixture(scope="module")
def child():
    """One child process for every refusal (it pays the import of torch once): no call gets as far as a launch."""
    proc = subprocess.run([sys.executable, "-c", CHILD] + REFUSED, capture_output=True, text=True, cwd=REPO, timeout=300)
    assert proc.returncode == 0, "child exit status %d\n%s" % (proc.returncode, proc.stderr[-2000:])
    return dict(line.split(" rc=") for line in proc.stdout.strip().splitlines())


@pytest.mark.parametrize("name", REFUSED)
def test_entry_points_refuse_bad_arguments(child, name):
    assert int(child[name]) == MG_ERR_ARG
