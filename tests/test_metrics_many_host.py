"""Packed metrics, host side (no device): plan_metrics against torch.stft's frame counts, the argument errors of plan_metrics and
compute_matrics_many, the keep_raw field of the front end's plan, and the new entry points in the header and the binding table."""
import dataclasses
import inspect
import os
import re
import types

import pytest
import torch

from mdctgan_amd import _lib
from mdctgan_amd.metrics import compute_matrics_many, plan_metrics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def metric_lengths(n_fft, hop, center):
    """n_fft / 2 + 1 is the deepest legal reflection (center only); then one whole frame, one sample more, a ragged tail, many frames."""
    return ([n_fft // 2 + 1] if center else []) + [n_fft, n_fft + 1, 7 * hop + 5, 9000]


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
@pytest.mark.parametrize("hop_div", [2, 4])
def test_plan_metrics_counts_torch_stft_frames(n_fft, hop_div, center):
    hop = n_fft // hop_div
    lengths = metric_lengths(n_fft, hop, center)
    plan = plan_metrics(lengths, n_fft, hop, center)
    window = torch.ones(n_fft)
    for u, T in enumerate(lengths):
        ts = torch.stft(torch.zeros(T), n_fft, hop_length=hop, win_length=n_fft, window=window, center=center, pad_mode="reflect",
                        return_complex=True)
        assert plan.frames[u] == ts.shape[-1], (T, plan.frames[u], ts.shape)
    assert plan.frame_start[0] == 0 and len(plan.frame_start) == len(lengths) + 1
    assert [b - a for a, b in zip(plan.frame_start, plan.frame_start[1:])] == plan.frames
    assert plan.total_frames == sum(plan.frames)


def test_plan_metrics_refuses_what_the_framing_kernel_refuses():
    with pytest.raises(ValueError, match="utterance 1"):
        plan_metrics([4000, 1023, 4000], 1024, 512, False)              # not one whole frame
    with pytest.raises(ValueError, match="utterance 2"):
        plan_metrics([4000, 4000, 512], 1024, 512, True)                # the reflection would need sample 512
    plan_metrics([513], 1024, 512, True)
    with pytest.raises(ValueError, match="utterance 0"):
        plan_metrics([0], 512, 256, True)
    with pytest.raises(ValueError):
        plan_metrics([], 512, 256, True)
    with pytest.raises(ValueError):
        plan_metrics([4000], 512, 0, True)


def test_compute_matrics_many_argument_errors():
    opt = types.SimpleNamespace(n_fft=512, hop_length=256, win_length=512, center=True)
    w = lambda n: torch.zeros(n)
    with pytest.raises(ValueError, match="no waveforms"):
        compute_matrics_many([], [], [], opt)
    with pytest.raises(ValueError, match="utterance 1: lr"):
        compute_matrics_many([w(4000), w(3000)], [w(4000), w(2999)], [w(4000), w(3000)], opt)
    with pytest.raises(ValueError, match="utterance 0: sr"):
        compute_matrics_many([w(4000), w(3000)], [w(4001), w(3000)], [w(3999), w(3000)], opt)
    with pytest.raises(ValueError, match="2 hr waveforms but 1 sr"):
        compute_matrics_many([w(4000), w(3000)], [w(4000), w(3000)], [w(4000)], opt)
    with pytest.raises(ValueError, match="utterance 1"):
        compute_matrics_many([w(4000), w(512)], [w(4000), w(512)], [w(4000), w(512)], opt)         # too short for n_fft 1024
    with pytest.raises(NotImplementedError, match="win_length"):
        compute_matrics_many([w(4000)], [w(4000)], [w(4000)],
                             types.SimpleNamespace(n_fft=512, hop_length=256, win_length=256, center=True))
    with pytest.raises(NotImplementedError, match="n_fft"):
        compute_matrics_many([w(4000)], [w(4000)], [w(4000)],
                             types.SimpleNamespace(n_fft=64, hop_length=32, win_length=64, center=True))


def test_front_end_plan_differs_only_by_the_raw_field():
    """keep_raw is opt-in: the host plan (which front_end_many launches from) has one new field, None unless asked for."""
    from mdctgan_amd.resample import FrontEndPlan, front_end_many, plan_front_end
    plan = plan_front_end([5000, 20000, 7001], [48000, 44100, 48000], 48000, 12000, False, 7936, 0, 4)
    assert plan.raw is None
    assert [f.name for f in dataclasses.fields(FrontEndPlan)] == ["rates", "lengths", "starts", "totals", "steps", "order",
                                                                  "utterances", "raw"]
    sig = inspect.signature(front_end_many)
    assert sig.parameters["keep_raw"].default is False
    assert list(sig.parameters)[:6] == ["raws", "rates", "opt_or_kwargs", "noise", "generator", "device"]
    assert plan.order == [0, 2, 1]                 # (mixed rates: the shift's row order is not the utterance order)


def test_new_entry_points_are_declared_and_bound():
    text = open(os.path.join(REPO, "include", "mdctgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("mg_metrics_rows_packed_workspace", "mg_metrics_rows_packed", "mg_lsd_rows"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert re.search(r"typedef struct \{ long long hr_pos, lr_pos, sr_pos, len; \} mg_metric_row;", code)
    assert _lib.ABI_VERSION == 4
