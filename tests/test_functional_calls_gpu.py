"""The Python side's conversation with the launchers is what tests/golden/functional_calls.json recorded (written by
scripts/gen_functional_calls_golden.py at commit 162687f, before functional.py's convolution nodes were folded): every call into
mdctgan_amd.ops with every argument's value, the order of the grad-ready notifications, and the gradient flags each step leaves on
every parameter -- for three eager float32 steps (separate kernels, then fused Adam and the persistent U) and two inference passes
("float32"), three --fp16 steps of the local generator ("fp16"), two --fp16 steps of a wider global trunk whose gradients are
stored as float16 and checked by their own kernels ("fp16_checked"), the three public convolution wrappers called bare ("bare"),
and a trunk layer through plain conv2d under fused_adam_scope, the fused-Adam tail that announces the bias only ("fused_tail").
See tests/functional_calls.py for the record format."""
import json

import pytest

import functional_calls as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(R.GOLDEN) as f:
        return R.unpack(json.load(f))


@pytest.mark.parametrize("scenario", sorted(R.SCENARIOS))
def test_calls_are_the_recorded_ones(recorded, scenario):
    want, got = recorded[scenario], R.normal(R.SCENARIOS[scenario]())
    for i, (a, b) in enumerate(zip(want, got)):
        assert a == b, "record %d of %d differs:\n  recorded %s\n  now      %s" % (i, len(want), json.dumps(a), json.dumps(b))
    assert len(got) == len(want), "the trace has %d records, the recorded one %d; the first one without a partner: %s" % (
        len(got), len(want), json.dumps(max(got, want, key=len)[min(len(got), len(want))]))
