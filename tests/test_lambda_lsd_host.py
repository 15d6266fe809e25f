"""--lambda_lsd without a GPU (options.py, pix2pixHD_model.py, metrics.lsd_loss_term; csrc/metrics_rows.hip, csrc/lsd_rows_grad.hip).

1. The flag parses; its default is 0.
2. loss_filter keeps its four-argument form and places the new term third.
3. What the term cannot serve is refused when the model is built (Pix2PixHDModel._check_lambda_lsd on a stand-in for the model:
   building a real one needs a device).
4. The two new entry points are declared, bound and exported, the ABI version stays 4, and both return MG_ERR_ARG before any
   launch for null pointers and non-positive counts (a child process with arbitrary non-null integers as pointers, never
   dereferenced because the call returns first -- the scheme of tests/test_lsd_loss_host.py).
5. to_audio's output length, which the step compares hr_audio with before it launches anything.
"""
import inspect
import json
import os
import re
import subprocess
import sys
import types

import pytest

import test_lsd_loss_host as H

REPO = H.REPO
NEW = ("mg_lsd_mean_loss", "mg_lsd_rows_backward_seeded")


def test_the_flag_parses_and_defaults_to_zero():
    from mdctgan_amd.options import make_opt
    assert make_opt("--lambda_lsd", "0.25").lambda_lsd == 0.25
    assert make_opt().lambda_lsd == 0.0


def test_loss_filter_keeps_its_four_argument_form():
    from mdctgan_amd.pix2pixHD_model import Pix2PixHDModel
    params = list(inspect.signature(Pix2PixHDModel.loss_filter).parameters.values())
    assert [p.name for p in params[:5]] == ["self", "g_gan", "g_gan_feat", "d_real", "d_fake"]
    assert all(p.default is inspect.Parameter.empty for p in params[1:5]) and all(p.default is None for p in params[5:])
    with_feat, without = types.SimpleNamespace(no_ganFeat_loss=False), types.SimpleNamespace(no_ganFeat_loss=True)
    assert Pix2PixHDModel.loss_filter(with_feat, 1, 2, 3, 4) == [1, 2, 3, 4]
    assert Pix2PixHDModel.loss_filter(without, 1, 2, 3, 4) == [1, 3, 4]
    assert Pix2PixHDModel.loss_filter(with_feat, 1, 2, 3, 4, 5) == [1, 2, 5, 3, 4]
    assert Pix2PixHDModel.loss_filter(without, 1, 2, 3, 4, g_lsd=5) == [1, 5, 3, 4]


def _check(in_kernel=True, **over):
    from mdctgan_amd.pix2pixHD_model import Pix2PixHDModel
    opt = types.SimpleNamespace(**dict(dict(lambda_lsd=1.0, n_fft=512, win_length=512, hop_length=256), **over))
    return Pix2PixHDModel._check_lambda_lsd(types.SimpleNamespace(preprocess=types.SimpleNamespace(_in_kernel=in_kernel)), opt)


def test_refusals_when_the_model_is_built():
    assert _check() == 1.0 and _check(lambda_lsd=0.25, n_fft=256, win_length=256) == 0.25 and _check(n_fft=1024, win_length=1024) == 1.0
    # 0 switches the term off whatever else is set: the default path checks nothing new
    assert _check(in_kernel=False, lambda_lsd=0.0, n_fft=2048, win_length=100) == 0.0
    for bad in (-1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="lambda_lsd"):
            _check(lambda_lsd=bad)
    with pytest.raises(NotImplementedError, match="lambda_lsd"):
        _check(in_kernel=False)                                         # the dB and explicit-encoding codecs
    with pytest.raises(NotImplementedError, match="lambda_lsd"):
        _check(n_fft=2048, win_length=2048)                             # 2 * n_fft = 4096
    with pytest.raises(NotImplementedError, match="lambda_lsd"):
        _check(n_fft=128, win_length=128)
    with pytest.raises(NotImplementedError, match="lambda_lsd.*win_length"):
        _check(win_length=256)


def test_new_entry_points_are_declared_bound_and_exported():
    from mdctgan_amd import _lib
    text = open(os.path.join(REPO, "include", "mdctgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the seeded entry point is mg_lsd_rows_backward's list with (go, scale) in the place of grad_rows
    plain, seeded = (_lib.SIGNATURES[n][1] for n in ("mg_lsd_rows_backward", "mg_lsd_rows_backward_seeded"))
    assert len(seeded) == len(plain) + 1 and seeded[:14] == plain[:14] and seeded[15:] == plain[14:]
    assert _lib.ABI_VERSION == 4 and lib.mg_abi_version() == 4


P = 4096                         # a non-null, 16-byte aligned "pointer"
FRAMES, NFFT = 40, 1024
WS = FRAMES * NFFT * 4
# per_frame, total_frames, scale, loss, stream
MEAN_GOOD = [P, FRAMES, 0.5, P, None]
MEAN_BAD = [(0, None), (3, None), (1, 0), (1, -7)]
# hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, hr_shift, window, n_fft, hop, center, go, scale, grad_sr,
# workspace, workspace_bytes, stream
SEED_GOOD = [P, 30000, P, 30000, P, 3, P, FRAMES, None, P, NFFT, 512, 1, P, 0.5, P, P, WS, None]
SEED_BAD = [(0, None), (2, None), (4, None), (6, None), (9, None), (13, None), (15, None), (16, None),       # null pointers (13: go)
            (10, 256), (10, 4096), (10, 1000), (10, 0),                                                     # other transform sizes
            (1, 0), (1, -5), (3, 0), (3, -5), (5, 0), (5, -1), (7, 0), (7, -3), (11, 0), (11, -512),        # counts, totals, hop
            (17, WS - 1), (17, 0), (16, P + 4)]                                                             # short / misaligned workspace

CHILD = """
import json, sys
sys.path.insert(0, %r)
from mdctgan_amd import _lib
lib = _lib.load()
for name, good, bad in json.loads(sys.argv[1]):
    for pos, value in bad:
        args = list(good)
        args[pos] = value
        print("rc %%s %%d %%d" %% (name, pos, getattr(lib, name)(*args)), flush=True)
""" % REPO


@pytest.fixture(scope="module")
def child():
    jobs = [["mg_lsd_mean_loss", MEAN_GOOD, MEAN_BAD], ["mg_lsd_rows_backward_seeded", SEED_GOOD, SEED_BAD]]
    p = subprocess.run([sys.executable, "-c", CHILD, json.dumps(jobs)], capture_output=True, text=True, cwd=REPO, timeout=300)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("name,bad", [("mg_lsd_mean_loss", MEAN_BAD), ("mg_lsd_rows_backward_seeded", SEED_BAD)])
def test_bad_arguments_are_rejected_before_any_launch(child, name, bad):
    rc, out, errtxt = child
    assert rc == 0, "child exit status %d\n%s" % (rc, errtxt[-2000:])
    lines = [ln.split()[2:] for ln in out.splitlines() if ln.startswith("rc %s " % name)]
    assert lines == [[str(pos), str(H.MG_ERR_ARG)] for pos, _ in bad]


def test_to_audio_length_is_known_before_any_launch():
    """(F - 1) hop samples for the F frames of a T-sample clip: what imdct4_codec, imdct4_pow2 and imdct4_generic return with
    win_length == n_fft on the always-centred codec transform."""
    from mdctgan_amd.pix2pixHD_model import Audio2MDCT
    for n_fft, hop, T, want in ((512, 256, 7936, 7936), (512, 256, 32512, 32512), (512, 256, 8000, 8192), (1024, 512, 7936, 8192),
                                (512, 128, 5000, 4864)):
        pre = types.SimpleNamespace(win_length=n_fft, hop_length=hop)
        assert Audio2MDCT.audio_length(pre, T) == want, (n_fft, hop, T)
