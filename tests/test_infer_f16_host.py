"""The opt-in half-precision inference mode (MG_PRECISION_F16_INFER, csrc/wino_h16.h) without a GPU:

1. the switches: the constant, amp.infer_f16, --infer_fp16;
2. the route: which geometries run on float16 Winograd images, shown by the plan name and the size queries, and that every other
   geometry of the precision carries exactly the plans and sizes it has under MG_PRECISION_F16;
3. the gradient workspace queries and entry points refuse an eligible geometry (fake pointers, in a child process: a call that
   went on would fault the child, not the test run).
"""
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, W43, HINF = 0, 1, 2, 3
MG_ERR_UNSUPPORTED = -2


def test_switches():
    from mdctgan_amd import _lib, amp, options
    assert _lib.PRECISION_F16_INFER == HINF
    assert _lib.is_half(F16) and _lib.is_half(HINF) and not _lib.is_half(F32) and not _lib.is_half(W43)
    assert options.make_opt("--infer_fp16").infer_fp16 is True and options.make_opt().infer_fp16 is False
    assert options.make_opt("--infer_fp16").fp16 is False            # --fp16 keeps meaning "train with AMP" and nothing else
    assert "infer_fp16" not in options.SPECTRAL_FLAGS and "--infer_fp16" not in options.SPECTRAL_FLAGS
    assert torch.is_grad_enabled() and amp.current_precision() == F32
    with torch.no_grad():
        assert amp.current_precision() == F32                        # off by default
    with amp.infer_f16():
        assert amp.current_precision() == F32                        # grad mode: nothing changes
        with amp.autocast(True):
            assert amp.current_precision() == F16
        with torch.no_grad():
            assert amp.current_precision() == HINF
            with amp.wino43():
                assert amp.current_precision() == HINF               # that mode covers float32 only
            with amp.autocast(True):
                assert amp.current_precision() == HINF
            with amp.infer_f16(False):
                assert amp.current_precision() == F32
            with torch.enable_grad():
                assert amp.current_precision() == F32
    with amp.wino43(), torch.no_grad():
        assert amp.current_precision() == W43
    with torch.no_grad():
        assert amp.current_precision() == F32


def geoms(row, reflect=True):
    from mdctgan_amd import ops
    B, Ci, Co, H, W = row
    return tuple(ops.conv_geom(B, H, W, Ci, Co, 3, 3, 1, 1, reflect, p) for p in (HINF, F16))


QUERIES = ("mg_conv_wino_weights_bytes", "mg_conv_fwd_workspace", "mg_conv_dgrad_workspace", "mg_conv_wgrad_workspace",
           "mg_conv_fwd_instnorm_workspace", "mg_conv_wino_vnext_ok", "mg_conv_wino_md_from_norm_ok", "mg_conv_wgrad_adam_ok",
           "mg_conv_wgrad_checks_finite")


def same_as_f16(g, g16):
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    assert [ops.plan_name(p, g) for p in range(3)] == [ops.plan_name(p, g16) for p in range(3)]
    for q in QUERIES:
        assert getattr(lib, q)(g) == getattr(lib, q)(g16), q
    for which in (0, 1):
        assert lib.mg_conv_wino_tiles_bytes(g, which) == lib.mg_conv_wino_tiles_bytes(g16, which)
    assert ops.precast_ok(0, g) == ops.precast_ok(0, g16) and ops.weights_are_casts(g) == ops.weights_are_casts(g16)
    assert ops.wino_vnext_positions(g) == 0 and not ops.wino_images_half(g)


@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
def test_route_at_the_default_thresholds(monkeypatch, reflect):
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    monkeypatch.delenv("MG_INFER_F16_MIN_C", raising=False)
    monkeypatch.delenv("MG_INFER_F16_MIN_TILES", raising=False)
    # the trunk layer of the whole-model test: 8 x 32 = 256 tiles of 256 channels
    row = (8, 256, 256, 8, 16)
    g, g16 = geoms(row, reflect)
    T = 8 * 4 * 8
    assert ops.plan_name(0, g) == "winoh_gemm_kernel<64, 64, 2, 2, 3>" and ops.plan_name(0, g16) != ops.plan_name(0, g)
    assert ops.wino_images_half(g)
    assert lib.mg_conv_wino_weights_bytes(g) == 16 * 256 * 256 * 2
    assert lib.mg_conv_wino_tiles_bytes(g, 0) == 16 * T * 256 * 2 and lib.mg_conv_wino_tiles_bytes(g, 1) == 0
    assert lib.mg_conv_fwd_workspace(g) >= 16 * 256 * 256 * 2 + 16 * T * 256 * 2 + 16 * T * 256 * 4
    assert lib.mg_conv_fwd_instnorm_workspace(g) >= lib.mg_conv_fwd_workspace(g)
    assert lib.mg_conv_plan_flops(0, g) == 2.0 * 16 * T * 256 * 256 and lib.mg_conv_plan_splits(0, g) == 1
    assert lib.mg_conv_wino_vnext_ok(g) and ops.wino_vnext_positions(g) == 16
    assert not lib.mg_conv_wino_md_from_norm_ok(g) and not lib.mg_conv_wgrad_adam_ok(g)
    assert not ops.precast_ok(0, g) and not ops.weights_are_casts(g)
    # the inference batch's trunk takes the 128 x 128 tiles
    big = geoms((64, 1024, 1024, 8, 16), reflect)[0]
    assert ops.plan_name(0, big) == "winoh_gemm_kernel<128, 128, 4, 2, 2>"
    # B = 1: 32 tiles, a weight-streaming layer (conv_h16.h keeps it); 128 channels: below the channel threshold; 255 tiles;
    # Co % 64 != 0; odd W; other kernels and strides
    for r in ((1, 256, 256, 8, 16), (8, 128, 128, 8, 16), (8, 256, 128, 8, 16), (5, 256, 256, 6, 34), (8, 256, 288, 8, 16)):
        same_as_f16(*geoms(r, reflect))
    assert ops.plan_name(0, geoms((1, 256, 256, 8, 16), reflect)[0]).startswith("hgemm_sa_kernel")
    for k, s, p in ((3, 2, 1), (4, 1, 2), (1, 1, 0), (3, 1, 0)):
        same_as_f16(*(ops.conv_geom(8, 16, 16, 256, 256, k, k, s, p, False, prec) for prec in (HINF, F16)))
    # the other three precisions do not know the route
    for prec in (F32, F16, W43):
        assert not ops.plan_name(0, ops.conv_geom(8, 8, 16, 256, 256, 3, 3, 1, 1, reflect, prec)).startswith("winoh")


def test_route_with_lowered_thresholds(monkeypatch):
    """The GPU tests' rows: MG_INFER_F16_MIN_C=64 and MG_INFER_F16_MIN_TILES=1 bring them onto the route (an explicit tile threshold
    is the whole rule about the tile count: it also lifts the small-batch claim of conv_h16.h); the fused tail's ranges are
    wino_out_norm_kernel's."""
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    monkeypatch.setenv("MG_INFER_F16_MIN_C", "64")
    monkeypatch.setenv("MG_INFER_F16_MIN_TILES", "1")
    for row in ((2, 64, 64, 2, 2), (3, 64, 128, 4, 32), (2, 128, 64, 8, 16), (1, 64, 64, 4, 164), (1, 64, 64, 20, 32), (1, 64, 64, 14, 46)):
        g, g16 = geoms(row)
        tiles = (row[3] // 2) * (row[4] // 2)
        assert ops.plan_name(0, g) == "winoh_gemm_kernel<64, 64, 2, 2, 3>", row
        assert bool(lib.mg_conv_wino_vnext_ok(g)) == (tiles <= 64) and ops.wino_vnext_positions(g) == (16 if tiles <= 64 else 0), row
        assert lib.mg_conv_wino_tiles_bytes(g, 0) == 16 * row[0] * tiles * row[1] * 2, row
    same_as_f16(*geoms((1, 64, 96, 8, 16)))              # Co % 64 != 0
    same_as_f16(*geoms((1, 96, 64, 8, 16)))              # Ci % 64 != 0
    monkeypatch.delenv("MG_INFER_F16_MIN_TILES")
    same_as_f16(*geoms((3, 64, 128, 4, 32)))             # 96 tiles: below the default tile threshold
    monkeypatch.setenv("MG_INFER_F16_MIN_TILES", "97")
    same_as_f16(*geoms((3, 64, 128, 4, 32)))
    monkeypatch.setenv("MG_INFER_F16_MIN_TILES", "96")
    assert ops.plan_name(0, geoms((3, 64, 128, 4, 32))[0]).startswith("winoh_gemm_kernel")


CHILD = """
import sys
sys.path.insert(0, %r)
from mdctgan_amd import _lib, ops
lib = _lib.load()
g = ops.conv_geom(8, 8, 16, 256, 256, 3, 3, 1, 1, True, 3)
assert ops.plan_name(0, g).startswith("winoh_gemm_kernel")
p, n = 4096, 1 << 30
t = _lib.WinoTiles(None, None, None, None, 0)
print("ws=%%d,%%d" %% (lib.mg_conv_dgrad_workspace(g), lib.mg_conv_wgrad_workspace(g)))
print("names=%%d,%%d" %% tuple(lib.mg_conv_plan_name(ps, g, b" " * 96, 96) for ps in (1, 2)))
print("splits=%%d,%%d" %% tuple(lib.mg_conv_plan_splits(ps, g) for ps in (1, 2)))
rcs = [lib.mg_conv_dgrad(g, p, p, None, p, 0, p, n, None), lib.mg_conv_dgrad_w(g, p, p, None, p, 0, p, n, None, t),
       lib.mg_conv_wgrad(g, p, p, p, None, 0, p, n, None), lib.mg_conv_wgrad_w(g, p, p, p, None, 0, p, n, None, t),
       lib.mg_conv_wgrad_chk(g, p, p, p, None, 0, p, n, None, t, None), lib.mg_instnorm_bwd_wino_md(g, p, p, p, p, 0, p, None)]
print("rc=" + ",".join(str(r) for r in rcs))
# the float32 hand-over entry point does not write this layer's float16 image
print("next=%%d" %% lib.mg_conv_fwd_instnorm_next(g, p, p, None, None, 1e-5, 0, None, p, p, p, p, n, None, t, p, 1))
""" % REPO


def test_gradient_entry_points_refuse_the_route():
    proc = subprocess.run([sys.executable, "-c", CHILD], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=REPO,
                          timeout=300)
    assert proc.returncode == 0, "child exit status %d\n%s" % (proc.returncode, proc.stderr[-2000:])
    lines = dict(ln.split("=", 1) for ln in proc.stdout.strip().splitlines())
    assert lines["ws"] == "0,0"
    assert lines["names"] == "%d,%d" % (MG_ERR_UNSUPPORTED, MG_ERR_UNSUPPORTED) and lines["splits"] == "0,0"
    assert lines["rc"] == ",".join([str(MG_ERR_UNSUPPORTED)] * 6)
    assert lines["next"] == "-1"
