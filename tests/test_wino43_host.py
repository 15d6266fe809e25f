"""The opt-in Winograd F(4x4,3x3) family (csrc/wino43.h, MG_PRECISION_F32_WINO43) without a GPU:

1. the three matrices, rebuilt in exact rationals from the point set (0, 1, -1, 1/2, -2, inf) by scripts/wino43_points.py, are the
   ones the kernels hold and reproduce a direct 2-D convolution exactly;
2. the library's host-side queries agree with a hand-written table about which geometries route to the family and which may use
   the fused output-transform + InstanceNorm kernel and its hand-over;
3. the gradient workspace queries and entry points refuse the route (fake pointers, in a child process: a call that went on
   would fault the child, not the test run);
4. the Python switches: amp.wino43, --wino43.
"""
import importlib.util
import os
import re
import subprocess
import sys
from fractions import Fraction as Fr

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, W43 = 0, 1, 2
MG_ERR_UNSUPPORTED = -2


def points_module():
    spec = importlib.util.spec_from_file_location("wino43_points", os.path.join(REPO, "scripts", "wino43_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# the matrices as the family's description states them
AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, Fr(1, 2), -2, 0], [0, 1, 1, Fr(1, 4), 4, 0], [0, 1, -1, Fr(1, 8), -8, 1]]
G = [[1, 0, 0], [Fr(1, 3), Fr(1, 3), Fr(1, 3)], [Fr(-1, 3), Fr(1, 3), Fr(-1, 3)], [Fr(-16, 15), Fr(-8, 15), Fr(-4, 15)],
     [Fr(1, 15), Fr(-2, 15), Fr(4, 15)], [0, 0, 1]]
BT = [[1, Fr(-3, 2), -2, Fr(3, 2), 1, 0], [0, -1, Fr(1, 2), Fr(5, 2), 1, 0], [0, 1, Fr(-5, 2), Fr(1, 2), 1, 0],
      [0, -2, -1, 2, 1, 0], [0, Fr(1, 2), -1, Fr(-1, 2), 1, 0], [0, 1, Fr(-3, 2), -2, Fr(3, 2), 1]]


def matmul(a, b):
    return [[sum(Fr(a[i][k]) * Fr(b[k][j]) for k in range(len(b))) for j in range(len(b[0]))] for i in range(len(a))]


def transpose(a):
    return [list(r) for r in zip(*a)]


def test_matrices_from_the_points_reproduce_a_direct_convolution_exactly():
    at, g, bt = points_module().toom_cook((0, 1, -1, Fr(1, 2), -2, None), 4, 3)
    assert at == [[Fr(v) for v in r] for r in AT]
    assert g == [[Fr(v) for v in r] for r in G]
    assert bt == [[Fr(v) for v in r] for r in BT]
    # an integer patch and kernel: Y = A^T [(G w G^T) .* (B^T d B)] A in rationals against the 16 sums of 9 products
    d = [[Fr((7 * r + 3 * c * c + r * c) % 11 - 5) for c in range(6)] for r in range(6)]
    w = [[Fr((5 * r + 2 * c + 1) % 7 - 3) for c in range(3)] for r in range(3)]
    u = matmul(matmul(g, w), transpose(g))
    v = matmul(matmul(bt, d), transpose(bt))
    m = [[u[i][j] * v[i][j] for j in range(6)] for i in range(6)]
    y = matmul(matmul(at, m), transpose(at))
    want = [[sum(d[oy + r][ox + c] * w[r][c] for r in range(3) for c in range(3)) for ox in range(4)] for oy in range(4)]
    assert y == want


def test_kernel_header_holds_these_matrices():
    """csrc/wino43.h's three constant tables, read as text and evaluated in rationals, are the matrices above."""
    src = open(os.path.join(REPO, "mdctgan_amd", "csrc", "wino43.h")).read()
    for name, want in (("W43_AT", AT), ("W43_G", G), ("W43_BT", BT)):
        body = re.search(r"struct %s \{.*?=\s*(\{\{.*?\}\});" % name, src, re.S).group(1)
        rows = re.findall(r"\{([^{}]*)\}", body)
        got = []
        for row in rows:
            vals = []
            for tok in row.split(","):
                tok = tok.strip().replace("f", "")
                if "/" in tok:
                    a, b = tok.split("/")
                    vals.append(Fr(a.strip()) / Fr(b.strip()))
                else:
                    vals.append(Fr(tok))
            got.append(vals)
        assert got == [[Fr(v) for v in r] for r in want], name


# (B, Ci, Co, H, W, MG_WINO43_MIN_C or None) -> (routes to F(4x4,3x3)?, fused kernel and hand-over?)
TABLE = {
    (2, 32, 32, 4, 4, "32"): (True, True),            # one tile
    (3, 64, 64, 4, 32, "32"): (True, True),           # Co % 64 == 0: the LDS-DMA dense GEMM with 36 positions
    (2, 32, 32, 8, 16, "32"): (True, True),
    (2, 48, 32, 8, 16, "32"): (True, True),           # Ci is not a multiple of 32
    (2, 32, 48, 8, 16, "32"): (True, False),          # Co % 32 != 0: the unfused sequence
    (1, 32, 32, 20, 32, "32"): (True, True),          # 40 tiles: the fused kernel's limit
    (1, 32, 32, 4, 164, "32"): (True, False),         # 41 tiles
    (1, 96, 96, 16, 8, "32"): (True, True),
    (2, 32, 32, 6, 16, "32"): (False, False),         # H % 4 != 0
    (2, 32, 32, 8, 18, "32"): (False, False),         # W % 4 != 0
    (2, 16, 32, 8, 16, "32"): (False, False),         # Ci below min_c
    (2, 32, 16, 8, 16, "32"): (False, False),         # Co below min_c
    (2, 40, 32, 8, 16, "32"): (False, False),         # Ci % 16 != 0
    (2, 32, 32, 8, 16, None): (False, False),         # default min_c = 256
    (2, 256, 128, 8, 16, None): (False, False),
    (1, 256, 256, 8, 16, None): (True, True),         # the weight-heavy layers the mode is for
    (1, 1024, 1024, 8, 16, None): (True, True),
}


@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
def test_route_table(monkeypatch, reflect):
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    for (B, Ci, Co, H, W, min_c), (routed, fused) in TABLE.items():
        if min_c is None:
            monkeypatch.delenv("MG_WINO43_MIN_C", raising=False)
        else:
            monkeypatch.setenv("MG_WINO43_MIN_C", min_c)
        row = (B, Ci, Co, H, W, min_c)
        g = ops.conv_geom(B, H, W, Ci, Co, 3, 3, 1, 1, reflect, W43)
        g32 = ops.conv_geom(B, H, W, Ci, Co, 3, 3, 1, 1, reflect, F32)
        name = ops.plan_name(0, g)
        if routed:
            T = B * (H // 4) * (W // 4)
            assert lib.mg_conv_wino_weights_bytes(g) == 36 * Co * Ci * 4, row
            assert lib.mg_conv_wino_tiles_bytes(g, 0) == 36 * T * Ci * 4 and lib.mg_conv_wino_tiles_bytes(g, 1) == 0, row
            # one batched launch of 36 positions: the dense GEMM's own instance, or the implicit-GEMM kernels' tag 5
            assert re.fullmatch(r"dgemm32g_kernel<.*, 36, 0>|dgemm32_kernel<.*>|conv_fwd(32)?_kernel<.*, 5>", name), (row, name)
            assert (Co % 64 == 0 and Ci % 32 == 0) == name.startswith("dgemm32g_kernel"), (row, name)
            assert lib.mg_conv_plan_flops(0, g) == 2.0 * 36 * T * Co * Ci, row
            assert lib.mg_conv_fwd_workspace(g) >= (36 * Co * Ci + 36 * T * (Ci + Co)) * 4, row
        else:           # the route, the sizes and the plan of MG_PRECISION_F32
            assert name == ops.plan_name(0, g32), (row, name)
            for q in (lib.mg_conv_wino_weights_bytes, lib.mg_conv_fwd_workspace, lib.mg_conv_dgrad_workspace,
                      lib.mg_conv_wgrad_workspace, lib.mg_conv_fwd_instnorm_workspace, lib.mg_conv_wino_vnext_ok,
                      lib.mg_conv_wino_md_from_norm_ok, lib.mg_conv_wgrad_adam_ok):
                assert q(g) == q(g32), (row, q.__name__)
            assert [ops.plan_name(p, g) for p in (1, 2)] == [ops.plan_name(p, g32) for p in (1, 2)], row
        assert bool(lib.mg_conv_wino_vnext_ok(g)) == (fused or (not routed and bool(lib.mg_conv_wino_vnext_ok(g32)))), row
        if routed:
            assert fused == (Co % 32 == 0 and (H // 4) * (W // 4) <= 40), row
            assert not lib.mg_conv_wino_md_from_norm_ok(g) and not lib.mg_conv_wgrad_adam_ok(g), row
            assert ops.wino_vnext_positions(g) == (36 if fused else 0), row
    # other kernel shapes and the float16 precision never reach the family
    monkeypatch.setenv("MG_WINO43_MIN_C", "32")
    for k, s, p in ((3, 2, 1), (4, 1, 2), (1, 1, 0), (3, 1, 0)):
        g, g32 = (ops.conv_geom(2, 16, 16, 32, 32, k, k, s, p, False, prec) for prec in (W43, F32))
        assert ops.plan_name(0, g) == ops.plan_name(0, g32) and lib.mg_conv_wino_weights_bytes(g) == lib.mg_conv_wino_weights_bytes(g32)
    g16 = ops.conv_geom(2, 8, 16, 32, 32, 3, 3, 1, 1, True, F16)
    assert lib.mg_conv_wino_weights_bytes(g16) != 36 * 32 * 32 * 4
    assert lib.mg_conv_wino_weights_bytes(ops.conv_geom(2, 8, 16, 32, 32, 3, 3, 1, 1, True, 3)) == 0      # no fourth value


CHILD = """
import sys
sys.path.insert(0, %r)
import os
os.environ["MG_WINO43_MIN_C"] = "32"
from mdctgan_amd import _lib, ops
lib = _lib.load()
g = ops.conv_geom(2, 8, 16, 32, 32, 3, 3, 1, 1, True, 2)
p, n = 4096, 1 << 30
t = _lib.WinoTiles(None, None, None, None, 0)
print("ws=%%d,%%d" %% (lib.mg_conv_dgrad_workspace(g), lib.mg_conv_wgrad_workspace(g)))
print("names=%%d,%%d" %% tuple(lib.mg_conv_plan_name(ps, g, b" " * 96, 96) for ps in (1, 2)))
print("splits=%%d,%%d" %% tuple(lib.mg_conv_plan_splits(ps, g) for ps in (1, 2)))
rcs = [lib.mg_conv_dgrad(g, p, p, None, p, 0, p, n, None), lib.mg_conv_dgrad_w(g, p, p, None, p, 0, p, n, None, t),
       lib.mg_conv_wgrad(g, p, p, p, None, 0, p, n, None), lib.mg_conv_wgrad_w(g, p, p, p, None, 0, p, n, None, t),
       lib.mg_conv_wgrad_chk(g, p, p, p, None, 0, p, n, None, t, None), lib.mg_instnorm_bwd_wino_md(g, p, p, p, p, 0, p, None)]
print("rc=" + ",".join(str(r) for r in rcs))
""" % REPO


def test_gradient_entry_points_refuse_the_route():
    proc = subprocess.run([sys.executable, "-c", CHILD], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=REPO,
                          timeout=300)
    assert proc.returncode == 0, "child exit status %d\n%s" % (proc.returncode, proc.stderr[-2000:])
    lines = dict(ln.split("=", 1) for ln in proc.stdout.strip().splitlines())
    assert lines["ws"] == "0,0"
    assert lines["names"] == "%d,%d" % (MG_ERR_UNSUPPORTED, MG_ERR_UNSUPPORTED) and lines["splits"] == "0,0"
    assert lines["rc"] == ",".join([str(MG_ERR_UNSUPPORTED)] * 6)


def test_switches():
    from mdctgan_amd import _lib, amp, options
    assert _lib.PRECISION_F32_WINO43 == W43
    assert options.make_opt("--wino43").wino43 is True and options.make_opt().wino43 is False
    assert "wino43" not in options.SPECTRAL_FLAGS and "--wino43" not in options.SPECTRAL_FLAGS
    assert torch.is_grad_enabled() and amp.current_precision() == F32
    with torch.no_grad():
        assert amp.current_precision() == F32                      # off by default
    with amp.wino43():
        assert amp.current_precision() == F32                      # grad mode: nothing changes
        with torch.no_grad():
            assert amp.current_precision() == W43
            with amp.autocast(True):
                assert amp.current_precision() == F16              # --fp16 is out of the mode's scope
            with amp.wino43(False):
                assert amp.current_precision() == F32
            with torch.enable_grad():
                assert amp.current_precision() == F32
        with amp.autocast(True), torch.no_grad():
            assert amp.current_precision() == F16
    with torch.no_grad():
        assert amp.current_precision() == F32
