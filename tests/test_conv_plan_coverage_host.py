"""Every convolution kernel instance the dispatchers of csrc/conv_igemm.hip, csrc/wino_host.h, csrc/conv_dma.h and dense_launch
can launch is reached by a per-element float64 parity case: the case tables of test_conv_gpu.py, test_amp_gpu.py and
test_conv_plans_gpu.py are walked with their planner hooks applied and mg_conv_plan_name collected for the three passes -- on
the host, no GPU.  The list below is written out by hand from the alternatives of dispatch_tile / dispatch_tag /
dispatch_wino_tag / dispatch_bool (csrc/conv_plan.h) as the three generic launchers and wino_gemm nest them, CD_TILE_DISPATCH / conv_dma_wgrad_launch and dense_launch: whoever adds
a tile or a tag adds it here and then needs a case.  (mg_conv_plan_name prints the pick the launcher dispatches on, so a name
seen here is an instance launched.)"""
import itertools
import os

import test_amp_gpu
import test_conv_gpu
import test_conv_plans_gpu as P

F32, F16 = 0, 1
IGEMM_TILES = ((128, 128), (128, 64), (64, 64))                  # dispatch_tile: conv_fwd, conv_dgrad, wino_gemm
WGRAD_TILES = ((128, 128), (64, 64))                             # ... its square tiles: mg_conv_wgrad_chk, wino_gemm's pass 2
DMA_TILES = ((64, 64), (64, 128), (128, 64), (128, 128))         # CD_TILE_DISPATCH, dense_launch
# tags: 0 float32 convolution, 2 float16 convolution, 1 / 5 the float32 Winograd-domain GEMMs of 16 / 25 positions, 3 the float16 ones


def expected_instances():
    want = set()
    for bm, bn in IGEMM_TILES:
        for tag in (0, 1, 2, 3, 5):
            want.add("conv_fwd_kernel<%d, %d, true, %d>" % (bm, bn, tag))
            want.add("conv_fwd32_kernel<%d, %d, %d>" % (bm, bn, tag))
            want.add("conv_dgrad_kernel<%d, %d, true, true, %d>" % (bm, bn, tag))
        for tag in (0, 2):           # the scalar-load instances exist for the convolutions only
            want.add("conv_fwd_kernel<%d, %d, false, %d>" % (bm, bn, tag))
            want.add("conv_dgrad_kernel<%d, %d, false, false, %d>" % (bm, bn, tag))
    for t, _ in WGRAD_TILES:
        for tag in (0, 1, 2, 3, 5):
            want.add("conv_wgrad_kernel<%d, %d, true, true, %d>" % (t, t, tag))
        for tag in (0, 2):
            want.add("conv_wgrad_kernel<%d, %d, false, false, %d>" % (t, t, tag))
    for (bm, bn), half in itertools.product(DMA_TILES, ("false", "true")):
        want.add("conv_fwd_dma_kernel<%d, %d, %s, 2>" % (bm, bn, half))
        want.add("conv_dgrad_dma_kernel<%d, %d, %s, 2>" % (bm, bn, half))
        for rr in ("false", "true"):
            want.add("conv_wgrad_dma_kernel<%d, %d, %s, 2, %s>" % (bm, bn, half, rr))
    for (bm, bn), positions, (al, bl) in itertools.product(DMA_TILES, (16, 25), ((0, 0), (0, 1), (1, 1))):
        want.add("dgemm32g_kernel<%d, %d, 2, 2, %d, %d, 2, %d, 0>" % (bm, bn, al, bl, positions))
    for bl in (0, 1):                # register-staged: forward and data-gradient layouts (the weight gradient always stages by DMA)
        want.add("dgemm32_kernel<64, 64, 2, 2, 0, %d, 0>" % bl)
        want.add("dgemm32_kernel<128, 128, 4, 2, 0, %d, 0>" % bl)
    return want


def walk_cases():
    """(shape (B, Ci, H, W, Co, k, stride, pad, reflect), precision, planner hooks, passes the case runs and compares)."""
    every = (0, 1, 2)
    for c in test_conv_gpu.CONV_CASES:
        yield tuple(c[1:]), F32, {"MG_WINO42_MIN_WORK": "0"}, every
    for c in test_conv_gpu.RR_CASES:          # test_wgrad_row_regular_gather_is_the_general_gather: the weight gradient only
        name, B, Ci, H, W, Co, k, s, p, _ = c
        yield (B, Ci, H, W, Co, k, s, p, False), F32, {}, (2,)
        yield (B, Ci, H, W, Co, k, s, p, False), F32, {"MG_NO_WGRAD_RR": "1"}, (2,)
    for name, B, Cin, h, w, Cout in test_conv_gpu.CONVT_CASES:
        yield (B, Cout, 2 * h, 2 * w, Cin, 3, 2, 1, False), F32, {}, every
    for c in test_amp_gpu.CASES:
        yield tuple(c[1:]), F16, {}, every
    yield from P.all_cases()


def test_every_dispatched_instance_has_a_parity_case(monkeypatch):
    from mdctgan_amd import ops
    # (MG_HALF_NBUF and MG_NO_BK32 are read once per process and rename instances: the list is that of the default build)
    assert "MG_HALF_NBUF" not in os.environ and "MG_NO_BK32" not in os.environ
    seen = set()
    for shape, prec, env, passes in walk_cases():
        P.apply_env(monkeypatch, env)
        g = P.geom_of(shape, prec)
        seen.update(ops.plan_name(ps, g) for ps in passes)
    missing = sorted(expected_instances() - seen)
    assert not missing, missing
