// Host-side planning layer of the convolution translation unit: the event probe and mg_launch, the geometry helpers, the dense
// Winograd-domain GEMM stage (dense_plan / dense_launch), the cd_* staging helpers of the DMA passes, gemm_plan with its tuned
// table, fwd_plan / dgrad_plan / wgrad_plan, GemmPick with its three fillers, the dispatch_* helpers and ConvRoute.
// Needs: conv_kernels.h, wino.h (wino_grid), mdctgan_hip.h, <type_traits>, <stdio.h>, <stdlib.h>, <hip/hip_ext.h>.
#pragma once

namespace {
// One-shot event probe: bench.py arms it right before a call whose main GEMM kernel it wants timed on the launch
// stream.  The LDS-DMA launchers (mg_launch below) hand the two events to hipExtLaunchKernelGGL, which stamps them with
// the dispatch's own begin / end times -- the duration rocprofv3 reports for that kernel; the older launch sites record the
// events immediately around their launch (a few microseconds of queue latency included).
hipEvent_t g_probe_e0 = nullptr, g_probe_e1 = nullptr;
bool g_probe_exact = false;
inline void probe_begin(hipStream_t st) {
    g_probe_exact = false;
    if (g_probe_e0) hipEventRecord(g_probe_e0, st);
}
inline void probe_end(hipStream_t st) {
    if (g_probe_e1 && !g_probe_exact) hipEventRecord(g_probe_e1, st);
    g_probe_e0 = g_probe_e1 = nullptr;
    g_probe_exact = false;
}
template <typename KernelT, typename ArgT>
inline void mg_launch(KernelT kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, const ArgT& a) {
    if (g_probe_e0 && g_probe_e1 && !g_probe_exact) {
        hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)lds, st, g_probe_e0, g_probe_e1, 0, a);
        g_probe_exact = true;
    } else {
        hipLaunchKernelGGL(kern, grid, block, lds, st, a);
    }
}

Geom to_geom(const mg_conv_geom* g) {
    return Geom{g->B, g->H, g->W, g->Ci, g->OH, g->OW, g->Co, g->KH, g->KW, g->stride, g->pad, g->reflect};
}

// half-precision arithmetic: autocast training, and the opt-in inference mode that shares its arithmetic
inline bool prec_h(const mg_conv_geom* g) { return MG_PRECISION_IS_HALF(g->precision); }

bool geom_ok(const mg_conv_geom* g) {
    if (g && g->precision != MG_PRECISION_F32 && !MG_PRECISION_IS_HALF(g->precision) && g->precision != MG_PRECISION_F32_WINO43) return false;
    if (!g || g->B <= 0 || g->H <= 0 || g->W <= 0 || g->Ci <= 0 || g->Co <= 0 || g->KH <= 0 || g->KW <= 0) return false;
    if (g->stride < 1 || g->stride > 2 || g->pad < 0) return false;
    if (g->OH != (g->H + 2 * g->pad - g->KH) / g->stride + 1) return false;
    if (g->OW != (g->W + 2 * g->pad - g->KW) / g->stride + 1) return false;
    if (g->reflect && (g->pad >= g->H || g->pad >= g->W)) return false;
    const long long lim = 1LL << 31;      // kernels index activations / weights with 32-bit element offsets
    if ((long long)g->B * g->H * g->W * g->Ci >= lim || (long long)g->B * g->OH * g->OW * g->Co >= lim ||
        (long long)g->Co * g->KH * g->KW * g->Ci >= lim)
        return false;
    return true;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// A forward convolution whose caller normalises the result right away (mg_conv_fwd_instnorm_*) may leave its split-K slabs
// unreduced: the InstanceNorm slab kernel sums them itself (instnorm.hip: mg_instnorm_fwd_slabs) -- one launch fewer per layer.
// The caller passes a FwdDefer; a path that can oblige fills it INSTEAD of launching splitk_epilogue_kernel.
struct FwdDefer { const float* part; int splits; const float* bias; int round_f16; bool filled; };
// The kernel families on LDS-DMA staging.  They have no namespace of their own and launch through the mg_launch of whoever
// includes them (scripts/ubench/gemm_bench.hip and hgemm_bench.hip supply a plain one), so they are included here, inside this
// namespace, behind the probe's mg_launch, to_geom and FwdDefer.
#include "dense_gemm.h"
#include "dense_gemm_h.h"
#include "conv_h16.h"
#include "conv_dma.h"
#include "conv_co1.h"

// ---------------------------------------------------------------------------------------------------------
// Batched dense GEMMs of the Winograd families on dense_gemm.h (float32 precision; the f16 path keeps the convolution
// kernels' dense instances).  pass 0: C[T][Co] = V[T][Kc] U[Co][Kc]^T; pass 1: dV[T][Kc] = Md[T][Co] U[Co][Kc];
// pass 2: dU[Co][Kc] = Md[T][Co]^T V[T][Kc].
// ---------------------------------------------------------------------------------------------------------
struct DensePlan { int bm, bn, splits, cps; bool dma, ok; };
struct DenseDims { long long M; int N, K; };
inline DenseDims dense_dims(int pass, long long T, int Co, int Kc) {
    if (pass == 0) return {T, Co, Kc};
    if (pass == 1) return {T, Kc, Co};
    return {(long long)Co, Kc, (int)T};
}
DensePlan dense_plan(int pass, int P, long long T, int Co, int Kc, bool hp) {
    const DenseDims dd = dense_dims(pass, T, Co, Kc);
    DensePlan p{64, 64, 1, 1 << 28, false, false};
    if (hp || dd.N % 64 != 0 || dd.K % 4 != 0 || dd.K < 4 || dd.M < 1 || T >= (1LL << 31)) return p;
    if (pass == 2 && dd.M % 4 != 0) return p;
    // every operand of one position must stay below 2 GiB (32-bit byte offsets of the LDS-DMA path)
    if ((double)dd.M * dd.K * 4.0 >= 2e9 || (double)dd.N * dd.K * 4.0 >= 2e9) return p;
    p.ok = true;
    // LDS-DMA staging: whole 32-deep chunks, or the weight-gradient GEMM (both operands [K][rows]: the K tail is zero-filled
    // by the buffer range check); the register-staged path stays for the shapes the DMA path does not take
    p.dma = dd.K % DG_BK == 0 || pass == 2;
    // Cost model calibrated on scripts/ubench/gemm_bench.hip (MI355X): the workgroups of one CU share its MFMA pipe, so a
    // launch takes ceil(workgroups / 256) tile-times; efficiencies are the measured large-grid figures per tile; a grid with
    // fewer than two workgroups per CU cannot cover its barrier drains (x 0.85); split-K pays one pass over the slabs.
    struct Cand { int bm, bn; double eff_dma, eff_reg; };
    static const Cand cands[4] = {{64, 64, 0.83, 0.71}, {64, 128, 0.885, 0.74}, {128, 64, 0.855, 0.74}, {128, 128, 0.91, 0.80}};
    static const int split_opts[8] = {1, 2, 3, 4, 6, 8, 12, 16};
    const int chunks = (dd.K + DG_BK - 1) / DG_BK;
    int f_bm = 0, f_bn = 0, f_sp = 0;
    if (const char* f = getenv("MG_FORCE_DENSE")) {      // tuning harness: "bm,bn,splits" (dropped where the shape does not admit it)
        if (sscanf(f, "%d,%d,%d", &f_bm, &f_bn, &f_sp) != 3) f_bm = f_bn = f_sp = 0;
    }
    double best = 1e300;
    auto search = [&]() {
        for (const Cand& c : cands) {
            if (dd.N % c.bn != 0) continue;
            if (!p.dma && !((c.bm == 64 && c.bn == 64) || (c.bm == 128 && c.bn == 128))) continue;   // register-path instances
            if (f_bm && (c.bm != f_bm || c.bn != f_bn)) continue;
            const long long w = ((dd.M + c.bm - 1) / c.bm) * (long long)(dd.N / c.bn) * P;
            const double tile_us = 2.0 * c.bm * c.bn * DG_BK / (157.3e12 / 256.0) * 1e6 / (p.dma ? c.eff_dma : c.eff_reg);
            for (int sp : split_opts) {
                if (sp > 1 && chunks / sp < 8) break;
                if (f_sp && sp != f_sp) continue;
                const int cps = (chunks + sp - 1) / sp;
                const int spl = (chunks + cps - 1) / cps;
                const long long wg = w * spl;
                double t = (double)((wg + 255) / 256) * tile_us * (cps + 1.2);
                // forward / data gradient: 500 workgroups already count as two rounds (17x33 maps on 128x128 tiles: 110 against
                // 125 us with the penalty); the weight gradient's short K loops keep the wider band (measured both ways)
                if (wg < (pass == 2 ? 512 : 384)) t /= 0.85;
                if (spl > 1) t += (double)(spl + 1) * P * (double)dd.M * dd.N * 4.0 / 4e12 * 1e6 + 3.0;
                if (t < best) { best = t; p.bm = c.bm; p.bn = c.bn; p.splits = spl; p.cps = cps; }
            }
        }
    };
    search();
    if (best == 1e300 && (f_bm || f_sp)) {      // a forced plan the shape does not admit is dropped, as the other hooks' are
        f_bm = f_bn = f_sp = 0;
        search();
    }
    if (best == 1e300) { p.ok = false; return p; }
    if (p.splits == 1) p.cps = 1 << 28;
    return p;
}
// MG_F32_SPLIT=1 (opt-in, read per call so a test can flip it): the Winograd-domain GEMMs multiply float32 operands as three
// exact bf16 pieces each on v_mfma_f32_32x32x16_bf16 (dense_gemm.h: dg_chunk_b8; 8 of the 9 piece products, float32
// accumulation) -- float32-accurate results (error vs float64 1.3e-6 of the output scale against 1.5e-6 for
// v_mfma_f32_32x32x2_f32) at half the MFMA cycles.  Off by default: the bench's float32 line is the float32 pipe.
inline bool f32_split() {
    const char* e = getenv("MG_F32_SPLIT");
    return e && e[0] == '1';
}
inline bool dense_split(const DensePlan& p, int P, int N) {
    return p.dma && (P == 16 || P == 25) && N % 128 == 0 && f32_split();
}
template <int AL, int BL>
void dense_launch(const DensePlan& p, const DgArgs& a, hipStream_t st) {
    if (dense_split(p, a.P, a.N)) {
        if (a.P == 16) dgemm32g_launch<128, 128, 2, 2, AL, BL, 2, 16, 1>(a, st);
        else dgemm32g_launch<128, 128, 2, 2, AL, BL, 2, 25, 1>(a, st);
    } else if (p.dma && a.P == 16) {
        if (p.bm == 128 && p.bn == 128) dgemm32g_launch<128, 128, 2, 2, AL, BL, 2, 16>(a, st);
        else if (p.bm == 64 && p.bn == 128) dgemm32g_launch<64, 128, 2, 2, AL, BL, 2, 16>(a, st);
        else if (p.bm == 128 && p.bn == 64) dgemm32g_launch<128, 64, 2, 2, AL, BL, 2, 16>(a, st);
        else dgemm32g_launch<64, 64, 2, 2, AL, BL, 2, 16>(a, st);
    } else if (p.dma && a.P == 36) {      // F(4x4,3x3) has a forward pass only
        if constexpr (AL == DG_KC && BL == DG_KC) {
            if (p.bm == 128 && p.bn == 128) dgemm32g_launch<128, 128, 2, 2, AL, BL, 2, 36>(a, st);
            else if (p.bm == 64 && p.bn == 128) dgemm32g_launch<64, 128, 2, 2, AL, BL, 2, 36>(a, st);
            else if (p.bm == 128 && p.bn == 64) dgemm32g_launch<128, 64, 2, 2, AL, BL, 2, 36>(a, st);
            else dgemm32g_launch<64, 64, 2, 2, AL, BL, 2, 36>(a, st);
        }
    } else if (p.dma) {
        if (p.bm == 128 && p.bn == 128) dgemm32g_launch<128, 128, 2, 2, AL, BL, 2, 25>(a, st);
        else if (p.bm == 64 && p.bn == 128) dgemm32g_launch<64, 128, 2, 2, AL, BL, 2, 25>(a, st);
        else if (p.bm == 128 && p.bn == 64) dgemm32g_launch<128, 64, 2, 2, AL, BL, 2, 25>(a, st);
        else dgemm32g_launch<64, 64, 2, 2, AL, BL, 2, 25>(a, st);
    } else {
        if (p.bm == 128) dgemm32_launch<128, 128, 4, 2, AL, BL>(a, st);
        else dgemm32_launch<64, 64, 2, 2, AL, BL>(a, st);
    }
}
void dense_name(int pass, int P, const DensePlan& p, int N, char* out, int out_len) {
    const int al = pass == 2 ? DG_RC : DG_KC, bl = pass == 0 ? DG_KC : DG_RC;
    if (dense_split(p, P, N)) snprintf(out, out_len, "dgemm32g_kernel<128, 128, 2, 2, %d, %d, 2, %d, 1>", al, bl, P);
    else if (p.dma) snprintf(out, out_len, "dgemm32g_kernel<%d, %d, 2, 2, %d, %d, 2, %d, 0>", p.bm, p.bn, al, bl, P);
    else snprintf(out, out_len, "dgemm32_kernel<%d, %d, %d, 2, %d, %d, 0>", p.bm, p.bn, p.bm == 128 ? 4 : 2, al, bl);
}
// Runs the GEMM (and its split-K combine) on plan p (p.ok)
void dense_wino_gemm(const DensePlan& p, int pass, int P, long long T, int Co, int Kc, const float* A, const float* B, float* C,
                     float* part, hipStream_t st) {
    const DenseDims dd = dense_dims(pass, T, Co, Kc);
    DgArgs a{};
    a.A = A; a.B = B; a.C = C; a.part = p.splits > 1 ? part : nullptr;
    a.M = (int)dd.M; a.N = dd.N; a.K = dd.K;
    a.P = P; a.splits = p.splits; a.cps = p.cps;
    a.sc = dd.M * dd.N;
    probe_begin(st);
    if (pass == 0) {            // V [T][Kc] x U [Co][Kc]^T
        a.lda = Kc; a.ldb = Kc; a.sa = T * Kc; a.sb = (long long)Co * Kc;
        dense_launch<DG_KC, DG_KC>(p, a, st);
    } else if (pass == 1) {     // Md [T][Co] x U [Co][Kc]
        a.lda = Co; a.ldb = Kc; a.sa = T * Co; a.sb = (long long)Co * Kc;
        dense_launch<DG_KC, DG_RC>(p, a, st);
    } else {                    // Md [T][Co]^T x V [T][Kc]
        a.lda = Co; a.ldb = Kc; a.sa = T * Co; a.sb = T * Kc;
        dense_launch<DG_RC, DG_RC>(p, a, st);
    }
    probe_end(st);
    if (p.splits > 1) {
        const size_t n = (size_t)P * dd.M * dd.N;
        splitk_reduce(wino_grid(n / 4), part, p.splits, n, C, 0, st);
    }
}
inline size_t slab_count(int old_splits, int dense) {      // split-K slabs a workspace must hold (either path may run)
    const int m = old_splits > dense ? old_splits : dense;
    return m > 1 ? (size_t)m : 0;
}
// float32 -> float16 staging copy of n elements (n % 8 == 0 for every eligible layer: Ci, Co % 64 == 0)
inline void cd_cast16(const float* src, void* dst, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(h16_cast_kernel, dim3(h16_grid(n / 8)), dim3(256), 0, st, src, (_Float16*)dst, n / 8);
}
// The float16 copy of an operand of a DMA pass: the caller's (kept) when handed over -- cast into it unless its producer filled
// it already -- else a cast into the workspace; either way the workspace pointer moves past the operand's slot
inline const void* cd_stage16(const float* src, const void* kept, bool filled, size_t n, size_t slot_bytes, char*& wsp, hipStream_t st) {
    void* dst = kept ? const_cast<void*>(kept) : (void*)wsp;
    if (!(kept && filled)) cd_cast16(src, dst, n, st);
    wsp += slot_bytes;
    return dst;
}
// ReflectionPad2d(1) + 3x3 stride-1 data gradient on the DMA kernel: the zero-padded "full" data gradient over the padded
// (H+2) x (W+2) domain (cd_reflect_geom: pad 0, same OH x OW), folded back onto H x W by wino_fold_reflect_kernel
inline mg_conv_geom cd_reflect_geom(const mg_conv_geom* g) {
    mg_conv_geom gp = *g;
    gp.H += 2; gp.W += 2; gp.pad = 0; gp.reflect = 0;
    return gp;
}
inline bool cd_reflect_dgrad_ok(const mg_conv_geom* g) {
    if (!g->reflect || g->stride != 1 || g->pad != 1 || g->KH != 3 || g->KW != 3 || g->Ci % 4) return false;
    const mg_conv_geom gp = cd_reflect_geom(g);
    return conv_dma_dgrad_ok(&gp);
}
// staging + split-K slabs of the DMA data gradient
inline size_t cd_dgrad_ws(const mg_conv_geom* g) {
    const CdPlan cp = conv_dma_dgrad_plan(g);
    const size_t stage = conv_dma_half(g) ? conv_dma_h_dy_bytes(g) + conv_dma_h_w_bytes(g) : 0;
    return stage + (cp.splits > 1 ? (size_t)cp.splits * g->B * g->H * g->W * g->Ci * sizeof(float) : 0) + 256;
}
inline size_t cd_reflect_dxp_bytes(const mg_conv_geom* gp) { return cd_al((size_t)gp->B * gp->H * gp->W * gp->Ci * sizeof(float)); }
// the DMA data gradient proper.  wsp: cd_dgrad_ws(g) bytes (may be null when nothing is needed); round_f16: autocast output
// rounding of the direct result (the reflect wrapper rounds after its fold instead)
int cd_dgrad_run(const mg_conv_geom* g, const float* dy, const float* w, const float* bias, float* dx, int act, char* wsp,
                 hipStream_t st, const float* u, float* md, int round_f16, int dy16_filled = 0) {
    CdPlan cp = conv_dma_dgrad_plan(g);
    const bool half = conv_dma_half(g);
    const void* dyin = dy;
    const void* win = w;
    if (half) {
        // dy: md is shared with the weight gradient; MG_TILES_MD_FILLED: the producer of dy wrote the copy (mg_instnorm_bwd_h)
        dyin = cd_stage16(dy, md, dy16_filled != 0, (size_t)g->B * g->OH * g->OW * g->Co, conv_dma_h_dy_bytes(g), wsp, st);
        win = cd_stage16(w, u, true, (size_t)g->Co * g->KH * g->KW * g->Ci, conv_dma_h_w_bytes(g), wsp, st);
        MG_CHECK_LAUNCH();
    }
    probe_begin(st);
    conv_dma_dgrad_launch(g, cp, dyin, win, bias, dx, act, (float*)wsp, st, round_f16);
    probe_end(st);
    MG_CHECK_LAUNCH();
    if (cp.splits > 1) {
        const size_t n = (size_t)g->B * g->H * g->W * g->Ci;
        splitk_epilogue(conv_grid(n / 4), (const float*)wsp, cp.splits, n, g->Ci, bias, act, dx, round_f16, st);
        MG_CHECK_LAUNCH();
    }
    return MG_OK;
}


// The 32-deep forward kernel needs dynamic LDS above the 64 KB static limit for its 128x128 tile.
inline bool fwd32_enabled() { static const bool off = getenv("MG_NO_BK32") != nullptr; return !off; }
template <int BM_, int BN_, int TAG_>
void launch_fwd32(dim3 grid, hipStream_t st, const Geom& gg, const float* x, const float* w, const float* bias, float* y,
                  int act, int cps32, float* part, const Batch& bt) {
    constexpr size_t lds = (size_t)2 * (BM_ + BN_) * LDK2 * sizeof(float);
    static bool once = false;
    if (!once) {
        hipFuncSetAttribute((const void*)conv_fwd32_kernel<BM_, BN_, TAG_>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
        once = true;
    }
    hipLaunchKernelGGL((conv_fwd32_kernel<BM_, BN_, TAG_>), grid, dim3(256), lds, st, gg, x, w, bias, y, act, cps32, part,
                       bt);
}
struct ColsumPlan { int splits; long long rows_per_split; };
ColsumPlan colsum_plan(long long M, int C) {
    if (M <= 256) return {1, M};                  // one launch: each block walks all rows of its 64 columns
    const int cb = (C + 63) / 64;
    long long splits = (1024 + cb - 1) / cb;
    if (splits > 256) splits = 256;
    if (splits > (M + 63) / 64) splits = (M + 63) / 64;
    if (splits < 1) splits = 1;
    long long rps = (M + splits - 1) / splits;
    splits = (M + rps - 1) / rps;
    return {(int)splits, rps};
}

// tile / split selection shared by the launchers and mg_conv_plan_name().  A pass needs >= ~2 workgroups per CU
// (256 CUs) to hide its own global-load latency behind other workgroups' MFMAs; deep-K, small-M*N layers (the
// 1024-channel 8x16 bottleneck: 64 tiles of 128x128) get there by splitting K across blockIdx.y.
struct TilePlan { int bm, bn, splits, cps; bool k32; };
// pass: 0 = forward-kernel GEMM (k-contiguous operands, may use the 32-deep kernel), 1 = data-gradient kernel
TilePlan gemm_plan(long long M, int N, int chunks, int classes, bool can_split, int pass) {
    // Cost model in units of one 32x32x2 MFMA (64 cycles): a workgroup's 4 waves own the CU's 4 SIMDs, so the
    // workgroups mapped to one CU serialise on the MFMA pipe; a lone workgroup per CU cannot hide its own staging;
    // split-K pays one extra pass over (splits + 1) output-sized slabs at ~4 TB/s.
    if (const char* f = getenv("MG_FORCE_PLAN")) {      // tuning harness: "bm,bn,splits"
        int bm = 0, bn = 0, sp = 1;
        if (sscanf(f, "%d,%d,%d", &bm, &bn, &sp) == 3 && sp >= 1) {
            if (!can_split || chunks / sp < 1) sp = 1;
            const int cps = (chunks + sp - 1) / sp;
            return {bm, bn, (chunks + cps - 1) / cps, cps, pass == 0};
        }
    }
    // Plans measured on MI355X for the layer shapes of BASELINE configs[1] at batch 8 (scripts/tune_conv.py sweeps
    // tile x split with MG_FORCE_PLAN and keeps the fastest); anything else falls through to the cost model.
    struct Tuned { int pass; long long M; int N, chunks, classes, bm, bn, sp, k32; };
    static const Tuned tuned[] = {
        {0, 256, 1024, 64, 16, 64, 64, 1, 1},      // Winograd forward GEMMs, 1024-channel 8x16 ResNet blocks
        {1, 256, 1024, 64, 16, 64, 64, 1, 0},      // Winograd data-gradient GEMMs (transposed pipeline: same 256 tiles)
        {1, 360, 1024, 64, 16, 128, 128, 2, 0},    // ... 360 tiles (measured for a since-removed padded-domain form; float16 keeps it)
        {0, 1024, 1024, 288, 1, 128, 128, 8, 1},   // 512->1024 stride-2 forward (and the 1024->512 ConvTranspose backward)
        {0, 4096, 512, 144, 1, 128, 128, 4, 1},    // 256->512
        {0, 16384, 256, 72, 1, 64, 64, 1, 1},      // 128->256
        {0, 65536, 128, 36, 1, 128, 128, 1, 1},    // 64->128
        {0, 4896, 512, 256, 1, 128, 128, 3, 1},    // D 256->512 4x4 s1 forward
        {0, 4488, 256, 128, 1, 64, 64, 6, 0},      // D 128->256 4x4 s2 forward
        {0, 17160, 128, 64, 1, 64, 64, 3, 1},      // D 64->128 4x4 s2 forward
        {1, 4488, 256, 512, 1, 64, 64, 8, 0},      // D 256->512 4x4 s1 data gradient
        {1, 1024, 512, 576, 4, 128, 64, 4, 0},     // stride-2 data gradients / ConvTranspose forwards (4 parity classes,
        {1, 4096, 256, 288, 4, 64, 64, 1, 0},      //  each splitting its own K range)
        {1, 16384, 128, 144, 4, 128, 64, 1, 0},
        {1, 65536, 64, 72, 4, 128, 64, 1, 0},
        {1, 4488, 128, 256, 4, 64, 64, 2, 0},
        {1, 17160, 64, 128, 4, 64, 64, 1, 0},
        {1, 1224, 128, 256, 4, 64, 64, 3, 0},      // second discriminator scale
        {1, 4488, 64, 128, 4, 64, 64, 3, 0},
        {1, 8976, 128, 256, 4, 64, 64, 1, 0},      // batch 16 (stacked discriminator-loss pass)
        {1, 34320, 64, 128, 4, 64, 64, 1, 0},
        {1, 2448, 128, 256, 4, 64, 64, 4, 0},
        {1, 8976, 64, 128, 4, 64, 64, 2, 0},
        // batch-64 inference (BASELINE configs[4]): forward only
        {0, 2048, 1024, 64, 16, 128, 128, 1, 1},   // F(2x2,3x3) forward GEMMs, 2048 tiles
        {0, 8192, 1024, 288, 1, 128, 128, 1, 1},   // 512->1024 stride-2 forward
        {0, 32768, 512, 144, 1, 128, 128, 1, 1},   // 256->512
        {0, 2448, 512, 16, 25, 64, 64, 1, 1},      // F(2x2,4x4) forward GEMMs of the 256->512 discriminator layer, batch 16
        // F(4x4,2x2) GEMMs of the stride-2 discriminator layers (K = 4 Ci): 128->256 at 17x33 out (720 tiles at batch 16,
        // 360 at batch 8), 64->128 at 33x65 out (2448 / 1224 tiles)
        {0, 720, 256, 32, 25, 64, 64, 1, 1},
        {0, 2448, 128, 16, 25, 128, 128, 1, 1},
        {1, 720, 512, 16, 25, 64, 64, 1, 0},
        {1, 360, 512, 16, 25, 64, 64, 1, 0},
        {1, 2448, 256, 8, 25, 64, 64, 1, 0},
        {1, 1224, 256, 8, 25, 128, 128, 1, 0},
        // configs[2] (LocalEnhancer) Winograd GEMMs: 2048-channel 4x8 trunk blocks (64 tiles), 128-channel 64x128 local blocks
        {0, 64, 2048, 128, 16, 64, 64, 4, 1},
        {1, 64, 2048, 128, 16, 64, 64, 1, 0},
        {0, 16384, 128, 8, 16, 64, 64, 1, 0},
        {1, 16384, 128, 8, 16, 128, 128, 1, 0},
        // second discriminator scale (64x128 input), batch 8
        {0, 1440, 512, 256, 1, 64, 64, 4, 1},
        {1, 1224, 256, 512, 1, 64, 64, 12, 0},
        {0, 1224, 256, 128, 1, 64, 64, 6, 1},
        {0, 4488, 128, 64, 1, 64, 64, 3, 1},
        // both scales at batch 16 (the stacked fake + real pass of the discriminator loss)
        {0, 9792, 512, 256, 1, 128, 128, 3, 1},
        {1, 8976, 256, 512, 1, 128, 128, 12, 0},
        {0, 8976, 256, 128, 1, 64, 64, 4, 1},
        {0, 34320, 128, 64, 1, 64, 64, 2, 1},
        {0, 2880, 512, 256, 1, 64, 64, 4, 1},
        {1, 2448, 256, 512, 1, 64, 64, 8, 0},
        {0, 2448, 256, 128, 1, 64, 64, 6, 1},
        {0, 8976, 128, 64, 1, 64, 64, 3, 1},
    };
    for (const Tuned& t : tuned)
        if (t.pass == pass && t.M == M && t.N == N && t.chunks == chunks && t.classes == classes &&
            (t.sp == 1 || can_split)) {
            const int cps = (chunks + t.sp - 1) / t.sp;
            return {t.bm, t.bn, (chunks + cps - 1) / cps, cps, t.k32 != 0};
        }
    struct Cand { int bm, bn; };
    const Cand cands[3] = {{128, 128}, {128, 64}, {64, 64}};
    const int split_opts[9] = {1, 2, 3, 4, 6, 8, 12, 16, 24};
    double best = 1e300;
    TilePlan out{64, 64, 1, chunks, false};
    for (const Cand& c : cands) {
        if (c.bm == 128 && c.bn == 128 && (N < 96 || M < 96)) continue;
        if (c.bm == 128 && c.bn == 64 && M < 96) continue;
        const long long tiles = ((M + c.bm - 1) / c.bm) * ((N + c.bn - 1) / c.bn) * classes;
        const double mfma = 8.0 * (c.bm / 64) * (c.bn / 64);
        for (int sp : split_opts) {
            if (sp > 1 && (!can_split || chunks / sp < 8)) break;
            const int cps = (chunks + sp - 1) / sp;
            const int spl = (chunks + cps - 1) / cps;
            const long long wgs = tiles * spl;
            const double work = cps * (mfma + 3.0) + 14.0;
            double t = (double)((wgs + 255) / 256) * work;
            if (wgs < 2 * 256) t *= 1.25;
            if (spl > 1) t += (double)(spl + 1) * (double)M * N * classes * 4.0 / 4e12 / 29e-9 * 256.0 / 256.0;
            // deep reductions measured faster on the 32-deep forward kernel wherever it was tried (>= 144 chunks)
            if (t < best) { best = t; out = {c.bm, c.bn, spl, cps, pass == 0 && chunks >= 128}; }
        }
    }
    return out;
}
// the 32-deep forward kernel takes whole 32-channel chunks and, when K is split, an even number of 16-deep chunks per split
inline bool k32_fits(int Ci, int splits, int cps) { return fwd32_enabled() && Ci % BK2 == 0 && (splits == 1 || cps % 2 == 0); }
// float32: where the plan asks for it; float16: whenever the shape allows it (its stage / fragment traffic is what the f16 loop
// is made of)
inline bool use_k32(const TilePlan& tp, int Ci) { return tp.k32 && k32_fits(Ci, tp.splits, tp.cps); }
template <typename Plan>
inline void one_split(Plan& p, int cps) {      // no K split (workspace or an alignment is missing): one split walks every chunk
    p.splits = 1;
    p.cps = cps;
}
TilePlan fwd_plan(const mg_conv_geom* g) {
    const long long M = (long long)g->B * g->OH * g->OW;
    const bool vec = g->Ci % BK == 0;
    const int chunks = vec ? g->KH * g->KW * (g->Ci / BK) : (g->KH * g->KW * g->Ci + BK - 1) / BK;
    return gemm_plan(M, g->Co, chunks, 1, g->Co % 4 == 0, 0);
}
TilePlan dgrad_plan(const mg_conv_geom* g) {
    const int s = g->stride;
    const long long Mc = (long long)g->B * ((g->H + s - 1) / s) * ((g->W + s - 1) / s);
    const bool vec = g->Co % BK == 0;
    const int chunks = vec ? g->KH * g->KW * (g->Co / BK) : (g->KH * g->KW * g->Co + BK - 1) / BK;
    return gemm_plan(Mc, g->Ci, chunks, s * s, g->Ci % 4 == 0, 1);
}

struct WgradPlan { bool big; int tiles; int splits; int cps; };
WgradPlan wgrad_plan(const mg_conv_geom* g) {
    const int R = g->Co, N = g->KH * g->KW * g->Ci;
    const long long Mtot = (long long)g->B * g->OH * g->OW;
    const int chunks = (int)((Mtot + BK - 1) / BK);
    const int t128 = ((R + 127) / 128) * ((N + 127) / 128);
    bool big = t128 >= 96 && R >= 128;
    int want = -1;
    if (const char* f = getenv("MG_FORCE_WGRAD")) {      // tuning harness: "big(0|1),splits"
        int b = 0, sp = 1;
        if (sscanf(f, "%d,%d", &b, &sp) == 2 && sp >= 1) { big = b != 0 && R >= 64; want = sp; }
    } else {
        // measured on MI355X (scripts/tune_conv.py --wgrad) for the configs[1] layers; the heuristic below covers the rest
        struct Tuned { int R, N; long long M; int big, sp; };
        static const Tuned tuned[] = {
#include "wgrad_plans.inc"
        };
        for (const Tuned& t : tuned)
            if (t.R == R && t.N == N && t.M == Mtot) { big = t.big != 0; want = t.sp; break; }
    }
    const int tiles = big ? t128 : ((R + 63) / 64) * ((N + 63) / 64);
    int splits = want > 0 ? want : (tiles >= 512 ? 1 : (768 + tiles - 1) / tiles);
    const int max_splits = chunks / 8 > 0 ? chunks / 8 : 1;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    int cps = (chunks + splits - 1) / splits;
    splits = (chunks + cps - 1) / cps;
    return {big, tiles, splits, cps};
}

// ---------------------------------------------------------------------------------------------------------
// The pick: the one instance of the generic implicit GEMM a pass launches -- conv_fwd_kernel<bm, bn, veca, tag> /
// conv_fwd32_kernel<bm, bn, tag> (k32), conv_dgrad_kernel / conv_wgrad_kernel<bm, bn, veca, vecb, tag> -- and its K split.
// A launcher fills it from the geometry and what its buffers allow and dispatches on it; mg_conv_plan_name fills it with
// everything allowed and prints it.  Neither holds a condition of its own.
// ---------------------------------------------------------------------------------------------------------
struct GemmPick { int bm, bn; bool veca, vecb; int tag; bool k32; int splits, cps; };
// What the entry point's buffers allow.  veca / vecb: the A / B operand (forward: both) is 16-byte aligned, so float4 loads may
// read it; split: a workspace of the queried size is there and it, the output and the bias are 16-byte aligned (the combine
// kernels read and write float4s)
struct BufFacts { bool veca, vecb, split; };
constexpr BufFacts kAnyBuf{true, true, true};
inline int conv_tag(const mg_conv_geom* g) { return MG_PRECISION_IS_HALF(g->precision) ? 2 : 0; }
GemmPick fwd_pick(const mg_conv_geom* g, BufFacts f) {
    TilePlan tp = fwd_plan(g);
    if (tp.splits > 1 && !f.split) one_split(tp, 1 << 30);
    const bool vec = g->Ci % BK == 0 && f.veca && f.vecb;
    const bool k32 = vec && (conv_tag(g) ? k32_fits(g->Ci, tp.splits, tp.cps) : use_k32(tp, g->Ci));
    return {tp.bm, tp.bn, vec, vec, conv_tag(g), k32, tp.splits, tp.cps};
}
GemmPick dgrad_pick(const mg_conv_geom* g, BufFacts f) {
    TilePlan tp = dgrad_plan(g);
    if (tp.splits > 1 && !f.split) one_split(tp, 1 << 30);
    return {tp.bm, tp.bn, g->Co % BK == 0 && f.veca, g->Ci % 4 == 0 && f.vecb, conv_tag(g), false, tp.splits, tp.cps};
}
GemmPick wgrad_pick(const mg_conv_geom* g, BufFacts f) {
    WgradPlan p = wgrad_plan(g);
    if (p.splits > 1 && !f.split) one_split(p, 1 << 30);
    const int t = p.big ? 128 : 64;
    return {t, t, g->Co % 4 == 0 && f.veca, g->Ci % 4 == 0 && f.vecb, conv_tag(g), false, p.splits, p.cps};
}
void gemm_pick_name(int pass, const GemmPick& p, char* out, int out_len) {
    const char* va = p.veca ? "true" : "false";
    const char* vb = p.vecb ? "true" : "false";
    if (pass == 0 && p.k32) snprintf(out, out_len, "conv_fwd32_kernel<%d, %d, %d>", p.bm, p.bn, p.tag);
    else if (pass == 0) snprintf(out, out_len, "conv_fwd_kernel<%d, %d, %s, %d>", p.bm, p.bn, va, p.tag);
    else snprintf(out, out_len, pass == 1 ? "conv_dgrad_kernel<%d, %d, %s, %s, %d>" : "conv_wgrad_kernel<%d, %d, %s, %s, %d>", p.bm,
                  p.bn, va, vb, p.tag);
}

// Dispatch of a pick's run-time values onto template arguments: each calls f with std::integral_constant / std::bool_constant
// values, so nesting them instantiates exactly the product of their alternatives.
template <typename F>
void dispatch_tile(int bm, int bn, F&& f) {      // 128x128, 64x64, 128x64
    if (bm == 128 && bn == 128) f(std::integral_constant<int, 128>{}, std::integral_constant<int, 128>{});
    else if (bm == 64) f(std::integral_constant<int, 64>{}, std::integral_constant<int, 64>{});
    else f(std::integral_constant<int, 128>{}, std::integral_constant<int, 64>{});
}
template <typename F>
void dispatch_bool(bool v, F&& f) {
    if (v) f(std::true_type{});
    else f(std::false_type{});
}
template <typename F>
void dispatch_tag(int tag, F&& f) {      // the convolutions' own tags: 0 float32, 2 float16
    if (tag == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 0>{});
}
template <typename F>
void dispatch_wino_tag(int tag, F&& f) {      // the Winograd-domain GEMMs' tags: 1 F(2x2,3x3), 3 float16, 5 the 25-position families
    if (tag == 1) f(std::integral_constant<int, 1>{});
    else if (tag == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 5>{});
}
// The weight gradient's reduce runs one block more than conv_grid unless capped.  splitk_reduce_kernel walks grid strides, so
// the extra block finds nothing to do -- except for a dw of fewer than 4 elements (n / 4 == 0), where it IS block 0, the one
// that sums the scalar tail, and the grid would otherwise be empty.
inline unsigned wgrad_reduce_grid(size_t n4) { return (n4 + 255) / 256 > 4096 ? 4096u : (unsigned)((n4 + 255) / 256 + 1); }

// ---------------------------------------------------------------------------------------------------------
// Kernel families.  conv_route() (after the family predicates, below) names the one a pass of a layer takes; the launchers,
// the workspace sizes, the shared images and mg_conv_plan_* all switch on it.  A pass whose buffers do not suit its family
// (alignment, workspace size, a bias / activation that data gradient cannot fuse) takes the generic tail instead --
// conv_route(pass, g, true): DMA (over the reflect-padded domain for a data gradient), else the implicit GEMM -- and a co1
// pass tries rowdot first.
// ---------------------------------------------------------------------------------------------------------
enum ConvRoute { R_IGEMM, R_DMA, R_DMA_REFLECT, R_CO1, R_ROWDOT, R_H16, R_WINO, R_WINO4, R_WINO42, R_WINO43, R_WINOH, R_SMALLC };
ConvRoute conv_route(int pass, const mg_conv_geom* g, bool generic = false);

}  // namespace
