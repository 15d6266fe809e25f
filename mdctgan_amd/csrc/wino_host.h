// Winograd orchestration on the host: the family predicates, WinoGeo, the GEMM-stage plan, the workspace layout, wino_gemm, the
// transforms and the three pipelines wino_fwd / wino_dgrad / wino_wgrad.
// Needs: conv_plan.h (plans, dispatchers, ConvRoute, h16_ok), wino.h, wino4.h, wino42.h, wino43.h, wino_h16.h.
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------------------
// Winograd orchestration: F(2x2,3x3) (wino.h), F(2x2,4x4) for the stride-1 4x4 PatchGAN layers (wino4.h) and F(4x4,2x2)
// over the space-to-depth view for the stride-2 ones (wino42.h), and the opt-in forward-only F(4x4,3x3) of an inference pass
// (wino43.h).  Every pass is one pipeline: transforms into the Winograd
// domain, the P position GEMMs as one batched launch, the transform back.
// ---------------------------------------------------------------------------------------------------------
bool h16_ok(const mg_conv_geom* g);
// MG_PRECISION_F32_WINO43 geometries (forward passes under no_grad, opted in): the weight-heavy GEMM-bound layers, where the
// 36-position GEMMs issue 1.78x fewer FLOPs than F(2x2,3x3)'s 16.  min_c is read per call so the parity tests reach small shapes.
// Disjoint from every other family's predicate by being asked first (conv_route); an ineligible geometry of this precision
// routes as MG_PRECISION_F32 does.
bool wino43_ok(const mg_conv_geom* g) {
    if (g->precision != MG_PRECISION_F32_WINO43) return false;
    const char* mc = getenv("MG_WINO43_MIN_C");
    const int min_c = mc ? atoi(mc) : 256;
    return g->KH == 3 && g->KW == 3 && g->stride == 1 && g->pad == 1 && g->H % 4 == 0 && g->W % 4 == 0 && g->Ci % 16 == 0 &&
           g->Co % 16 == 0 && g->Ci >= min_c && g->Co >= min_c;
}
// MG_PRECISION_F16_INFER geometries (forward passes under no_grad, opted in) that run F(2x2,3x3) on two-byte images (wino_h16.h):
// the float16 Winograd branch's own channel and tile thresholds (below; read per call here so the parity tests reach small
// shapes), whole 64-deep chunks and 64-column tiles, and every operand of one position below 2 GiB (32-bit DMA byte offsets).
// Asked first by conv_route, as wino43_ok is; an ineligible geometry of this precision routes as MG_PRECISION_F16 does.
bool winoh_ok(const mg_conv_geom* g) {
    if (g->precision != MG_PRECISION_F16_INFER) return false;
    if (g->KH != 3 || g->KW != 3 || g->stride != 1 || g->pad != 1 || g->H % 2 || g->W % 2 || g->H < 2 || g->W < 2) return false;
    if (g->Ci % 64 != 0 || g->Co % 64 != 0) return false;
    const char* mc = getenv("MG_INFER_F16_MIN_C");
    const char* mt = getenv("MG_INFER_F16_MIN_TILES");
    // the weight-streaming layers of small batches keep the hgemm_sa path (conv_h16.h) -- unless the caller names a tile threshold
    // of its own, which then is the whole rule about the tile count
    if (!mt && h16_ok(g)) return false;
    const int min_c = mc ? atoi(mc) : 256;
    const long long min_tiles = mt ? atoll(mt) : 256, T = (long long)g->B * (g->H / 2) * (g->W / 2);
    if (g->Ci < min_c || g->Co < min_c || T < min_tiles) return false;
    const long long lim = 1LL << 31;
    return T * g->Ci * 2 < lim && (long long)g->Co * g->Ci * 2 < lim && T * g->Co * 4 < lim;
}
bool wino_ok(const mg_conv_geom* g) {
    static const bool off = getenv("MG_NO_WINOGRAD") != nullptr;
    if (h16_ok(g)) return false;             // weight-dominated autocast layers take the float16 GEMM path (conv_h16.h)
    // f16 GEMMs are fast enough that Winograd only pays where the 16 transformed-weight matrices are amortised over
    // many tiles: wide layers (>= 256 channels) with >= 256 tiles (the 1024-channel 8x16 blocks of configs[1]; not the
    // 2048-channel 4x8 trunk of configs[2], where reading 16 * Co * Ci transformed weights would dominate)
    constexpr int min_tiles_h = 256;       // (64 measured slower on configs[2])
    if (prec_h(g) && (g->Ci < 256 || g->Co < 256 || (long long)g->B * (g->H / 2) * (g->W / 2) < min_tiles_h)) return false;
    return !off && g->KH == 3 && g->KW == 3 && g->stride == 1 && g->pad == 1 && g->Ci % 16 == 0 && g->Co % 16 == 0 &&
           g->Ci >= 32 && g->Co >= 32 && g->H % 2 == 0 && g->W % 2 == 0 && g->H >= 2 && g->W >= 2;
}
bool wino4_ok(const mg_conv_geom* g) {
    static const bool off = getenv("MG_NO_WINOGRAD4") != nullptr;
    constexpr int min_c = 32;
    return !off && !prec_h(g) && g->KH == 4 && g->KW == 4 && g->stride == 1 && g->pad == 2 && !g->reflect &&
           g->Ci % 16 == 0 && g->Co % 16 == 0 && g->Ci >= min_c && g->Co >= min_c && (g->H & 1) && (g->W & 1);
}
bool wino42_ok(const mg_conv_geom* g) {
    static const bool off = getenv("MG_NO_WINOGRAD42") != nullptr;
    constexpr int min_c = 16;
    if (off || prec_h(g) || g->KH != 4 || g->KW != 4 || g->stride != 2 || g->pad != 2 || g->reflect || g->Ci % 16 ||
        g->Co % 16 || g->Ci < min_c || g->Co < min_c || g->H < 2 || g->W < 2)
        return false;
    // the transforms move 25/16 of the phase-channel data per pass: measured faster than the direct kernels from
    // T * 4Ci * Co ~ 4e7 up (batch 16: 64->128 at 33x65 out 124 -> 91 us, 128->256 at 17x33 out 136 -> 97 us forward),
    // slower below (64->128 at 17x33 out: 39 -> 48 us).  Read per call so the parity tests can exercise small shapes.
    const char* mw = getenv("MG_WINO42_MIN_WORK");
    const double min_work = mw ? atof(mw) : 4e7;
    const double T = (double)g->B * ((g->OH + 3) / 4) * ((g->OW + 3) / 4);
    return T * 4.0 * g->Ci * g->Co >= min_work;
}

// Per family: positions P, channels per thread of the transform kernels (their grid divisor), and the weight-gradient plan's
// tile count above which it takes 128x128 tiles, and whether a full grid still splits a deep reduction in three
struct WinoFamily { int P, vec; long long big_T; bool split3; };
constexpr WinoFamily kWinoFamily[5] = {
    {16, 4, 1024, false},      // F(2x2,3x3); short reductions (the 8x16 blocks of configs[1]): 64x64 tiles measured 125 vs 148 us
    {25, 2, 4096, true},       // F(2x2,4x4); measured at 2448 tiles: 64x64 232 us, 128x128 252 us
    {25, 2, 4096, true},       // F(4x4,2x2)
    {36, 2, 4096, true},       // F(4x4,3x3): forward only, the weight-gradient fields are never read
    {16, 4, 1024, false},      // F(2x2,3x3) on float16 images: forward only
};
// A layer in the Winograd domain: T = B * TH * TW tiles, Kc = the GEMMs' input depth (4 Ci for F(4x4,2x2))
struct WinoGeo { ConvRoute r; WinoFamily f; long long T; int TH, TW, Kc; bool hp; };
WinoGeo wino_geo(ConvRoute r, const mg_conv_geom* g) {
    WinoGeo w{r, kWinoFamily[r - R_WINO], 0, 0, 0, r == R_WINO42 ? 4 * g->Ci : g->Ci, prec_h(g)};
    if (r == R_WINO || r == R_WINOH) { w.TH = g->H / 2; w.TW = g->W / 2; }
    else if (r == R_WINO4) { w.TH = (g->H + 1) / 2; w.TW = (g->W + 1) / 2; }
    else if (r == R_WINO43) { w.TH = g->H / 4; w.TW = g->W / 4; }
    else { w.TH = (g->OH + 3) / 4; w.TW = (g->OW + 3) / 4; }
    w.T = (long long)g->B * w.TH * w.TW;
    return w;
}
inline size_t al256(size_t n) { return (n + 63) / 64 * 64; }   // in floats

// The GEMM stage of a pass (dense_dims): dense_gemm.h where dense_plan takes the shape, else the convolution kernels (TAG 1;
// 3 = float16; 5 = the 25- and 36-position families) on tile plan tp (forward: k32 = the 32-deep kernel).  The one plan that the
// launch, the workspace (split-K slabs of either path) and mg_conv_plan_name use.
struct WinoGemm { DensePlan dp; TilePlan tp; int tag; };
WinoGemm wino_gemm_plan(const WinoGeo& w, int pass, const mg_conv_geom* g) {
    WinoGemm s{dense_plan(pass, w.f.P, w.T, g->Co, w.Kc, w.hp), {}, w.hp ? 3 : w.f.P == 16 ? 1 : 5};
    if (pass == 0) {
        s.tp = gemm_plan(w.T, g->Co, w.Kc / BK, w.f.P, true, 0);
        s.tp.k32 = w.hp ? k32_fits(w.Kc, s.tp.splits, s.tp.cps) : use_k32(s.tp, w.Kc);
    } else if (pass == 1) {
        s.tp = gemm_plan(w.T, w.Kc, g->Co / BK, w.f.P, true, 1);
    } else {        // dU [Co][Kc] on 64x64 or 128x128 tiles, the tiles' reduction split over blockIdx.z
        const int chunks = (int)((w.T + BK - 1) / BK);
        const int t = g->Co >= 128 && w.Kc >= 128 && w.T > w.f.big_T ? 128 : 64;
        const int wgs = ((g->Co + t - 1) / t) * ((w.Kc + t - 1) / t) * w.f.P;
        int splits = wgs >= 512 ? (w.f.split3 && chunks >= 128 ? 3 : 1) : (768 + wgs - 1) / wgs;
        const int max_splits = chunks / 8 > 0 ? chunks / 8 : 1;
        if (splits > max_splits) splits = max_splits;
        const int cps = (chunks + splits - 1) / splits;
        s.tp = {t, t, (chunks + cps - 1) / cps, cps, false};
    }
    return s;
}

// Workspace of a pass (float offsets, 256-byte aligned): forward U | V | Mx | slabs, data gradient U | Md | dV | dd | slabs,
// weight gradient V | Md | dU | slabs | the bias gradient's column sums
struct WinoWs { size_t u, v, md, mx, dv, dd, du, part, cs, bytes; };
WinoWs wino_ws(const WinoGeo& w, const WinoGemm& s, int pass, const mg_conv_geom* g) {
    const size_t P = w.f.P, nu = al256(P * g->Co * w.Kc), nv = al256(P * w.T * w.Kc), nm = al256(P * w.T * g->Co);
    const size_t slabs = slab_count(s.tp.splits, s.dp.ok ? s.dp.splits : 0);
    WinoWs o{};
    size_t at = 0;
    auto take = [&](size_t& off, size_t n) { off = at; at += n; };
    if (pass == 0) {
        take(o.u, nu); take(o.v, nv); take(o.mx, nm); take(o.part, al256(slabs * P * w.T * g->Co));
    } else if (pass == 1) {
        take(o.u, nu); take(o.md, nm); take(o.dv, nv); take(o.dd, nv); take(o.part, al256(slabs * P * w.T * w.Kc));
    } else {
        take(o.v, nv); take(o.md, nm); take(o.du, nu); take(o.part, al256(slabs * P * g->Co * w.Kc));
        take(o.cs, al256((mg_colsum_workspace((long long)g->B * g->OH * g->OW, g->Co) + 255) / 4));
    }
    o.bytes = at * sizeof(float) + 256;
    return o;
}
size_t wino_ws_bytes(ConvRoute r, int pass, const mg_conv_geom* g) {
    const WinoGeo w = wino_geo(r, g);
    return wino_ws(w, wino_gemm_plan(w, pass, g), pass, g).bytes;
}

// pass 0: Mx = V U^T (a = V, b = U); 1: dV = Md U (a = Md, b = U); 2: dU = Md^T V (a = Md, b = V).  part: split-K slabs.
void wino_gemm(const WinoGeo& w, const WinoGemm& s, int pass, const mg_conv_geom* g, const float* a, const float* b, float* c,
               float* part, hipStream_t st) {
    const int P = w.f.P, Co = g->Co, Kc = w.Kc;
    const long long T = w.T;
    if (s.dp.ok) {
        dense_wino_gemm(s.dp, pass, P, T, Co, Kc, a, b, c, part, st);
        return;
    }
    const TilePlan& tp = s.tp;
    const Geom gg{1, 1, (int)T, Kc, 1, (int)T, Co, 1, 1, 1, 0, 0};
    float* pp = tp.splits > 1 ? part : nullptr;
    auto launch = [&](auto tag) {
        constexpr int TAG = decltype(tag)::value;
        dispatch_tile(tp.bm, tp.bn, [&](auto bm, auto bn) {
            constexpr int BM_ = decltype(bm)::value, BN_ = decltype(bn)::value;
            if (pass == 2) {      // wino_gemm_plan gives pass 2 tp.bm == tp.bn in {64, 128} only: the square tiles, as in mg_conv_wgrad
                if constexpr (BM_ == BN_) {
                    const dim3 grid((unsigned)(((Co + BM_ - 1) / BM_) * ((Kc + BN_ - 1) / BN_)), P, tp.splits);
                    hipLaunchKernelGGL((conv_wgrad_kernel<BM_, BN_, true, true, TAG>), grid, dim3(256), 0, st, gg, b, a, pp ? pp : c, tp.cps, 0,
                                       Batch{T * Kc, T * Co, (long long)Co * Kc, 0});
                }
                return;
            }
            const dim3 grid((unsigned)(((T + BM_ - 1) / BM_) * (((pass == 0 ? Co : Kc) + BN_ - 1) / BN_)), tp.splits, P);
            if (pass == 1)          // dV_z = dM_z U_z: same position, no flip
                hipLaunchKernelGGL((conv_dgrad_kernel<BM_, BN_, true, true, TAG>), grid, dim3(256), 0, st, gg, a, b, (const float*)nullptr,
                                   c, MG_ACT_NONE, tp.cps, pp, Batch{T * Co, (long long)Co * Kc, T * Kc, 0});
            else if (tp.k32)
                launch_fwd32<BM_, BN_, TAG>(grid, st, gg, a, b, nullptr, c, MG_ACT_NONE, tp.splits == 1 ? (1 << 29) : tp.cps / 2, pp,
                                            Batch{T * Kc, (long long)Co * Kc, T * Co, 0});
            else
                hipLaunchKernelGGL((conv_fwd_kernel<BM_, BN_, true, TAG>), grid, dim3(256), 0, st, gg, a, b, (const float*)nullptr, c,
                                   MG_ACT_NONE, tp.cps, pp, Batch{T * Kc, (long long)Co * Kc, T * Co, 0});
        });
    };
    probe_begin(st);
    dispatch_wino_tag(s.tag, launch);
    probe_end(st);
    if (!pp) return;
    if (pass == 2) {
        const size_t n = (size_t)P * Co * Kc;
        splitk_reduce(wino_grid(n / 4), pp, tp.splits, n, c, 0, st);
    } else {
        const int N = pass == 0 ? Co : Kc;
        const size_t n = (size_t)P * T * N;
        splitk_epilogue(wino_grid(n / 4), pp, tp.splits, n, N, nullptr, MG_ACT_NONE, c, 0, st);
    }
}

// The family's transforms into the Winograd domain: U = G w G^T, V = B^T x B, Md = A dy A^T
void wino_xform_u(const WinoGeo& w, const mg_conv_geom* g, const float* wt, float* U, hipStream_t st) {
    const dim3 grid(wino_grid((size_t)g->Co * w.Kc / w.f.vec));
    if (w.r == R_WINO) hipLaunchKernelGGL(wino_weight_xform_kernel, grid, dim3(256), 0, st, wt, g->Co, g->Ci, U);
    else if (w.r == R_WINO4) hipLaunchKernelGGL(wino4_weight_xform_kernel, grid, dim3(256), 0, st, wt, g->Co, g->Ci, U);
    else if (w.r == R_WINO43) hipLaunchKernelGGL(wino43_weight_xform_kernel, grid, dim3(256), 0, st, wt, g->Co, g->Ci, U);
    else hipLaunchKernelGGL(wino42_weight_xform_kernel, grid, dim3(256), 0, st, wt, g->Co, g->Ci, U);
}
void wino_xform_v(const WinoGeo& w, const mg_conv_geom* g, const float* x, float* V, hipStream_t st) {
    const dim3 grid(wino_grid((size_t)w.T * w.Kc / w.f.vec));
    if (w.r == R_WINO)
        hipLaunchKernelGGL(wino_input_xform_kernel, grid, dim3(256), 0, st, x, g->B, g->H, g->W, g->Ci, w.TH, w.TW, 1, g->reflect, V);
    else if (w.r == R_WINO4)
        hipLaunchKernelGGL(wino4_input_xform_kernel, grid, dim3(256), 0, st, x, g->B, g->H, g->W, g->Ci, w.TH, w.TW, V);
    else if (w.r == R_WINO43)
        hipLaunchKernelGGL(wino43_input_xform_kernel, grid, dim3(256), 0, st, x, g->B, g->H, g->W, g->Ci, w.TH, w.TW, g->reflect, V);
    else
        hipLaunchKernelGGL(wino42_input_xform_kernel, grid, dim3(256), 0, st, x, g->B, g->H, g->W, g->Ci, w.TH, w.TW, V);
}
void wino_xform_md(const WinoGeo& w, const mg_conv_geom* g, const float* dy, float* Md, hipStream_t st) {
    const dim3 grid(wino_grid((size_t)w.T * g->Co / w.f.vec));
    if (w.r == R_WINO) hipLaunchKernelGGL(wino_dy_xform_kernel, grid, dim3(256), 0, st, dy, g->B, w.TH, w.TW, g->Co, Md);
    else if (w.r == R_WINO4) hipLaunchKernelGGL(wino4_dy_xform_kernel, grid, dim3(256), 0, st, dy, g->B, w.TH, w.TW, g->Co, Md);
    else hipLaunchKernelGGL(wino42_dy_xform_kernel, grid, dim3(256), 0, st, dy, g->B, g->OH, g->OW, w.TH, w.TW, g->Co, Md);
}

// u_pre: the caller's U (mg_conv_wino_prepare); v_keep: the caller keeps V for the weight gradient; v_filled: x's producer
// wrote V already (mg_conv_fwd_instnorm_next of the layer in front).  nrm (F(2x2,3x3) and F(4x4,3x3), float32): output transform
// + InstanceNorm in one kernel (y = the raw convolution output, nrm->y the normalised one).
int wino_fwd(const WinoGeo& w, const mg_conv_geom* g, const float* x, const float* wt, const float* bias, float* y, int act,
             float* ws, hipStream_t st, const float* u_pre, float* v_keep, bool v_filled, const WinoNorm* nrm = nullptr) {
    const WinoGemm s = wino_gemm_plan(w, 0, g);
    const WinoWs o = wino_ws(w, s, 0, g);
    float* U = u_pre ? const_cast<float*>(u_pre) : ws + o.u;
    float* V = v_keep ? v_keep : ws + o.v;
    float* Mx = ws + o.mx;
    if (!u_pre) wino_xform_u(w, g, wt, U, st);
    if (!(v_filled && v_keep)) wino_xform_v(w, g, x, V, st);
    wino_gemm(w, s, 0, g, V, U, Mx, ws + o.part, st);
    if (nrm && w.r == R_WINO43) {       // (callers ask wino43_out_norm_ok first: <= 40 tiles, NT <= 3)
        const dim3 grid(g->Co / 32, g->B);
        const int nt = (w.TH * w.TW + 15) / 16;
        auto go = [&](auto kern, size_t lds) {
            if (lds) hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wino43_plane_bytes(1, W43_NORM_TILES));
            hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, (const float*)Mx, g->B, w.TH, w.TW, g->Co, bias, *nrm, y);
        };
        const size_t plane = wino43_plane_bytes(w.TH, w.TW);
        if (nt > 3) return MG_ERR_ARG;
        if (nrm->v_next) {
            if (nt == 1) go(wino43_out_norm_kernel<1, true>, plane); else if (nt == 2) go(wino43_out_norm_kernel<2, true>, plane); else go(wino43_out_norm_kernel<3, true>, plane);
        } else {
            if (nt == 1) go(wino43_out_norm_kernel<1>, 0); else if (nt == 2) go(wino43_out_norm_kernel<2>, 0); else go(wino43_out_norm_kernel<3>, 0);
        }
        MG_CHECK_LAUNCH();
        return MG_OK;
    }
    if (nrm) {
        const dim3 grid(g->Co / 32, g->B);
        const int nt = (w.TH * w.TW + 31) / 32;
#define MG_OUT_NORM(NT_) hipLaunchKernelGGL(wino_out_norm_kernel<NT_>, grid, dim3(256), 0, st, (const float*)Mx, g->B, w.TH, w.TW, g->Co, bias, *nrm, y)
#define MG_OUT_NORM_NEXT(NT_) hipLaunchKernelGGL((wino_out_norm_kernel<NT_, true>), grid, dim3(256), 0, st, (const float*)Mx, g->B, w.TH, w.TW, g->Co, bias, *nrm, y)
        if (nrm->v_next && nt == 1) MG_OUT_NORM_NEXT(1);
        else if (nrm->v_next && nt == 2) MG_OUT_NORM_NEXT(2);
        else if (nrm->v_next) return MG_ERR_ARG;       // (callers ask mg_conv_wino_vnext_ok first)
        else if (nt == 1) MG_OUT_NORM(1); else if (nt == 2) MG_OUT_NORM(2); else if (nt == 3) MG_OUT_NORM(3); else if (nt == 4) MG_OUT_NORM(4); else MG_OUT_NORM(5);
#undef MG_OUT_NORM_NEXT
#undef MG_OUT_NORM
        MG_CHECK_LAUNCH();
        return MG_OK;
    }
    const dim3 grid(wino_grid((size_t)w.T * g->Co / w.f.vec));
    if (w.r == R_WINO)
        hipLaunchKernelGGL(wino_output_xform_kernel, grid, dim3(256), 0, st, (const float*)Mx, g->B, w.TH, w.TW, g->Co, bias, act, y,
                           (int)w.hp);
    else if (w.r == R_WINO4)
        hipLaunchKernelGGL(wino4_output_xform_kernel, grid, dim3(256), 0, st, (const float*)Mx, g->B, w.TH, w.TW, g->Co, bias, act, y);
    else if (w.r == R_WINO43)
        hipLaunchKernelGGL(wino43_output_xform_kernel, grid, dim3(256), 0, st, (const float*)Mx, g->B, w.TH, w.TW, g->Co, bias, act, y);
    else
        hipLaunchKernelGGL(wino42_output_xform_kernel, grid, dim3(256), 0, st, (const float*)Mx, g->B, g->OH, g->OW, w.TH, w.TW, g->Co,
                           bias, act, y);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

// The forward pass on float16 images (wino_h16.h).  Workspace: U16 | V16 | M (float32), each 256-byte aligned.  u_pre / v_keep /
// v_filled as in wino_fwd, the images being halves; nrm (maps of <= 160 tiles per sample; its v_next: <= 64): the fused tail.
struct WinohWs { size_t u, v, mx, bytes; };
inline WinohWs winoh_ws(const WinoGeo& w, const mg_conv_geom* g) {
    auto al = [](size_t n) { return (n + 255) / 256 * 256; };
    WinohWs o{};
    o.u = 0;
    o.v = o.u + al((size_t)16 * g->Co * g->Ci * 2);
    o.mx = o.v + al((size_t)16 * w.T * g->Ci * 2);
    o.bytes = o.mx + al((size_t)16 * w.T * g->Co * 4) + 256;
    return o;
}
void winoh_xform_u(const mg_conv_geom* g, const float* wt, _Float16* U, hipStream_t st) {
    hipLaunchKernelGGL(winoh_weight_xform_kernel, dim3(wino_grid((size_t)g->Co * g->Ci / 4)), dim3(256), 0, st, wt, g->Co, g->Ci, U);
}
int winoh_fwd(const WinoGeo& w, const mg_conv_geom* g, const float* x, const float* wt, const float* bias, float* y, int act,
              char* ws, hipStream_t st, const void* u_pre, void* v_keep, bool v_filled, const WinohNorm* nrm = nullptr) {
    const WinohWs o = winoh_ws(w, g);
    _Float16* U = u_pre ? (_Float16*)const_cast<void*>(u_pre) : (_Float16*)(ws + o.u);
    _Float16* V = v_keep ? (_Float16*)v_keep : (_Float16*)(ws + o.v);
    float* Mx = (float*)(ws + o.mx);
    if (!u_pre) winoh_xform_u(g, wt, U, st);
    if (!(v_filled && v_keep))
        hipLaunchKernelGGL(winoh_input_xform_kernel, dim3(wino_grid((size_t)w.T * g->Ci / 4)), dim3(256), 0, st, x, g->B, g->H, g->W,
                           g->Ci, w.TH, w.TW, g->reflect, V);
    probe_begin(st);
    winoh_gemm_launch(V, U, Mx, w.T, g->Co, g->Ci, st);
    probe_end(st);
    if (nrm) {
        const dim3 grid(g->Co / 32, g->B);
        const int nt = (w.TH * w.TW + 31) / 32;
#define MG_OUT_NORM(NT_) hipLaunchKernelGGL(winoh_out_norm_kernel<NT_>, grid, dim3(256), 0, st, (const float*)Mx, g->B, w.TH, w.TW, g->Co, bias, *nrm, y)
#define MG_OUT_NORM_NEXT(NT_) hipLaunchKernelGGL((winoh_out_norm_kernel<NT_, true>), grid, dim3(256), 0, st, (const float*)Mx, g->B, w.TH, w.TW, g->Co, bias, *nrm, y)
        if (nrm->v_next && nt == 1) MG_OUT_NORM_NEXT(1);
        else if (nrm->v_next && nt == 2) MG_OUT_NORM_NEXT(2);
        else if (nrm->v_next || nt > 5) return MG_ERR_ARG;       // (callers ask winoh_norm_ok / mg_conv_wino_vnext_ok first)
        else if (nt == 1) MG_OUT_NORM(1); else if (nt == 2) MG_OUT_NORM(2); else if (nt == 3) MG_OUT_NORM(3); else if (nt == 4) MG_OUT_NORM(4); else MG_OUT_NORM(5);
#undef MG_OUT_NORM_NEXT
#undef MG_OUT_NORM
        MG_CHECK_LAUNCH();
        return MG_OK;
    }
    hipLaunchKernelGGL(wino_output_xform_kernel, dim3(wino_grid((size_t)w.T * g->Co / 4)), dim3(256), 0, st, (const float*)Mx, g->B,
                       w.TH, w.TW, g->Co, bias, act, y, 1);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

// Data gradient as the transpose of the forward pipeline (T tiles, no padded domain).  md_keep: the caller keeps Md for the
// weight gradient; dy == nullptr (F(2x2,3x3)): md_keep already holds it (mg_instnorm_bwd_wino_md).  bias / act: F(2x2,3x3)
// only.  addend (in / out): a tensor to add to dx (mg_wino_tiles.add); the one-kernel gather of small maps takes it and
// clears *addend.
int wino_dgrad(const WinoGeo& w, const mg_conv_geom* g, const float* dy, const float* wt, const float* bias, float* dx, int act,
               float* ws, hipStream_t st, const float* u_pre, float* md_keep, const float** addend) {
    const WinoGemm s = wino_gemm_plan(w, 1, g);
    const WinoWs o = wino_ws(w, s, 1, g);
    float* U = u_pre ? const_cast<float*>(u_pre) : ws + o.u;
    float* Md = md_keep ? md_keep : ws + o.md;
    float* dV = ws + o.dv;
    float* dd = ws + o.dd;
    if (!u_pre) wino_xform_u(w, g, wt, U, st);
    if (dy) wino_xform_md(w, g, dy, Md, st);
    wino_gemm(w, s, 1, g, Md, U, dV, ws + o.part, st);
    if (w.r == R_WINO && !w.hp && wino_dd_gather_ok(g->H, g->W, g->Ci)) {      // small maps: patches through LDS, one kernel
        const int ts = w.TH * w.TW;
        const size_t lds = (size_t)ts * 16 * 8 * sizeof(float4);
        const dim3 grid(g->Ci / 32, g->B);
        const float* add = *addend;
        *addend = nullptr;                     // consumed: mg_conv_dgrad_w has nothing left to add
        auto go = [&](auto kern) {
            hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, (const float*)dV, g->B, g->H, g->W, g->Ci, g->reflect, bias, act, dx, add);
        };
        if (ts <= 32) go(wino_dd_gather_kernel<1>); else go(wino_dd_gather_kernel<2>);
        MG_CHECK_LAUNCH();
        return MG_OK;
    }
    const dim3 grid(wino_grid((size_t)w.T * w.Kc / w.f.vec)), gx(wino_grid((size_t)g->B * g->H * g->W * g->Ci / 4));
    if (w.r == R_WINO) {
        hipLaunchKernelGGL(wino_dd_xform_kernel, grid, dim3(256), 0, st, (const float*)dV, w.T, w.Kc, dd);
        hipLaunchKernelGGL(wino_dx_gather_kernel, gx, dim3(256), 0, st, (const float*)dd, g->B, g->H, g->W, g->Ci, g->reflect, bias,
                           act, dx, (int)w.hp);
    } else {
        hipLaunchKernelGGL(wino4_dd_xform_kernel, grid, dim3(256), 0, st, (const float*)dV, w.T, w.Kc, dd);
        if (w.r == R_WINO4)
            hipLaunchKernelGGL(wino4_dx_gather_kernel, gx, dim3(256), 0, st, (const float*)dd, g->B, g->H, g->W, g->Ci, w.TH, w.TW, dx);
        else
            hipLaunchKernelGGL(wino42_dx_gather_kernel, gx, dim3(256), 0, st, (const float*)dd, g->B, g->H, g->W, g->Ci, w.TH, w.TW, dx);
    }
    MG_CHECK_LAUNCH();
    return MG_OK;
}

// v_in / md_in: the images the forward / data-gradient calls kept.  ad (F(2x2,3x3), float32): dw IS the weight tensor --
// inverse transform + Adam + next iteration's forward transform in one pass.  dbias: the bias gradient (column sums of dy).
int wino_wgrad(const WinoGeo& w, const mg_conv_geom* g, const float* x, const float* dy, float* dw, float* dbias, int accumulate,
               float* ws, hipStream_t st, const float* v_in, const float* md_in, const mg_wino_adam* ad = nullptr) {
    const WinoGemm s = wino_gemm_plan(w, 2, g);
    const WinoWs o = wino_ws(w, s, 2, g);
    float* V = v_in ? const_cast<float*>(v_in) : ws + o.v;
    float* Md = md_in ? const_cast<float*>(md_in) : ws + o.md;
    float* dU = ws + o.du;
    if (!v_in) wino_xform_v(w, g, x, V, st);
    if (!md_in) wino_xform_md(w, g, dy, Md, st);
    wino_gemm(w, s, 2, g, Md, V, dU, ws + o.part, st);
    const dim3 grid(wino_grid((size_t)g->Co * w.Kc / w.f.vec));
    if (ad)
        hipLaunchKernelGGL(wino_adam_kernel, grid, dim3(256), 0, st, (const float*)dU, g->Co, g->Ci, dw, ad->m, ad->v, ad->u,
                           ad->state, ad->beta1, ad->beta2, ad->eps, ad->grad_scale);
    else if (w.r == R_WINO)
        hipLaunchKernelGGL(wino_dweight_xform_kernel, grid, dim3(256), 0, st, (const float*)dU, g->Co, g->Ci, dw, accumulate);
    else if (w.r == R_WINO4)
        hipLaunchKernelGGL(wino4_dweight_xform_kernel, grid, dim3(256), 0, st, (const float*)dU, g->Co, g->Ci, dw, accumulate);
    else
        hipLaunchKernelGGL(wino42_dweight_xform_kernel, grid, dim3(256), 0, st, (const float*)dU, g->Co, g->Ci, dw, accumulate);
    MG_CHECK_LAUNCH();
    if (dbias) {
        const long long M = (long long)g->B * g->OH * g->OW;
        return mg_colsum(dy, M, g->Co, dbias, accumulate, ws + o.cs, mg_colsum_workspace(M, g->Co), st);
    }
    return MG_OK;
}

}  // namespace
