// K3 / K4 / K6: the convolution translation unit.  The kernels and the host code of every family live in the headers below, one
// subject each; this file holds conv_route, which names the family a pass of a layer takes, and the extern "C" entry points.
#include "common.h"
#include "mdctgan_hip.h"
#include "internal.h"
#include <stdio.h>
#include <stdlib.h>
#include <cstring>
#include <type_traits>
#include <map>
#include <mutex>
#include <tuple>
#include <hip/hip_ext.h>
// the generic implicit-GEMM kernels and the split-K combine launches
#include "conv_kernels.h"
// the Winograd and small-channel kernels
#include "wino.h"
#include "wino4.h"
#include "wino42.h"
#include "wino43.h"
#include "conv_smallc.h"
// host side: probe, plans and picks (with the LDS-DMA families inside its namespace), then the two orchestrations
#include "conv_plan.h"
#include "wino_h16.h"
#include "wino_host.h"
#include "conv_smallc_host.h"

namespace {

// The kernel family of a pass (0 fwd, 1 dgrad, 2 wgrad) of a layer; generic: only the tail every family falls back to.  The
// special families' predicates are pairwise disjoint apart from co1 / rowdot (both Co == 1: co1 first), so their order here
// is no priority.  F(4x4,3x3) is asked first: its precision value is its own, and a geometry of that value which it does not
// take meets every other predicate as MG_PRECISION_F32 does.  It names all three passes (the route is a function of the geometry
// alone); the gradient entry points refuse it.
ConvRoute conv_route(int pass, const mg_conv_geom* g, bool generic) {
    if (!generic) {
        if (wino43_ok(g)) return R_WINO43;
        if (winoh_ok(g)) return R_WINOH;           // (likewise: its precision value is its own; the rest as MG_PRECISION_F16)
        if (co1_gemm_ok(g)) return R_CO1;
        if (pass != 1 && mg_conv_rowdot_kq(g)) return R_ROWDOT;
        if (h16_ok(g)) return R_H16;
        if (wino_ok(g)) return R_WINO;
        if (wino4_ok(g)) return R_WINO4;
        if (wino42_ok(g)) return R_WINO42;
        if (pass == 0 ? smallc_fwd_kind(g) != 0 : pass == 1 ? smallc_dgrad_ok(g) : smallc_wgrad_kind(g) != 0) return R_SMALLC;
    }
    if (pass == 0) return conv_dma_fwd_ok(g) ? R_DMA : R_IGEMM;
    if (pass == 2) return conv_dma_wgrad_ok(g) ? R_DMA : R_IGEMM;
    return conv_dma_dgrad_ok(g) ? R_DMA : cd_reflect_dgrad_ok(g) ? R_DMA_REFLECT : R_IGEMM;
}
// The images a layer keeps between the passes of a step (mg_wino_tiles), from the routes of its three passes: the kind of the
// weight image mg_conv_wino_prepare writes (MG_IMAGE_*), its Winograd positions P (0: not a Winograd image) and element size, and
// the byte sizes of u, v and md.  r: the forward route.  The size queries, mg_conv_wino_prepare and mg_conv_traits are views of it.
struct ConvImages { ConvRoute r; int kind, P, elem; size_t u, v, md; };
ConvImages conv_images(const mg_conv_geom* g) {
    const ConvRoute r = conv_route(0, g);
    switch (r) {
    case R_CO1:         // tap GEMM: the weights zero-padded to 64 tap rows; v: the rounded x (autocast), md: Gt (data -> weight gradient)
        return {r, MG_IMAGE_CO1, 0, 4, (size_t)CO1_TAPS * g->Ci * sizeof(float), co1_xr_bytes(g), co1_zt_bytes(g)};
    case R_H16:         // the float16 weight copy of the autocast GEMM path (conv_h16.h); no tiles
        return {r, MG_IMAGE_CAST, 0, 2, h16_weights_bytes(g), 0, 0};
    case R_WINO: case R_WINO4: case R_WINO42: case R_WINO43: case R_WINOH: {
        const WinoGeo w = wino_geo(r, g);
        const size_t e = r == R_WINOH ? 2 : sizeof(float), P = w.f.P;
        const bool fwd_only = r == R_WINO43 || r == R_WINOH;      // V only: no gradient pass reads an image of the output gradient
        return {r, r == R_WINOH ? MG_IMAGE_WINO_F16 : MG_IMAGE_WINO_F32, w.f.P, (int)e, P * g->Co * w.Kc * e, P * w.T * w.Kc * e,
                fwd_only ? 0 : P * w.T * g->Co * e};
    }
    default: {
        // a layer whose forward pass or data gradient runs on the float16 implicit GEMMs (conv_dma.h) keeps a float16 copy of its
        // weights, and -- where its weight gradient runs there too -- the float16 copies of x (forward -> weight gradient) and of dy
        // (data gradient -> weight gradient) as its "tiles", so that each tensor is cast once per step.  (A Winograd layer keeps
        // float32 U / V / Md images under MG_PRECISION_F16: it must never be handed the float16-sized buffers of this path.)
        const ConvRoute d = conv_route(1, g);
        const bool fh = r == R_DMA, dh = d == R_DMA || d == R_DMA_REFLECT, wh = conv_route(2, g) == R_DMA;
        if (!conv_dma_half(g) || !(fh || dh)) return {r, MG_IMAGE_NONE, 0, 0, 0, 0, 0};
        return {r, MG_IMAGE_CAST, 0, 2, h16_weights_bytes(g), wh && fh ? conv_dma_h_x_bytes(g) : 0, wh && dh ? conv_dma_h_dy_bytes(g) : 0};
    }
    }
}

}  // namespace

extern "C" {

int mg_abi_version(void) { return 4; }
int mg_conv_geom_size(void) { return (int)sizeof(mg_conv_geom); }

void mg_probe_arm(void* e0, void* e1) {
    g_probe_e0 = (hipEvent_t)e0;
    g_probe_e1 = (hipEvent_t)e1;
}

// FLOPs the main GEMM kernel of a pass issues for this geometry (2*M*N*K of the GEMM it actually runs: the direct
// convolution's 2*MACs, or P Winograd-domain GEMMs -- 16 of them = 1/2.25 of that on the unpadded tile grid).
double mg_conv_plan_flops(int pass, const mg_conv_geom* g) {
    if (!geom_ok(g)) return 0.0;
    switch (const ConvRoute r = conv_route(pass, g)) {
    case R_CO1: return 2.0 * CO1_TAPS * (double)g->B * g->H * g->W * g->Ci;      // the 64-tap GEMM (conv_co1.h)
    case R_WINO: case R_WINO4: case R_WINO42: case R_WINO43: case R_WINOH: {
        const WinoGeo w = wino_geo(r, g);
        return 2.0 * w.f.P * (double)w.T * (double)g->Co * w.Kc;
    }
    default: return 2.0 * g->B * g->OH * g->OW * (double)g->Co * g->KH * g->KW * g->Ci;
    }
}

// Split-K factor of the LDS-DMA kernels or of the Winograd-domain GEMM a pass runs (0: another family)
int mg_conv_plan_splits(int pass, const mg_conv_geom* g) {
    if (!geom_ok(g) || pass < 0 || pass > 2) return 0;
    const ConvRoute r = conv_route(pass, g);
    if (r == R_DMA_REFLECT) {
        const mg_conv_geom gp = cd_reflect_geom(g);
        return conv_dma_dgrad_plan(&gp).splits;
    }
    if (r == R_WINO43 && pass != 0) return 0;      // forward only
    if (r == R_WINOH) return pass == 0 ? 1 : 0;    // forward only, never split
    if (r == R_WINO || r == R_WINO4 || r == R_WINO42 || r == R_WINO43) {      // the Winograd-domain GEMM stage, on either kernel family
        const WinoGemm s = wino_gemm_plan(wino_geo(r, g), pass, g);
        return s.dp.ok ? s.dp.splits : s.tp.splits;
    }
    if (r != R_DMA) return 0;
    return (pass == 0 ? conv_dma_fwd_plan(g) : pass == 1 ? conv_dma_dgrad_plan(g) : conv_dma_wgrad_plan(g)).splits;
}
// Launch order of the LDS-DMA forward pass / data gradient (CdArgs.gm, CdArgs.cls_order) under the current environment: what
// conv_dma_fwd_launch / conv_dma_dgrad_launch compute for the pass's plan.  0 / 0 for every other pass and family.
int mg_conv_plan_order(int pass, const mg_conv_geom* g, int* gm, int* cls_order) {
    if (!geom_ok(g) || !gm || !cls_order || pass < 0 || pass > 2) return MG_ERR_ARG;
    *gm = 0;
    *cls_order = 0;
    const ConvRoute r = conv_route(pass, g);
    if (pass == 0 && r == R_DMA) {
        *gm = conv_dma_fwd_gm(g, conv_dma_fwd_plan(g));
    } else if (pass == 1 && (r == R_DMA || r == R_DMA_REFLECT)) {
        const mg_conv_geom gp = r == R_DMA ? *g : cd_reflect_geom(g);
        const CdOrder o = conv_dma_dgrad_order(&gp, conv_dma_dgrad_plan(&gp));
        *gm = o.gm;
        *cls_order = o.cls_order;
    }
    return MG_OK;
}
// Name of the kernel instance a pass would launch for this geometry (matches the symbol rocprofv3 reports,
// minus the anonymous-namespace prefix).  pass: 0 fwd, 1 dgrad, 2 wgrad.
int mg_conv_plan_name(int pass, const mg_conv_geom* g, char* out, int out_len) {
    if (!geom_ok(g) || !out || out_len < 64 || pass < 0 || pass > 2) return MG_ERR_ARG;
    const char* half = prec_h(g) ? "true" : "false";
    if (pass != 0 && conv_route(pass, g) == R_WINO43) return MG_ERR_UNSUPPORTED;      // F(4x4,3x3) has no gradient passes
    if (pass != 0 && conv_route(pass, g) == R_WINOH) return MG_ERR_UNSUPPORTED;       // nor have the float16 images
    switch (const ConvRoute r = conv_route(pass, g)) {
    case R_CO1:          // single-output-channel layers as tap GEMMs (conv_co1.h)
        snprintf(out, out_len, pass == 0 ? "dgemm32g_kernel<64, 128, 2, 2, 0, 0, 2, 0, 0>"
                               : pass == 1 ? "dgemm32g_kernel<128, 64, 2, 2, 1, 1, 2, 0, 0>" : "dgemm32g_kernel<64, 64, 2, 2, 0, 1, 2, 0, 0>");
        break;
    case R_ROWDOT:
        snprintf(out, out_len, pass == 0 ? "conv_rowdot_fwd_kernel<%d>" : "conv_rowdot_wgrad_kernel<%d>", mg_conv_rowdot_kq(g));
        break;
    case R_H16: {
        const long long px = (long long)g->B * g->OH * g->OW;
        const int Kw = g->KH * g->KW * g->Ci;
        bool deep;
        if (pass == 0) deep = h16_deep(px, g->Co, h16_plan(px, g->Co, Kw, false).splits, false);
        else if (pass == 1) deep = h16_deep((long long)g->B * g->H * g->W, g->Ci, h16_plan((long long)g->B * g->H * g->W, g->Ci, g->KH * g->KW * g->Co, true).splits, true);
        else deep = h16_deep(g->Co, Kw, h16_plan(g->Co, Kw, h16_mp(px), false).splits, false);
        if (pass == 2 && h16_wgrad_as(g)) snprintf(out, out_len, "hgemm_as_kernel<%d, false, false>", h16_mp(px) / 64);
        else if (pass != 2 && h16_sa(pass, g)) snprintf(out, out_len, pass == 1 ? "hgemm_sa_kernel<true, false>" : "hgemm_sa_kernel<false, true>");
        else
        snprintf(out, out_len, pass == 1 ? "hgemm_kernel<128, 128, 4, 2, true, %d>" : "hgemm_kernel<128, 128, 4, 2, false, %d>", deep ? 3 : 2);
        break;
    }
    case R_WINO: case R_WINO4: case R_WINO42: case R_WINO43: {
        const WinoGeo w = wino_geo(r, g);
        const WinoGemm s = wino_gemm_plan(w, pass, g);
        if (s.dp.ok) dense_name(pass, w.f.P, s.dp, dense_dims(pass, w.T, g->Co, w.Kc).N, out, out_len);
        else gemm_pick_name(pass, GemmPick{s.tp.bm, s.tp.bn, true, true, s.tag, s.tp.k32, s.tp.splits, s.tp.cps}, out, out_len);
        break;
    }
    case R_WINOH: snprintf(out, out_len, "%s", winoh_gemm_name(wino_geo(r, g).T, g->Co)); break;
    case R_SMALLC:
        if (pass == 0) snprintf(out, out_len, "conv_smallc_fwd_kernel<%d, %d, %d, %d>", g->KH, g->KW, g->Ci, g->stride);
        else if (pass == 1) snprintf(out, out_len, "conv_smallc_dgrad_kernel<%d, %s>", g->Ci, half);
        else if (smallc_wgrad_plan(g).mfma_g) snprintf(out, out_len, "conv_smallc_wgrad_mfma_kernel<%d, %d, %d, %d>", g->KH, g->KW, g->Ci, g->stride);
        else snprintf(out, out_len, "conv_smallc_wgrad_kernel<%d, %d, %d>", g->KH, g->KW, g->Ci);
        break;
    case R_DMA: case R_DMA_REFLECT: {
        const int nbuf = prec_h(g) ? cd_half_nbuf() : 2;
        if (pass == 0) {
            const CdPlan cp = conv_dma_fwd_plan(g);
            snprintf(out, out_len, "conv_fwd_dma_kernel<%d, %d, %s, %d>", cp.bm, cp.bn, half, nbuf);
        } else if (pass == 1) {
            const mg_conv_geom gp = r == R_DMA ? *g : cd_reflect_geom(g);
            const CdPlan cp = conv_dma_dgrad_plan(&gp);
            snprintf(out, out_len, "conv_dgrad_dma_kernel<%d, %d, %s, %d>", cp.bm, cp.bn, half, nbuf);
        } else {
            const CdPlan cp = conv_dma_wgrad_plan(g);
            snprintf(out, out_len, "conv_wgrad_dma_kernel<%d, %d, %s, %d, %s>", cp.bm, cp.bn, half, nbuf, conv_dma_wgrad_rr(g) ? "true" : "false");
        }
        break;
    }
    default:
        gemm_pick_name(pass, pass == 0 ? fwd_pick(g, kAnyBuf) : pass == 1 ? dgrad_pick(g, kAnyBuf) : wgrad_pick(g, kAnyBuf), out, out_len);
    }
    return MG_OK;
}

size_t mg_conv_fwd_workspace(const mg_conv_geom* g) {
    if (!geom_ok(g)) return 0;
    const ConvRoute r = conv_route(0, g);
    switch (r) {
    case R_CO1: return co1_fwd_ws(g);
    case R_H16: return h16_fwd_ws(g);
    case R_WINO: case R_WINO4: case R_WINO42: case R_WINO43: return wino_ws_bytes(r, 0, g);
    case R_WINOH: return winoh_ws(wino_geo(r, g), g).bytes;
    default: break;
    }
    const TilePlan tp = fwd_plan(g);
    int sp = tp.splits;
    if (r == R_DMA && conv_dma_fwd_plan(g).splits > sp) sp = conv_dma_fwd_plan(g).splits;
    const size_t stage = (r == R_DMA && conv_dma_half(g)) ? conv_dma_h_x_bytes(g) + conv_dma_h_w_bytes(g) : 0;
    return stage + (sp > 1 ? (size_t)sp * g->B * g->OH * g->OW * g->Co * sizeof(float) + 256 : 256);
}
size_t mg_conv_dgrad_workspace(const mg_conv_geom* g) {
    if (!geom_ok(g)) return 0;
    const ConvRoute r = conv_route(1, g);
    switch (r) {
    case R_CO1: return co1_dgrad_ws(g);
    case R_H16: return h16_dgrad_ws(g);
    case R_WINO: case R_WINO4: case R_WINO42: return wino_ws_bytes(r, 1, g);
    case R_WINO43: case R_WINOH: return 0;          // no data gradient on these routes: mg_conv_dgrad_w refuses the geometry
    default: break;
    }
    const TilePlan tp = dgrad_plan(g);
    int sp = tp.splits;
    size_t base = sp > 1 ? (size_t)sp * g->B * g->H * g->W * g->Ci * sizeof(float) + 256 : 256;
    if (r == R_DMA) {
        if (cd_dgrad_ws(g) > base) base = cd_dgrad_ws(g);
    } else if (r == R_DMA_REFLECT) {
        const mg_conv_geom gp = cd_reflect_geom(g);
        const size_t need = cd_reflect_dxp_bytes(&gp) + cd_dgrad_ws(&gp);
        if (need > base) base = need;
    }
    return base;
}

size_t mg_conv_wino_weights_bytes(const mg_conv_geom* g) { return geom_ok(g) ? conv_images(g).u : 0; }
size_t mg_conv_wino_tiles_bytes(const mg_conv_geom* g, int which) {
    if (!geom_ok(g) || which < 0 || which > 1) return 0;
    const ConvImages m = conv_images(g);
    return which == 0 ? m.v : m.md;
}
int mg_conv_wino_prepare(const mg_conv_geom* g, const float* w, float* u, void* stream) {
    if (!geom_ok(g) || !w || !u || !aligned16(w) || !aligned16(u)) return MG_ERR_ARG;
    const ConvImages m = conv_images(g);
    switch (m.kind) {
    case MG_IMAGE_CO1: co1_pad_w(g, w, u, (hipStream_t)stream); break;
    case MG_IMAGE_WINO_F32: wino_xform_u(wino_geo(m.r, g), g, w, u, (hipStream_t)stream); break;
    case MG_IMAGE_WINO_F16: winoh_xform_u(g, w, (_Float16*)u, (hipStream_t)stream); break;
    case MG_IMAGE_CAST: return h16_prepare(g, w, u, (hipStream_t)stream);
    default: return MG_ERR_ARG;
    }
    MG_CHECK_LAUNCH();
    return MG_OK;
}
static bool wino_tiles_ok(const mg_conv_geom* g, const mg_wino_tiles* t) {
    if (!t || (!t->u && !t->v && !t->md)) return true;
    if (!mg_conv_wino_weights_bytes(g)) return false;
    return (!t->u || aligned16(t->u)) && (!t->v || aligned16(t->v)) && (!t->md || aligned16(t->md));
}

int mg_conv_fwd(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y, int act,
                void* workspace, size_t workspace_bytes, void* stream) {
    return mg_conv_fwd_w(g, x, w, bias, y, act, workspace, workspace_bytes, stream, nullptr);
}
int mg_conv_dgrad(const mg_conv_geom* g, const float* dy, const float* w, const float* bias, float* dx, int act,
                  void* workspace, size_t workspace_bytes, void* stream) {
    return mg_conv_dgrad_w(g, dy, w, bias, dx, act, workspace, workspace_bytes, stream, nullptr);
}
int mg_conv_wgrad(const mg_conv_geom* g, const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                  void* workspace, size_t workspace_bytes, void* stream) {
    return mg_conv_wgrad_w(g, x, dy, dw, dbias, accumulate, workspace, workspace_bytes, stream, nullptr);
}

// The F(2x2,3x3) output transform + InstanceNorm kernel (wino.h: wino_out_norm_kernel) and its backward: float32, maps of
// <= 160 tiles per sample
static bool wino_norm_ok(const mg_conv_geom* g) {
    return geom_ok(g) && conv_route(0, g) == R_WINO && !prec_h(g) && wino_out_norm_ok(g->OH / 2, g->OW / 2, g->Co);
}
// ... and the F(4x4,3x3) one (wino43.h: wino43_out_norm_kernel): maps of <= 40 tiles per sample, which also admit the hand-over
static bool wino43_norm_ok(const mg_conv_geom* g) {
    return geom_ok(g) && conv_route(0, g) == R_WINO43 && wino43_out_norm_ok(g->OH / 4, g->OW / 4, g->Co);
}
// ... and the one on float16 images (wino_h16.h: winoh_out_norm_kernel): the F(2x2,3x3) ranges, <= 160 tiles and <= 64 for the hand-over
static bool winoh_norm_ok(const mg_conv_geom* g) {
    return geom_ok(g) && conv_route(0, g) == R_WINOH && wino_out_norm_ok(g->OH / 2, g->OW / 2, g->Co);
}
int mg_conv_wino_md_from_norm_ok(const mg_conv_geom* g) { return wino_norm_ok(g) ? 1 : 0; }
int mg_instnorm_bwd_wino_md(const mg_conv_geom* g, const float* gy, const float* y_raw, const float* mean, const float* rstd,
                            int act, float* md, void* stream) {
    if (!gy || !y_raw || !mean || !rstd || !md) return MG_ERR_ARG;
    if (!mg_conv_wino_md_from_norm_ok(g)) return MG_ERR_UNSUPPORTED;
    if (act != MG_ACT_NONE && act != MG_ACT_RELU && act != MG_ACT_LRELU02) return MG_ERR_UNSUPPORTED;   // the only derivatives wino_norm_bwd_dy_kernel has
    if (!aligned16(gy) || !aligned16(y_raw) || !aligned16(mean) || !aligned16(rstd) || !aligned16(md)) return MG_ERR_ARG;
    const WinoGeo d = wino_geo(R_WINO, g);
    const dim3 grid(g->Co / 32, g->B);
    const int nt = (d.TH * d.TW + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
#define MG_NORM_BWD_DY(NT_) hipLaunchKernelGGL(wino_norm_bwd_dy_kernel<NT_>, grid, dim3(256), 0, st, gy, y_raw, mean, rstd, g->B, d.TH, d.TW, g->Co, act, md)
    if (nt == 1) MG_NORM_BWD_DY(1); else if (nt == 2) MG_NORM_BWD_DY(2); else if (nt == 3) MG_NORM_BWD_DY(3); else if (nt == 4) MG_NORM_BWD_DY(4); else MG_NORM_BWD_DY(5);
#undef MG_NORM_BWD_DY
    MG_CHECK_LAUNCH();
    return MG_OK;
}
size_t mg_conv_fwd_instnorm_workspace(const mg_conv_geom* g) {
    if (!geom_ok(g)) return 0;
    const size_t a = mg_conv_fwd_workspace(g), b = mg_instnorm_workspace(g->B, g->OH * g->OW, g->Co);
    return a > b ? a : b;
}
int mg_conv_fwd_instnorm_w(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                           int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                           size_t workspace_bytes, void* stream, const mg_wino_tiles* wt) {
    return mg_conv_fwd_instnorm_h(g, x, w, bias, y_raw, eps, act, residual, y, mean, rstd, workspace, workspace_bytes, stream, wt, nullptr);
}
// The fused F(2x2,3x3) output transform + InstanceNorm kernel can also write the NEXT 3x3 stride-1 pad-1 layer's input image
// (wino.h: wino_out_norm_kernel<NT, true>): maps of <= 64 tiles per sample.
static bool wino_vnext_ok(const mg_conv_geom* g) {
    if (wino43_norm_ok(g)) return true;
    if (winoh_norm_ok(g)) return wino_out_norm_next_ok(g->OH / 2, g->OW / 2, g->Co);
    return wino_norm_ok(g) && wino_out_norm_next_ok(g->OH / 2, g->OW / 2, g->Co) && g->Co % 16 == 0;
}
int mg_conv_wino_vnext_ok(const mg_conv_geom* g) { return g && wino_vnext_ok(g) ? 1 : 0; }

// Everything a caller that holds a layer's images between passes asks about the layer (include/mdctgan_hip.h), in one answer
int mg_conv_traits(const mg_conv_geom* g, struct mg_conv_traits* out) {
    if (!out || !geom_ok(g)) return MG_ERR_ARG;
    const ConvImages m = conv_images(g);
    const ConvRoute d = conv_route(1, g);
    const bool half = prec_h(g);
    *out = {};
    out->weight_image = m.kind;
    out->weight_positions = m.P;
    out->weight_elem = m.elem;
    out->images_half = m.kind == MG_IMAGE_WINO_F16;
    // (a forward-only route is neither: its gradient passes do not exist)
    out->tiles = m.kind == MG_IMAGE_CO1 ? 2 : (half && conv_route(2, g) == R_DMA) ? 1 : 0;
    out->precast[0] = half && (m.r == R_DMA || (m.r == R_H16 && h16_sa(0, g)));
    out->precast[1] = half && (d == R_DMA || d == R_DMA_REFLECT);
    out->vnext_positions = wino_vnext_ok(g) ? m.P : 0;
    out->md_from_norm = mg_conv_wino_md_from_norm_ok(g);
    out->wgrad_adam = mg_conv_wgrad_adam_ok(g);
    out->wgrad_checks_finite = mg_conv_wgrad_checks_finite(g);
    out->wgrad_h16 = mg_conv_wgrad_h16_ok(g);
    return MG_OK;
}

static int conv_fwd_instnorm_impl(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                                  int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                                  size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, void* y16, void* v_next,
                                  int next_reflect);
static int conv_fwd(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y, int act, void* workspace,
                    size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, FwdDefer* defer);

int mg_conv_fwd_instnorm_next(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                              int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                              size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, float* v_next, int next_reflect) {
    if (!g || !v_next || !aligned16(v_next) || !wino_vnext_ok(g)) return MG_ERR_ARG;
    if (conv_route(0, g) == R_WINOH) return MG_ERR_ARG;       // that layer's image is halves: mg_conv_fwd_instnorm_next_h
    return conv_fwd_instnorm_impl(g, x, w, bias, y_raw, eps, act, residual, y, mean, rstd, workspace, workspace_bytes, stream, wt, nullptr,
                                  v_next, next_reflect);
}

int mg_conv_fwd_instnorm_next_h(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                                int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                                size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, void* v_next16, int next_reflect,
                                void* y16) {
    if (!g || !geom_ok(g) || conv_route(0, g) != R_WINOH || !wino_vnext_ok(g)) return MG_ERR_ARG;
    if ((v_next16 && !aligned16(v_next16)) || (y16 && !aligned16(y16))) return MG_ERR_ARG;
    return conv_fwd_instnorm_impl(g, x, w, bias, y_raw, eps, act, residual, y, mean, rstd, workspace, workspace_bytes, stream, wt, y16,
                                  v_next16, next_reflect);
}

int mg_conv_fwd_instnorm_h(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                           int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                           size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, void* y16) {
    return conv_fwd_instnorm_impl(g, x, w, bias, y_raw, eps, act, residual, y, mean, rstd, workspace, workspace_bytes, stream, wt, y16,
                                  nullptr, 0);
}

static int conv_fwd_instnorm_impl(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y_raw, float eps,
                                  int act, const float* residual, float* y, float* mean, float* rstd, void* workspace,
                                  size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, void* y16, void* v_next,
                                  int next_reflect) {
    if (y16 && !prec_h(g)) return MG_ERR_UNSUPPORTED;          // the float32 layers' fused inverse transform + norm has no float16 output
    if (!geom_ok(g) || !x || !w || !y || !mean || !rstd) return MG_ERR_ARG;
    if (!wino_tiles_ok(g, wt)) return MG_ERR_ARG;
    if (!workspace || workspace_bytes < mg_conv_fwd_instnorm_workspace(g)) return MG_ERR_ARG;
    // y_raw == NULL (inference: no backward pass will read the raw convolution output): the fused kernel skips that store -- a
    // fifth of its HBM bytes at batch 64 -- and the two-call path normalises in place
    if (winoh_norm_ok(g) && aligned16(x) && aligned16(w) && (!y_raw || aligned16(y_raw)) && aligned16(y) && aligned16(mean) &&
        aligned16(rstd) && aligned16(workspace) && (!bias || aligned16(bias)) && (!residual || aligned16(residual)) &&
        (!y16 || (reinterpret_cast<uintptr_t>(y16) & 7) == 0)) {
        const WinohNorm nrm{eps, act, residual, y, mean, rstd, (_Float16*)y16, (_Float16*)v_next, next_reflect};
        return winoh_fwd(wino_geo(R_WINOH, g), g, x, w, bias, y_raw, MG_ACT_NONE, (char*)workspace, (hipStream_t)stream,
                         wt ? (const void*)wt->u : nullptr, wt ? (void*)wt->v : nullptr, wt && wt->v && (wt->flags & MG_TILES_V_FILLED),
                         &nrm);
    }
    const bool n43 = wino43_norm_ok(g);
    if ((n43 || wino_norm_ok(g)) && aligned16(x) && aligned16(w) && (!y_raw || aligned16(y_raw)) && aligned16(y) && aligned16(mean) &&
        aligned16(rstd) && aligned16(workspace) && (!bias || aligned16(bias)) && (!residual || aligned16(residual))) {
        const WinoNorm nrm{eps, act, residual, y, mean, rstd, (float*)v_next, next_reflect};
        return wino_fwd(wino_geo(n43 ? R_WINO43 : R_WINO, g), g, x, w, bias, y_raw, MG_ACT_NONE, (float*)workspace, (hipStream_t)stream,
                        wt ? wt->u : nullptr, wt ? wt->v : nullptr, wt && wt->v && (wt->flags & MG_TILES_V_FILLED), &nrm);
    }
    if (v_next) return MG_ERR_ARG;           // (unreachable after wino_vnext_ok: the fused path above is the only writer of v_next)
    float* const raw_out = y_raw;            // NULL under no_grad: the slab kernel then skips that store, the two-launch path normalises in place
    if (!y_raw) y_raw = y;
    // small maps: the one-launch InstanceNorm kernel also finishes a split-K convolution (sums the slabs, bias, autocast rounding)
    FwdDefer defer{nullptr, 0, nullptr, 0, false};
    const bool no_defer = getenv("MG_NO_FWD_DEFER") != nullptr;      // (read per call: the bit-identity test flips it)
    const bool can_defer = !no_defer && mg_instnorm_slab_ok(g->OH * g->OW, g->Co) && g->Co % 4 == 0 && (!bias || aligned16(bias));
    const int rc = conv_fwd(g, x, w, bias, y_raw, MG_ACT_NONE, workspace, workspace_bytes, stream, wt, can_defer ? &defer : nullptr);
    if (rc != MG_OK) return rc;
    if (defer.filled)
        return mg_instnorm_fwd_slabs(defer.part, defer.splits, defer.bias, defer.round_f16, raw_out, g->B, g->OH * g->OW, g->Co, eps, act,
                                     residual, y, mean, rstd, stream, y16);
    return mg_instnorm_fwd_h(y_raw, g->B, g->OH * g->OW, g->Co, eps, act, residual, y, mean, rstd, workspace, workspace_bytes, stream, y16);
}

int mg_conv_fwd_w(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y, int act,
                  void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* wt) {
    return conv_fwd(g, x, w, bias, y, act, workspace, workspace_bytes, stream, wt, nullptr);
}
// defer (nullable): the caller's InstanceNorm sums the split-K slabs of a DMA / h16 forward pass (FwdDefer)
static int conv_fwd(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y, int act, void* workspace,
                    size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, FwdDefer* defer) {
    if (!geom_ok(g) || !x || !w || !y) return MG_ERR_ARG;
    if (!wino_tiles_ok(g, wt)) return MG_ERR_ARG;
    const float* u = wt ? wt->u : nullptr;
    float* v = wt ? wt->v : nullptr;
    const bool v_filled = v && (wt->flags & MG_TILES_V_FILLED);
    hipStream_t st = (hipStream_t)stream;
    const bool al = workspace && aligned16(x) && aligned16(w) && aligned16(y) && aligned16(workspace) && (!bias || aligned16(bias));
    switch (const ConvRoute r = conv_route(0, g)) {
    case R_H16:
        if (al && workspace_bytes >= h16_fwd_ws(g)) return h16_fwd(g, x, w, bias, y, act, (char*)workspace, st, u, v_filled ? v : nullptr, defer);
        break;
    case R_CO1:
        if (workspace && workspace_bytes >= co1_fwd_ws(g) && aligned16(x) && aligned16(w) && aligned16(workspace))
            return co1_fwd(g, x, w, bias, y, act, (char*)workspace, st, u, v);
        [[fallthrough]];
    case R_ROWDOT:
        if (mg_conv_rowdot_kq(g) && aligned16(x) && aligned16(w)) {
            probe_begin(st);
            const int rc = mg_conv_rowdot_fwd(g, x, w, bias, y, act, stream);
            probe_end(st);
            return rc;
        }
        break;
    case R_WINO: case R_WINO4: case R_WINO42: case R_WINO43:
        if (al && workspace_bytes >= wino_ws_bytes(r, 0, g))
            return wino_fwd(wino_geo(r, g), g, x, w, bias, y, act, (float*)workspace, st, u, v,
                            (r == R_WINO43 || (r == R_WINO && !prec_h(g))) && v_filled);
        break;
    case R_WINOH:
        if (al && workspace_bytes >= winoh_ws(wino_geo(r, g), g).bytes)
            return winoh_fwd(wino_geo(r, g), g, x, w, bias, y, act, (char*)workspace, st, u, v, v_filled);
        break;
    case R_SMALLC:
        if ((reinterpret_cast<uintptr_t>(w) & 7) == 0) {      // conv_smallc_fwd_kernel reads its weights as float2s
            probe_begin(st);
            const int rc = smallc_fwd(g, x, w, bias, y, act, st);
            probe_end(st);
            return rc;
        }
        break;
    default: break;
    }
    const Geom gg = to_geom(g);
    const long long M = (long long)g->B * g->OH * g->OW;
    const int N = g->Co;
    const bool cd_half = conv_dma_half(g);
    if (conv_route(0, g, true) == R_DMA && aligned16(x) && aligned16(w) && aligned16(y) && (!bias || aligned16(bias)) &&
        (!cd_half || (workspace && aligned16(workspace) && workspace_bytes >= mg_conv_fwd_workspace(g)))) {
        CdPlan cp = conv_dma_fwd_plan(g);
        if (cp.splits > 1 && (!workspace || workspace_bytes < mg_conv_fwd_workspace(g) || !aligned16(workspace)))
            one_split(cp, 1 << 28);
        const void* xin = x;
        const void* win = w;
        char* wsp = (char*)workspace;
        if (cd_half) {          // float16 copies: the activation by a cast pass, the weights from the cache when there is one
            // x: v is kept by the caller for the weight gradient; v_filled: x's producer already wrote it (mg_instnorm_fwd_h)
            xin = cd_stage16(x, v, v_filled, (size_t)g->B * g->H * g->W * g->Ci, conv_dma_h_x_bytes(g), wsp, st);
            win = cd_stage16(w, u, true, (size_t)g->Co * g->KH * g->KW * g->Ci, conv_dma_h_w_bytes(g), wsp, st);
            MG_CHECK_LAUNCH();
        }
        probe_begin(st);
        conv_dma_fwd_launch(g, cp, xin, win, bias, y, act, (float*)wsp, st);
        probe_end(st);
        MG_CHECK_LAUNCH();
        if (cp.splits > 1) {
            const size_t n = (size_t)M * N;
            if (defer && act == MG_ACT_NONE) {
                *defer = FwdDefer{(const float*)wsp, cp.splits, bias, cd_half ? 1 : 0, true};
                return MG_OK;
            }
            splitk_epilogue(conv_grid(n / 4), (const float*)wsp, cp.splits, n, N, bias, act, y, cd_half ? 1 : 0, st);
            MG_CHECK_LAUNCH();
        }
        return MG_OK;
    }
    const GemmPick p = fwd_pick(g, BufFacts{aligned16(x), aligned16(w),
                                            workspace && aligned16(workspace) && aligned16(y) && (!bias || aligned16(bias)) &&
                                                workspace_bytes >= mg_conv_fwd_workspace(g)});
    float* part = p.splits > 1 ? (float*)workspace : nullptr;
    probe_begin(st);
    dispatch_tile(p.bm, p.bn, [&](auto bm, auto bn) {
        constexpr int BM_ = decltype(bm)::value, BN_ = decltype(bn)::value;
        const dim3 grid((unsigned)(((M + BM_ - 1) / BM_) * ((N + BN_ - 1) / BN_)), p.splits);
        dispatch_tag(p.tag, [&](auto tag) {
            constexpr int TAG = decltype(tag)::value;
            if (p.k32)
                launch_fwd32<BM_, BN_, TAG>(grid, st, gg, x, w, bias, y, act, p.splits == 1 ? (1 << 29) : p.cps / 2, part, Batch{0, 0, 0, 0});
            else
                dispatch_bool(p.veca, [&](auto vec) {
                    hipLaunchKernelGGL((conv_fwd_kernel<BM_, BN_, decltype(vec)::value, TAG>), grid, dim3(256), 0, st, gg, x, w, bias, y,
                                       act, p.cps, part, Batch{0, 0, 0, 0});
                });
        });
    });
    probe_end(st);
    MG_CHECK_LAUNCH();
    if (part) {
        const size_t n = (size_t)M * N;
        splitk_epilogue(conv_grid(n / 4), part, p.splits, n, N, bias, act, y, p.tag == 2, st);
        MG_CHECK_LAUNCH();
    }
    return MG_OK;
}

static int conv_dgrad(const mg_conv_geom* g, const float* dy, const float* w, const float* bias, float* dx, int act,
                      void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, const float** addend);
int mg_conv_dgrad_w(const mg_conv_geom* g, const float* dy, const float* w, const float* bias, float* dx, int act,
                    void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* wt) {
    if (wt && wt->add && !aligned16(wt->add)) return MG_ERR_ARG;
    const float* left = wt ? wt->add : nullptr;       // a path that can fold "dx += add" into its last kernel takes it
    int rc = conv_dgrad(g, dy, w, bias, dx, act, workspace, workspace_bytes, stream, wt, &left);
    if (rc == MG_OK && left) rc = mg_add(dx, left, dx, (long long)g->B * g->H * g->W * g->Ci, stream);
    return rc;
}
// addend (in / out): mg_wino_tiles.add, cleared by the path that adds it
static int conv_dgrad(const mg_conv_geom* g, const float* dy, const float* w, const float* bias, float* dx, int act,
                      void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, const float** addend) {
    if (!geom_ok(g) || !w || !dx) return MG_ERR_ARG;
    if (!wino_tiles_ok(g, wt)) return MG_ERR_ARG;
    // dy == NULL: wt->md already holds A dy A^T (mg_instnorm_bwd_wino_md) -- F(2x2,3x3) layers in the transposed formulation
    if (!dy && !(wt && wt->md && mg_conv_wino_md_from_norm_ok(g) && !bias && act == MG_ACT_NONE && workspace &&
                 workspace_bytes >= mg_conv_dgrad_workspace(g) && aligned16(w) && aligned16(dx) && aligned16(workspace)))
        return MG_ERR_ARG;
    const float* u = wt ? wt->u : nullptr;
    float* md = wt ? wt->md : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (g->reflect && g->stride != 1) return MG_ERR_UNSUPPORTED;
    if (conv_route(1, g) == R_WINO43 || conv_route(1, g) == R_WINOH) return MG_ERR_UNSUPPORTED;      // forward only: a training pass never carries these precisions
    const bool plain = !bias && act == MG_ACT_NONE;       // all but the F(2x2,3x3) and generic data gradients need it
    const bool al = workspace && aligned16(dy) && aligned16(w) && aligned16(dx) && aligned16(workspace);
    switch (const ConvRoute r = conv_route(1, g)) {
    case R_H16:
        if (plain && al && workspace_bytes >= h16_dgrad_ws(g)) return h16_dgrad(g, dy, w, dx, (char*)workspace, st, u, addend);
        break;
    case R_CO1:
        if (plain && workspace && workspace_bytes >= co1_dgrad_ws(g) && aligned16(w) && aligned16(dx) && aligned16(workspace))
            return co1_dgrad(g, dy, w, dx, (char*)workspace, st, u, md);
        break;
    case R_SMALLC:
        if (plain && aligned16(dy)) {
            probe_begin(st);
            const int rc = smallc_dgrad(g, dy, w, dx, st);
            probe_end(st);
            return rc;
        }
        break;
    case R_WINO: case R_WINO4: case R_WINO42:
        if ((r == R_WINO ? !bias || aligned16(bias) : plain) && al && workspace_bytes >= wino_ws_bytes(r, 1, g))
            return wino_dgrad(wino_geo(r, g), g, dy, w, bias, dx, act, (float*)workspace, st, u, md, addend);
        break;
    default: break;
    }
    const Geom gg = to_geom(g);
    const int s = g->stride;
    if (aligned16(dy) && aligned16(w) && aligned16(dx) && (!bias || aligned16(bias)) && workspace && aligned16(workspace) &&
        workspace_bytes >= mg_conv_dgrad_workspace(g)) {
        const ConvRoute r = conv_route(1, g, true);
        if (r == R_DMA)
            return cd_dgrad_run(g, dy, w, bias, dx, act, (char*)workspace, st, u, md, conv_dma_half(g) ? 1 : 0,
                                (wt && (wt->flags & MG_TILES_MD_FILLED)) ? 1 : 0);
        if (r == R_DMA_REFLECT && plain) {
            const mg_conv_geom gp = cd_reflect_geom(g);
            float* dxp = (float*)workspace;
            const int rc = cd_dgrad_run(&gp, dy, w, nullptr, dxp, MG_ACT_NONE, (char*)workspace + cd_reflect_dxp_bytes(&gp), st, u,
                                        md, 0, (wt && (wt->flags & MG_TILES_MD_FILLED)) ? 1 : 0);
            if (rc != MG_OK) return rc;
            const float* add = *addend;      // the skip connection's gradient rides in the fold (mg_wino_tiles.add)
            *addend = nullptr;
            hipLaunchKernelGGL(wino_fold_reflect_kernel, dim3(wino_grid((size_t)g->B * g->H * g->W * g->Ci / 4)), dim3(256), 0,
                               st, (const float*)dxp, g->B, g->H, g->W, g->Ci, dx, (int)prec_h(g), add);
            MG_CHECK_LAUNCH();
            return MG_OK;
        }
    }
    // every input pixel is produced by exactly one class launch; classes cover all of [0,H)x[0,W)
    const long long Mc = (long long)g->B * ((g->H + s - 1) / s) * ((g->W + s - 1) / s);   // largest class
    const int N = g->Ci;
    const GemmPick p = dgrad_pick(g, BufFacts{aligned16(dy), aligned16(w),
                                              workspace && aligned16(workspace) && aligned16(dx) && (!bias || aligned16(bias)) &&
                                                  workspace_bytes >= mg_conv_dgrad_workspace(g)});
    float* part = p.splits > 1 ? (float*)workspace : nullptr;
    probe_begin(st);
    dispatch_tile(p.bm, p.bn, [&](auto bm, auto bn) {
        constexpr int BM_ = decltype(bm)::value, BN_ = decltype(bn)::value;
        const dim3 grid((unsigned)(((Mc + BM_ - 1) / BM_) * ((N + BN_ - 1) / BN_)), p.splits, s * s);
        dispatch_tag(p.tag, [&](auto tag) {
            dispatch_bool(p.veca, [&](auto veca) {
                dispatch_bool(p.vecb, [&](auto vecb) {
                    hipLaunchKernelGGL((conv_dgrad_kernel<BM_, BN_, decltype(veca)::value, decltype(vecb)::value, decltype(tag)::value>),
                                       grid, dim3(256), 0, st, gg, dy, w, bias, dx, act, p.cps, part, Batch{0, 0, 0, 0});
                });
            });
        });
    });
    probe_end(st);
    MG_CHECK_LAUNCH();
    if (part) {
        const size_t n = (size_t)g->B * g->H * g->W * N;
        splitk_epilogue(conv_grid(n / 4), part, p.splits, n, N, bias, act, dx, p.tag == 2, st);
        MG_CHECK_LAUNCH();
    }
    return MG_OK;
}

size_t mg_colsum_workspace(long long M, int C) {
    const ColsumPlan p = colsum_plan(M, C);
    return ((size_t)p.splits + 1) * C * sizeof(float);
}

int mg_colsum(const float* a, long long M, int C, float* out, int accumulate, void* workspace,
              size_t workspace_bytes, void* stream) {
    if (!a || !out || M <= 0 || C <= 0 || !workspace) return MG_ERR_ARG;
    if (workspace_bytes < mg_colsum_workspace(M, C)) return MG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const ColsumPlan p = colsum_plan(M, C);
    float* part = (float*)workspace;                 // [splits][C]
    if (p.splits == 1) {
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((C + 63) / 64, 1), dim3(256), 0, st, a, M, C, M, out, 1, accumulate);
    } else {
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((C + 63) / 64, p.splits), dim3(256), 0, st, a, M, C,
                           p.rows_per_split, part, 0, 0);
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((C + 63) / 64, 1), dim3(256), 0, st, (const float*)part,
                           (long long)p.splits, C, (long long)p.splits, out, 1, accumulate);
    }
    MG_CHECK_LAUNCH();
    return MG_OK;
}

size_t mg_conv_wgrad_workspace(const mg_conv_geom* g) {
    if (!geom_ok(g)) return 0;
    const ConvRoute r = conv_route(2, g);
    switch (r) {
    case R_CO1: return co1_wgrad_ws(g);
    case R_ROWDOT: return mg_conv_rowdot_wgrad_workspace(g);
    case R_H16: return h16_wgrad_ws(g);
    case R_WINO: case R_WINO4: case R_WINO42: return wino_ws_bytes(r, 2, g);
    case R_WINO43: case R_WINOH: return 0;          // no weight gradient on these routes: mg_conv_wgrad_chk refuses the geometry
    case R_SMALLC: return smallc_wgrad_ws(g);
    default: break;
    }
    const WgradPlan p = wgrad_plan(g);
    int sp = p.splits;
    if (r == R_DMA && conv_dma_wgrad_plan(g).splits > sp) sp = conv_dma_wgrad_plan(g).splits;
    size_t wg = sp > 1 ? (size_t)sp * g->Co * g->KH * g->KW * g->Ci * sizeof(float) : 0;
    if (r == R_DMA && conv_dma_half(g)) wg += conv_dma_h_x_bytes(g) + conv_dma_h_dy_bytes(g);
    const size_t cs = mg_colsum_workspace((long long)g->B * g->OH * g->OW, g->Co);
    return (wg > cs ? wg : cs) + 256;
}

int mg_conv_wgrad_adam_ok(const mg_conv_geom* g) {
    return (geom_ok(g) && conv_route(2, g) == R_WINO && !prec_h(g) && g->Ci % 4 == 0) ? 1 : 0;
}
int mg_conv_wgrad_adam_w(const mg_conv_geom* g, const float* x, const float* dy, float* w, const mg_wino_adam* ad,
                         void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* wt) {
    if (!mg_conv_wgrad_adam_ok(g)) return MG_ERR_UNSUPPORTED;
    if (!w || !ad || !ad->m || !ad->v || !ad->u || !ad->state || !wino_tiles_ok(g, wt)) return MG_ERR_ARG;
    if ((!x || !dy) && !(wt && wt->v && wt->md && mg_conv_wino_md_from_norm_ok(g))) return MG_ERR_ARG;
    if (!workspace || workspace_bytes < mg_conv_wgrad_workspace(g)) return MG_ERR_ARG;
    if (!aligned16(w) || !aligned16(ad->m) || !aligned16(ad->v) || !aligned16(ad->u) || !aligned16(workspace) ||
        (x && !aligned16(x)) || (dy && !aligned16(dy)))
        return MG_ERR_ARG;
    return wino_wgrad(wino_geo(R_WINO, g), g, x, dy, w, nullptr, 0, (float*)workspace, (hipStream_t)stream, wt ? wt->v : nullptr,
                      wt ? wt->md : nullptr, ad);
}

int mg_conv_wgrad_w(const mg_conv_geom* g, const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                    void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* wt) {
    return mg_conv_wgrad_chk(g, x, dy, dw, dbias, accumulate, workspace, workspace_bytes, stream, wt, nullptr);
}
int mg_conv_wgrad_checks_finite(const mg_conv_geom* g) {
    return (geom_ok(g) && conv_route(2, g) == R_H16 && h16_wgrad_as(g)) ? 1 : 0;
}
int mg_conv_wgrad_h16_ok(const mg_conv_geom* g) { return mg_conv_wgrad_checks_finite(g); }
int mg_conv_wgrad_h16(const mg_conv_geom* g, const float* x, const float* dy, void* dw16, int accumulate, void* workspace,
                      size_t workspace_bytes, void* stream, float* found_inf) {
    if (!geom_ok(g) || !dw16 || !x || !dy) return MG_ERR_ARG;
    if (!mg_conv_wgrad_h16_ok(g)) return MG_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < mg_conv_wgrad_workspace(g)) return MG_ERR_ARG;
    if (!aligned16(x) || !aligned16(dy) || !aligned16(dw16) || !aligned16(workspace)) return MG_ERR_ARG;
    return h16_wgrad(g, x, dy, nullptr, accumulate, (char*)workspace, (hipStream_t)stream, found_inf, dw16);
}
int mg_conv_wgrad_chk(const mg_conv_geom* g, const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream, const mg_wino_tiles* wt, float* found_inf) {
    if (!geom_ok(g) || !dw) return MG_ERR_ARG;
    if (conv_route(2, g) == R_WINO43 || conv_route(2, g) == R_WINOH) return MG_ERR_UNSUPPORTED;      // forward only
    if (found_inf && !mg_conv_wgrad_checks_finite(g)) return MG_ERR_UNSUPPORTED;   // nobody would look at dw: refuse instead of skipping silently
    if (found_inf && !(x && dy && aligned16(x) && aligned16(dy) && aligned16(dw) && aligned16(workspace))) return MG_ERR_ARG;
    if (!wino_tiles_ok(g, wt)) return MG_ERR_ARG;
    // x / dy may be NULL when the caller hands over both Winograd images of an F(2x2,3x3) layer (no bias gradient then)
    if ((!x || !dy) && !(wt && wt->v && wt->md && mg_conv_wino_md_from_norm_ok(g) && !dbias && aligned16(dw) && aligned16(workspace)))
        return MG_ERR_ARG;
    if (workspace_bytes < mg_conv_wgrad_workspace(g) || !workspace) return MG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)g->B * g->OH * g->OW;
    const bool al = aligned16(x) && aligned16(dy) && aligned16(dw) && aligned16(workspace);
    switch (const ConvRoute r = conv_route(2, g)) {
    case R_CO1:
        if (aligned16(x) && aligned16(workspace))
            return co1_wgrad(g, x, dy, dw, dbias, accumulate, (char*)workspace, st, wt ? wt->v : nullptr, wt ? wt->md : nullptr);
        [[fallthrough]];
    case R_ROWDOT:
        if (mg_conv_rowdot_kq(g) && aligned16(x) && aligned16(workspace)) {
            probe_begin(st);
            const int rc = mg_conv_rowdot_wgrad(g, x, dy, dw, dbias, accumulate, workspace, workspace_bytes, stream);
            probe_end(st);
            return rc;
        }
        break;
    case R_H16:
        if (al) {
            const int rc = h16_wgrad(g, x, dy, dw, accumulate, (char*)workspace, st, found_inf);
            if (rc != MG_OK || !dbias) return rc;
            return mg_colsum(dy, M, g->Co, dbias, accumulate, (char*)workspace + h16_wgrad_cs_offset(g), mg_colsum_workspace(M, g->Co),
                             stream);
        }
        break;
    case R_WINO: case R_WINO4: case R_WINO42:
        if (al)
            return wino_wgrad(wino_geo(r, g), g, x, dy, dw, dbias, accumulate, (float*)workspace, st, wt ? wt->v : nullptr,
                              wt ? wt->md : nullptr);
        break;
    case R_SMALLC:
        // (conv_smallc_wgrad_mfma_kernel reads dy as float2s)
        if (aligned16(dw) && aligned16(workspace) && (reinterpret_cast<uintptr_t>(dy) & 7) == 0) {
            probe_begin(st);
            const int rc = smallc_wgrad(g, x, dy, dw, accumulate, (float*)workspace, st);
            probe_end(st);
            if (rc != MG_OK || !dbias) return rc;
            return mg_colsum(dy, M, g->Co, dbias, accumulate, (float*)workspace + smallc_wgrad_layout(g).cs,
                             mg_colsum_workspace(M, g->Co), stream);
        }
        break;
    default: break;
    }
    const Geom gg = to_geom(g);
    if (conv_route(2, g, true) == R_DMA && al) {
        const CdPlan cp = conv_dma_wgrad_plan(g);
        const size_t n_out = (size_t)g->Co * g->KH * g->KW * g->Ci;
        const void* xin = x;
        const void* dyin = dy;
        char* wsp = (char*)workspace;
        if (conv_dma_half(g)) {          // float16 copies: the caller's (made by the forward / data-gradient call) or cast here
            xin = cd_stage16(x, wt ? wt->v : nullptr, true, (size_t)g->B * g->H * g->W * g->Ci, conv_dma_h_x_bytes(g), wsp, st);
            dyin = cd_stage16(dy, wt ? wt->md : nullptr, true, (size_t)g->B * g->OH * g->OW * g->Co, conv_dma_h_dy_bytes(g), wsp, st);
            MG_CHECK_LAUNCH();
        }
        probe_begin(st);
        conv_dma_wgrad_launch(g, cp, xin, dyin, dw, accumulate, (float*)wsp, st);
        probe_end(st);
        MG_CHECK_LAUNCH();
        if (cp.splits > 1) {
            splitk_reduce(wgrad_reduce_grid(n_out / 4), (const float*)wsp, cp.splits, n_out, dw, accumulate, st);
            MG_CHECK_LAUNCH();
        }
        if (dbias)
            return mg_colsum(dy, (long long)g->B * g->OH * g->OW, g->Co, dbias, accumulate, workspace, workspace_bytes, stream);
        return MG_OK;
    }
    // (split: splitk_reduce_kernel reads the slabs and stores / accumulates into dw as float4s)
    const GemmPick p = wgrad_pick(g, BufFacts{aligned16(dy), aligned16(x), aligned16(dw) && aligned16(workspace)});
    const size_t n_out = (size_t)g->Co * g->KH * g->KW * g->Ci;
    float* target = p.splits > 1 ? (float*)workspace : dw;
    const int acc_direct = (p.splits > 1) ? 0 : accumulate;
    probe_begin(st);
    dispatch_tile(p.bm, p.bn, [&](auto bm, auto bn) {
        constexpr int BM_ = decltype(bm)::value, BN_ = decltype(bn)::value;
        if constexpr (BM_ == BN_) {      // (the weight gradient has square tiles only)
            const dim3 grid((unsigned)(((g->Co + BM_ - 1) / BM_) * ((g->KH * g->KW * g->Ci + BN_ - 1) / BN_)), 1, p.splits);
            dispatch_tag(p.tag, [&](auto tag) {
                dispatch_bool(p.veca, [&](auto veca) {
                    dispatch_bool(p.vecb, [&](auto vecb) {
                        hipLaunchKernelGGL((conv_wgrad_kernel<BM_, BN_, decltype(veca)::value, decltype(vecb)::value, decltype(tag)::value>),
                                           grid, dim3(256), 0, st, gg, x, dy, target, p.cps, acc_direct, Batch{0, 0, 0, 0});
                    });
                });
            });
        }
    });
    probe_end(st);
    MG_CHECK_LAUNCH();
    if (p.splits > 1) {
        splitk_reduce(wgrad_reduce_grid(n_out / 4), (const float*)workspace, p.splits, n_out, dw, accumulate, st);
        MG_CHECK_LAUNCH();
    }
    if (dbias) {
        const int rc = mg_colsum(dy, (long long)g->B * g->OH * g->OW, g->Co, dbias, accumulate, workspace,
                                 workspace_bytes, stream);
        if (rc != MG_OK) return rc;
    }
    return MG_OK;
}

}  // extern "C"
