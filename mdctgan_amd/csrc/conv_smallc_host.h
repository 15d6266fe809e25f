// Small-channel orchestration on the host (Ci <= 4): eligibility, plans, workspace layout and launches of the conv_smallc.h kernels.
// Needs: conv_smallc.h, conv_plan.h (to_geom, prec_h), wino_host.h (al256).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------------------
// Ci <= 4 layers (conv_smallc.h): VALU kernels for the data gradient and the weight gradient
// ---------------------------------------------------------------------------------------------------------
bool smallc_dgrad_ok(const mg_conv_geom* g) {
    const int s = g->stride;       // the class's weights sit in LDS: taps x Co float4s
    return g->Ci >= 1 && g->Ci <= 4 && !g->reflect && g->Co % 4 == 0 && g->Co >= 16 &&
           (size_t)((g->KH + s - 1) / s) * ((g->KW + s - 1) / s) * g->Co * 16 <= 60 * 1024;
}
// 0: not eligible; otherwise the template instance id
int smallc_wgrad_kind(const mg_conv_geom* g) {
    if (g->Co < 16 || ((g->stride * g->Ci) & 1)) return 0;
    if ((size_t)g->KH * (((g->OW - 1) * g->stride + g->KW) * g->Ci + 4) * sizeof(float) > 60000) return 0;
    if ((long long)g->B * g->OH > 65535LL * 32) return 0;
    if (g->KH == 4 && g->KW == 4 && g->Ci == 3) return 1;
    if (g->KH == 7 && g->KW == 7 && g->Ci == 2) return 2;
    if (g->KH == 3 && g->KW == 3 && g->Ci == 4) return 3;
    return 0;
}
// even stride * Ci keeps every pixel's patch segment 8-byte aligned in the staged rows
struct SmallcWgradPlan { int wgs, rowlen; size_t lds; int mfma_g; };     // wgs: partial rows; mfma_g: 0 or the MFMA kernel's pixel groups
// the MFMA form (conv_smallc_wgrad_mfma_kernel): pixel groups per output row (each writes a partial row), 0 = VALU kernel
int smallc_wgrad_mfma_groups(const mg_conv_geom* g, int rowlen) {
    if ((size_t)g->KH * rowlen > 256 * 16 || g->Co % 64 != 0) return 0;
    if (g->KH == 7 && g->KW == 7 && g->Ci == 2 && g->stride == 1) return 1;     // K = 98: four k blocks, one per wave
    if (g->KH == 4 && g->KW == 4 && g->Ci == 3 && g->stride == 2) return 2;     // K = 48: two k blocks x two pixel groups
    return 0;
}
SmallcWgradPlan smallc_wgrad_plan(const mg_conv_geom* g) {
    const int ncols = (g->OW - 1) * g->stride + g->KW;
    const int rowlen = (ncols * g->Ci + 3) / 4 * 4;
    const int mg = smallc_wgrad_mfma_groups(g, rowlen);
    return {g->B * g->OH * (mg ? mg : 1), rowlen, (size_t)g->KH * rowlen * sizeof(float), mg};
}
// workspace: per-row partials | column-sum scratch of their reduction | column-sum scratch of the bias gradient
struct SmallcWs { size_t part, red, cs, total; };      // float offsets / counts
SmallcWs smallc_wgrad_layout(const mg_conv_geom* g) {
    const SmallcWgradPlan p = smallc_wgrad_plan(g);
    const size_t n = (size_t)g->Co * g->KH * g->KW * g->Ci;
    SmallcWs w;
    w.part = 0;
    w.red = al256((size_t)p.wgs * n);
    w.cs = w.red + al256((mg_colsum_workspace(p.wgs, (int)n) + 255) / 4);
    w.total = w.cs + al256((mg_colsum_workspace((long long)g->B * g->OH * g->OW, g->Co) + 255) / 4);
    return w;
}
size_t smallc_wgrad_ws(const mg_conv_geom* g) { return smallc_wgrad_layout(g).total * sizeof(float) + 256; }
int smallc_wgrad(const mg_conv_geom* g, const float* x, const float* dy, float* dw, int accumulate, float* ws,
                 hipStream_t st) {
    const SmallcWgradPlan p = smallc_wgrad_plan(g);
    const SmallcWs lay = smallc_wgrad_layout(g);
    const Geom gg = to_geom(g);
    const dim3 grid((unsigned)(g->B * g->OH), (unsigned)((g->Co + 63) / 64));
    if (p.mfma_g) {
        const size_t lds = p.lds + 16;               // + the zeroed slot the k >= K lanes read
        if (g->KH == 7) hipLaunchKernelGGL((conv_smallc_wgrad_mfma_kernel<7, 7, 2, 1>), grid, dim3(256), lds, st, gg, x, dy, ws, p.rowlen, (int)prec_h(g));
        else hipLaunchKernelGGL((conv_smallc_wgrad_mfma_kernel<4, 4, 3, 2>), grid, dim3(256), lds, st, gg, x, dy, ws, p.rowlen, (int)prec_h(g));
    } else
    switch (smallc_wgrad_kind(g)) {
    case 1: hipLaunchKernelGGL((conv_smallc_wgrad_kernel<4, 4, 3>), grid, dim3(256), p.lds, st, gg, x, dy, ws, p.rowlen, (int)prec_h(g)); break;
    case 2: hipLaunchKernelGGL((conv_smallc_wgrad_kernel<7, 7, 2>), grid, dim3(448), p.lds, st, gg, x, dy, ws, p.rowlen, (int)prec_h(g)); break;
    case 3: hipLaunchKernelGGL((conv_smallc_wgrad_kernel<3, 3, 4>), grid, dim3(192), p.lds, st, gg, x, dy, ws, p.rowlen, (int)prec_h(g)); break;
    default: return MG_ERR_UNSUPPORTED;
    }
    MG_CHECK_LAUNCH();
    const size_t n = (size_t)g->Co * g->KH * g->KW * g->Ci;
    return mg_colsum(ws, p.wgs, (int)n, dw, accumulate, ws + lay.red, mg_colsum_workspace(p.wgs, (int)n), st);
}
// forward on the MFMA pipe (conv_smallc_fwd_kernel): 0 = not eligible, else the template instance
int smallc_fwd_kind(const mg_conv_geom* g) {
    if (g->Co % 64 != 0 || (long long)g->B * g->OH > 0x7fffffffLL) return 0;
    if ((size_t)g->KH * (((g->OW - 1) * g->stride + g->KW) * g->Ci + 4) > 256 * 16) return 0;      // staged through 16 registers per thread
    if (g->KH == 7 && g->KW == 7 && g->Ci == 2 && g->stride == 1) return 1;      // the generator stem: 66 against 93 us
    // (the 3 -> 64 4x4 stride-2 first discriminator layer -- K = 48, 129-pixel rows = 5 pixel blocks for 4 waves -- measured
    // SLOWER here than on the generic kernel: 44 against 37 us at batch 16)
    return 0;
}
int smallc_fwd(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y, int act, hipStream_t st) {
    const SmallcWgradPlan p = smallc_wgrad_plan(g);     // the same staged rows
    const Geom gg = to_geom(g);
    const int rows = g->B * g->OH, cblocks = (g->Co + 63) / 64;
    int rpw = 1;       // rows per workgroup (the weights' LDS image is paid once per workgroup): ~4 resident workgroups per CU (81 VGPRs, 40 KB)
    while ((long long)((rows + rpw - 1) / rpw) * cblocks > 1024 && rpw < 8) ++rpw;
    const dim3 grid((unsigned)((rows + rpw - 1) / rpw), (unsigned)cblocks);
    const size_t lds = p.lds + (size_t)64 * ((g->KH * g->KW * g->Ci) | 1) * sizeof(float);
    if (smallc_fwd_kind(g) != 1) return MG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((conv_smallc_fwd_kernel<7, 7, 2, 1>), grid, dim3(256), lds, st, gg, x, w, bias, y, act, p.rowlen, rpw, (int)prec_h(g));
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int smallc_dgrad(const mg_conv_geom* g, const float* dy, const float* w, float* dx, hipStream_t st) {
    const Geom gg = to_geom(g);
    const int s = g->stride;
    const long long Mc = (long long)g->B * ((g->H + s - 1) / s) * ((g->W + s - 1) / s);
    const dim3 grid((unsigned)((Mc + 255) / 256), (unsigned)(s * s));
    // the heaviest class's taps x Co float4s of weights in LDS
    const size_t wl_bytes = (size_t)((g->KH + s - 1) / s) * ((g->KW + s - 1) / s) * g->Co * 16;
#define MG_SMALLC_DG(CI_) do { \
        if (prec_h(g)) hipLaunchKernelGGL((conv_smallc_dgrad_kernel<CI_, true>), grid, dim3(256), wl_bytes, st, gg, dy, w, dx); \
        else hipLaunchKernelGGL((conv_smallc_dgrad_kernel<CI_, false>), grid, dim3(256), wl_bytes, st, gg, dy, w, dx); } while (0)
    switch (g->Ci) {
    case 1: MG_SMALLC_DG(1); break;
    case 2: MG_SMALLC_DG(2); break;
    case 3: MG_SMALLC_DG(3); break;
    default: MG_SMALLC_DG(4); break;
    }
#undef MG_SMALLC_DG
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // namespace
