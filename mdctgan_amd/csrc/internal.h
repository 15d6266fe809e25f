// Functions one translation unit of the library calls in another: not part of the C ABI (include/mdctgan_hip.h), hidden from the
// .so's exports.  The defining file and every caller include this header, so a signature that drifts does not compile.
// Needs: mdctgan_hip.h (mg_conv_geom).
#pragma once
#include <stddef.h>
#define MG_INTERNAL __attribute__((visibility("hidden")))
extern "C" {

// conv_rowdot.hip -> conv_igemm.hip (conv_route, the Co == 1 entry-point branches)
MG_INTERNAL int mg_conv_rowdot_kq(const mg_conv_geom* g);
MG_INTERNAL int mg_conv_rowdot_fwd(const mg_conv_geom* g, const float* x, const float* w, const float* bias, float* y, int act,
                                   void* stream);
MG_INTERNAL size_t mg_conv_rowdot_wgrad_workspace(const mg_conv_geom* g);
MG_INTERNAL int mg_conv_rowdot_wgrad(const mg_conv_geom* g, const float* x, const float* dy, float* dw, float* dbias,
                                     int accumulate, void* workspace, size_t workspace_bytes, void* stream);

// instnorm.hip -> conv_igemm.hip (mg_conv_fwd_instnorm_*): InstanceNorm straight from a convolution's split-K slabs
MG_INTERNAL int mg_instnorm_slab_ok(int HW, int C);
MG_INTERNAL int mg_instnorm_fwd_slabs(const float* part, int S, const float* bias, int round_f16, float* x_out, int B, int HW,
                                      int C, float eps, int act, const float* residual, float* y, float* mean, float* rstd,
                                      void* stream, void* y16);

// mdct.hip -> mdct_pow2.hip: the kernel name mg_mdct_last_kernel reports (which: 0 forward, 1 inverse)
MG_INTERNAL void mg_mdct_note_kernel(int which, const char* name);

}  // extern "C"
