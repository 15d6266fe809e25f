// The Adam update of one element, stated once for every kernel that applies it: adam_kernel, adam_dev_kernel and
// adam_seg_kernel (optim.hip) and the trunk's fused weight pass wino_adam_kernel (wino.h).  They are bit-identical to one
// another (tests/test_trunk_fused_gpu.py::test_wgrad_adam_fusion_is_bit_identical, tests/test_amp_gpu.py) because they all
// call this; the library is built with -ffp-contract=off, so inlining it fuses nothing.
#pragma once
#include <hip/hip_runtime.h>

// torch.optim.Adam (pix2pixHD_model.py:350-364) with step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step)
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, float gscale, float step_size,
                                            float bc2_sqrt, float b1, float b2, float eps) {
    const float gi = g * gscale;
    const float mi = m + (gi - m) * (1.0f - b1);           // lerp, as torch's exp_avg.lerp_(grad, 1-beta1)
    const float vi = v * b2 + (1.0f - b2) * gi * gi;       // mul_(beta2).addcmul_(g, g, 1-beta2)
    m = mi;
    v = vi;
    p = p - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
}
