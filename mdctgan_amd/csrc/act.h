// The MG_ACT_* activations and their derivatives, as InstanceNorm (instnorm.hip) and the activation backward
// (elementwise.hip) apply them.
#pragma once
#include "common.h"
#include "mdctgan_hip.h"

__device__ __forceinline__ float act_fwd(float v, int act) {
    if (act == MG_ACT_RELU) return fmaxf(v, 0.0f);
    if (act == MG_ACT_LRELU02) return v > 0.0f ? v : 0.2f * v;
    if (act == MG_ACT_TANH) return tanhf(v);
    return v;
}
// derivative given the PRE-activation value
__device__ __forceinline__ float act_grad_pre(float pre, int act) {
    if (act == MG_ACT_RELU) return pre > 0.0f ? 1.0f : 0.0f;
    if (act == MG_ACT_LRELU02) return pre > 0.0f ? 1.0f : 0.2f;
    return 1.0f;
}
// derivative given the POST-activation value
__device__ __forceinline__ float act_grad_post(float y, int act) {
    if (act == MG_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
    if (act == MG_ACT_LRELU02) return y > 0.0f ? 1.0f : 0.2f;
    if (act == MG_ACT_TANH) return 1.0f - y * y;
    return 1.0f;
}
