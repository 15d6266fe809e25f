// K7 / K8 / K9: the small elementwise and layout passes: activation backward, sigmoid, add, pooling / upsampling,
// discriminator- and generator-input assembly, channel concatenation, the statistics finalize.  All HBM-bound grid-stride loops.
//
// Replaces (reference): ReLU / LeakyReLU(0.2) backward networks.py:306, :650-666; nn.Sigmoid :676-677;
// nn.AvgPool2d(3,2,1,count_include_pad=False) :249-250, :525-526; interpolate(nearest, x2) :396;
// cat(lr, s, 2|s|+nr0) pix2pixHD_model.py:420-424.
#include "act.h"

namespace {

__global__ void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx,
                               size_t n, int act, const float* __restrict__ dy2 = nullptr) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dx[i] = (dy2 ? dy[i] + dy2[i] : dy[i]) * act_grad_post(y[i], act);
}
// nn.Sigmoid (the PatchGAN output under --no_lsgan, networks.py:676-677): y = 1 / (1 + exp(-x)); backward dx = dy y (1 - y)
__global__ void sigmoid_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = 1.0f / (1.0f + expf(-x[i]));
}
__global__ void sigmoid_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dx[i] = dy[i] * (y[i] * (1.0f - y[i]));
}
__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        o[i] = a[i] + b[i];
}

// AvgPool2d(3, stride=2, padding=1, count_include_pad=False)
__global__ void avgpool_fwd_kernel(const float* __restrict__ x, int B, int H, int W, int C, int OH, int OW,
                                   float* __restrict__ y) {
    const size_t total = (size_t)B * OH * OW * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t r = i / C;
        const int ox = (int)(r % OW); r /= OW;
        const int oy = (int)(r % OH);
        const int b = (int)(r / OH);
        const int y0 = max(0, 2 * oy - 1), y1 = min(H - 1, 2 * oy + 1);
        const int x0 = max(0, 2 * ox - 1), x1 = min(W - 1, 2 * ox + 1);
        float s = 0.0f;
        for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) s += x[((size_t)(b * H + yy) * W + xx) * C + c];
        y[i] = s / (float)((y1 - y0 + 1) * (x1 - x0 + 1));
    }
}
__global__ void avgpool_bwd_kernel(const float* __restrict__ dy, int B, int H, int W, int C, int OH, int OW,
                                   float* __restrict__ dx) {
    const size_t total = (size_t)B * H * W * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t r = i / C;
        const int ix = (int)(r % W); r /= W;
        const int iy = (int)(r % H);
        const int b = (int)(r / H);
        float s = 0.0f;
        for (int oy = iy / 2; oy <= (iy + 1) / 2; ++oy) {
            if (oy >= OH) continue;
            const int ny = min(H - 1, 2 * oy + 1) - max(0, 2 * oy - 1) + 1;
            for (int ox = ix / 2; ox <= (ix + 1) / 2; ++ox) {
                if (ox >= OW) continue;
                const int nx = min(W - 1, 2 * ox + 1) - max(0, 2 * ox - 1) + 1;
                s += dy[((size_t)(b * OH + oy) * OW + ox) * C + c] / (float)(ny * nx);
            }
        }
        dx[i] = s;
    }
}

__global__ void upsample_fwd_kernel(const float* __restrict__ x, int B, int H, int W, int C, float* __restrict__ y) {
    const size_t total = (size_t)B * 2 * H * 2 * W * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t r = i / C;
        const int ox = (int)(r % (2 * W)); r /= (2 * W);
        const int oy = (int)(r % (2 * H));
        const int b = (int)(r / (2 * H));
        y[i] = x[((size_t)(b * H + oy / 2) * W + ox / 2) * C + c];
    }
}
__global__ void upsample_bwd_kernel(const float* __restrict__ dy, int B, int H, int W, int C, float* __restrict__ dx) {
    const size_t total = (size_t)B * H * W * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        size_t r = i / C;
        const int ix = (int)(r % W); r /= W;
        const int iy = (int)(r % H);
        const int b = (int)(r / H);
        const size_t o = ((size_t)(b * 2 * H + 2 * iy) * 2 * W + 2 * ix) * C + c;
        dx[i] = dy[o] + dy[o + C] + dy[o + (size_t)2 * W * C] + dy[o + (size_t)2 * W * C + C];
    }
}

__global__ void dinput_fwd_kernel(const float* __restrict__ lr, const float* __restrict__ s, size_t n, float nr0,
                                  float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = s[i];
        out[3 * i] = lr[i];
        out[3 * i + 1] = v;
        out[3 * i + 2] = fabsf(v) * 2.0f + nr0;
    }
}
__global__ void dinput_bwd_kernel(const float* __restrict__ g, const float* __restrict__ s, size_t n,
                                  float* __restrict__ ds) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = s[i];
        const float sg = (v > 0.0f) ? 1.0f : (v < 0.0f ? -1.0f : 0.0f);
        ds[i] = g[3 * i + 1] + 2.0f * sg * g[3 * i + 2];
    }
}
// torch.cat((a, b), dim=1) of NHWC tensors: out[p][0..Ca) = a[p], out[p][Ca..Ca+Cb) = b[p]; and its backward (a split)
__global__ void cat2_fwd_kernel(const float* __restrict__ a, int Ca, const float* __restrict__ b, int Cb, size_t n,
                                float* __restrict__ out) {
    const int Cc = Ca + Cb;
    const size_t total = n * Cc;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / Cc;
        const int c = (int)(i - p * Cc);
        out[i] = c < Ca ? a[p * Ca + c] : b[p * Cb + (c - Ca)];
    }
}
__global__ void cat2_bwd_kernel(const float* __restrict__ g, int Ca, int Cb, size_t n, float* __restrict__ ga,
                                float* __restrict__ gb) {
    const int Cc = Ca + Cb;
    const size_t total = n * Cc;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / Cc;
        const int c = (int)(i - p * Cc);
        if (c < Ca) { if (ga) ga[p * Ca + c] = g[i]; }
        else if (gb) gb[p * Cb + (c - Ca)] = g[i];
    }
}
__global__ void pair_fwd_kernel(const float* __restrict__ s, size_t n, float nr0, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = s[i];
        *reinterpret_cast<float2*>(out + 2 * i) = make_float2(v, fabsf(v) * 2.0f + nr0);
    }
}

// mean / unbiased std of a tensor from its {sum, sum of squares} (K1's statistics output): the float64 operations of
// (s0 / n).float(), ((s1 - s0 * s0 / n) / (n - 1)).clamp_min(0).sqrt().float() in one launch
__global__ void stats_finalize_kernel(const double* __restrict__ st, double n, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const double s0 = st[0], s1 = st[1];
        out[0] = (float)(s0 / n);
        double var = (s1 - s0 * s0 / n) / (n - 1.0);
        if (!(var > 0.0)) var = var != var ? var : 0.0;       // clamp_min(0) keeps nan
        out[1] = (float)sqrt(var);
    }
}

}  // namespace

extern "C" {

int mg_act_bwd(const float* dy, const float* y, float* dx, long long n, int act, void* stream) {
    return mg_act_bwd_add(dy, nullptr, y, dx, n, act, stream);
}
int mg_act_bwd_add(const float* dy, const float* dy2, const float* y, float* dx, long long n, int act, void* stream) {
    if (!dy || !y || !dx || n <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, dy, y, dx,
                       (size_t)n, act, dy2);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_add(const float* a, const float* b, float* out, long long n, void* stream) {
    if (!a || !b || !out || n <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(add_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, a, b, out, (size_t)n);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_avgpool3s2_fwd(const float* x, int B, int H, int W, int C, float* y, void* stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return MG_ERR_ARG;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(grid_for((size_t)B * OH * OW * C)), dim3(256), 0, (hipStream_t)stream,
                       x, B, H, W, C, OH, OW, y);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_avgpool3s2_bwd(const float* dy, int B, int H, int W, int C, float* dx, void* stream) {
    if (!dy || !dx || B <= 0 || H <= 0 || W <= 0 || C <= 0) return MG_ERR_ARG;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(grid_for((size_t)B * H * W * C)), dim3(256), 0, (hipStream_t)stream, dy,
                       B, H, W, C, OH, OW, dx);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_upsample2x_fwd(const float* x, int B, int H, int W, int C, float* y, void* stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(upsample_fwd_kernel, dim3(grid_for((size_t)B * 4 * H * W * C)), dim3(256), 0,
                       (hipStream_t)stream, x, B, H, W, C, y);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_upsample2x_bwd(const float* dy, int B, int H, int W, int C, float* dx, void* stream) {
    if (!dy || !dx || B <= 0 || H <= 0 || W <= 0 || C <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3(grid_for((size_t)B * H * W * C)), dim3(256), 0, (hipStream_t)stream,
                       dy, B, H, W, C, dx);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_dinput_fwd(const float* lr, const float* s, long long n, float nr0, float* out, void* stream) {
    if (!lr || !s || !out || n <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(dinput_fwd_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, lr, s,
                       (size_t)n, nr0, out);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_dinput_bwd(const float* dout, const float* s, long long n, float* ds, void* stream) {
    if (!dout || !s || !ds || n <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(dinput_bwd_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, dout, s,
                       (size_t)n, ds);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_cat2_fwd(const float* a, int Ca, const float* b, int Cb, long long n, float* out, void* stream) {
    if (!a || !b || !out || n <= 0 || Ca <= 0 || Cb <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(cat2_fwd_kernel, dim3(grid_for((size_t)n * (Ca + Cb))), dim3(256), 0, (hipStream_t)stream, a, Ca, b, Cb,
                       (size_t)n, out);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_cat2_bwd(const float* g, int Ca, int Cb, long long n, float* ga, float* gb, void* stream) {
    if (!g || (!ga && !gb) || n <= 0 || Ca <= 0 || Cb <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(cat2_bwd_kernel, dim3(grid_for((size_t)n * (Ca + Cb))), dim3(256), 0, (hipStream_t)stream, g, Ca, Cb,
                       (size_t)n, ga, gb);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_stats_finalize(const double* stats, long long n, float* mean_std, void* stream) {
    if (!stats || !mean_std || n < 2) return MG_ERR_ARG;
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, (double)n, mean_std);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_pair_fwd(const float* s, long long n, float nr0, float* out, void* stream) {
    if (!s || !out || n <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(pair_fwd_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, s, (size_t)n,
                       nr0, out);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_sigmoid_fwd(const float* x, float* y, long long n, void* stream) {
    if (!x || !y || n <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(sigmoid_fwd_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, x, y, (size_t)n);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
int mg_sigmoid_bwd(const float* dy, const float* y, float* dx, long long n, void* stream) {
    if (!dy || !y || !dx || n <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, (size_t)n);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"
