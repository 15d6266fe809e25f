// K10: the bottleneck-transformer block pieces that are not 1x1 convolutions (those run on conv_igemm.hip):
// BatchNorm2d (training statistics + running buffers, affine, fused ReLU / residual) and multi-head self
// attention with absolute position embeddings, forward and backward, float32.
//
// Reference call sites: models/networks.py:232-235, 341-344 (BottleStack(..., downsample=False,
// rel_pos_emb=False) from bottleneck_transformer_pytorch==0.1.4, a third-party package that is not vendored by the
// reference; restated from its published algorithm -- parity UNPINNED):
//     q, k, v = to_qkv(x).chunk(3);  q *= dim_head^-0.5
//     sim = q k^T + q (h_emb (+) w_emb)^T  ==  q (k + e)^T ;  out = softmax(sim) v
// Token counts are tiny (32 at 4x8, 128 at 8x16), so up to 128 tokens this is a latency-bound VALU kernel: one workgroup
// per (sample, head) keeps K+E and V in LDS; the FLOPs are < 0.01 % of the step.
// 129 to 256 tokens (256 at 8x32: the n_fft-1024 map, and at 16x16: 256 frames of n_fft 512) no longer fit two [n][d+1]
// operands into a CU's LDS; they run on the "wide" family below (attn_wide_*): one workgroup per (sample, head, block of 32
// queries), every contraction on the exact-float32 MFMA, 38 KB of LDS.  More than 256 tokens are rejected.
#include "common.h"
#include "mdctgan_hip.h"

namespace {

__device__ __forceinline__ float act_fwd(float v, int act) {
    if (act == MG_ACT_RELU) return fmaxf(v, 0.0f);
    return v;
}

// ------------------------------------------------------------------------------------------------------------
// BatchNorm2d over rows = B*H*W of an NHWC tensor [R, C], as sums -> apply (round 3).  The one-launch kernels of rounds
// 1-2 ran 8 workgroups for the 512-channel layers of configs[2] (40 / 69 us forward / backward, latency-bound); now the rows
// are cut into BN_RS slices: a sums kernel writes per-slice double-precision partials [BN_RS][2][C] (fixed-order, no atomics)
// and the apply kernel adds them in slice order.  Between the two launches a data-parallel run may all-reduce the partials
// (SyncBN, SURVEY 8e opt-in): the apply kernels take the statistics' row count separately from the local R.
// ------------------------------------------------------------------------------------------------------------
constexpr int BN_RS = 8;

// which == 0: (sum x, sum x^2);  which == 1: (sum g, sum g * xhat) with g = dy masked by the ReLU of y
template <int BWD>
__global__ __launch_bounds__(256) void bn_sums_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                      const float* __restrict__ y, int R, int C,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd, int act,
                                                      double* __restrict__ part) {
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl, sl = blockIdx.y;
    const int r0 = (int)((long long)R * sl / BN_RS), r1 = (int)((long long)R * (sl + 1) / BN_RS);
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        const float mu = BWD ? mean[c] : 0.f, rs = BWD ? rstd[c] : 0.f;
        for (int r = r0 + rg; r < r1; r += 4) {
            const size_t i = (size_t)r * C + c;
            if (BWD) {
                float g = dy[i];
                if (act == MG_ACT_RELU && !(y[i] > 0.0f)) g = 0.0f;
                s1 += (double)g;
                s2 += (double)g * (double)((x[i] - mu) * rs);
            } else {
                const float v = x[i];
                s1 += (double)v;
                s2 += (double)v * (double)v;
            }
        }
    }
    red[0][rg][cl] = s1;
    red[1][rg][cl] = s2;
    __syncthreads();
    if (rg == 0 && c < C) {
        part[((size_t)sl * 2 + 0) * C + c] = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
        part[((size_t)sl * 2 + 1) * C + c] = (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]);
    }
}
__device__ __forceinline__ void bn_total(const double* __restrict__ part, int C, int c, double& a, double& b) {
    a = 0.0; b = 0.0;
#pragma unroll
    for (int s = 0; s < BN_RS; ++s) { a += part[((size_t)s * 2 + 0) * C + c]; b += part[((size_t)s * 2 + 1) * C + c]; }
}

__global__ __launch_bounds__(256) void bn_apply_fwd_kernel(const float* __restrict__ x, int R, int C, float eps,
                                                           float momentum, int training, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ run_mean,
                                                           float* __restrict__ run_var, const float* __restrict__ residual,
                                                           int act, float* __restrict__ y, float* __restrict__ save_mean,
                                                           float* __restrict__ save_rstd, const double* __restrict__ part,
                                                           double count) {
    // stat[2]: what float32 dropped from the batch mean.  x - mean is exact for x near the mean, so with the remainder taken
    // off as well xhat keeps float32 accuracy however far the data sit from zero (at mean = 1e4 sigma the rounding of the mean
    // alone moved xhat by 4e-4 and with it ReLU decisions at |z| ~ 1e-5 max|z|; found by the offset case of
    // tests/test_bot_attn_gpu.py).  save_mean, the running buffers and the backward pass keep the float32 mean.
    __shared__ float stat[3][64];
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl, sl = blockIdx.y;
    if (rg == 0 && c < C) {
        if (training) {
            double a, b;
            bn_total(part, C, c, a, b);
            const double mu = a / count;
            double var = b / count - mu * mu;
            if (var < 0.0) var = 0.0;
            stat[0][cl] = (float)mu;
            stat[2][cl] = (float)(mu - (double)stat[0][cl]);
            stat[1][cl] = (float)(1.0 / sqrt(var + (double)eps));
            if (sl == 0) {
                save_mean[c] = stat[0][cl];
                save_rstd[c] = stat[1][cl];
                if (run_mean) {   // nn.BatchNorm2d: running = (1-m) running + m batch (unbiased variance)
                    const double unb = (count > 1.0) ? var * count / (count - 1.0) : var;
                    run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * (float)mu;
                    run_var[c] = (1.0f - momentum) * run_var[c] + momentum * (float)unb;
                }
            }
        } else {
            stat[0][cl] = run_mean[c];
            stat[1][cl] = 1.0f / sqrtf(run_var[c] + eps);
            stat[2][cl] = 0.0f;
            if (sl == 0 && save_mean) { save_mean[c] = stat[0][cl]; save_rstd[c] = stat[1][cl]; }
        }
    }
    __syncthreads();
    if (c >= C) return;
    const int r0 = (int)((long long)R * sl / BN_RS), r1 = (int)((long long)R * (sl + 1) / BN_RS);
    const float mu = stat[0][cl], rs = stat[1][cl], lo = stat[2][cl], ga = gamma ? gamma[c] : 1.0f, be = beta ? beta[c] : 0.0f;
    for (int r = r0 + rg; r < r1; r += 4) {
        const size_t i = (size_t)r * C + c;
        float z = ga * (((x[i] - mu) - lo) * rs) + be;
        if (residual) z += residual[i];
        y[i] = act_fwd(z, act);
    }
}

// dy -> dx, dgamma, dbeta (+ dresidual = masked dy).  y is the forward output (ReLU mask).  lpart: this rank's sums (the
// parameter gradients, reduced later with every other gradient); gpart: the sums over the statistics' batch (== lpart
// unless SyncBN all-reduced them), count = its row count.
__global__ __launch_bounds__(256) void bn_apply_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ y, int R, int C,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, int act, int training,
                                                           float* __restrict__ dx, float* __restrict__ dres,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           int accumulate, const double* __restrict__ lpart,
                                                           const double* __restrict__ gpart, double count) {
    __shared__ float stat[2][64];
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl, sl = blockIdx.y;
    if (rg == 0 && c < C) {
        double a, b;
        bn_total(gpart, C, c, a, b);
        stat[0][cl] = (float)(a / count);
        stat[1][cl] = (float)(b / count);
        if (sl == 0 && (dbeta || dgamma)) {
            bn_total(lpart, C, c, a, b);
            if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)a : (float)a;
            if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)b : (float)b;
        }
    }
    __syncthreads();
    if (c >= C) return;
    const int r0 = (int)((long long)R * sl / BN_RS), r1 = (int)((long long)R * (sl + 1) / BN_RS);
    const float mu = mean[c], rs = rstd[c], ga = gamma ? gamma[c] : 1.0f;
    const float m1 = stat[0][cl], m2 = stat[1][cl];
    for (int r = r0 + rg; r < r1; r += 4) {
        const size_t i = (size_t)r * C + c;
        float g = dy[i];
        if (act == MG_ACT_RELU && !(y[i] > 0.0f)) g = 0.0f;
        if (dres) dres[i] = g;
        const float xh = (x[i] - mu) * rs;
        dx[i] = training ? rs * ga * (g - m1 - xh * m2) : rs * ga * g;
    }
}

// ------------------------------------------------------------------------------------------------------------
// attention.  qkv [B, n, 3*HD] (NHWC of the to_qkv conv, channel = which*HD + head*d + dd), n = fh*fw tokens.
// One workgroup per (b, head).  LDS: KE [n][d+1] = k + (height[y] + width[x]), V [n][d+1], P row scratch.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ eh,
                                                       const float* __restrict__ ew, int n, int fw, int heads, int d,
                                                       float scale, float* __restrict__ out, float* __restrict__ P) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int ld = d + 1, HD = heads * d;
    float* ke = sm;                 // [n][ld]
    float* vv = ke + n * ld;        // [n][ld]
    float* pr = vv + n * ld;        // [4 waves][n]  softmax row per wave
    float* qs = pr + 4 * n;         // [4 waves][d]  scaled query per wave
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* base = qkv + (size_t)b * n * 3 * HD;
    for (int i = threadIdx.x; i < n * d; i += 256) {
        const int j = i / d, dd = i % d;
        const float e = eh[(j / fw) * d + dd] + ew[(j % fw) * d + dd];
        ke[j * ld + dd] = base[(size_t)j * 3 * HD + HD + h * d + dd] + e;
        vv[j * ld + dd] = base[(size_t)j * 3 * HD + 2 * HD + h * d + dd];
    }
    __syncthreads();
    // gridDim.y workgroups share a (sample, head): each stages K / V for itself and takes every gridDim.y-th group of four queries
    for (int i = 4 * blockIdx.y + wave; i < n; i += 4 * gridDim.y) {              // query i handled by one wave
        for (int dd = lane; dd < d; dd += 64) qs[wave * d + dd] = base[(size_t)i * 3 * HD + h * d + dd] * scale;
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        float s[2];                                   // keys lane, lane + 64
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            float a = -INFINITY;
            if (j < n) {
                a = 0.0f;
                for (int dd = 0; dd < d; ++dd) a = fmaf(qs[wave * d + dd], ke[j * ld + dd], a);
            }
            s[t] = a;
            mx = fmaxf(mx, a);
        }
        mx = wave_max(mx);
        float sum = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            s[t] = (lane + 64 * t < n) ? expf(s[t] - mx) : 0.0f;
            sum += s[t];
        }
        sum = wave_sum(sum);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            if (j < n) {
                const float p = s[t] * inv;
                pr[wave * n + j] = p;
                P[(((size_t)b * heads + h) * n + i) * n + j] = p;
            }
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        for (int dd = lane; dd < d; dd += 64) {
            float o = 0.0f;
            for (int j = 0; j < n; ++j) o = fmaf(pr[wave * n + j], vv[j * ld + dd], o);
            out[((size_t)b * n + i) * HD + h * d + dd] = o;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// backward, part A: dV = P^T dO, dS = P .* (dP - rowsum(P .* dP)), dP = dO V^T.  LDS: dO [n][ld], V [n][ld].
__global__ __launch_bounds__(256) void attn_bwd_a_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                         const float* __restrict__ P, int n, int heads, int d,
                                                         float* __restrict__ dqkv, float* __restrict__ dS) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int ld = d + 1, HD = heads * d;
    float* dos = sm;               // [n][ld]
    float* vv = dos + n * ld;      // [n][ld]
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* base = qkv + (size_t)b * n * 3 * HD;
    const float* Pb = P + ((size_t)b * heads + h) * n * n;
    float* dSb = dS + ((size_t)b * heads + h) * n * n;
    for (int i = threadIdx.x; i < n * d; i += 256) {
        const int j = i / d, dd = i % d;
        dos[j * ld + dd] = dout[((size_t)b * n + j) * HD + h * d + dd];
        vv[j * ld + dd] = base[(size_t)j * 3 * HD + 2 * HD + h * d + dd];
    }
    __syncthreads();
    for (int i = 4 * blockIdx.y + wave; i < n; i += 4 * gridDim.y) {              // row i of dS
        float dp[2], pv[2], dot = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            dp[t] = 0.0f;
            pv[t] = 0.0f;
            if (j < n) {
                float a = 0.0f;
                for (int dd = 0; dd < d; ++dd) a = fmaf(dos[i * ld + dd], vv[j * ld + dd], a);
                dp[t] = a;
                pv[t] = Pb[(size_t)i * n + j];
                dot += pv[t] * a;
            }
        }
        dot = wave_sum(dot);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            if (j < n) dSb[(size_t)i * n + j] = pv[t] * (dp[t] - dot);
        }
    }
    // dV[j][dd] = sum_i P[i][j] dO[i][dd]
    for (int idx = 256 * blockIdx.y + threadIdx.x; idx < n * d; idx += 256 * gridDim.y) {
        const int j = idx / d, dd = idx % d;
        float a = 0.0f;
        for (int i = 0; i < n; ++i) a = fmaf(Pb[(size_t)i * n + j], dos[i * ld + dd], a);
        dqkv[((size_t)b * n + j) * 3 * HD + 2 * HD + h * d + dd] = a;
    }
}

// backward, part B: dq = scale * dS KE, dKE = dS^T q' (q' = scale * q) -> dk, and the embedding gradient partials
// dE[b, h][j][dd] = dKE (summed over (b, h) per (y | x) by a later pass).  LDS: KE [n][ld], Q' [n][ld].
__global__ __launch_bounds__(256) void attn_bwd_b_kernel(const float* __restrict__ qkv, const float* __restrict__ eh,
                                                         const float* __restrict__ ew, const float* __restrict__ dS,
                                                         int n, int fw, int heads, int d, float scale,
                                                         float* __restrict__ dqkv, float* __restrict__ dE) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int ld = d + 1, HD = heads * d;
    float* ke = sm;
    float* qq = ke + n * ld;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const float* base = qkv + (size_t)b * n * 3 * HD;
    const float* dSb = dS + ((size_t)b * heads + h) * n * n;
    for (int i = threadIdx.x; i < n * d; i += 256) {
        const int j = i / d, dd = i % d;
        const float e = eh[(j / fw) * d + dd] + ew[(j % fw) * d + dd];
        ke[j * ld + dd] = base[(size_t)j * 3 * HD + HD + h * d + dd] + e;
        qq[j * ld + dd] = base[(size_t)j * 3 * HD + h * d + dd] * scale;
    }
    __syncthreads();
    for (int idx = 256 * blockIdx.y + threadIdx.x; idx < n * d; idx += 256 * gridDim.y) {
        const int i = idx / d, dd = idx % d;
        float aq = 0.0f, ak = 0.0f;
        for (int j = 0; j < n; ++j) {
            aq = fmaf(dSb[(size_t)i * n + j], ke[j * ld + dd], aq);      // dq'_i
            ak = fmaf(dSb[(size_t)j * n + i], qq[j * ld + dd], ak);      // dKE_i = sum_j dS[j][i] q'_j
        }
        dqkv[((size_t)b * n + i) * 3 * HD + h * d + dd] = aq * scale;
        dqkv[((size_t)b * n + i) * 3 * HD + HD + h * d + dd] = ak;
        dE[(((size_t)b * heads + h) * n + i) * d + dd] = ak;
    }
}

// ------------------------------------------------------------------------------------------------------------
// attention, 128 < n <= 256: the "wide" family.  Same algorithm, same buffers; one workgroup (4 waves) per (b, head, block of
// AW_Q = 32 rows), every contraction as 32x32 tiles of v_mfma_f32_32x32x2_f32 (a float32 fmaf chain in k order: exact float32,
// fixed order).  P and dS live in HBM anyway, so a pass is a sequence of phases around one LDS tile st [32][257]:
//   scores   st = X[32 rows][d] Y[n][d]^T      X, Y staged in feature chunks of 32 (xt [32][33], yt [256][33]; st reuses yt);
//                                              wave w owns key tiles w and w + 4
//   rows     softmax (forward) / dS = P .* (dP - rowsum(P .* dP)) (backward A): wave w owns rows 8w .. 8w + 7, a lane keys
//            lane + 64 t as in the narrow kernels; the result goes to HBM and, forward, back into st
//   apply    O[32 rows][d] = st Y[n][d]        wave w owns features 32w .. 32w + 31; Y straight from HBM (a row of Y is read
//                                              by one wave, once: nothing to share through LDS), loads one batch ahead
//   tn       O[32 keys][d] = M[n][n]^T Y[n][d] (dV = P^T dO, dKE = dS^T Q'): both operands straight from HBM, lanes along a
//                                              row of M / of Y
// Rows, keys and features past n / d are staged as zeros or read at a clamped index into a tile row / column that is never
// written out.  LDS: (256 + 32) * 33 floats = 38 KB, static: no raised limit, four workgroups fit a CU.
// A block's bits depend on (b, head, block) alone, never on the grid: a sample alone has the bits it has in a batch.
// ------------------------------------------------------------------------------------------------------------
constexpr int AW_Q = 32;                 // rows per workgroup
constexpr int AW_N = 256;                // most tokens
constexpr int AW_LS = AW_N + 1;          // row stride of st
constexpr int AW_LC = 32 + 1;            // row stride of a staged feature chunk
constexpr int AW_U = 8;                  // k steps per batch of HBM operand loads

// st[32][AW_LS] = X[i0 .. i0 + 31][d] * xscale  x  (Y[n][d] (+ E))^T.  xt [32][AW_LC], yt [AW_N][AW_LC]; st may be yt.
template <bool EMB>
__device__ __forceinline__ void aw_scores(const float* __restrict__ xg, size_t xs, float xscale, int i0,
                                          const float* __restrict__ yg, size_t ys, const float* __restrict__ eh,
                                          const float* __restrict__ ew, int fw, int n, int d, float* xt, float* yt, float* st) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nk = (n + 31) >> 5;
    const int lr = lane & 31, lh = lane >> 5;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    for (int d0 = 0; d0 < d; d0 += 32) {
        for (int idx = threadIdx.x; idx < AW_Q * 32; idx += 256) {
            const int r = idx >> 5, c = idx & 31, i = i0 + r, dd = d0 + c;
            xt[r * AW_LC + c] = (i < n && dd < d) ? xg[(size_t)i * xs + dd] * xscale : 0.0f;
        }
        for (int idx = threadIdx.x; idx < nk * 32 * 32; idx += 256) {
            const int j = idx >> 5, c = idx & 31, dd = d0 + c;
            float v = 0.0f;
            if (j < n && dd < d) {
                v = yg[(size_t)j * ys + dd];
                if (EMB) v += eh[(j / fw) * d + dd] + ew[(j % fw) * d + dd];
            }
            yt[j * AW_LC + c] = v;
        }
        __syncthreads();
        const int kmax = min(32, (d - d0 + 1) & ~1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int kt = wave + 4 * t;
            if (kt < nk)
                for (int k = 0; k < kmax; k += 2)
                    acc[t] = mfma32x32x2(xt[lr * AW_LC + k + lh], yt[(kt * 32 + lr) * AW_LC + k + lh], acc[t]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int kt = wave + 4 * t;
        if (kt < nk)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[mfma32_row(r, lane) * AW_LS + kt * 32 + lr] = acc[t][r];
    }
    __syncthreads();
}

// acc (this wave's features 32 * wave + (lane & 31), rows mfma32_row) = st[32][n] (Y[n][d] (+ E)).  st is zero in columns
// n .. 255; et (EMB): [j] = (j / fw) * d, [AW_N + j] = (j % fw) * d.  Returns false for a wave without features.
template <bool EMB>
__device__ __forceinline__ bool aw_apply(const float* st, const float* __restrict__ yg, size_t ys,
                                         const float* __restrict__ eh, const float* __restrict__ ew, const int* et, int n, int d,
                                         f32x16& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 31, lh = lane >> 5;
    if (32 * wave >= d) return false;
    const int ddc = min(32 * wave + lr, d - 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    float yn[AW_U], hn[AW_U], wn[AW_U];
    auto load = [&](int k) {
#pragma unroll
        for (int u = 0; u < AW_U; ++u) {
            const int j = min(k + 2 * u + lh, n - 1);
            yn[u] = yg[(size_t)j * ys + ddc];
            if (EMB) { hn[u] = eh[et[j] + ddc]; wn[u] = ew[et[AW_N + j] + ddc]; }
        }
    };
    load(0);
    for (int k = 0; k < n; k += 2 * AW_U) {
        float yc[AW_U];
#pragma unroll
        for (int u = 0; u < AW_U; ++u) yc[u] = EMB ? yn[u] + (hn[u] + wn[u]) : yn[u];
        load(k + 2 * AW_U);
#pragma unroll
        for (int u = 0; u < AW_U; ++u) acc = mfma32x32x2(st[lr * AW_LS + k + 2 * u + lh], yc[u], acc);
    }
    return true;
}

// acc (features 32 * wave + (lane & 31), keys j0 + mfma32_row) = M[n][n]^T[j0 .. j0 + 31] (Y[n][d] * yscale)
__device__ __forceinline__ bool aw_tn(const float* __restrict__ M, const float* __restrict__ yg, size_t ys, float yscale,
                                      int j0, int n, int d, f32x16& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 31, lh = lane >> 5;
    if (32 * wave >= d) return false;
    const int ddc = min(32 * wave + lr, d - 1), jc = min(j0 + lr, n - 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    float mn[AW_U], yn[AW_U];
    auto load = [&](int k) {
#pragma unroll
        for (int u = 0; u < AW_U; ++u) {
            const int i = k + 2 * u + lh, ic = min(i, n - 1);
            mn[u] = i < n ? M[(size_t)ic * n + jc] : 0.0f;
            yn[u] = yg[(size_t)ic * ys + ddc];
        }
    };
    load(0);
    for (int k = 0; k < n; k += 2 * AW_U) {
        float mc[AW_U], yc[AW_U];
#pragma unroll
        for (int u = 0; u < AW_U; ++u) { mc[u] = mn[u]; yc[u] = yn[u] * yscale; }
        load(k + 2 * AW_U);
#pragma unroll
        for (int u = 0; u < AW_U; ++u) acc = mfma32x32x2(mc[u], yc[u], acc);
    }
    return true;
}

__global__ __launch_bounds__(256) void attn_wide_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ eh,
                                                            const float* __restrict__ ew, int n, int fw, int heads, int d,
                                                            float scale, float* __restrict__ out, float* __restrict__ P) {
    __shared__ float yt[AW_N * AW_LC];
    __shared__ float xt[AW_Q * AW_LC];
    float* st = yt;                 // [32][AW_LS] <= [256][33]
    const int HD = heads * d, b = blockIdx.x / heads, h = blockIdx.x % heads, i0 = AW_Q * blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* base = qkv + (size_t)b * n * 3 * HD + h * d;
    aw_scores<true>(base, (size_t)3 * HD, scale, i0, base + HD, (size_t)3 * HD, eh, ew, fw, n, d, xt, yt, st);
    float* Pb = P + ((size_t)b * heads + h) * n * n;
    for (int r = 8 * wave; r < 8 * wave + 8; ++r) {
        const int i = i0 + r;
        if (i >= n) break;
        float s[4], mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = lane + 64 * t;
            s[t] = j < n ? st[r * AW_LS + j] : -INFINITY;
            mx = fmaxf(mx, s[t]);
        }
        mx = wave_max(mx);
        float sum = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = (lane + 64 * t < n) ? expf(s[t] - mx) : 0.0f;
            sum += s[t];
        }
        sum = wave_sum(sum);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = lane + 64 * t;
            const float p = s[t] * inv;                 // 0 past n: apply's clamped loads meet it there
            st[r * AW_LS + j] = p;
            if (j < n) Pb[(size_t)i * n + j] = p;
        }
    }
    __syncthreads();
    f32x16 acc;
    if (aw_apply<false>(st, base + 2 * HD, (size_t)3 * HD, nullptr, nullptr, nullptr, n, d, acc)) {
        const int dd = 32 * wave + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + mfma32_row(r, lane);
            if (i < n && dd < d) out[((size_t)b * n + i) * HD + h * d + dd] = acc[r];
        }
    }
}

// backward, part A: dS rows i0 .. i0 + 31 and dV of keys i0 .. i0 + 31
__global__ __launch_bounds__(256) void attn_wide_bwd_a_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                              const float* __restrict__ P, int n, int heads, int d,
                                                              float* __restrict__ dqkv, float* __restrict__ dS) {
    __shared__ float yt[AW_N * AW_LC];
    __shared__ float xt[AW_Q * AW_LC];
    float* st = yt;
    const int HD = heads * d, b = blockIdx.x / heads, h = blockIdx.x % heads, i0 = AW_Q * blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* vb = qkv + (size_t)b * n * 3 * HD + 2 * HD + h * d;
    const float* dob = dout + (size_t)b * n * HD + h * d;
    const float* Pb = P + ((size_t)b * heads + h) * n * n;
    float* dSb = dS + ((size_t)b * heads + h) * n * n;
    aw_scores<false>(dob, (size_t)HD, 1.0f, i0, vb, (size_t)3 * HD, nullptr, nullptr, 1, n, d, xt, yt, st);      // dP
    for (int r = 8 * wave; r < 8 * wave + 8; ++r) {
        const int i = i0 + r;
        if (i >= n) break;
        float dp[4], pv[4], dot = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = lane + 64 * t;
            dp[t] = 0.0f;
            pv[t] = 0.0f;
            if (j < n) {
                dp[t] = st[r * AW_LS + j];
                pv[t] = Pb[(size_t)i * n + j];
                dot += pv[t] * dp[t];
            }
        }
        dot = wave_sum(dot);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = lane + 64 * t;
            if (j < n) dSb[(size_t)i * n + j] = pv[t] * (dp[t] - dot);
        }
    }
    f32x16 acc;
    if (aw_tn(Pb, dob, (size_t)HD, 1.0f, i0, n, d, acc)) {
        const int dd = 32 * wave + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = i0 + mfma32_row(r, lane);
            if (j < n && dd < d) dqkv[((size_t)b * n + j) * 3 * HD + 2 * HD + h * d + dd] = acc[r];
        }
    }
}

// backward, part B: dq of rows i0 .. i0 + 31 (scale * dS KE), dk and the dE partials of keys i0 .. i0 + 31 (dS^T Q')
__global__ __launch_bounds__(256) void attn_wide_bwd_b_kernel(const float* __restrict__ qkv, const float* __restrict__ eh,
                                                              const float* __restrict__ ew, const float* __restrict__ dS,
                                                              int n, int fw, int heads, int d, float scale,
                                                              float* __restrict__ dqkv, float* __restrict__ dE) {
    __shared__ float st[AW_Q * AW_LS];
    __shared__ int et[2 * AW_N];
    const int HD = heads * d, b = blockIdx.x / heads, h = blockIdx.x % heads, i0 = AW_Q * blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* base = qkv + (size_t)b * n * 3 * HD + h * d;
    const float* dSb = dS + ((size_t)b * heads + h) * n * n;
    for (int idx = threadIdx.x; idx < AW_Q * AW_N; idx += 256) {
        const int r = idx >> 8, j = idx & 255, i = i0 + r;
        st[r * AW_LS + j] = (i < n && j < n) ? dSb[(size_t)i * n + j] : 0.0f;
    }
    {
        const int j = min((int)threadIdx.x, n - 1);
        et[threadIdx.x] = (j / fw) * d;
        et[AW_N + threadIdx.x] = (j % fw) * d;
    }
    __syncthreads();
    f32x16 acc;
    const int dd = 32 * wave + (lane & 31);
    if (aw_apply<true>(st, base + HD, (size_t)3 * HD, eh, ew, et, n, d, acc)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + mfma32_row(r, lane);
            if (i < n && dd < d) dqkv[((size_t)b * n + i) * 3 * HD + h * d + dd] = acc[r] * scale;
        }
    }
    if (aw_tn(dSb, base, (size_t)3 * HD, scale, i0, n, d, acc)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = i0 + mfma32_row(r, lane);
            if (j < n && dd < d) {
                dqkv[((size_t)b * n + j) * 3 * HD + HD + h * d + dd] = acc[r];
                dE[(((size_t)b * heads + h) * n + j) * d + dd] = acc[r];
            }
        }
    }
}

// d height[y][dd] = sum_{b,h,x} dE[b,h][(y,x)][dd];  d width[x][dd] = sum_{b,h,y} dE[...]
// one workgroup per row of the two tables (fh + fw of them), 1024 threads = (1024 / d) groups x d lanes: a group walks every
// (1024 / d)-th (b, head) pair in ascending order, the groups meet in LDS in fixed order (deterministic).  (Rounds 1-2: one
// thread per table element, 512 strided loads each -- 127 us for 24 KB of result.)
__global__ __launch_bounds__(1024) void posemb_grad_kernel(const float* __restrict__ dE, int BH, int fh, int fw, int d,
                                                           float* __restrict__ dheight, float* __restrict__ dwidth,
                                                           int accumulate) {
    __shared__ float red[1024];
    const int n = fh * fw, groups = 1024 / d, dd = threadIdx.x % d, g = threadIdx.x / d;
    const bool is_h = (int)blockIdx.x < fh;
    const int idx = is_h ? blockIdx.x : blockIdx.x - fh;
    float a = 0.0f;
    if (g < groups) {
        for (int bh = g; bh < BH; bh += groups) {
            const float* base = dE + (size_t)bh * n * d + dd;
            if (is_h) for (int x = 0; x < fw; ++x) a += base[(size_t)(idx * fw + x) * d];
            else for (int y = 0; y < fh; ++y) a += base[(size_t)(y * fw + idx) * d];
        }
    }
    red[threadIdx.x] = a;
    __syncthreads();
    if (g == 0) {
        float t = 0.0f;
        for (int q = 0; q < groups; ++q) t += red[q * d + dd];
        float* out = is_h ? dheight + idx * d + dd : dwidth + idx * d + dd;
        *out = accumulate ? *out + t : t;
    }
}

}  // namespace

extern "C" {

size_t mg_batchnorm_workspace(int C) { return C > 0 ? (size_t)BN_RS * 2 * C * sizeof(double) : 0; }
int mg_batchnorm_slices(void) { return BN_RS; }

int mg_batchnorm_sums(const float* x, int R, int C, void* sums, void* stream) {
    if (!x || !sums || R <= 0 || C <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(bn_sums_kernel<0>, dim3((C + 63) / 64, BN_RS), dim3(256), 0, (hipStream_t)stream, x, (const float*)nullptr,
                       (const float*)nullptr, R, C, (const float*)nullptr, (const float*)nullptr, 0, (double*)sums);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_batchnorm_fwd(const float* x, int R, int C, float eps, float momentum, int training, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, const float* residual, int act,
                     float* y, float* save_mean, float* save_rstd, const void* sums, double count, void* stream) {
    if (!x || !y || R <= 0 || C <= 0) return MG_ERR_ARG;
    if (training && (!save_mean || !save_rstd || !sums || !(count >= 1.0))) return MG_ERR_ARG;
    if (!training && (!running_mean || !running_var)) return MG_ERR_ARG;
    hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3((C + 63) / 64, BN_RS), dim3(256), 0, (hipStream_t)stream, x, R, C, eps,
                       momentum, training, gamma, beta, running_mean, running_var, residual, act, y, save_mean, save_rstd,
                       (const double*)sums, count);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_batchnorm_bwd_sums(const float* dy, const float* x, const float* y, int R, int C, const float* mean,
                          const float* rstd, int act, void* sums, void* stream) {
    if (!dy || !x || !y || !mean || !rstd || !sums || R <= 0 || C <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(bn_sums_kernel<1>, dim3((C + 63) / 64, BN_RS), dim3(256), 0, (hipStream_t)stream, x, dy, y, R, C, mean,
                       rstd, act, (double*)sums);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_batchnorm_bwd(const float* dy, const float* x, const float* y, int R, int C, const float* gamma,
                     const float* mean, const float* rstd, int act, int training, float* dx, float* dresidual,
                     float* dgamma, float* dbeta, int accumulate, const void* local_sums, const void* batch_sums,
                     double count, void* stream) {
    if (!dy || !x || !y || !mean || !rstd || !dx || !local_sums || !batch_sums || !(count >= 1.0) || R <= 0 || C <= 0)
        return MG_ERR_ARG;
    hipLaunchKernelGGL(bn_apply_bwd_kernel, dim3((C + 63) / 64, BN_RS), dim3(256), 0, (hipStream_t)stream, dy, x, y, R, C,
                       gamma, mean, rstd, act, training, dx, dresidual, dgamma, dbeta, accumulate, (const double*)local_sums,
                       (const double*)batch_sums, count);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

// Workgroups per (sample, head): the kernels are a few microseconds of serial VALU work per query / output element, and B x heads
// (64 at the bench's batch) workgroups leave three quarters of the chip idle -- split the queries / outputs over up to n / 4 groups
// until ~256 workgroups exist.  Every output element is computed by the same instructions as before: the same bits.
static unsigned attn_groups(int BH, int n) {
    int g = (256 + BH - 1) / BH;
    if (g > n / 4) g = n / 4;
    return (unsigned)(g < 1 ? 1 : g);
}
static size_t attn_lds(int n, int d, bool fwd) {
    return ((size_t)2 * n * (d + 1) + (fwd ? 4 * n + 4 * d : 0)) * sizeof(float);
}

int mg_attention_fwd(const float* qkv, const float* emb_h, const float* emb_w, int B, int fh, int fw, int heads, int d,
                     float* out, float* P, void* stream) {
    const int n = fh * fw;
    if (!qkv || !emb_h || !emb_w || !out || !P || B <= 0 || heads <= 0 || fh <= 0 || fw <= 0 || n > 256 || d <= 0 || d > 128)
        return MG_ERR_ARG;     // attn_groups divides by B * heads
    if (n > 128) {             // the wide family: a workgroup per block of 32 queries, static LDS
        hipLaunchKernelGGL(attn_wide_fwd_kernel, dim3(B * heads, (n + AW_Q - 1) / AW_Q), dim3(256), 0, (hipStream_t)stream, qkv, emb_h,
                           emb_w, n, fw, heads, d, 1.0f / sqrtf((float)d), out, P);
        MG_CHECK_LAUNCH();
        return MG_OK;
    }
    const size_t lds = attn_lds(n, d, true);
    if (lds > 160 * 1024) return MG_ERR_UNSUPPORTED;
    static size_t granted = 0;     // raised once, outside any graph capture (warm-up steps run first)
    if (lds > 64 * 1024 && lds > granted) {
        hipFuncSetAttribute((const void*)attn_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        granted = lds;
    }
    hipLaunchKernelGGL(attn_fwd_kernel, dim3(B * heads, attn_groups(B * heads, n)), dim3(256), lds, (hipStream_t)stream, qkv, emb_h, emb_w, n, fw,
                       heads, d, 1.0f / sqrtf((float)d), out, P);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

size_t mg_attention_bwd_workspace(int B, int fh, int fw, int heads, int d) {
    const size_t n = (size_t)fh * fw;
    return ((size_t)B * heads * n * n + (size_t)B * heads * n * d) * sizeof(float) + 256;
}

int mg_attention_bwd(const float* qkv, const float* emb_h, const float* emb_w, const float* dout, const float* P, int B,
                     int fh, int fw, int heads, int d, float* dqkv, float* demb_h, float* demb_w, int accumulate,
                     void* workspace, size_t workspace_bytes, void* stream) {
    const int n = fh * fw;
    if (!qkv || !emb_h || !emb_w || !dout || !P || !dqkv || !workspace || B <= 0 || heads <= 0 || fh <= 0 || fw <= 0 || n > 256 ||
        d <= 0 || d > 128)
        return MG_ERR_ARG;     // as mg_attention_fwd: nothing below divides by, or launches over, an empty dimension
    if (workspace_bytes < mg_attention_bwd_workspace(B, fh, fw, heads, d)) return MG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* dS = (float*)workspace;
    float* dE = dS + (size_t)B * heads * n * n;
    if (n > 128) {             // the wide family
        const dim3 grid(B * heads, (n + AW_Q - 1) / AW_Q);
        hipLaunchKernelGGL(attn_wide_bwd_a_kernel, grid, dim3(256), 0, st, qkv, dout, P, n, heads, d, dqkv, dS);
        hipLaunchKernelGGL(attn_wide_bwd_b_kernel, grid, dim3(256), 0, st, qkv, emb_h, emb_w, (const float*)dS, n, fw, heads, d,
                           1.0f / sqrtf((float)d), dqkv, dE);
        if (demb_h && demb_w)
            hipLaunchKernelGGL(posemb_grad_kernel, dim3(fh + fw), dim3(1024), 0, st, (const float*)dE, B * heads, fh, fw, d, demb_h,
                               demb_w, accumulate);
        MG_CHECK_LAUNCH();
        return MG_OK;
    }
    const size_t lds = attn_lds(n, d, false);
    if (lds > 160 * 1024) return MG_ERR_UNSUPPORTED;
    static size_t granted = 0;
    if (lds > 64 * 1024 && lds > granted) {
        hipFuncSetAttribute((const void*)attn_bwd_a_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipFuncSetAttribute((const void*)attn_bwd_b_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        granted = lds;
    }
    hipLaunchKernelGGL(attn_bwd_a_kernel, dim3(B * heads, attn_groups(B * heads, n)), dim3(256), lds, st, qkv, dout, P, n, heads, d, dqkv, dS);
    hipLaunchKernelGGL(attn_bwd_b_kernel, dim3(B * heads, attn_groups(B * heads, n)), dim3(256), lds, st, qkv, emb_h, emb_w, (const float*)dS, n, fw,
                       heads, d, 1.0f / sqrtf((float)d), dqkv, dE);
    if (demb_h && demb_w)
        hipLaunchKernelGGL(posemb_grad_kernel, dim3(fh + fw), dim3(1024), 0, st, (const float*)dE, B * heads, fh, fw, d, demb_h,
                           demb_w, accumulate);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"
