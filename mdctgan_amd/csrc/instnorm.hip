// K5: InstanceNorm (+activation, +residual) forward / backward.  HBM-bound: float4 (16 B / lane) coalesced NHWC streams,
// double-precision statistics.
//
// Replaces (reference): nn.InstanceNorm2d(affine=False) networks.py:26 with the ReLU / LeakyReLU(0.2) :306, :650-666 and the
// residual add :462 that follow it.
#include <cstdlib>
#include "act.h"
#include "internal.h"

namespace {

struct NormPlan { int cblocks, splits, rows_per_split; };
NormPlan norm_plan(int B, int HW, int C) {
    const int cb = (C + 63) / 64;
    int splits = (1024 + B * cb - 1) / (B * cb);
    if (splits > 32) splits = 32;          // the finalize kernel walks the splits serially: keep that loop short
    if (splits > (HW + 31) / 32) splits = (HW + 31) / 32;
    if (splits < 1) splits = 1;
    int rps = (HW + splits - 1) / splits;
    splits = (HW + rps - 1) / rps;
    return {cb, splits, rps};
}

// partial per-(b, c) sums over a slice of pixels.  MODE 0: (sum x, sum x^2).
// MODE 1 (backward): g = dy * act'(xhat); (sum g, sum g * xhat).
// VEC: 16 lanes x float4 cover the block's 64 channels (256 B per pixel), 16 pixel rows in flight per iteration.
// dy2 (optional, MODE 1): a second gradient of the same tensor (dy + dy2, one float32 addition -- what autograd's accumulation add
// computes when the tensor has two consumers: the discriminator features that also feed the feature-matching loss)
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void norm_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, int HW, int C,
                                                           int rows_per_split, int act, double* __restrict__ part,
                                                           const float* __restrict__ dy2 = nullptr) {
    constexpr int V = VEC ? 4 : 1, CL = 64 / V, RG = 256 / CL;
    __shared__ double red[2][RG][64];
    const int cl = threadIdx.x % CL, rg = threadIdx.x / CL;
    const int c = blockIdx.x * 64 + cl * V, b = blockIdx.y, sp = blockIdx.z;
    const int p0 = sp * rows_per_split, p1 = min(HW, p0 + rows_per_split);
    double s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0;
    if (c < C) {
        const size_t base = (size_t)b * HW * C + c;
        float mu[V], rs[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { mu[j] = 0.f; rs[j] = 0.f; }
        if (MODE == 1) {
#pragma unroll
            for (int j = 0; j < V; ++j) { mu[j] = mean[b * C + c + j]; rs[j] = rstd[b * C + c + j]; }
        }
        auto fetch = [&](int p, float* xv, float* gv) {
            if (VEC) {
                *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(x + base + (size_t)p * C);
                if (MODE == 1) *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(dy + base + (size_t)p * C);
                if (MODE == 1 && dy2) {
                    const float4 e = *reinterpret_cast<const float4*>(dy2 + base + (size_t)p * C);
                    gv[0] += e.x; gv[1] += e.y; gv[2] += e.z; gv[3] += e.w;
                }
            } else {
                xv[0] = x[base + (size_t)p * C];
                if (MODE == 1) { gv[0] = dy[base + (size_t)p * C]; if (dy2) gv[0] += dy2[base + (size_t)p * C]; }
            }
        };
        auto add = [&](const float* xv, const float* gv) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (MODE == 0) {
                    s1[j] += (double)xv[j];
                    s2[j] += (double)xv[j] * (double)xv[j];
                } else {
                    const float xh = (xv[j] - mu[j]) * rs[j];
                    const float gq = gv[j] * act_grad_pre(xh, act);
                    s1[j] += (double)gq;
                    s2[j] += (double)gq * (double)xh;
                }
            }
        };
        // four pixel rows per trip: their loads are in flight together (one load per thread and trip is latency-bound at ~4.5 TB/s
        // on the batch-64 maps); the sums take the rows in the same order as a row-per-trip loop -- the same bits
        constexpr int U = 4;
        int p = p0 + rg;
        for (; p + (U - 1) * RG < p1; p += U * RG) {
            float xv[U][V], gv[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) fetch(p + u * RG, xv[u], gv[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) add(xv[u], gv[u]);
        }
        for (; p < p1; p += RG) {
            float xv[V], gv[V];
            fetch(p, xv, gv);
            add(xv, gv);
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        red[0][rg][cl * V + j] = s1[j];
        red[1][rg][cl * V + j] = s2[j];
    }
    __syncthreads();
    if (threadIdx.x < 64 && blockIdx.x * 64 + threadIdx.x < C) {
        double a = 0.0, q = 0.0;
#pragma unroll
        for (int i = 0; i < RG; ++i) { a += red[0][i][threadIdx.x]; q += red[1][i][threadIdx.x]; }
        const size_t o = (((size_t)b * gridDim.z + sp) * C + blockIdx.x * 64 + threadIdx.x) * 2;
        part[o] = a;
        part[o + 1] = q;
    }
}

// MODE 0: mean, rstd = 1/sqrt(var_biased + eps).  MODE 1: (sum g)/HW, (sum g*xhat)/HW.
template <int MODE>
__global__ void norm_finalize_kernel(const double* __restrict__ part, int B, int S, int C, int HW, float eps,
                                     float* __restrict__ o1, float* __restrict__ o2) {
    // eight lanes per (b, c): the S partials are a serial chain of dependent-latency loads otherwise (9 us for 512
    // outputs); fixed summation order -> deterministic
    constexpr int G = 8;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = t / G, sl = t % G;
    const bool live = i < B * C;
    const int b = live ? i / C : 0, c = live ? i - b * C : 0;
    double s1 = 0.0, s2 = 0.0;
    if (live)
        for (int s = sl; s < S; s += G) {
            const size_t o = (((size_t)b * S + s) * C + c) * 2;
            s1 += part[o];
            s2 += part[o + 1];
        }
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {
        s1 += __shfl_xor(s1, d, G);
        s2 += __shfl_xor(s2, d, G);
    }
    if (!live || sl != 0) return;
    if (MODE == 0) {
        const double mu = s1 / HW;
        double var = s2 / HW - mu * mu;
        if (var < 0.0) var = 0.0;
        o1[i] = (float)mu;
        o2[i] = (float)(1.0 / sqrt(var + (double)eps));
    } else {
        o1[i] = (float)(s1 / HW);
        o2[i] = (float)(s2 / HW);
    }
}

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__global__ void norm_apply_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                      const float* __restrict__ rstd, const float* __restrict__ residual, int HW,
                                      int C, int act, float* __restrict__ y, size_t total, _Float16* __restrict__ y16 = nullptr) {
    // y16 (optional, autocast): the float16 copy the next convolution's operand staging would otherwise make in a pass of its own
    constexpr int V = VEC ? 4 : 1;
    const size_t per_b = (size_t)HW * C;
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V; i < total;
         i += (size_t)gridDim.x * blockDim.x * V) {
        const int b = (int)(i / per_b);
        const int c = (int)(i % C);
        if (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(x + i);
            const float4 mu = *reinterpret_cast<const float4*>(mean + b * C + c);
            const float4 rs = *reinterpret_cast<const float4*>(rstd + b * C + c);
            float4 o;
            o.x = act_fwd((v.x - mu.x) * rs.x, act);
            o.y = act_fwd((v.y - mu.y) * rs.y, act);
            o.z = act_fwd((v.z - mu.z) * rs.z, act);
            o.w = act_fwd((v.w - mu.w) * rs.w, act);
            if (residual) {
                const float4 r = *reinterpret_cast<const float4*>(residual + i);
                o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
            }
            *reinterpret_cast<float4*>(y + i) = o;
            if (y16) *reinterpret_cast<h16x4*>(y16 + i) = h16x4{(_Float16)o.x, (_Float16)o.y, (_Float16)o.z, (_Float16)o.w};
        } else {
            float o = act_fwd((x[i] - mean[b * C + c]) * rstd[b * C + c], act);
            if (residual) o += residual[i];
            y[i] = o;
            if (y16) y16[i] = (_Float16)o;
        }
    }
}

template <bool VEC>
__global__ void norm_apply_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                      const float* __restrict__ m1, const float* __restrict__ m2, int HW, int C,
                                      int act, float* __restrict__ dx, size_t total, _Float16* __restrict__ dx16 = nullptr,
                                      const float* __restrict__ dy2 = nullptr) {
    constexpr int V = VEC ? 4 : 1;
    const size_t per_b = (size_t)HW * C;
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V; i < total;
         i += (size_t)gridDim.x * blockDim.x * V) {
        const int b = (int)(i / per_b);
        const int c = (int)(i % C);
        float xv[4], gv[4], o[4];
        if (VEC) {
            *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(x + i);
            *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(dy + i);
            if (dy2) {
                const float4 e = *reinterpret_cast<const float4*>(dy2 + i);
                gv[0] += e.x; gv[1] += e.y; gv[2] += e.z; gv[3] += e.w;
            }
        } else {
            xv[0] = x[i];
            gv[0] = dy[i];
            if (dy2) gv[0] += dy2[i];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int sc = b * C + c + j;
            const float rs = rstd[sc];
            const float xh = (xv[j] - mean[sc]) * rs;
            const float gq = gv[j] * act_grad_pre(xh, act);
            o[j] = rs * (gq - m1[sc] - xh * m2[sc]);
        }
        if (VEC) {
            *reinterpret_cast<float4*>(dx + i) = *reinterpret_cast<float4*>(o);
            if (dx16) *reinterpret_cast<h16x4*>(dx16 + i) = h16x4{(_Float16)o[0], (_Float16)o[1], (_Float16)o[2], (_Float16)o[3]};
        } else {
            dx[i] = o[0];
            if (dx16) dx16[i] = (_Float16)o[0];
        }
    }
}

// The apply passes for C % 4 == 0 with the (sample, channel) bookkeeping hoisted out of the element loop: a block is 16 channel
// quads (64 channels, 256 B of a pixel) x 16 pixel rows, a thread keeps its four channels' statistics in registers and walks pixel
// rows -- norm_apply_{fwd,bwd}_kernel pay two 64-bit integer divisions and up to 16 scalar statistic loads per float4
// (measured 2.8 TB/s on the 64-channel full-resolution maps).  Same arithmetic per element: same bits.
// grid (ceil(C / 64), B, row splits), block 256.
template <bool BWD>
__global__ __launch_bounds__(256) void norm_apply_rows_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ m1, const float* __restrict__ m2,
                                                              const float* __restrict__ residual, int HW, int C, int rows_per_split,
                                                              int act, float* __restrict__ out, _Float16* __restrict__ out16,
                                                              const float* __restrict__ dy2 = nullptr) {
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + 4 * cl, b = blockIdx.y;
    if (c >= C) return;
    const float4 mu = *reinterpret_cast<const float4*>(mean + b * C + c);
    const float4 rs = *reinterpret_cast<const float4*>(rstd + b * C + c);
    float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
    if (BWD) {
        a1 = *reinterpret_cast<const float4*>(m1 + b * C + c);
        a2 = *reinterpret_cast<const float4*>(m2 + b * C + c);
    }
    const int p0 = blockIdx.z * rows_per_split, p1 = min(HW, p0 + rows_per_split);
    const size_t base = (size_t)b * HW * C + c;
    auto one = [&](size_t i, const float4 v, float4 g, const float4 r) {
        float4 o;
        if (!BWD) {
            o.x = act_fwd((v.x - mu.x) * rs.x, act);
            o.y = act_fwd((v.y - mu.y) * rs.y, act);
            o.z = act_fwd((v.z - mu.z) * rs.z, act);
            o.w = act_fwd((v.w - mu.w) * rs.w, act);
            if (residual) { o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w; }
        } else {
            if (dy2) { g.x += r.x; g.y += r.y; g.z += r.z; g.w += r.w; }
            const float xh0 = (v.x - mu.x) * rs.x, xh1 = (v.y - mu.y) * rs.y, xh2 = (v.z - mu.z) * rs.z, xh3 = (v.w - mu.w) * rs.w;
            const float g0 = g.x * act_grad_pre(xh0, act), g1 = g.y * act_grad_pre(xh1, act);
            const float g2 = g.z * act_grad_pre(xh2, act), g3 = g.w * act_grad_pre(xh3, act);
            o.x = rs.x * (g0 - a1.x - xh0 * a2.x);
            o.y = rs.y * (g1 - a1.y - xh1 * a2.y);
            o.z = rs.z * (g2 - a1.z - xh2 * a2.z);
            o.w = rs.w * (g3 - a1.w - xh3 * a2.w);
        }
        *reinterpret_cast<float4*>(out + i) = o;
        if (out16) *reinterpret_cast<h16x4*>(out16 + i) = h16x4{(_Float16)o.x, (_Float16)o.y, (_Float16)o.z, (_Float16)o.w};
    };
    // r: the residual (forward) / the second gradient dy2 (backward)
    const float* third = BWD ? dy2 : residual;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // four pixel rows per trip: their loads are in flight together (elementwise: the same bits as a row per trip)
    constexpr int U = 4;
    int p = p0 + rg;
    for (; p + (U - 1) * 16 < p1; p += U * 16) {
        float4 v[U], g[U], r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = base + (size_t)(p + 16 * u) * C;
            v[u] = *reinterpret_cast<const float4*>(x + i);
            g[u] = BWD ? *reinterpret_cast<const float4*>(dy + i) : z4;
            r[u] = third ? *reinterpret_cast<const float4*>(third + i) : z4;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) one(base + (size_t)(p + 16 * u) * C, v[u], g[u], r[u]);
    }
    for (; p < p1; p += 16) {
        const size_t i = base + (size_t)p * C;
        one(i, *reinterpret_cast<const float4*>(x + i), BWD ? *reinterpret_cast<const float4*>(dy + i) : z4,
            third ? *reinterpret_cast<const float4*>(third + i) : z4);
    }
}
// row splits so that the launch has ~4096 workgroups (16 rows per pass and block: at least 16 rows per split)
inline dim3 norm_rows_grid(int B, int HW, int C, int* rows_per_split) {
    const int cb = (C + 63) / 64;
    int splits = (4096 + B * cb - 1) / (B * cb);
    if (splits > (HW + 15) / 16) splits = (HW + 15) / 16;
    if (splits < 1) splits = 1;
    if (splits > 65535) splits = 65535;
    *rows_per_split = (HW + splits - 1) / splits;
    return dim3((unsigned)cb, (unsigned)B, (unsigned)((HW + *rows_per_split - 1) / *rows_per_split));
}
inline bool norm_rows_on() { return getenv("MG_NO_NORM_ROWS") == nullptr; }      // (read per call: the parity test flips it)

// ------------------------------------------------------------------------------------------------------------
// Single-launch InstanceNorm for small maps (HW <= 32 * NP): one workgroup owns a (sample, 32-channel) slab
// (HW x 128 B, coalesced as 8 pixels x 128 B per wave load), keeps it in registers, reduces the statistics
// through LDS in double precision, and applies the normalisation without re-reading HBM.  Replaces the
// partial / finalize / apply sequence (3 launches, 2 reads) for the 8x16 ... 18x34 maps where those launches
// are pure latency.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void slab_reduce(double s1[4], double s2[4], double (*red)[32][32], int cq, int pl,
                                            double* o1, double* o2) {
    // red[0/1][pixel-lane][channel]; then 32 threads... every thread ends with the totals of its 4 channels
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[0][pl][4 * cq + j] = s1[j];
        red[1][pl][4 * cq + j] = s2[j];
    }
    __syncthreads();
    const int c = threadIdx.x & 31, part = threadIdx.x >> 5;   // 8 parts x 4 pixel-lanes
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a += red[0][4 * part + i][c];
        b += red[1][4 * part + i][c];
    }
    __syncthreads();
    red[0][part][c] = a;
    red[1][part][c] = b;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double x = 0.0, y = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            x += red[0][i][4 * cq + j];
            y += red[1][i][4 * cq + j];
        }
        o1[j] = x;
        o2[j] = y;
    }
}

// SLABS: x is not a tensor yet but the S split-K slabs of the convolution in front (part[z][B*HW][C], summed in slab order, + bias,
// rounded through float16 for an autocast layer: exactly splitk_epilogue_kernel's arithmetic) -- the kernel finishes the
// convolution, writes its raw output to x_out (nullable: nobody reads it under no_grad) and normalises, one launch instead of two.
struct NormSlabSrc { const float* part; const float* bias; float* x_out; size_t n; int S, round_f16; };
__device__ __forceinline__ float norm_round_h(float v) { return (float)(_Float16)v; }
template <int NP, bool SLABS = false>
__global__ __launch_bounds__(256) void norm_slab_fwd_kernel(const float* __restrict__ x, int HW, int C, float eps,
                                                            int act, const float* __restrict__ residual,
                                                            float* __restrict__ y, float* __restrict__ mean,
                                                            float* __restrict__ rstd, _Float16* __restrict__ y16 = nullptr,
                                                            NormSlabSrc src = NormSlabSrc{}) {
    __shared__ double red[2][32][32];
    const int cq = threadIdx.x & 7, pl = threadIdx.x >> 3;
    const int b = blockIdx.y, c0 = blockIdx.x * 32 + 4 * cq;
    const size_t base = (size_t)b * HW * C + c0;
    float4 v[NP];
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (SLABS && src.bias) bias4 = *reinterpret_cast<const float4*>(src.bias + c0);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int p = pl + 32 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < HW) {
            if (SLABS) {
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int z = 0; z < src.S; ++z) {
                    const float4 q = *reinterpret_cast<const float4*>(src.part + (size_t)z * src.n + base + (size_t)p * C);
                    a.x += q.x; a.y += q.y; a.z += q.z; a.w += q.w;
                }
                a.x += bias4.x; a.y += bias4.y; a.z += bias4.z; a.w += bias4.w;
                if (src.round_f16) { a.x = norm_round_h(a.x); a.y = norm_round_h(a.y); a.z = norm_round_h(a.z); a.w = norm_round_h(a.w); }
                if (src.x_out) *reinterpret_cast<float4*>(src.x_out + base + (size_t)p * C) = a;
                v[i] = a;
            } else {
                v[i] = *reinterpret_cast<const float4*>(x + base + (size_t)p * C);
            }
            s1[0] += (double)v[i].x; s2[0] += (double)v[i].x * (double)v[i].x;
            s1[1] += (double)v[i].y; s2[1] += (double)v[i].y * (double)v[i].y;
            s1[2] += (double)v[i].z; s2[2] += (double)v[i].z * (double)v[i].z;
            s1[3] += (double)v[i].w; s2[3] += (double)v[i].w * (double)v[i].w;
        }
    }
    double t1[4], t2[4];
    slab_reduce(s1, s2, red, cq, pl, t1, t2);
    float mu[4], rs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double m = t1[j] / HW;
        double var = t2[j] / HW - m * m;
        if (var < 0.0) var = 0.0;
        mu[j] = (float)m;
        rs[j] = (float)(1.0 / sqrt(var + (double)eps));
    }
    if (pl == 0) {
        *reinterpret_cast<float4*>(mean + b * C + c0) = make_float4(mu[0], mu[1], mu[2], mu[3]);
        *reinterpret_cast<float4*>(rstd + b * C + c0) = make_float4(rs[0], rs[1], rs[2], rs[3]);
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int p = pl + 32 * i;
        if (p < HW) {
            float4 o;
            o.x = act_fwd((v[i].x - mu[0]) * rs[0], act);
            o.y = act_fwd((v[i].y - mu[1]) * rs[1], act);
            o.z = act_fwd((v[i].z - mu[2]) * rs[2], act);
            o.w = act_fwd((v[i].w - mu[3]) * rs[3], act);
            if (residual) {
                const float4 r = *reinterpret_cast<const float4*>(residual + base + (size_t)p * C);
                o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
            }
            *reinterpret_cast<float4*>(y + base + (size_t)p * C) = o;
            if (y16) *reinterpret_cast<h16x4*>(y16 + base + (size_t)p * C) = h16x4{(_Float16)o.x, (_Float16)o.y, (_Float16)o.z, (_Float16)o.w};
        }
    }
}

template <int NP>
__global__ __launch_bounds__(256) void norm_slab_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, int HW, int C, int act,
                                                            float* __restrict__ dx, _Float16* __restrict__ dx16 = nullptr,
                                                            const float* __restrict__ dy2 = nullptr) {
    __shared__ double red[2][32][32];
    const int cq = threadIdx.x & 7, pl = threadIdx.x >> 3;
    const int b = blockIdx.y, c0 = blockIdx.x * 32 + 4 * cq;
    const size_t base = (size_t)b * HW * C + c0;
    const float4 mu4 = *reinterpret_cast<const float4*>(mean + b * C + c0);
    const float4 rs4 = *reinterpret_cast<const float4*>(rstd + b * C + c0);
    const float mu[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, rs[4] = {rs4.x, rs4.y, rs4.z, rs4.w};
    float xh[NP][4], gq[NP][4];
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int p = pl + 32 * i;
        if (p < HW) {
            float xv[4], gv[4];
            *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(x + base + (size_t)p * C);
            *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(dy + base + (size_t)p * C);
            if (dy2) {
                const float4 e = *reinterpret_cast<const float4*>(dy2 + base + (size_t)p * C);
                gv[0] += e.x; gv[1] += e.y; gv[2] += e.z; gv[3] += e.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xh[i][j] = (xv[j] - mu[j]) * rs[j];
                gq[i][j] = gv[j] * act_grad_pre(xh[i][j], act);
                s1[j] += (double)gq[i][j];
                s2[j] += (double)gq[i][j] * (double)xh[i][j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) xh[i][j] = gq[i][j] = 0.f;
        }
    }
    double t1[4], t2[4];
    slab_reduce(s1, s2, red, cq, pl, t1, t2);
    float m1[4], m2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m1[j] = (float)(t1[j] / HW);
        m2[j] = (float)(t2[j] / HW);
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int p = pl + 32 * i;
        if (p < HW) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = rs[j] * (gq[i][j] - m1[j] - xh[i][j] * m2[j]);
            *reinterpret_cast<float4*>(dx + base + (size_t)p * C) = *reinterpret_cast<float4*>(o);
            if (dx16) *reinterpret_cast<h16x4*>(dx16 + base + (size_t)p * C) = h16x4{(_Float16)o[0], (_Float16)o[1], (_Float16)o[2], (_Float16)o[3]};
        }
    }
}

inline int slab_np(int HW, int C) {     // 0: not eligible
    constexpr bool off = false;
    if (off || C % 32 != 0 || HW > 640) return 0;
    return HW <= 128 ? 4 : HW <= 256 ? 8 : HW <= 512 ? 16 : 20;
}

}  // namespace

extern "C" {

size_t mg_instnorm_workspace(int B, int HW, int C) {
    const NormPlan p = norm_plan(B, HW, C);
    return ((size_t)B * p.splits * C * 2) * sizeof(double) + (size_t)2 * B * C * sizeof(float) + 256;
}

int mg_instnorm_fwd(const float* x, int B, int HW, int C, float eps, int act, const float* residual, float* y,
                    float* mean, float* rstd, void* workspace, size_t workspace_bytes, void* stream) {
    return mg_instnorm_fwd_h(x, B, HW, C, eps, act, residual, y, mean, rstd, workspace, workspace_bytes, stream, nullptr);
}
int mg_instnorm_fwd_h(const float* x, int B, int HW, int C, float eps, int act, const float* residual, float* y,
                      float* mean, float* rstd, void* workspace, size_t workspace_bytes, void* stream, void* y16v) {
    _Float16* y16 = (_Float16*)y16v;
    if (y16 && ((reinterpret_cast<uintptr_t>(y16) & 7) != 0 || C % 4 != 0)) return MG_ERR_ARG;
    if (!x || !y || !mean || !rstd || !workspace || B <= 0 || HW <= 0 || C <= 0) return MG_ERR_ARG;
    if (workspace_bytes < mg_instnorm_workspace(B, HW, C)) return MG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (const int np = slab_np(HW, C); np && al16(x) && al16(y) && al16(mean) && al16(rstd) && (!residual || al16(residual))) {
        const dim3 grid(C / 32, B);
#define MG_SLAB_FWD(NP_) hipLaunchKernelGGL((norm_slab_fwd_kernel<NP_, false>), grid, dim3(256), 0, st, x, HW, C, eps, act, residual, y, mean, rstd, y16, NormSlabSrc{})
        if (np == 4) MG_SLAB_FWD(4); else if (np == 8) MG_SLAB_FWD(8); else if (np == 16) MG_SLAB_FWD(16); else MG_SLAB_FWD(20);
#undef MG_SLAB_FWD
        MG_CHECK_LAUNCH();
        return MG_OK;
    }
    const NormPlan p = norm_plan(B, HW, C);
    double* part = (double*)workspace;
    if (C % 4 == 0 && al16(x))
        hipLaunchKernelGGL((norm_partial_kernel<0, true>), dim3(p.cblocks, B, p.splits), dim3(256), 0, st, x, nullptr,
                           nullptr, nullptr, HW, C, p.rows_per_split, act, part);
    else
        hipLaunchKernelGGL((norm_partial_kernel<0, false>), dim3(p.cblocks, B, p.splits), dim3(256), 0, st, x, nullptr,
                           nullptr, nullptr, HW, C, p.rows_per_split, act, part);
    hipLaunchKernelGGL(norm_finalize_kernel<0>, dim3((B * C * 8 + 255) / 256), dim3(256), 0, st, part, B, p.splits, C, HW,
                       eps, mean, rstd);
    const size_t total = (size_t)B * HW * C;
    const bool vec = (C % 4 == 0) && al16(x) && al16(y) && (!residual || al16(residual));
    if (vec && norm_rows_on() && B <= 65535) {
        int rps = 0;
        const dim3 grid = norm_rows_grid(B, HW, C, &rps);
        hipLaunchKernelGGL(norm_apply_rows_kernel<false>, grid, dim3(256), 0, st, x, (const float*)nullptr, mean, rstd,
                           (const float*)nullptr, (const float*)nullptr, residual, HW, C, rps, act, y, y16);
    } else if (vec)
        hipLaunchKernelGGL(norm_apply_fwd_kernel<true>, dim3(grid_for(total, 4)), dim3(256), 0, st, x, mean, rstd,
                           residual, HW, C, act, y, total, y16);
    else
        hipLaunchKernelGGL(norm_apply_fwd_kernel<false>, dim3(grid_for(total)), dim3(256), 0, st, x, mean, rstd,
                           residual, HW, C, act, y, total, y16);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

// library-internal (internal.h; conv_igemm.hip: mg_conv_fwd_instnorm_*): InstanceNorm straight from a convolution's split-K slabs
int mg_instnorm_slab_ok(int HW, int C) { return slab_np(HW, C) ? 1 : 0; }
int mg_instnorm_fwd_slabs(const float* part, int S, const float* bias, int round_f16, float* x_out, int B, int HW, int C, float eps,
                          int act, const float* residual, float* y, float* mean, float* rstd, void* stream, void* y16v) {
    const int np = slab_np(HW, C);
    _Float16* y16 = (_Float16*)y16v;
    if (!np || !part || S < 1 || !y || !mean || !rstd) return MG_ERR_ARG;
    if (!al16(part) || !al16(y) || !al16(mean) || !al16(rstd) || (residual && !al16(residual)) || (bias && !al16(bias)) ||
        (x_out && !al16(x_out)) || (y16 && (reinterpret_cast<uintptr_t>(y16) & 7)))
        return MG_ERR_ARG;
    const NormSlabSrc src{part, bias, x_out, (size_t)B * HW * C, S, round_f16};
    const dim3 grid(C / 32, B);
    hipStream_t st = (hipStream_t)stream;
#define MG_SLAB_FWD_S(NP_) hipLaunchKernelGGL((norm_slab_fwd_kernel<NP_, true>), grid, dim3(256), 0, st, (const float*)nullptr, HW, C, eps, act, residual, y, mean, rstd, y16, src)
    if (np == 4) MG_SLAB_FWD_S(4); else if (np == 8) MG_SLAB_FWD_S(8); else if (np == 16) MG_SLAB_FWD_S(16); else MG_SLAB_FWD_S(20);
#undef MG_SLAB_FWD_S
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_instnorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, int B, int HW, int C,
                    int act, float* dx, void* workspace, size_t workspace_bytes, void* stream) {
    return mg_instnorm_bwd_h(dy, x, mean, rstd, B, HW, C, act, dx, workspace, workspace_bytes, stream, nullptr);
}
int mg_instnorm_bwd_h(const float* dy, const float* x, const float* mean, const float* rstd, int B, int HW, int C,
                      int act, float* dx, void* workspace, size_t workspace_bytes, void* stream, void* dx16v) {
    return mg_instnorm_bwd_add(dy, nullptr, x, mean, rstd, B, HW, C, act, dx, workspace, workspace_bytes, stream, dx16v);
}
int mg_instnorm_bwd_add(const float* dy, const float* dy2, const float* x, const float* mean, const float* rstd, int B, int HW, int C,
                        int act, float* dx, void* workspace, size_t workspace_bytes, void* stream, void* dx16v) {
    _Float16* dx16 = (_Float16*)dx16v;
    if (dy2 && !al16(dy2)) return MG_ERR_ARG;
    if (dx16 && ((reinterpret_cast<uintptr_t>(dx16) & 7) != 0 || C % 4 != 0)) return MG_ERR_ARG;
    if (!dy || !x || !mean || !rstd || !dx || !workspace || B <= 0 || HW <= 0 || C <= 0) return MG_ERR_ARG;
    if (workspace_bytes < mg_instnorm_workspace(B, HW, C)) return MG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (const int np = slab_np(HW, C); np && al16(x) && al16(dy) && al16(dx) && al16(mean) && al16(rstd)) {
        const dim3 grid(C / 32, B);
#define MG_SLAB_BWD(NP_) hipLaunchKernelGGL(norm_slab_bwd_kernel<NP_>, grid, dim3(256), 0, st, dy, x, mean, rstd, HW, C, act, dx, dx16, dy2)
        if (np == 4) MG_SLAB_BWD(4); else if (np == 8) MG_SLAB_BWD(8); else if (np == 16) MG_SLAB_BWD(16); else MG_SLAB_BWD(20);
#undef MG_SLAB_BWD
        MG_CHECK_LAUNCH();
        return MG_OK;
    }
    const NormPlan p = norm_plan(B, HW, C);
    double* part = (double*)workspace;
    float* m1 = (float*)((char*)workspace + (size_t)B * p.splits * C * 2 * sizeof(double));
    float* m2 = m1 + (size_t)B * C;
    if (C % 4 == 0 && al16(x) && al16(dy))
        hipLaunchKernelGGL((norm_partial_kernel<1, true>), dim3(p.cblocks, B, p.splits), dim3(256), 0, st, x, dy, mean,
                           rstd, HW, C, p.rows_per_split, act, part, dy2);
    else
        hipLaunchKernelGGL((norm_partial_kernel<1, false>), dim3(p.cblocks, B, p.splits), dim3(256), 0, st, x, dy, mean,
                           rstd, HW, C, p.rows_per_split, act, part, dy2);
    hipLaunchKernelGGL(norm_finalize_kernel<1>, dim3((B * C * 8 + 255) / 256), dim3(256), 0, st, part, B, p.splits, C, HW,
                       0.0f, m1, m2);
    const size_t total = (size_t)B * HW * C;
    const bool vec = (C % 4 == 0) && al16(x) && al16(dy) && al16(dx);
    if (vec && norm_rows_on() && B <= 65535) {
        int rps = 0;
        const dim3 grid = norm_rows_grid(B, HW, C, &rps);
        hipLaunchKernelGGL(norm_apply_rows_kernel<true>, grid, dim3(256), 0, st, x, dy, mean, rstd, (const float*)m1,
                           (const float*)m2, (const float*)nullptr, HW, C, rps, act, dx, dx16, dy2);
    } else if (vec)
        hipLaunchKernelGGL(norm_apply_bwd_kernel<true>, dim3(grid_for(total, 4)), dim3(256), 0, st, dy, x, mean, rstd,
                           m1, m2, HW, C, act, dx, total, dx16, dy2);
    else
        hipLaunchKernelGGL(norm_apply_bwd_kernel<false>, dim3(grid_for(total)), dim3(256), 0, st, dy, x, mean, rstd,
                           m1, m2, HW, C, act, dx, total, dx16, dy2);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"
