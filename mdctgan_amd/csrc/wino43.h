// Winograd F(4x4, 3x3) for the stride-1 3x3 convolutions of an inference pass (opt-in: MG_PRECISION_F32_WINO43): 36 multiplies
// per 4x4 output tile and channel pair instead of 144, i.e. the MFMA work drops 4x against the direct convolution and 1.78x
// against F(2x2,3x3) (wino.h).  Forward only: there is no data or weight gradient in this arithmetic.
// Interpolation points (0, 1, -1, 1/2, -2, inf) -- scripts/wino43_points.py builds the matrices below from them and prints the
// error table: in a float32 model at Ci = 1024 the asymmetric set has 2.4x less error than Lavin's (0, +-1, +-2, inf), 3.5e-6
// of the output scale, inside the 3e-5 parity bound of the convolution tests.
//
//   forward   Y  = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A      d: 6x6 input patch at (4 ty - 1, 4 tx - 1), reflect / zero pad 1
// Geometry: H, W multiples of 4 (TH = H / 4, TW = W / 4).  Layouts: V / M: [36][T][C], U: [36][Co][Ci].  The 36 GEMMs run as one
// batched launch, as for the other families (wino_host.h).
#pragma once

namespace {

struct W43_AT {
    static constexpr float m[4][6] = {{1, 1, 1, 1, 1, 0},
                                      {0, 1, -1, 0.5f, -2, 0},
                                      {0, 1, 1, 0.25f, 4, 0},
                                      {0, 1, -1, 0.125f, -8, 1}};
};
struct W43_G {
    static constexpr float m[6][3] = {{1, 0, 0},
                                      {1.0f / 3, 1.0f / 3, 1.0f / 3},
                                      {-1.0f / 3, 1.0f / 3, -1.0f / 3},
                                      {-16.0f / 15, -8.0f / 15, -4.0f / 15},
                                      {1.0f / 15, -2.0f / 15, 4.0f / 15},
                                      {0, 0, 1}};
};
struct W43_BT {
    static constexpr float m[6][6] = {{1, -1.5f, -2, 1.5f, 1, 0},
                                      {0, -1, 0.5f, 2.5f, 1, 0},
                                      {0, 1, -2.5f, 0.5f, 1, 0},
                                      {0, -2, -1, 2, 1, 0},
                                      {0, 0.5f, -1, -0.5f, 1, 0},
                                      {0, 1, -1.5f, -2, 1.5f, 1}};
};

// (the plain transforms are launched with 256 threads and say so: a 36-element tile and its half-transformed copy stay in registers)
// U[36][Co][Ci] = G g G^T from OHWI weights [Co][3][3][Ci]
__global__ __launch_bounds__(256) void wino43_weight_xform_kernel(const float* __restrict__ w, int Co, int Ci, float* __restrict__ U) {
    const int C2 = Ci / 2;
    const size_t total = (size_t)Co * C2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c2 = (int)(i % C2), co = (int)(i / C2);
        w4v g[3][3], tmp[6][3], o[6][6];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) g[r][c] = w4ld(w + ((size_t)(co * 3 + r) * 3 + c) * Ci + 2 * c2);
        w4rows<W43_G, 6, 3, 3>(g, tmp);
        w4cols<W43_G, 6, 3, 6>(tmp, o);
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) w4st(U + ((size_t)(r * 6 + c) * Co + co) * Ci + 2 * c2, o[r][c]);
    }
}

// One tile's V = B^T d B: d[r][c] = ld(r, c), the 36 results go to st(position, value).  The one piece of arithmetic both writers
// of an input image share (wino43_input_xform_kernel; the hand-over of wino43_out_norm_kernel), so their bits agree.
template <class Load, class Store>
__device__ __forceinline__ void w43_input_tile(Load ld, Store st) {
    w4v d[6][6], tmp[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) d[r][c] = ld(r, c);
    w4rows<W43_BT, 6, 6, 6>(d, tmp);
#pragma unroll
    for (int r = 0; r < 6; ++r) {           // one output row at a time: keeps the live set at tmp + 6
        w4v in1[1][6], o1[1][6];
#pragma unroll
        for (int c = 0; c < 6; ++c) in1[0][c] = tmp[r][c];
        w4cols<W43_BT, 6, 6, 1>(in1, o1);
#pragma unroll
        for (int c = 0; c < 6; ++c) st(r * 6 + c, o1[0][c]);
    }
}
// One tile's Y = A^T M A, M[r][c] = ld(r * 6 + c): shared by wino43_output_xform_kernel and wino43_out_norm_kernel
template <class Load>
__device__ __forceinline__ void w43_output_tile(Load ld, w4v (&y)[4][4]) {
    w4v m[6][6], tmp[4][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) m[r][c] = ld(r * 6 + c);
    w4rows<W43_AT, 4, 6, 6>(m, tmp);
    w4cols<W43_AT, 4, 6, 4>(tmp, y);
}
// Row / column iy of a 6x6 patch over a map of n pixels: the reflected pixel (ReflectionPad2d(1)), or -1 for a zero
__device__ __forceinline__ int w43_src(int i, int n, int reflect) {
    if (reflect) return reflect_idx(i, n);
    return (i >= 0 && i < n) ? i : -1;
}

// V[36][T][C] = B^T d B, d = x[b][4 ty - 1 .. +5][4 tx - 1 .. +5]; outside [0,H)x[0,W): the reflected pixel (ReflectionPad2d(1)) or 0
__global__ __launch_bounds__(256) void wino43_input_xform_kernel(const float* __restrict__ x, int B, int H, int W, int C, int TH, int TW, int reflect,
                                          float* __restrict__ V) {
    const int C2 = C / 2;
    const size_t T = (size_t)B * TH * TW, total = T * C2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c2 = (int)(i % C2);
        const size_t t = i / C2;
        const int tx = (int)(t % TW), ty = (int)((t / TW) % TH), b = (int)(t / ((size_t)TW * TH));
        w43_input_tile(
            [&](int r, int c) {
                const int iy = w43_src(4 * ty - 1 + r, H, reflect), ix = w43_src(4 * tx - 1 + c, W, reflect);
                return (iy >= 0 && ix >= 0) ? w4ld(x + ((size_t)(b * H + iy) * W + ix) * C + 2 * c2) : w4zero();
            },
            [&](int p, const w4v v) { w4st(V + ((size_t)p * T + t) * C + 2 * c2, v); });
    }
}

// out[B][4TH][4TW][C] = act(A^T M A + bias)
__global__ __launch_bounds__(256) void wino43_output_xform_kernel(const float* __restrict__ Mx, int B, int TH, int TW, int C,
                                           const float* __restrict__ bias, int act, float* __restrict__ out) {
    const int C2 = C / 2;
    const size_t T = (size_t)B * TH * TW, total = T * C2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c2 = (int)(i % C2);
        const size_t t = i / C2;
        const int tx = (int)(t % TW), ty = (int)((t / TW) % TH), b = (int)(t / ((size_t)TW * TH));
        w4v y[4][4];
        w43_output_tile([&](int p) { return w4ld(Mx + ((size_t)p * T + t) * C + 2 * c2); }, y);
        const w4v bv = bias ? w4ld(bias + 2 * c2) : w4zero();
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const w4v v = make_float2(apply_act(y[r][c].x + bv.x, act), apply_act(y[r][c].y + bv.y, act));
                w4st(out + ((size_t)(b * 4 * TH + 4 * ty + r) * (4 * TW) + 4 * tx + c) * C + 2 * c2, v);
            }
    }
}

// ---- output transform fused with InstanceNorm2d(affine=False) (+ activation, + residual), and the hand-over --------------------
// The counterpart of wino_out_norm_kernel (wino.h) for the trunk's small maps: one workgroup owns a (sample, 32 output channels)
// slab of Mx, inverse-transforms it, adds the bias, takes the InstanceNorm statistics over all its pixels (sums in double, fixed
// order: deterministic), normalises, applies the activation, adds the residual and writes y -- no second kernel, no second read.
// Thread = (channel pair, tile lane): NT tiles of 4x4 pixels each, kept in registers between the statistics and the apply; up to
// 48 tiles fit, the host admits 40 (640 pixels, the pixel limit of the F(2x2,3x3) kernel's 160 tiles).
// NEXT: the slab's output plane is also staged in LDS (dynamic: 16 * TH * TW pixels x 32 channels) and every thread builds the
// NEXT F(4x4,3x3) layer's input tiles from it -- 6x6 patches at stride 4 with the one-pixel halo in that layer's padding mode,
// through w43_input_tile, so v_next is bit for bit what wino43_input_xform_kernel computes from y.
template <int NT, bool NEXT = false>
__global__ __launch_bounds__(256) void wino43_out_norm_kernel(const float* __restrict__ Mx, int B, int TH, int TW, int C,
                                                              const float* __restrict__ bias, WinoNorm nrm,
                                                              float* __restrict__ y_raw) {
    __shared__ double red[2][16][32];
    extern __shared__ __attribute__((aligned(16))) float w43_plane[];      // NEXT: [pixel][32 channels]
    const int cp = threadIdx.x & 15, tl = threadIdx.x >> 4;
    const int b = blockIdx.y, c0 = blockIdx.x * 32 + 2 * cp;
    const int Ts = TH * TW, H = 4 * TH, W = 4 * TW;
    const size_t T = (size_t)B * Ts;
    w4v v[NT][16];
    double s1[2] = {0, 0}, s2[2] = {0, 0};
    const w4v bv = bias ? w4ld(bias + c0) : w4zero();
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int tile = tl + 16 * i;
        if (tile < Ts) {
            const size_t t = (size_t)b * Ts + tile;
            w4v y[4][4];
            w43_output_tile([&](int p) { return w4ld(Mx + ((size_t)p * T + t) * C + c0); }, y);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const w4v o = make_float2(y[q >> 2][q & 3].x + bv.x, y[q >> 2][q & 3].y + bv.y);
                v[i][q] = o;
                s1[0] += (double)o.x; s2[0] += (double)o.x * (double)o.x;
                s1[1] += (double)o.y; s2[1] += (double)o.y * (double)o.y;
            }
        }
    }
    // red[0/1][tile lane][channel]; every thread of a channel pair then sums the 16 partials in the same order
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        red[0][tl][2 * cp + j] = s1[j];
        red[1][tl][2 * cp + j] = s2[j];
    }
    __syncthreads();
    const int HW = 16 * Ts;
    float mu[2], rs[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        double x1 = 0.0, x2 = 0.0;
#pragma unroll
        for (int l = 0; l < 16; ++l) {
            x1 += red[0][l][2 * cp + j];
            x2 += red[1][l][2 * cp + j];
        }
        const double mval = x1 / HW;
        double var = x2 / HW - mval * mval;
        if (var < 0.0) var = 0.0;
        mu[j] = (float)mval;
        rs[j] = (float)(1.0 / sqrt(var + (double)nrm.eps));
    }
    if (tl == 0) {
        w4st(nrm.mean + (size_t)b * C + c0, make_float2(mu[0], mu[1]));
        w4st(nrm.rstd + (size_t)b * C + c0, make_float2(rs[0], rs[1]));
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int tile = tl + 16 * i;
        if (tile < Ts) {
            const int ty = tile / TW, tx = tile - ty * TW;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int py = 4 * ty + (q >> 2), px = 4 * tx + (q & 3);
                const size_t off = ((size_t)(b * H + py) * W + px) * C + c0;
                if (y_raw) w4st(y_raw + off, v[i][q]);      // (inference: nobody reads the raw output again)
                w4v o = make_float2(apply_act((v[i][q].x - mu[0]) * rs[0], nrm.act), apply_act((v[i][q].y - mu[1]) * rs[1], nrm.act));
                if (nrm.residual) {
                    const w4v rr = w4ld(nrm.residual + off);
                    o.x += rr.x; o.y += rr.y;
                }
                w4st(nrm.y + off, o);
                if (NEXT) w4st(w43_plane + (py * W + px) * 32 + 2 * cp, o);
            }
        }
    }
    if (NEXT) {
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < NT; ++i) {
            const int tile = tl + 16 * i;
            if (tile < Ts) {
                const int ty = tile / TW, tx = tile - ty * TW;
                const size_t t = (size_t)b * Ts + tile;
                w43_input_tile(
                    [&](int r, int c) {
                        const int iy = w43_src(4 * ty - 1 + r, H, nrm.next_reflect), ix = w43_src(4 * tx - 1 + c, W, nrm.next_reflect);
                        return (iy >= 0 && ix >= 0) ? w4ld(w43_plane + (iy * W + ix) * 32 + 2 * cp) : w4zero();
                    },
                    [&](int p, const w4v o) { w4st(nrm.v_next + ((size_t)p * T + t) * C + c0, o); });
            }
        }
    }
}
// <= 40 tiles per sample (NT <= 3); the NEXT instances keep the slab's plane in LDS: 16 * 40 pixels x 32 channels = 80 KiB
constexpr int W43_NORM_TILES = 40;
inline bool wino43_out_norm_ok(int TH, int TW, int C) { return C % 32 == 0 && TH * TW <= W43_NORM_TILES; }
inline size_t wino43_plane_bytes(int TH, int TW) { return (size_t)16 * TH * TW * 32 * sizeof(float); }

}  // namespace
