// K1' / K2': the fused MDCT / IMDCT codec kernels for the Princen-Bradley power-of-two geometries other than 512
// (win_length == n_fft == 2 hop, centre padding; M = n_fft / 2 in {128, 512, 1024}).  One template per direction, instantiated per M.
//
// Per frame: window, TDAC fold to M values u, DCT-IV of size M, epilogue.  The DCT-IV is an M/2-point complex DFT between two
// twiddles (the identity mdct_ct.h uses for M = 256; models/mdct.py:596-628 FastMDCT4 in the reference):
//     c[n] = (u[2n] + i u[M-1-2n]) pre[n],     pre[n]  = exp(-i pi (4n + 1) / (4M))
//     Z    = DFT_{M/2}(c)
//     Y[k] = Z[k] post[k],                     post[k] = exp(-i pi 4k / (4M))
//     X[2k] = Re Y[k],   X[M-1-2k] = -Im Y[k]
// The DFT is a Stockham autosort FFT on the VALU in plain float32: radix-8 stages (one radix-2 / radix-4 stage first when needed),
// every stage in place in LDS: all butterflies of a tile are read into registers, a barrier, then written to their autosort
// positions (natural order out, no bit reversal).  The first stage multiplies by pre[] as it reads, the last by post[] as it
// writes and leaves X in natural bin order, so the twiddles cost no pass of their own.  The DCT-IV is its own inverse up to
// 2 / M, so K2' runs the same stages on the decoded coefficients and unfolds / windows / overlap-adds in its store.
//
// Twiddles (mg_mdct_pow2_twiddles, built on the host): [pre (M/2 complex) | post (M/2 complex) | root (M/2 complex)],
// root[t] = exp(-2 pi i t / (M/2)); every entry is exp(-i pi p / (4M)) with an integer p, evaluated in float64 after an exact
// reduction of p to the first octant and rounded once to float32.
//
// Tile = PW_TILE floats of LDS = FT = PW_TILE / M frames (64 / 16 / 8), 256 threads, + 3M floats of twiddles:
// 32 KiB + 1.5 / 6 / 12 KiB per workgroup -> three workgroups (12 waves) per CU (152-188 VGPRs; LDS at M = 1024).  Every stage is
// 2 radix-8 (4 radix-4) butterflies per thread.  A workgroup walks tiles grid-stride and loads the twiddles once.  Tiles cut the
// flattened [B * F] frame index, so a tile may hold the end of one clip and the start of the next and only the last one is ragged.
//   K1': tile = rows r0 .. r0 + FT - 1.  The fold reads the audio straight from HBM / L2 (16 bytes per lane where T and the
//        pointers allow, else 4), the epilogue stores FT * M contiguous floats, 16 bytes per lane.
//   K2': tile = rows r0 - 1 .. r0 + FT - 2: row 0 is the frame in front (recomputed: 1 / FT of the work), rows 1 .. FT - 1 emit
//        their hop blocks (frame f >= 1 of a clip against frame f - 1, the row before; a clip's frame 0 emits nothing).  Every
//        output sample is written once by the workgroup that owns it: no atomics, identical bits run to run.  The stitched form adds the halved cross-fade zones into the zeroed waveform as mdct_ct.h does (at most two
//        segments meet in a sample and a two-term float sum has no order), and stores everything else.
#include <cmath>
#include <cstdlib>
#include "common.h"
#include "mdctgan_hip.h"
#include "internal.h"

namespace {

enum Codec { CODEC_RAW = 0, CODEC_ARCSINH = 1, CODEC_RANGE = 2 };
struct CodecParams {
    int mode;
    float gain;
    float nr0, nr1;
    float mn, mx;
    const float* mn_b;
    const float* mx_b;
    int per_sample;
};
struct StitchArgs { union { long long base; const SegRow* rows; }; long long total; int pitch, overlap; };   // as in mdct.hip
enum Stitch { ST_NONE = 0, ST_SEG = 1, ST_ROWS = 2 };
constexpr float LN10F = 2.3025851249694824f;   // float32(log(10)), as torch.log(torch.tensor(10.0))

}  // namespace

#include "mdct_codec.h"

namespace {

constexpr int PW_NT = 256;
constexpr int PW_TILE = 8192;       // floats of frame data per workgroup

__device__ __forceinline__ float2 pw_cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

template <int R>
__device__ __forceinline__ void pw_butterfly(float2 (&v)[R]) {
    if (R == 2) {
        const float2 a = v[0], b = v[1];
        v[0] = make_float2(a.x + b.x, a.y + b.y);
        v[1] = make_float2(a.x - b.x, a.y - b.y);
    } else if (R == 4) {
        const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
        const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), a3 = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
        v[0] = make_float2(a0.x + a2.x, a0.y + a2.y);
        v[2] = make_float2(a0.x - a2.x, a0.y - a2.y);
        v[1] = make_float2(a1.x + a3.y, a1.y - a3.x);      // a1 - i a3
        v[3] = make_float2(a1.x - a3.y, a1.y + a3.x);      // a1 + i a3
    } else {
        // 8 points: two 4-point transforms (even / odd inputs), then out[k] = E[k] + W8^k O[k], out[k + 4] = E[k] - W8^k O[k]
        float2 e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
        pw_butterfly<4>(e);
        pw_butterfly<4>(o);
        constexpr float H = 0.70710678118654752440f;
        const float2 t0 = o[0];
        const float2 t1 = make_float2((o[1].x + o[1].y) * H, (o[1].y - o[1].x) * H);       // (1 - i) / sqrt 2
        const float2 t2 = make_float2(o[2].y, -o[2].x);                                     // -i
        const float2 t3 = make_float2((o[3].y - o[3].x) * H, (-o[3].x - o[3].y) * H);      // (-1 - i) / sqrt 2
        v[0] = make_float2(e[0].x + t0.x, e[0].y + t0.y); v[4] = make_float2(e[0].x - t0.x, e[0].y - t0.y);
        v[1] = make_float2(e[1].x + t1.x, e[1].y + t1.y); v[5] = make_float2(e[1].x - t1.x, e[1].y - t1.y);
        v[2] = make_float2(e[2].x + t2.x, e[2].y + t2.y); v[6] = make_float2(e[2].x - t2.x, e[2].y - t2.y);
        v[3] = make_float2(e[3].x + t3.x, e[3].y + t3.y); v[7] = make_float2(e[3].x - t3.x, e[3].y - t3.y);
    }
}

// One Stockham stage over the FT frames of the tile.  buf: [FT][N2] complex (frame pitch M floats); NS = size of the
// sub-transforms done so far.  Butterfly j of a frame reads points j + r N2 / R and writes (j / NS) NS R + j % NS + r NS.
// Contains both barriers: on entry every earlier write to buf must already be fenced by the caller's barrier.
template <int M_, int R, int NS, bool FIRST, bool LAST>
__device__ __forceinline__ void pw_stage(float* __restrict__ fbuf, const float2* __restrict__ tw, int tid) {
    constexpr int N2 = M_ / 2, NB = N2 / R, FT = PW_TILE / M_, IT = FT * NB / PW_NT;
    static_assert(FT * NB % PW_NT == 0, "whole butterflies per thread");
    float2* buf = reinterpret_cast<float2*>(fbuf);
    const float2* pre = tw;
    const float2* post = tw + N2;
    const float2* root = tw + 2 * N2;
    float2 v[IT][R];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * PW_NT, fr = idx / NB, j = idx % NB;
#pragma unroll
        for (int r = 0; r < R; ++r) v[it][r] = buf[fr * N2 + j + r * NB];
        if (FIRST) {
#pragma unroll
            for (int r = 0; r < R; ++r) v[it][r] = pw_cmul(v[it][r], pre[j + r * NB]);
        }
        if (NS > 1) {
            const int k = j % NS;
#pragma unroll
            for (int r = 1; r < R; ++r) v[it][r] = pw_cmul(v[it][r], root[r * k * (N2 / (NS * R))]);
        }
        pw_butterfly<R>(v[it]);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * PW_NT, fr = idx / NB, j = idx % NB;
        const int d = (j / NS) * NS * R + j % NS;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int kk = d + r * NS;
            if (!LAST) {
                buf[fr * N2 + kk] = v[it][r];
            } else {
                const float2 y = pw_cmul(v[it][r], post[kk]);
                fbuf[fr * M_ + 2 * kk] = y.x;
                fbuf[fr * M_ + M_ - 1 - 2 * kk] = -y.y;
            }
        }
    }
    __syncthreads();
}

template <int M_, int NS, bool FIRST>
__device__ __forceinline__ void pw_stages8(float* fbuf, const float2* tw, int tid) {
    constexpr int N2 = M_ / 2;
    if constexpr (NS * 8 == N2) {
        pw_stage<M_, 8, NS, FIRST, true>(fbuf, tw, tid);
    } else {
        pw_stage<M_, 8, NS, FIRST, false>(fbuf, tw, tid);
        pw_stages8<M_, NS * 8, false>(fbuf, tw, tid);
    }
}

constexpr int pw_log2(int n) { int l = 0; while (n > 1) { n >>= 1; ++l; } return l; }

// DCT-IV of the FT frames in fbuf, in place.  In: u[m] of a frame at float m (m even) or M - m (m odd), i.e. complex n =
// (u[2n], u[M-1-2n]); out: X[m] at float m.  The caller fences the input with a barrier; the output is fenced on return.
// Stage radices: 8 wherever possible, one radix-2 or radix-4 stage first when log2(M/2) is not a multiple of 3
// (M = 128: 8 8;  M = 512: 4 8 8;  M = 1024: 8 8 8) -- mdct.py::pow2_radices says the same to the host model.
template <int M_>
__device__ __forceinline__ void pw_dct4(float* fbuf, const float2* tw, int tid) {
    constexpr int REM = pw_log2(M_ / 2) % 3;
    if constexpr (REM == 0) {
        pw_stages8<M_, 1, true>(fbuf, tw, tid);
    } else {
        pw_stage<M_, 1 << REM, 1, true, false>(fbuf, tw, tid);
        pw_stages8<M_, 1 << REM, false>(fbuf, tw, tid);
    }
}

// where u[m] of a frame goes (floats from the frame's start)
template <int M_>
__device__ __forceinline__ int pw_u_word(int m) { return (m & 1) ? M_ - m : m; }

// ------------------------------------------------------------------------------------------------------------------
// K1'.  grid = min(tiles, cap), block = 256.  audio [B, T] -> spec [B, F, M]; frame f covers audio f M - M .. f M + M - 1, zeros
// outside [0, T) (so any F the caller names is served: the backward of to_audio frames out_len samples into F frames).
// ------------------------------------------------------------------------------------------------------------------
template <int M_, int MODE, bool STATS, bool VEC>
__global__ __launch_bounds__(PW_NT) void mdct4_pow2_kernel(const float* __restrict__ audio, int B, int T, int F,
                                                           const float* __restrict__ window, const float* __restrict__ twg,
                                                           CodecParams cp, float* __restrict__ spec, double* __restrict__ stats) {
    constexpr int Q = M_ / 2, FT = PW_TILE / M_;
    __shared__ __attribute__((aligned(16))) float fbuf[PW_TILE];
    __shared__ __attribute__((aligned(16))) float twf[3 * M_];
    __shared__ double red[2 * (PW_NT / 64)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 3 * M_; i += PW_NT) twf[i] = twg[i];
    const float2* tw = reinterpret_cast<const float2*>(twf);
    const int rows = B * F, n_tiles = (rows + FT - 1) / FT;          // (the host checked B * F * M < 2^31)
    const BsCodec bc = bs_codec(cp);
    double sd1 = 0.0, sd2 = 0.0;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int r0 = tile * FT;
        // four windowed samples z[n0 .. n0 + 3] of frame f:  z[n] = fl32(x[f M + n - M] w[n])  (mdct.py:410)
        auto z4 = [&](const float* x, int f, int n0) -> float4 {
            const long long t0 = (long long)f * M_ + n0 - M_;
            float4 a, w;
            if (VEC && t0 >= 0 && t0 + 3 < T) {
                a = bs_ld4(x + t0);
            } else {
                a.x = (t0 >= 0 && t0 < T) ? x[t0] : 0.0f;
                a.y = (t0 + 1 >= 0 && t0 + 1 < T) ? x[t0 + 1] : 0.0f;
                a.z = (t0 + 2 >= 0 && t0 + 2 < T) ? x[t0 + 2] : 0.0f;
                a.w = (t0 + 3 >= 0 && t0 + 3 < T) ? x[t0 + 3] : 0.0f;
            }
            if (VEC) w = bs_ld4(window + n0);
            else w = make_float4(window[n0], window[n0 + 1], window[n0 + 2], window[n0 + 3]);
            return make_float4(__fmul_rn(a.x, w.x), __fmul_rn(a.y, w.y), __fmul_rn(a.z, w.z), __fmul_rn(a.w, w.w));
        };
        // fold u = [-c_r - d, a - b_r] (quarters a, b, c, d of z), four consecutive u per thread and step
#pragma unroll 2
        for (int i = tid; i < PW_TILE / 4; i += PW_NT) {
            const int fr = i / (M_ / 4), m = 4 * (i % (M_ / 4)), row = r0 + fr;
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < rows) {
                const int b = row / F, f = row - b * F;
                const float* x = audio + (size_t)b * T;
                const float4 r = z4(x, f, 3 * Q - 4 - m);            // z[3Q-1-m-e] = r[3 - e]
                if (m < Q) {
                    const float4 d = z4(x, f, 3 * Q + m);
                    u = make_float4(-r.w - d.x, -r.z - d.y, -r.y - d.z, -r.x - d.w);
                } else {
                    const float4 a = z4(x, f, m - Q);
                    u = make_float4(a.x - r.w, a.y - r.z, a.z - r.y, a.w - r.x);
                }
            }
            float* dst = fbuf + fr * M_;
            dst[pw_u_word<M_>(m)] = u.x; dst[pw_u_word<M_>(m + 1)] = u.y;
            dst[pw_u_word<M_>(m + 2)] = u.z; dst[pw_u_word<M_>(m + 3)] = u.w;
        }
        __syncthreads();
        pw_dct4<M_>(fbuf, tw, tid);
        // codec, statistics, 16-byte stores of FT * M contiguous floats
        float f1 = 0.0f, f2 = 0.0f;
        float* out = spec + (size_t)r0 * M_;
#pragma unroll 2
        for (int i = tid; i < PW_TILE / 4; i += PW_NT) {
            const int fr = i / (M_ / 4);
            if (r0 + fr >= rows) continue;
            const float4 xv = bs_ld4(fbuf + 4 * i);
            float4 v = xv;
            if (MODE != CODEC_RAW) {
                float4 l;
                v.x = bs_encode(xv.x, bc, l.x); v.y = bs_encode(xv.y, bc, l.y);
                v.z = bs_encode(xv.z, bc, l.z); v.w = bs_encode(xv.w, bc, l.w);
                if (STATS) {
                    f1 += (l.x + l.y) + (l.z + l.w);
                    f2 += (l.x * l.x + l.y * l.y) + (l.z * l.z + l.w * l.w);
                }
            }
            *reinterpret_cast<float4*>(out + 4 * i) = v;
        }
        if (STATS && MODE != CODEC_RAW) { sd1 += (double)f1; sd2 += (double)f2; }
        __syncthreads();                                  // the tile has been read: the next fold may overwrite it
    }
    if (STATS && MODE != CODEC_RAW) {
        // one pair of double atomics per workgroup, as K1
        sd1 = wave_sum_d(sd1); sd2 = wave_sum_d(sd2);
        if (lane == 0) { red[2 * wave] = sd1; red[2 * wave + 1] = sd2; }
        __syncthreads();
        if (tid < 2) {
            double a = 0.0;
#pragma unroll
            for (int w = 0; w < PW_NT / 64; ++w) a += red[2 * w + tid];
            atomicAdd(stats + tid, a);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// K2'.  grid = min(tiles, cap), block = 256.  spec [B, F, M] -> audio [B, out_len] (or the stitched waveform, ST):
//   out[(h - 1) M + n] = scale (w[n] y_h[n] + w[n + M] y_{h-1}[n + M]),   h = 1 .. F - 1,   y = unfold(DCT-IV(decode(spec)))
// ------------------------------------------------------------------------------------------------------------------
template <int M_, int MODE, int ST, bool VEC>
__global__ __launch_bounds__(PW_NT) void imdct4_pow2_kernel(const float* __restrict__ spec, int B, int F,
                                                            const float* __restrict__ window, const float* __restrict__ twg,
                                                            CodecParams cp, float* __restrict__ audio, int out_len, float scale,
                                                            StitchArgs sa) {
    constexpr int Q = M_ / 2, FT = PW_TILE / M_, HB = FT - 1;      // hop blocks per tile
    __shared__ __attribute__((aligned(16))) float fbuf[PW_TILE];
    __shared__ __attribute__((aligned(16))) float twf[3 * M_];
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * M_; i += PW_NT) twf[i] = twg[i];
    const float2* tw = reinterpret_cast<const float2*>(twf);
    const int rows = B * F, n_tiles = (rows + HB - 1) / HB;          // (the host checked B * F * M < 2^31)
    const float rgain = 1.0f / cp.gain;
    // decode:  x = v c1 + c0 (= ln10 ((v - nr0) / (nr1 - nr0) (max - min) + min)),  X = sinh(x) / gain   (the constants of K2)
    auto consts = [&](float mn, float mx, float& c1, float& c0) {
        const double k = ((double)mx - (double)mn) / ((double)cp.nr1 - (double)cp.nr0);
        const double sc = (MODE == CODEC_ARCSINH) ? (double)LN10F : 1.0;
        c1 = (float)(k * sc); c0 = (float)(((double)mn - (double)cp.nr0 * k) * sc);
    };
    float c1f, c0f;
    consts(cp.mn, cp.mx, c1f, c0f);

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int r0 = tile * HB;                                  // row fr of the tile is flattened frame r0 - 1 + fr
#pragma unroll 2
        for (int i = tid; i < PW_TILE / 4; i += PW_NT) {
            const int fr = i / (M_ / 4), m = 4 * (i % (M_ / 4)), row = r0 - 1 + fr;
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f);            // rows outside the batch contribute nothing (decode(0) != 0)
            if (row >= 0 && row < rows) {
                float c1 = c1f, c0 = c0f;
                if (MODE != CODEC_RAW && cp.per_sample) { const int b = row / F; consts(cp.mn_b[b], cp.mx_b[b], c1, c0); }
                auto dec1 = [&](float v) -> float {
                    if (MODE == CODEC_RAW) return v;
                    const float xx = fmaf(v, c1, c0);
                    return MODE == CODEC_ARCSINH ? sinh_fast(xx) * rgain : xx;
                };
                const float4 s = bs_ld4(spec + (size_t)row * M_ + m);
                u = make_float4(dec1(s.x), dec1(s.y), dec1(s.z), dec1(s.w));
            }
            float* dst = fbuf + fr * M_;
            dst[pw_u_word<M_>(m)] = u.x; dst[pw_u_word<M_>(m + 1)] = u.y;
            dst[pw_u_word<M_>(m + 2)] = u.z; dst[pw_u_word<M_>(m + 3)] = u.w;
        }
        __syncthreads();
        pw_dct4<M_>(fbuf, tw, tid);
        // unfold y = [v2, -v2_r, -v1_r, -v1], window, overlap-add, scale, centre crop: rows 1 .. FT - 1 against the row before
#pragma unroll 2
        for (int i = tid; i < HB * (M_ / 4); i += PW_NT) {
            const int fr = 1 + i / (M_ / 4), n = 4 * (i % (M_ / 4)), row = r0 - 1 + fr;
            if (row >= rows) continue;
            const int b = row / F, h = row - b * F;
            if (h == 0) continue;                                                  // a clip's first frame has no block of its own
            const float* vc = fbuf + fr * M_;
            const float* vp = vc - M_;
            float4 yc, yp;
            if (n < Q) {
                yc = bs_ld4(vc + Q + n);                                       // y_h[n] = v_h[Q + n]
                const float4 q = bs_ld4(vp + Q - 4 - n);                       // y_{h-1}[n + M] = -v_{h-1}[Q - 1 - n]
                yp = make_float4(-q.w, -q.z, -q.y, -q.x);
            } else {
                const float4 c = bs_ld4(vc + 3 * Q - 4 - n);                   // y_h[n] = -v_h[3Q - 1 - n]
                yc = make_float4(-c.w, -c.z, -c.y, -c.x);
                const float4 q = bs_ld4(vp + n - Q);                           // y_{h-1}[n + M] = -v_{h-1}[n - Q]
                yp = make_float4(-q.x, -q.y, -q.z, -q.w);
            }
            float4 w0, w1;
            if (VEC) { w0 = bs_ld4(window + n); w1 = bs_ld4(window + n + M_); }
            else {
                w0 = make_float4(window[n], window[n + 1], window[n + 2], window[n + 3]);
                w1 = make_float4(window[n + M_], window[n + M_ + 1], window[n + M_ + 2], window[n + M_ + 3]);
            }
            const float4 o = make_float4(scale * (w0.x * yc.x + w1.x * yp.x), scale * (w0.y * yc.y + w1.y * yp.y),
                                         scale * (w0.z * yc.z + w1.z * yp.z), scale * (w0.w * yc.w + w1.w * yp.w));
            const long long t0 = (long long)(h - 1) * M_ + n;
            if (t0 >= out_len) continue;
            const float oe[4] = {o.x, o.y, o.z, o.w};
            if (!ST) {
                float* dst = audio + (size_t)b * out_len + t0;
                if (VEC && t0 + 3 < out_len) { *reinterpret_cast<float4*>(dst) = o; continue; }
#pragma unroll
                for (int e = 0; e < 4; ++e) if (t0 + e < out_len) dst[e] = oe[e];
            } else if (ST == ST_ROWS) {
                // clip b is row sa.rows[b] of a packed buffer: sample t lands at pos + t, dropped outside the row's window [lo, hi)
                // (a dead row, lo == hi, writes nothing).  VEC: overlap, out_len % 4 == 0 and a 16-byte aligned buffer; the 16-byte
                // store also needs a position that is a multiple of 4
                const SegRow rw = seg_row_clamped(sa.rows, b, sa.total);
                const long long g0 = rw.pos + t0;
                if (VEC && (g0 & 3) == 0 && t0 >= sa.overlap && t0 + 3 < out_len - sa.overlap && g0 >= rw.lo && g0 + 3 < rw.hi) {
                    *reinterpret_cast<float4*>(audio + g0) = o;
                    continue;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long long t = t0 + e, gi = g0 + e;
                    if (t >= out_len || gi < rw.lo || gi >= rw.hi) continue;
                    if (t < sa.overlap || t >= out_len - sa.overlap) unsafeAtomicAdd(audio + gi, 0.5f * oe[e]);
                    else audio[gi] = oe[e];
                }
            } else {
                // clip b is segment first + b of one waveform: halved and added inside the cross-fade zones, stored elsewhere;
                // positions outside [0, total) are the reference's final crop.  VEC: pitch, overlap, out_len % 4 == 0 and a
                // 16-byte aligned waveform -- a float4 is inside or outside a zone as a whole
                const long long g0 = sa.base + (long long)b * sa.pitch + t0;
                if (VEC && t0 >= sa.overlap && t0 + 3 < out_len - sa.overlap && g0 >= 0 && g0 + 3 < sa.total) {
                    *reinterpret_cast<float4*>(audio + g0) = o;
                    continue;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long long t = t0 + e, gi = sa.base + (long long)b * sa.pitch + t;
                    if (t >= out_len || gi < 0 || gi >= sa.total) continue;
                    if (t < sa.overlap || t >= out_len - sa.overlap) unsafeAtomicAdd(audio + gi, 0.5f * oe[e]);
                    else audio[gi] = oe[e];
                }
            }
        }
        __syncthreads();
    }
}

// exp(-i pi p / D), D a multiple of 4: p reduced exactly to the first octant, float64
void pw_cis(long long p, long long D, double* re, double* im) {
    p %= 2 * D;
    const long long q = p / (D / 2), r = p % (D / 2);
    double c, s;
    if (r == 0) { c = 1.0; s = 0.0; }
    else if (4 * r == D) { c = s = 0.70710678118654752440; }
    else if (4 * r < D) { c = cos(M_PI * (double)r / (double)D); s = sin(M_PI * (double)r / (double)D); }
    else { c = sin(M_PI * (double)(D / 2 - r) / (double)D); s = cos(M_PI * (double)(D / 2 - r) / (double)D); }
    switch (q) {                     // (c - i s) (-i)^q
        case 0: *re = c; *im = -s; break;
        case 1: *re = -s; *im = -c; break;
        case 2: *re = -c; *im = s; break;
        default: *re = s; *im = c; break;
    }
}

bool pw_size_ok(int n_fft) { return n_fft == 256 || n_fft == 1024 || n_fft == 2048; }
bool pw_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
unsigned pw_grid(long long n_tiles) { return (unsigned)(n_tiles < 2048 ? n_tiles : 2048); }

int imdct4_pow2_dispatch(const float* spec, int B, int F, int n_fft, const float* window, const float* tw, int codec, float gain,
                         float nr0, float nr1, float src_min, float src_max, const float* min_b, const float* max_b, void* audio,
                         int out_len, int out_f64, float scale, StitchArgs sa, void* stream, bool row_table = false);

}  // namespace

extern "C" {

// See include/mdctgan_hip.h for the contracts.
int mg_mdct_pow2_supported(int n_fft, int hop_length, int win_length, int center) {
    return (pw_size_ok(n_fft) && win_length == n_fft && 2 * hop_length == n_fft && center) ? 1 : 0;
}

long long mg_mdct_pow2_twiddle_floats(int n_fft) { return pw_size_ok(n_fft) ? 3LL * (n_fft / 2) : 0; }

int mg_mdct_pow2_twiddles(int n_fft, void* out, int as_f64) {
    if (!out) return MG_ERR_ARG;
    if (!pw_size_ok(n_fft)) return MG_ERR_UNSUPPORTED;
    const int M_ = n_fft / 2, N2 = M_ / 2;
    for (int i = 0; i < 3 * N2; ++i) {
        const int n = i % N2;
        const long long p = i < N2 ? 4LL * n + 1 : (i < 2 * N2 ? 4LL * n : 16LL * n);
        double re, im;
        pw_cis(p, 4LL * M_, &re, &im);
        if (as_f64) { ((double*)out)[2 * i] = re; ((double*)out)[2 * i + 1] = im; }
        else { ((float*)out)[2 * i] = (float)re; ((float*)out)[2 * i + 1] = (float)im; }
    }
    return MG_OK;
}

int mg_mdct4_pow2_forward(const float* audio, int B, int T, int F, int n_fft, const float* window, const float* twiddles, int codec,
                          float gain, float nr0, float nr1, float src_min, float src_max, int per_sample, float* spec,
                          float* frames_out, double* stats, void* stream) {
    if (!audio || !window || !twiddles || !spec || B <= 0 || T <= 0 || F <= 0) return MG_ERR_ARG;
    if (!pw_size_ok(n_fft) || per_sample || frames_out || codec < CODEC_RAW || codec > CODEC_RANGE || !pw_al16(spec) ||
        !pw_al16(twiddles) || (long long)B * F * (n_fft / 2) >= (1ll << 31))
        return MG_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    CodecParams cp{codec, gain, nr0, nr1, src_min, src_max, nullptr, nullptr, 0};
    if (stats) hipMemsetAsync(stats, 0, 2 * sizeof(double), st);
    const bool vec = T % 4 == 0 && pw_al16(audio) && pw_al16(window);
    const bool want_stats = stats && codec != CODEC_RAW;
#define MG_PW_K1(M_, MODE_, STATS_, VEC_)                                                                                  \
    do {                                                                                                                   \
        constexpr int ft = PW_TILE / (M_);                                                                                 \
        const long long n_tiles = ((long long)B * F + ft - 1) / ft;                                                        \
        hipLaunchKernelGGL((mdct4_pow2_kernel<M_, MODE_, STATS_, VEC_>), dim3(pw_grid(n_tiles)), dim3(PW_NT), 0, st, audio, B, T, F, \
                           window, twiddles, cp, spec, stats);                                                             \
    } while (0)
#define MG_PW_K1_V(M_, MODE_, STATS_) do { if (vec) MG_PW_K1(M_, MODE_, STATS_, true); else MG_PW_K1(M_, MODE_, STATS_, false); } while (0)
#define MG_PW_K1_S(M_, MODE_) do { if (want_stats) MG_PW_K1_V(M_, MODE_, true); else MG_PW_K1_V(M_, MODE_, false); } while (0)
#define MG_PW_K1_C(M_)                                                                                                     \
    do {                                                                                                                   \
        if (codec == CODEC_RAW) MG_PW_K1_V(M_, CODEC_RAW, false);                                                          \
        else if (codec == CODEC_ARCSINH) MG_PW_K1_S(M_, CODEC_ARCSINH);                                                    \
        else MG_PW_K1_S(M_, CODEC_RANGE);                                                                                  \
    } while (0)
    if (n_fft == 256) MG_PW_K1_C(128); else if (n_fft == 1024) MG_PW_K1_C(512); else MG_PW_K1_C(1024);
#undef MG_PW_K1_C
#undef MG_PW_K1_S
#undef MG_PW_K1_V
#undef MG_PW_K1
    MG_CHECK_LAUNCH();
    mg_mdct_note_kernel(0, "mdct4_pow2_kernel (csrc/mdct_pow2.hip)");
    return MG_OK;
}

int mg_imdct4_pow2_forward(const float* spec, int B, int F, int n_fft, const float* window, const float* twiddles, int codec,
                           float gain, float nr0, float nr1, float src_min, float src_max, const float* min_b, const float* max_b,
                           void* audio, int out_len, int out_f64, float out_scale, void* stream) {
    return imdct4_pow2_dispatch(spec, B, F, n_fft, window, twiddles, codec, gain, nr0, nr1, src_min, src_max, min_b, max_b, audio,
                                out_len, out_f64, out_scale, StitchArgs{0, 0, 0, 0}, stream);
}

int mg_imdct4_pow2_stitched(const float* spec, int B, int F, int n_fft, const float* window, const float* twiddles, int codec,
                            float gain, float nr0, float nr1, float src_min, float src_max, const float* min_b, const float* max_b,
                            void* out, long long out_total, int seg_len, int overlap, long long first_seg, int zero_out,
                            int out_f64, void* stream) {
    if (!out || seg_len <= 0 || overlap < 0 || 2 * overlap >= seg_len || first_seg < 0 || out_total <= 0) return MG_ERR_ARG;
    if (out_f64 || !pw_size_ok(n_fft)) return MG_ERR_UNSUPPORTED;           // (before the clear: a refused call leaves `out` alone)
    if (zero_out && overlap > 0) hipMemsetAsync(out, 0, (size_t)out_total * 4, (hipStream_t)stream);
    const int pitch = seg_len - overlap;
    return imdct4_pow2_dispatch(spec, B, F, n_fft, window, twiddles, codec, gain, nr0, nr1, src_min, src_max, min_b, max_b, out,
                                seg_len, out_f64, 4.0f / (float)n_fft, StitchArgs{first_seg * pitch - overlap, out_total, pitch, overlap},
                                stream);
}

int mg_imdct4_pow2_stitched_rows(const float* spec, int B, int F, int n_fft, const float* window, const float* twiddles, int codec,
                                 float gain, float nr0, float nr1, float src_min, float src_max, const float* min_b,
                                 const float* max_b, void* out, long long out_total, int seg_len, int overlap,
                                 const mg_seg_row* rows, int zero_out, int out_f64, void* stream) {
    if (!out || !rows || seg_len <= 0 || overlap < 0 || 2 * overlap >= seg_len || out_total <= 0) return MG_ERR_ARG;
    if (out_f64 || !pw_size_ok(n_fft)) return MG_ERR_UNSUPPORTED;           // (before the clear: a refused call leaves `out` alone)
    if (zero_out) hipMemsetAsync(out, 0, (size_t)out_total * 4, (hipStream_t)stream);
    StitchArgs sa{0, out_total, seg_len - overlap, overlap};
    sa.rows = reinterpret_cast<const SegRow*>(rows);
    return imdct4_pow2_dispatch(spec, B, F, n_fft, window, twiddles, codec, gain, nr0, nr1, src_min, src_max, min_b, max_b, out,
                                seg_len, out_f64, 4.0f / (float)n_fft, sa, stream, true);
}

}  // extern "C"

namespace {

int imdct4_pow2_dispatch(const float* spec, int B, int F, int n_fft, const float* window, const float* tw, int codec, float gain,
                         float nr0, float nr1, float src_min, float src_max, const float* min_b, const float* max_b, void* audio,
                         int out_len, int out_f64, float scale, StitchArgs sa, void* stream, bool row_table) {
    if (!spec || !window || !tw || !audio || B <= 0 || F <= 1 || ((min_b == nullptr) != (max_b == nullptr))) return MG_ERR_ARG;
    if (!pw_size_ok(n_fft)) return MG_ERR_UNSUPPORTED;
    if (out_len <= 0 || (long long)out_len > (long long)(F - 1) * (n_fft / 2)) return MG_ERR_ARG;
    if (out_f64 || codec < CODEC_RAW || codec > CODEC_RANGE || !pw_al16(spec) || !pw_al16(tw) ||
        (long long)B * F * (n_fft / 2) >= (1ll << 31))
        return MG_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    CodecParams cp{codec, gain, nr0, nr1, src_min, src_max, min_b, max_b, (min_b && max_b) ? 1 : 0};
    const bool stitched = sa.pitch != 0;
    const bool vec = pw_al16(window) && out_len % 4 == 0 && pw_al16(audio) && (!stitched || (sa.pitch % 4 == 0 && sa.overlap % 4 == 0));
#define MG_PW_K2(M_, MODE_, ST_, VEC_)                                                                                     \
    do {                                                                                                                   \
        constexpr int hb = PW_TILE / (M_) - 1;                                                                             \
        const long long n_tiles = ((long long)B * F + hb - 1) / hb;                                                        \
        hipLaunchKernelGGL((imdct4_pow2_kernel<M_, MODE_, ST_, VEC_>), dim3(pw_grid(n_tiles)), dim3(PW_NT), 0, st, spec, B, F, window, \
                           tw, cp, (float*)audio, out_len, scale, sa);                                                     \
    } while (0)
#define MG_PW_K2_V(M_, MODE_, ST_) do { if (vec) MG_PW_K2(M_, MODE_, ST_, true); else MG_PW_K2(M_, MODE_, ST_, false); } while (0)
#define MG_PW_K2_S(M_, MODE_)                                                                                              \
    do {                                                                                                                   \
        if (row_table) MG_PW_K2_V(M_, MODE_, ST_ROWS); else if (stitched) MG_PW_K2_V(M_, MODE_, ST_SEG); else MG_PW_K2_V(M_, MODE_, ST_NONE); \
    } while (0)
#define MG_PW_K2_C(M_)                                                                                                     \
    do {                                                                                                                   \
        if (codec == CODEC_RAW) MG_PW_K2_S(M_, CODEC_RAW);                                                                 \
        else if (codec == CODEC_ARCSINH) MG_PW_K2_S(M_, CODEC_ARCSINH);                                                    \
        else MG_PW_K2_S(M_, CODEC_RANGE);                                                                                  \
    } while (0)
    if (n_fft == 256) MG_PW_K2_C(128); else if (n_fft == 1024) MG_PW_K2_C(512); else MG_PW_K2_C(1024);
#undef MG_PW_K2_C
#undef MG_PW_K2_S
#undef MG_PW_K2_V
#undef MG_PW_K2
    MG_CHECK_LAUNCH();
    mg_mdct_note_kernel(1, row_table ? "imdct4_pow2_kernel<stitched rows> (csrc/mdct_pow2.hip)"
                           : stitched ? "imdct4_pow2_kernel<stitched> (csrc/mdct_pow2.hip)" : "imdct4_pow2_kernel (csrc/mdct_pow2.hip)");
    return MG_OK;
}

}  // namespace
