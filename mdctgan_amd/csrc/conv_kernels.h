// K3 / K4 / K6: implicit-GEMM convolution (forward, data-gradient == transposed convolution,
// weight-gradient) on the gfx950 f32 MFMA pipe (v_mfma_f32_32x32x2_f32, exact float32).
//
// Replaces nn.Conv2d / nn.ConvTranspose2d / nn.ReflectionPad2d forward + backward of the reference
// (models/networks.py:207-210, 308-309, 329, 349-352, 387-392, 406-411, 440, 456, 649-670).
//
// Layout: activations NHWC, weights OHWI ([Co][KH][KW][Ci]).  Every pass is one GEMM
//      FWD    Y[m=(b,oy,ox)][n=co]     = sum_{k=(ky,kx,ci)} Xgather[m][k]  * W[n][k]
//      DGRAD  dX[m=(b,iy,ix)][n=ci]    = sum_{k=(ky,kx,co)} dYgather[m][k] * W[k.co][k.tap][n]
//      WGRAD  dW[co][n=(ky,kx,ci)]     = sum_{k=(b,oy,ox)}  dY[k][co]      * Xgather[k][n]
// The gathers fold zero padding, ReflectionPad2d (forward: index reflection; backward: the up-to-4
// padded positions that alias an interior pixel are summed in the loader), the stride (DGRAD runs
// one launch slice per output-parity class so no MFMA work is spent on structural zeros) and the
// transposed-convolution geometry into address generation: no padded / dilated tensor ever exists.
//
// Tile: BM x BN x 16, 256 threads = 2x2 waves, each wave (BM/2)x(BN/2) as 32x32 MFMA blocks.
// LDS tiles are k-major ([16][rows + 4]): the MFMA fragment read is one conflict-free ds_read_b32 per
// operand per MFMA (lanes 0-31 consecutive rows), k-contiguous global float4s are scattered with
// 2-way (free) ds_write_b32, row-contiguous ones land as ds_write_b128.  Register-staged double
// buffering, one barrier per k-chunk; with 64-cycle MFMAs the loader hides completely.
//
// This header: the four generic kernels (forward, 32-deep forward, data gradient, weight gradient) with Geom, Batch and the
// MFMA chunk helpers, the split-K combine and column-sum kernels, conv_grid and splitk_epilogue / splitk_reduce.
// Needs: common.h, mdctgan_hip.h (MG_ACT_*).
#pragma once

namespace {

constexpr int BK = 16;

struct Geom {
    int B, H, W, Ci, OH, OW, Co, KH, KW, s, p, reflect;
};

// Batched launches (the 16 Winograd positions run as one grid): element strides between consecutive problems.
// wino_perm: the data-gradient uses the 180-degree rotated filter, which in the Winograd domain is the position
// permutation xi -> (3,1,2,0)[xi] on both axes (G * flip == P * G).
struct Batch {
    long long sa, sw, so;
    int wino_perm;
};
__device__ __forceinline__ int wino_flip(int z) {
    const int xi = z >> 2, nu = z & 3;
    const int fx = (xi == 0) ? 3 : (xi == 3 ? 0 : xi), fn = (nu == 0) ? 3 : (nu == 3 ? 0 : nu);
    return fx * 4 + fn;
}

__device__ __forceinline__ int reflect_idx(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == MG_ACT_RELU) return fmaxf(v, 0.0f);
    if (act == MG_ACT_LRELU02) return v > 0.0f ? v : 0.2f * v;
    if (act == MG_ACT_TANH) return tanhf(v);
    return v;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

// k-contiguous float4 (4 consecutive k of one row) -> k-major LDS tile.
// P = 1 (f16 compute, TAG 2 kernels): the tile holds halves, two consecutive k of a row packed in one 32-bit word at
// [k / 2][row] (same pitch in words), so a lane's 8 k of one MFMA step are 4 words of its row.
template <int LD, int P = 0>
__device__ __forceinline__ void st_kcontig(float* S, int row, int q, const float4 v) {
    if (P) {
        uint32_t* W = reinterpret_cast<uint32_t*>(S);
        W[(2 * q + 0) * LD + row] = pack_h2(v.x, v.y);
        W[(2 * q + 1) * LD + row] = pack_h2(v.z, v.w);
    } else {
        S[(4 * q + 0) * LD + row] = v.x;
        S[(4 * q + 1) * LD + row] = v.y;
        S[(4 * q + 2) * LD + row] = v.z;
        S[(4 * q + 3) * LD + row] = v.w;
    }
}
// row-contiguous float4 (4 consecutive rows at one k)
template <int LD, int P = 0>
__device__ __forceinline__ void st_rowcontig(float* S, int k, int row, const float4 v) {
    if (P) {
        _Float16* H = reinterpret_cast<_Float16*>(S) + (((k >> 1) * LD + row) << 1) + (k & 1);
        H[0] = (_Float16)v.x;
        H[2] = (_Float16)v.y;
        H[4] = (_Float16)v.z;
        H[6] = (_Float16)v.w;
    } else {
        *reinterpret_cast<float4*>(S + k * LD + row) = v;
    }
}

// One 16-deep chunk on the f16 MFMA pipe: one 32x32x16 instruction per accumulator tile.
template <int MB, int NB, int LDA, int LDB, typename F0, typename F1>
__device__ __forceinline__ void mma_chunk_h(const float* Ap, const float* Bp, f32x16 (&acc)[MB][NB], int wm0, int wn0,
                                            int lane, F0&& after_kp0, F1&& after_kp1) {
    const int r = lane & 31, kh = lane >> 5;
    const uint32_t* ap = reinterpret_cast<const uint32_t*>(Ap) + (4 * kh) * LDA + wm0 + r;
    const uint32_t* bp = reinterpret_cast<const uint32_t*>(Bp) + (4 * kh) * LDB + wn0 + r;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 a[MB], b[NB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[mi][j] = ap[j * LDA + 32 * mi];
#pragma unroll
    for (int ni = 0; ni < NB; ++ni)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[ni][j] = bp[j * LDB + 32 * ni];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni)
            acc[mi][ni] = mfma32x32x16h(__builtin_bit_cast(f16x8, a[mi]), __builtin_bit_cast(f16x8, b[ni]), acc[mi][ni]);
    __builtin_amdgcn_sched_barrier(0);
    after_kp0();
    after_kp1();
}

// One 16-deep k-chunk of MFMAs, software-pipelined by hand (the compiler will not do either on its own):
//  * the A/B fragments of k-pair kp+1 are read from LDS into a second register set BEFORE the MFMAs of k-pair kp
//    are issued, so the ds_read latency sits under 256 cycles of queued MFMA work;
//  * the staging work of the NEXT chunks rides inside this chunk's MFMA stream: after k-pair 0 the registers that
//    hold chunk c+1 (loaded one chunk ago) are written to the idle LDS buffer (`after_kp0`), after k-pair 1 the
//    global loads + address arithmetic for chunk c+2 are issued into the same registers (`after_kp1`).  VALU /
//    VMEM / DS instructions issue while the 64-cycle MFMAs execute, instead of in a serial phase between chunks
//    (ablation on the 1024-channel layer: loads 17 %, LDS stores + barrier 5 % of the kernel before this).
template <int MB, int NB, int LDA, int LDB, typename F0, typename F1>
__device__ __forceinline__ void mma_chunk(const float* Ap, const float* Bp, f32x16 (&acc)[MB][NB], int wm0, int wn0,
                                          int lane, F0&& after_kp0, F1&& after_kp1) {
    const int r = lane & 31, kh = lane >> 5;
    const float* ap = Ap + kh * LDA + wm0 + r;
    const float* bp = Bp + kh * LDB + wn0 + r;
    constexpr int NKP = BK / 2, RING = 4, AHEAD = 3;   // fragments are read 3 k-pairs ahead of their MFMAs
    float a[RING][MB], b[RING][NB];
#pragma unroll
    for (int pk = 0; pk < AHEAD; ++pk) {
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) a[pk][mi] = ap[2 * pk * LDA + 32 * mi];
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) b[pk][ni] = bp[2 * pk * LDB + 32 * ni];
    }
#pragma unroll
    for (int kp = 0; kp < NKP; ++kp) {
        const int cur = kp % RING, nxt = (kp + AHEAD) % RING;
        if (kp + AHEAD < NKP) {
#pragma unroll
            for (int mi = 0; mi < MB; ++mi) a[nxt][mi] = ap[2 * (kp + AHEAD) * LDA + 32 * mi];
#pragma unroll
            for (int ni = 0; ni < NB; ++ni) b[nxt][ni] = bp[2 * (kp + AHEAD) * LDB + 32 * ni];
        }
        __builtin_amdgcn_sched_barrier(0);     // keep the prefetch ds_reads ahead of this k-pair's MFMAs
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
#pragma unroll
            for (int ni = 0; ni < NB; ++ni) acc[mi][ni] = mfma32x32x2(a[cur][mi], b[cur][ni], acc[mi][ni]);
        __builtin_amdgcn_sched_barrier(0);
        if (kp == 0) after_kp0();
        if (kp == 1) after_kp1();
        if (kp <= 1) __builtin_amdgcn_sched_barrier(0);
    }
}

// ================================================================================================
// FWD
// ================================================================================================
template <int BM, int BN, bool VEC, int TAG = 0>   // TAG bit 0: dense batched GEMM operands (1: Winograd F(2x2,3x3), 5: the
                                                   // 25-position families of wino4.h / wino42.h -- distinct symbols for profilers); bit 1: f16 compute
__global__ __launch_bounds__(256) void conv_fwd_kernel(Geom g, const float* __restrict__ x,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ y,
                                                       int act, int chunks_per_split, float* __restrict__ part,
                                                       Batch bt) {
    constexpr int MB = BM / 64, NB = BN / 64, LDA = BM + 4, LDB = BN + 4;
    constexpr int NVA = BM * 4 / 256, NVB = BN * 4 / 256;
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * (LDA + LDB)];
    auto As = [&](int buf) -> float* { return smem + buf * (BK * LDA); };
    auto Bs = [&](int buf) -> float* { return smem + 2 * BK * LDA + buf * (BK * LDB); };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = g.B * g.OH * g.OW, N = g.Co, K = g.KH * g.KW * g.Ci;
    x += (size_t)blockIdx.z * bt.sa;
    w += (size_t)blockIdx.z * bt.sw;
    y += (size_t)blockIdx.z * bt.so;
    if (part) part += ((size_t)blockIdx.y * gridDim.z + blockIdx.z) * ((size_t)M * N);
    const int cpt = g.Ci / BK;   // chunks per tap (VEC)
    const int total_chunks = VEC ? g.KH * g.KW * cpt : (K + BK - 1) / BK;
    const int c_begin = blockIdx.y * chunks_per_split;
    const int nchunks = min(total_chunks, c_begin + chunks_per_split);   // exclusive end of this split
    const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int m0 = (t % tiles_m) * BM, n0 = (t / tiles_m) * BN;
    const int q = tid & 3, r0 = tid >> 2;

    int iy0[NVA], ix0[NVA], pb[NVA];
    bool va_ok[NVA];
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
        const int m = m0 + r0 + 64 * i;
        va_ok[i] = m < M;
        const int mm = va_ok[i] ? m : 0;
        const int b = mm / (g.OH * g.OW), rem = mm - b * (g.OH * g.OW);
        const int oy = rem / g.OW, ox = rem - oy * g.OW;
        iy0[i] = oy * g.s - g.p;
        ix0[i] = ox * g.s - g.p;
        pb[i] = b * g.H * g.W;
    }

    auto src_pixel = [&](int i, int ky, int kx) -> int {   // -1: zero padding
        int iy = iy0[i] + ky, ix = ix0[i] + kx;
        if (g.reflect) {
            iy = reflect_idx(iy, g.H);
            ix = reflect_idx(ix, g.W);
        } else if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) {
            return -1;
        }
        return pb[i] + iy * g.W + ix;
    };

    auto load_a = [&](int c, float4 (&va)[NVA]) {
        if (VEC) {
            const int tap = c / cpt, ci0 = (c - tap * cpt) * BK;
            const int ky = tap / g.KW, kx = tap - ky * g.KW;
#pragma unroll
            for (int i = 0; i < NVA; ++i) {
                va[i] = zero4();
                if (!va_ok[i]) continue;
                const int px = src_pixel(i, ky, kx);
                if (px >= 0) va[i] = ld4(x + (size_t)px * g.Ci + ci0 + 4 * q);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NVA; ++i) {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = c * BK + 4 * q + j;
                    e[j] = 0.0f;
                    if (va_ok[i] && k < K) {
                        const int tap = k / g.Ci, ci = k - tap * g.Ci;
                        const int ky = tap / g.KW, kx = tap - ky * g.KW;
                        const int px = src_pixel(i, ky, kx);
                        if (px >= 0) e[j] = x[(size_t)px * g.Ci + ci];
                    }
                }
                va[i] = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
    };
    auto load_b = [&](int c, float4 (&vb)[NVB]) {
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            const int n = n0 + r0 + 64 * i;
            vb[i] = zero4();
            if (n >= N) continue;
            if (VEC) {
                vb[i] = ld4(w + (size_t)n * K + c * BK + 4 * q);
            } else {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = c * BK + 4 * q + j;
                    e[j] = (k < K) ? w[(size_t)n * K + k] : 0.0f;
                }
                vb[i] = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
    };

    f32x16 acc[MB][NB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) acc[mi][ni] = f32x16{0};
    const int wm0 = (wave >> 1) * (BM / 2), wn0 = (wave & 1) * (BN / 2);

    float4 va[NVA], vb[NVB];
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NVA; ++i) st_kcontig<LDA, ((TAG & 2) != 0)>(As(buf), r0 + 64 * i, q, va[i]);
#pragma unroll
        for (int i = 0; i < NVB; ++i) st_kcontig<LDB, ((TAG & 2) != 0)>(Bs(buf), r0 + 64 * i, q, vb[i]);
    };
    if (c_begin < nchunks) {
        load_a(c_begin, va);
        load_b(c_begin, vb);
        stash(0);
    }
    __syncthreads();
    if (c_begin + 1 < nchunks) {
        load_a(c_begin + 1, va);
        load_b(c_begin + 1, vb);
    }
    for (int c = c_begin; c < nchunks; ++c) {
        const int cur = (c - c_begin) & 1;
        auto f0 = [&]() { if (c + 1 < nchunks) stash(cur ^ 1); };
        auto f1 = [&]() { if (c + 2 < nchunks) { load_a(c + 2, va); load_b(c + 2, vb); } };
        if ((TAG & 2) != 0) mma_chunk_h<MB, NB, LDA, LDB>(As(cur), Bs(cur), acc, wm0, wn0, lane, f0, f1);
        else mma_chunk<MB, NB, LDA, LDB>(As(cur), Bs(cur), acc, wm0, wn0, lane, f0, f1);
        __syncthreads();
    }

#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) {
            const int col = n0 + wn0 + 32 * ni + (lane & 31);
            const float bv = (bias && !part && col < N) ? bias[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm0 + 32 * mi + mfma32_row(r, lane);
                if (row < M && col < N) {
                    if (part) part[(size_t)row * N + col] = acc[mi][ni][r];
                    else {
                        const float v = apply_act(acc[mi][ni][r] + bv, act);
                        y[(size_t)row * N + col] = ((TAG & 2) != 0) ? round_h(v) : v;
                    }
                }
            }
        }
}

// ================================================================================================
// FWD, 32-deep chunks, row-major LDS images ("full-line staging").
// Both operands of the forward GEMM are k-contiguous in HBM (NHWC activations, OHWI weights, and the Winograd
// V/U matrices), so a chunk of 32 k is one full 128-byte line per row: a wave-wide global_load_dwordx4 covers
// 8 rows x 128 B instead of 16 rows x 64 B (half the texture-addresser work for the same bytes), the stage is one
// ds_write_b128 per 16 bytes instead of four ds_write_b32, and a lane fetches 4 consecutive k of its row with one
// ds_read_b128.  The MFMA k index inside a chunk is free as long as A and B agree: lane half `kh` owns
// k = 8*s + 4*kh + j for MFMA (s, j).  Row pitch 36 floats: 16-byte aligned rows, conflict-free for both the
// 8-lanes-per-row writes and the 32-rows-at-one-k reads.
// ================================================================================================
#include "gemm32.h"      // (here, inside this namespace: mdct.hip includes the same text into its own)

template <int BM, int BN, int TAG = 0>
__global__ __launch_bounds__(256) void conv_fwd32_kernel(Geom g, const float* __restrict__ x,
                                                         const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y,
                                                         int act, int chunks_per_split, float* __restrict__ part,
                                                         Batch bt) {
    constexpr int MB = BM / 64, NB = BN / 64;
    constexpr int NVA = BM / 32, NVB = BN / 32;
    extern __shared__ __attribute__((aligned(16))) float smem32[];
    auto As = [&](int buf) -> float* { return smem32 + buf * (BM * LDK2); };
    auto Bs = [&](int buf) -> float* { return smem32 + 2 * BM * LDK2 + buf * (BN * LDK2); };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = g.B * g.OH * g.OW, N = g.Co, K = g.KH * g.KW * g.Ci;
    x += (size_t)blockIdx.z * bt.sa;
    w += (size_t)blockIdx.z * bt.sw;
    y += (size_t)blockIdx.z * bt.so;
    if (part) part += ((size_t)blockIdx.y * gridDim.z + blockIdx.z) * ((size_t)M * N);
    const int cpt = g.Ci / BK2;
    const int total_chunks = g.KH * g.KW * cpt;
    const int c_begin = blockIdx.y * chunks_per_split;
    const int nchunks = min(total_chunks, c_begin + chunks_per_split);
    const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int m0 = (t % tiles_m) * BM, n0 = (t / tiles_m) * BN;
    const int q = tid & 7, r0 = tid >> 3;

    int iy0[NVA], ix0[NVA], pb[NVA];
    bool va_ok[NVA];
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
        const int m = m0 + r0 + 32 * i;
        va_ok[i] = m < M;
        const int mm = va_ok[i] ? m : 0;
        const int b = mm / (g.OH * g.OW), rem = mm - b * (g.OH * g.OW);
        const int oy = rem / g.OW, ox = rem - oy * g.OW;
        iy0[i] = oy * g.s - g.p;
        ix0[i] = ox * g.s - g.p;
        pb[i] = b * g.H * g.W;
    }
    const float* wrow[NVB];
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
        const int n = n0 + r0 + 32 * i;
        wrow[i] = (n < N) ? w + (size_t)n * K + 4 * q : nullptr;
    }

    // TAG 1 / 3 (batched plain GEMM of the Winograd path): both operands are dense row-major matrices, so staging is a
    // pointer per row fixed for the whole K loop + one load per chunk -- no tap / padding / reflection arithmetic.  An
    // MFMA-bound loop pays ~2.6 cycles for every staging instruction even in the MFMAs' shadow (scripts/ubench), so the
    // instruction count of the stage, not its placement, is what the remaining efficiency hangs on.  Rows past M / N
    // re-read the last row: their accumulators are never stored.
    const float* pa[NVA];
    const float* pbq[NVB];
#pragma unroll
    for (int i = 0; i < NVA; ++i) pa[i] = x + (size_t)min(m0 + r0 + 32 * i, M - 1) * K + 4 * q;
#pragma unroll
    for (int i = 0; i < NVB; ++i) pbq[i] = w + (size_t)min(n0 + r0 + 32 * i, N - 1) * K + 4 * q;
    int a_ky, a_kx, a_ci0;       // position of the next chunk load_a will stage
    {
        const int tap = c_begin / cpt;
        a_ci0 = (c_begin - tap * cpt) * BK2;
        a_ky = tap / g.KW;
        a_kx = tap - a_ky * g.KW;
    }
    auto load_a = [&](int c, float4 (&va)[NVA]) {
        if (TAG & 1) {
#pragma unroll
            for (int i = 0; i < NVA; ++i) va[i] = ld4(pa[i] + (size_t)c * BK2);
            return;
        }
        // load_a runs once per chunk in increasing c, so (ky, kx, ci0) is a running wave-uniform state, not c / cpt
        const int ky = a_ky, kx = a_kx, ci0 = a_ci0;
        a_ci0 += BK2;
        if (a_ci0 >= g.Ci) {
            a_ci0 = 0;
            if (++a_kx == g.KW) { a_kx = 0; ++a_ky; }
        }
#pragma unroll
        for (int i = 0; i < NVA; ++i) {
            // branch-free: out-of-range taps load pixel (0, 0) of the row's sample and are masked afterwards
            int iy = iy0[i] + ky, ix = ix0[i] + kx;
            bool ok = va_ok[i];
            if (g.reflect) {
                iy = reflect_idx(iy, g.H);
                ix = reflect_idx(ix, g.W);
            } else {
                ok = ok && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            }
            iy = ok ? iy : 0;
            ix = ok ? ix : 0;
            // 32-bit element offset (geom_ok bounds every tensor below 2^31 elements): base + voffset addressing
            const float4 v = ld4(x + (unsigned)(pb[i] + iy * g.W + ix) * (unsigned)g.Ci + (unsigned)(ci0 + 4 * q));
            va[i] = ok ? v : zero4();
        }
    };
    auto load_b = [&](int c, float4 (&vb)[NVB]) {
        if (TAG & 1) {
#pragma unroll
            for (int i = 0; i < NVB; ++i) vb[i] = ld4(pbq[i] + (size_t)c * BK2);
            return;
        }
#pragma unroll
        for (int i = 0; i < NVB; ++i) vb[i] = wrow[i] ? ld4(wrow[i] + (size_t)c * BK2) : zero4();
    };

    f32x16 acc[MB][NB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) acc[mi][ni] = f32x16{0};
    const int wm0 = (wave >> 1) * (BM / 2), wn0 = (wave & 1) * (BN / 2);

    float4 va[NVA], vb[NVB];
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NVA; ++i) {
            if ((TAG & 2) != 0) g32_st_h4(As(buf) + (r0 + 32 * i) * LDK2, q, va[i]);
            else *reinterpret_cast<float4*>(As(buf) + (r0 + 32 * i) * LDK2 + 4 * q) = va[i];
        }
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            if ((TAG & 2) != 0) g32_st_h4(Bs(buf) + (r0 + 32 * i) * LDK2, q, vb[i]);
            else *reinterpret_cast<float4*>(Bs(buf) + (r0 + 32 * i) * LDK2 + 4 * q) = vb[i];
        }
    };
    if (c_begin < nchunks) {
        load_a(c_begin, va);
        load_b(c_begin, vb);
        stash(0);
    }
    __syncthreads();
    if (c_begin + 1 < nchunks) {
        load_a(c_begin + 1, va);
        load_b(c_begin + 1, vb);
    }
    for (int c = c_begin; c < nchunks; ++c) {
        const int cur = (c - c_begin) & 1;
        auto f0 = [&]() { if (c + 1 < nchunks) stash(cur ^ 1); };
        auto f1 = [&]() { if (c + 2 < nchunks) { load_a(c + 2, va); load_b(c + 2, vb); } };
        if ((TAG & 2) != 0) mma_chunk32_h<MB, NB>(As(cur), Bs(cur), acc, wm0, wn0, lane, f0, f1);
        else mma_chunk32<MB, NB>(As(cur), Bs(cur), acc, wm0, wn0, lane, f0, f1);
        __syncthreads();
    }

#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) {
            const int col = n0 + wn0 + 32 * ni + (lane & 31);
            const float bv = (bias && !part && col < N) ? bias[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm0 + 32 * mi + mfma32_row(r, lane);
                if (row < M && col < N) {
                    if (part) part[(size_t)row * N + col] = acc[mi][ni][r];
                    else {
                        const float v = apply_act(acc[mi][ni][r] + bv, act);
                        y[(size_t)row * N + col] = ((TAG & 2) != 0) ? round_h(v) : v;
                    }
                }
            }
        }
}

// ================================================================================================
// DGRAD (== transposed convolution forward).  blockIdx.z = output-parity class (stride^2 of them).
// ================================================================================================
template <int BM, int BN, bool VECA, bool VECB, int TAG = 0>
__global__ __launch_bounds__(256) void conv_dgrad_kernel(Geom g, const float* __restrict__ dy,
                                                         const float* __restrict__ w,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ dx, int act, int chunks_per_split,
                                                         float* __restrict__ part, Batch bt) {
    constexpr int MB = BM / 64, NB = BN / 64, LDA = BM + 4, LDB = BN + 4;
    constexpr int NVA = BM * 4 / 256, NVB = BN * 4 / 256;
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * (LDA + LDB)];
    auto As = [&](int buf) -> float* { return smem + buf * (BK * LDA); };
    auto Bs = [&](int buf) -> float* { return smem + 2 * BK * LDA + buf * (BK * LDB); };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = g.s;
    const int cls = blockIdx.z % (s * s), batch = blockIdx.z / (s * s);
    // Parity classes differ in tap count (3x3 stride 2: 1, 2, 2, 4 taps).  Workgroups are dispatched in blockIdx.z
    // order, so the class with the most taps goes first (longest-processing-time-first: the short ones fill the tail).
    int py = 0, px = 0;
    if (s > 1) {
        const int zi = cls / s, zj = cls - zi * s;
        const int t0y = (g.KH - (g.p % s) + s - 1) / s, t1y = (g.KH - ((1 + g.p) % s) + s - 1) / s;
        const int t0x = (g.KW - (g.p % s) + s - 1) / s, t1x = (g.KW - ((1 + g.p) % s) + s - 1) / s;
        const int hy = t1y > t0y ? 1 : 0, hx = t1x > t0x ? 1 : 0;      // the heavier parity per axis (s == 2)
        py = zi == 0 ? hy : 1 - hy;
        px = zj == 0 ? hx : 1 - hx;
    }
    const int Hc = (g.H - py + s - 1) / s, Wc = (g.W - px + s - 1) / s;   // pixels of this class
    const int M = g.B * Hc * Wc, N = g.Ci;
    dy += (size_t)batch * bt.sa;
    w += (size_t)(bt.wino_perm ? wino_flip(batch) : batch) * bt.sw;
    dx += (size_t)batch * bt.so;
    // split-K slabs are whole dx images (classes write disjoint pixels of the same slab)
    if (part) part += ((size_t)blockIdx.y * (gridDim.z / (s * s)) + batch) * ((size_t)g.B * g.H * g.W * N);
    const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    if ((int)blockIdx.x >= tiles_m * tiles_n) return;
    // taps that reach this class: ky = ky0 + s*i
    const int ky0 = (py + g.p) % s, kx0 = (px + g.p) % s;
    const int nky = (g.KH - ky0 + s - 1) / s, nkx = (g.KW - kx0 + s - 1) / s;
    const int oyb = (py + g.p) / s, oxb = (px + g.p) / s;                 // oy = yy + oyb - tyi
    const int ntap = nky * nkx;
    const int Kc = ntap * g.Co;
    const int cpt = g.Co / BK;
    const int total_chunks = VECA ? ntap * cpt : (Kc + BK - 1) / BK;
    // stride > 1: the classes have different K, so each splits its own chunk range evenly over gridDim.y
    const int cps = (s > 1 && gridDim.y > 1) ? (total_chunks + (int)gridDim.y - 1) / (int)gridDim.y : chunks_per_split;
    const int c_begin = blockIdx.y * cps;
    const int nchunks = min(total_chunks, c_begin + cps);   // exclusive end of this split
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int m0 = (t % tiles_m) * BM, n0 = (t / tiles_m) * BN;
    const int q = tid & 3, r0 = tid >> 2;

    int yy[NVA], xx[NVA], bb[NVA];
    bool va_ok[NVA];
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
        const int m = m0 + r0 + 64 * i;
        va_ok[i] = m < M;
        const int mm = va_ok[i] ? m : 0;
        bb[i] = mm / (Hc * Wc);
        const int rem = mm - bb[i] * (Hc * Wc);
        yy[i] = rem / Wc;
        xx[i] = rem - yy[i] * Wc;
    }

    // reflect (stride 1): the padded rows / cols that alias this pixel: i+p, p-i, 2(H-1)-i+p (fixed per row)
    int cy[NVA][3], cx[NVA][3];
    if (g.reflect) {
#pragma unroll
        for (int i = 0; i < NVA; ++i) {
            const int iy = yy[i], ix = xx[i], p = g.p;
            cy[i][0] = iy + p;
            cy[i][1] = (iy >= 1 && iy <= p) ? p - iy : -1000000;
            cy[i][2] = (iy >= g.H - 1 - p && iy <= g.H - 2) ? 2 * (g.H - 1) - iy + p : -1000000;
            cx[i][0] = ix + p;
            cx[i][1] = (ix >= 1 && ix <= p) ? p - ix : -1000000;
            cx[i][2] = (ix >= g.W - 1 - p && ix <= g.W - 2) ? 2 * (g.W - 1) - ix + p : -1000000;
        }
    }

    // gather of dY for row i and tap index (tyi, txi): float4 at channel offset co (VEC) or scalar
    auto gather4 = [&](int i, int tyi, int txi, int co) -> float4 {
        float4 v = zero4();
        if (!g.reflect) {
            const int oy = yy[i] + oyb - tyi, ox = xx[i] + oxb - txi;
            if (oy >= 0 && oy < g.OH && ox >= 0 && ox < g.OW)
                v = ld4(dy + (unsigned)((bb[i] * g.OH + oy) * g.OW + ox) * (unsigned)g.Co + (unsigned)co);
        } else {   // stride 1: iy = yy, ky = tyi.  Issue every (usually one) aliasing load first, sum afterwards:
                   // accumulating inside the branches would put a vmcnt wait behind each taken load.
            float4 t[9];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int oy = cy[i][a] - tyi;
#pragma unroll
                for (int c2 = 0; c2 < 3; ++c2) {
                    const int ox = cx[i][c2] - txi;
                    const bool ok = (unsigned)oy < (unsigned)g.OH && (unsigned)ox < (unsigned)g.OW;
                    t[a * 3 + c2] = ok ? ld4(dy + (unsigned)((bb[i] * g.OH + oy) * g.OW + ox) * (unsigned)g.Co + (unsigned)co) : zero4();
                }
            }
#pragma unroll
            for (int j = 0; j < 9; ++j) add4(v, t[j]);
        }
        return v;
    };
    auto gather1 = [&](int i, int tyi, int txi, int co) -> float {
        float v = 0.0f;
        if (!g.reflect) {
            const int oy = yy[i] + oyb - tyi, ox = xx[i] + oxb - txi;
            if (oy >= 0 && oy < g.OH && ox >= 0 && ox < g.OW)
                v = dy[((size_t)(bb[i] * g.OH + oy) * g.OW + ox) * g.Co + co];
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int oy = cy[i][a] - tyi;
                if (oy < 0 || oy >= g.OH) continue;
#pragma unroll
                for (int c2 = 0; c2 < 3; ++c2) {
                    const int ox = cx[i][c2] - txi;
                    if (ox < 0 || ox >= g.OW) continue;
                    v += dy[((size_t)(bb[i] * g.OH + oy) * g.OW + ox) * g.Co + co];
                }
            }
        }
        return v;
    };

    // TAG 1 / 3 (batched plain GEMM of the Winograd path: 1x1 geometry, one class, dense operands): a pointer per
    // staged row fixed for the whole K loop, one load per chunk (see conv_fwd32_kernel).  Rows / columns past the
    // edge re-read the last valid ones; their accumulators are never stored.
    const float* pa[NVA];
    const float* pbq[NVB];
    if (TAG & 1) {
#pragma unroll
        for (int i = 0; i < NVA; ++i) pa[i] = dy + (size_t)min(m0 + r0 + 64 * i, M - 1) * g.Co + 4 * q;
#pragma unroll
        for (int i = 0; i < NVB; ++i)
            pbq[i] = w + (size_t)(tid / (BN / 4) + i * (1024 / BN)) * g.Ci + min(n0 + 4 * (tid % (BN / 4)), N - 4);
    }
    auto load_a = [&](int c, float4 (&va)[NVA]) {
        if (TAG & 1) {
#pragma unroll
            for (int i = 0; i < NVA; ++i) va[i] = ld4(pa[i] + (size_t)c * BK);
            return;
        }
        if (VECA) {
            const int tap = c / cpt, co0 = (c - tap * cpt) * BK;
            const int tyi = tap / nkx, txi = tap - tyi * nkx;
#pragma unroll
            for (int i = 0; i < NVA; ++i) va[i] = va_ok[i] ? gather4(i, tyi, txi, co0 + 4 * q) : zero4();
        } else {
#pragma unroll
            for (int i = 0; i < NVA; ++i) {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = c * BK + 4 * q + j;
                    e[j] = 0.0f;
                    if (va_ok[i] && k < Kc) {
                        const int tap = k / g.Co, co = k - tap * g.Co;
                        const int tyi = tap / nkx, txi = tap - tyi * nkx;
                        e[j] = gather1(i, tyi, txi, co);
                    }
                }
                va[i] = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
    };
    // B[k=(tap,co)][n=ci] = W[co][ky][kx][ci]: contiguous along n
    const int bk_l = tid / (BN / 4), bn_q = tid % (BN / 4);       // NVB passes step k by 256/(BN/4)
    auto load_b = [&](int c, float4 (&vb)[NVB]) {
        if (TAG & 1) {
#pragma unroll
            for (int i = 0; i < NVB; ++i) vb[i] = ld4(pbq[i] + (size_t)c * BK * g.Ci);
            return;
        }
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            const int kl = bk_l + i * (1024 / BN);
            int tap, co;
            if (VECA) {
                tap = c / cpt;
                co = (c - tap * cpt) * BK + kl;
            } else {
                const int k = c * BK + kl;
                tap = k / g.Co;
                co = k - tap * g.Co;
                if (k >= Kc) { vb[i] = zero4(); continue; }
            }
            const int tyi = tap / nkx, txi = tap - tyi * nkx;
            const int ky = ky0 + s * tyi, kx = kx0 + s * txi;
            const float* wp = w + (unsigned)((co * g.KH + ky) * g.KW + kx) * (unsigned)g.Ci;
            const int n = n0 + 4 * bn_q;
            if (VECB) {
                vb[i] = (n < N) ? ld4(wp + n) : zero4();
            } else {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = (n + j < N) ? wp[n + j] : 0.0f;
                vb[i] = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
    };

    f32x16 acc[MB][NB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) acc[mi][ni] = f32x16{0};
    const int wm0 = (wave >> 1) * (BM / 2), wn0 = (wave & 1) * (BN / 2);

    float4 va[NVA], vb[NVB];
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NVA; ++i) st_kcontig<LDA, ((TAG & 2) != 0)>(As(buf), r0 + 64 * i, q, va[i]);
#pragma unroll
        for (int i = 0; i < NVB; ++i) st_rowcontig<LDB, ((TAG & 2) != 0)>(Bs(buf), bk_l + i * (1024 / BN), 4 * bn_q, vb[i]);
    };
    if (c_begin < nchunks) {
        load_a(c_begin, va);
        load_b(c_begin, vb);
        stash(0);
    }
    __syncthreads();
    if (c_begin + 1 < nchunks) {
        load_a(c_begin + 1, va);
        load_b(c_begin + 1, vb);
    }
    for (int c = c_begin; c < nchunks; ++c) {
        const int cur = (c - c_begin) & 1;
        auto f0 = [&]() { if (c + 1 < nchunks) stash(cur ^ 1); };
        auto f1 = [&]() { if (c + 2 < nchunks) { load_a(c + 2, va); load_b(c + 2, vb); } };
        if ((TAG & 2) != 0) mma_chunk_h<MB, NB, LDA, LDB>(As(cur), Bs(cur), acc, wm0, wn0, lane, f0, f1);
        else mma_chunk<MB, NB, LDA, LDB>(As(cur), Bs(cur), acc, wm0, wn0, lane, f0, f1);
        __syncthreads();
    }

#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm0 + 32 * mi + mfma32_row(r, lane);
            if (m >= M) continue;
            const int b = m / (Hc * Wc), rem = m - b * (Hc * Wc);
            const int y2 = rem / Wc, x2 = rem - y2 * Wc;
            const size_t o = ((size_t)(b * g.H + y2 * s + py) * g.W + x2 * s + px) * g.Ci;
#pragma unroll
            for (int ni = 0; ni < NB; ++ni) {
                const int col = n0 + wn0 + 32 * ni + (lane & 31);
                if (col < N) {
                    if (part) {   // split-K: raw partial sums at the pixel's own offset in the slab
                        part[o + col] = acc[mi][ni][r];
                    } else {
                        const float bv = bias ? bias[col] : 0.0f;
                        const float v = apply_act(acc[mi][ni][r] + bv, act);
                        dx[o + col] = ((TAG & 2) != 0) ? round_h(v) : v;
                    }
                }
            }
        }
    }
}

// ================================================================================================
// WGRAD.  rows = co, cols = n = (ky,kx,ci), reduction over pixels m; blockIdx.z = split of m.
// ================================================================================================
template <int BM, int BN, bool VECA, bool VECB, int TAG = 0>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(Geom g, const float* __restrict__ x,
                                                         const float* __restrict__ dy, float* __restrict__ out,
                                                         int chunks_per_split, int accumulate, Batch bt) {
    constexpr int MB = BM / 64, NB = BN / 64, LDA = BM + 4, LDB = BN + 4;
    constexpr int NVA = BM * 4 / 256, NVB = BN * 4 / 256;
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * (LDA + LDB)];
    auto As = [&](int buf) -> float* { return smem + buf * (BK * LDA); };
    auto Bs = [&](int buf) -> float* { return smem + 2 * BK * LDA + buf * (BK * LDB); };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Mtot = g.B * g.OH * g.OW;          // reduction length
    const int R = g.Co, N = g.KH * g.KW * g.Ci;  // output rows / cols
    x += (size_t)blockIdx.y * bt.sa;
    dy += (size_t)blockIdx.y * bt.sw;
    const int tiles_m = (R + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int r_0 = (t % tiles_m) * BM, n0 = (t / tiles_m) * BN;
    const int total_chunks = (Mtot + BK - 1) / BK;
    const int c_begin = blockIdx.z * chunks_per_split;
    const int c_end = min(total_chunks, c_begin + chunks_per_split);

    const int ak_l = tid / (BM / 4), a_q = tid % (BM / 4);
    const int bk_l = tid / (BN / 4), b_q = tid % (BN / 4);

    // this thread's B columns (fixed through the loop)
    int b_tap[4], b_ci[4];
    {
        const int n = n0 + 4 * b_q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nn = n + (VECB ? 0 : j);
            b_tap[j] = (nn < N) ? nn / g.Ci : -1;
            b_ci[j] = (nn < N) ? nn - b_tap[j] * g.Ci : 0;
        }
    }

    // TAG 1 / 3 with a reduction length that is a multiple of 16 (the Winograd tile count): dense [t][channel]
    // operands, a pointer per staged row + one load per chunk
    const bool plain = (TAG & 1) && (Mtot % BK == 0);
    const float* pa[NVA];
    const float* pbq[NVB];
    if (TAG & 1) {
#pragma unroll
        for (int i = 0; i < NVA; ++i) pa[i] = dy + (size_t)(ak_l + i * (1024 / BM)) * g.Co + min(r_0 + 4 * a_q, R - 4);
#pragma unroll
        for (int i = 0; i < NVB; ++i) pbq[i] = x + (size_t)(bk_l + i * (1024 / BN)) * g.Ci + min(n0 + 4 * b_q, N - 4);
    }
    auto load_a = [&](int c, float4 (&va)[NVA]) {
        if (plain) {
#pragma unroll
            for (int i = 0; i < NVA; ++i) va[i] = ld4(pa[i] + (size_t)c * BK * g.Co);
            return;
        }
#pragma unroll
        for (int i = 0; i < NVA; ++i) {
            const int m = c * BK + ak_l + i * (1024 / BM);
            const int co = r_0 + 4 * a_q;
            va[i] = zero4();
            if (m >= Mtot) continue;
            if (VECA) {
                if (co < R) va[i] = ld4(dy + (unsigned)m * (unsigned)g.Co + (unsigned)co);
            } else {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = (co + j < R) ? dy[(size_t)m * g.Co + co + j] : 0.0f;
                va[i] = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
    };
    // This thread's B taps as (ky, kx) (fixed through the loop), and its reduction pixels (b, oy, ox): chunk c stages
    // pixel m = 16 c + row, so consecutive load_b calls (which come in increasing c, each chunk exactly once) advance
    // every staged pixel by 16 -- kept as a running (b, oy, ox) instead of two integer divisions per row and chunk.
    int b_ky[4], b_kx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        b_ky[j] = b_tap[j] >= 0 ? b_tap[j] / g.KW : 0;
        b_kx[j] = b_tap[j] >= 0 ? b_tap[j] - b_ky[j] * g.KW : 0;
    }
    const int adv_oy = BK / g.OW, adv_ox = BK - adv_oy * g.OW;
    int pm[NVB], pbb[NVB], poy[NVB], pox[NVB];
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
        pm[i] = c_begin * BK + bk_l + i * (1024 / BN);
        pbb[i] = pm[i] / (g.OH * g.OW);
        const int rem = pm[i] - pbb[i] * (g.OH * g.OW);
        poy[i] = rem / g.OW;
        pox[i] = rem - poy[i] * g.OW;
    }
    auto src_pixel = [&](int b, int oy, int ox, int ky, int kx) -> int {
        int iy = oy * g.s - g.p + ky, ix = ox * g.s - g.p + kx;
        if (g.reflect) {
            iy = reflect_idx(iy, g.H);
            ix = reflect_idx(ix, g.W);
        } else if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) {
            return -1;
        }
        return (b * g.H + iy) * g.W + ix;
    };
    auto load_b = [&](int c, float4 (&vb)[NVB]) {
        if (plain) {
#pragma unroll
            for (int i = 0; i < NVB; ++i) vb[i] = ld4(pbq[i] + (size_t)c * BK * g.Ci);
            return;
        }
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            const int m = pm[i], b = pbb[i], oy = poy[i], ox = pox[i];
            // advance this row's pixel to the next chunk
            pm[i] += BK;
            pox[i] += adv_ox;
            poy[i] += adv_oy;
            if (pox[i] >= g.OW) { pox[i] -= g.OW; ++poy[i]; }
            while (poy[i] >= g.OH) { poy[i] -= g.OH; ++pbb[i]; }
            vb[i] = zero4();
            if (m >= Mtot) continue;
            if (VECB) {
                if (b_tap[0] < 0) continue;
                const int px = src_pixel(b, oy, ox, b_ky[0], b_kx[0]);
                if (px >= 0) vb[i] = ld4(x + (unsigned)px * (unsigned)g.Ci + (unsigned)b_ci[0]);
            } else {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    e[j] = 0.0f;
                    if (b_tap[j] < 0) continue;
                    const int px = src_pixel(b, oy, ox, b_ky[j], b_kx[j]);
                    if (px >= 0) e[j] = x[(size_t)px * g.Ci + b_ci[j]];
                }
                vb[i] = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
    };

    f32x16 acc[MB][NB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) acc[mi][ni] = f32x16{0};
    const int wm0 = (wave >> 1) * (BM / 2), wn0 = (wave & 1) * (BN / 2);

    float4 va[NVA], vb[NVB];
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NVA; ++i) st_rowcontig<LDA, ((TAG & 2) != 0)>(As(buf), ak_l + i * (1024 / BM), 4 * a_q, va[i]);
#pragma unroll
        for (int i = 0; i < NVB; ++i) st_rowcontig<LDB, ((TAG & 2) != 0)>(Bs(buf), bk_l + i * (1024 / BN), 4 * b_q, vb[i]);
    };
    if (c_begin < c_end) {
        load_a(c_begin, va);
        load_b(c_begin, vb);
        stash(0);
    }
    __syncthreads();
    if (c_begin + 1 < c_end) {
        load_a(c_begin + 1, va);
        load_b(c_begin + 1, vb);
    }
    for (int c = c_begin; c < c_end; ++c) {
        const int cur = (c - c_begin) & 1;
        auto f0 = [&]() { if (c + 1 < c_end) stash(cur ^ 1); };
        auto f1 = [&]() { if (c + 2 < c_end) { load_a(c + 2, va); load_b(c + 2, vb); } };
        if ((TAG & 2) != 0) mma_chunk_h<MB, NB, LDA, LDB>(As(cur), Bs(cur), acc, wm0, wn0, lane, f0, f1);
        else mma_chunk<MB, NB, LDA, LDB>(As(cur), Bs(cur), acc, wm0, wn0, lane, f0, f1);
        __syncthreads();
    }

    float* o = out + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * ((size_t)R * N) ;
    if (gridDim.z == 1) o = out + (size_t)blockIdx.y * bt.so;
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) {
            const int col = n0 + wn0 + 32 * ni + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = r_0 + wm0 + 32 * mi + mfma32_row(r, lane);
                if (row < R && col < N) {
                    const size_t idx = (size_t)row * N + col;
                    o[idx] = accumulate ? o[idx] + acc[mi][ni][r] : acc[mi][ni][r];
                }
            }
        }
}

__global__ void splitk_reduce_kernel(const float* __restrict__ part, int S, size_t n, float* __restrict__ out,
                                     int accumulate) {
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 s = zero4();
        int z = 0;
        for (; z + 3 < S; z += 4) {          // four slabs per trip in flight; added in slab order (the same bits)
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = ld4(part + (size_t)(z + u) * n + 4 * i);
#pragma unroll
            for (int u = 0; u < 4; ++u) add4(s, v[u]);
        }
        for (; z < S; ++z) add4(s, ld4(part + (size_t)z * n + 4 * i));
        if (accumulate) add4(s, ld4(out + 4 * i));
        *reinterpret_cast<float4*>(out + 4 * i) = s;
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
            float s = 0.0f;
            for (int z = 0; z < S; ++z) s += part[(size_t)z * n + i];
            out[i] = accumulate ? out[i] + s : s;
        }
}

// split-K epilogue of the forward / data-gradient passes: out = act(sum_s part[s] + bias[col])
// addend (optional): out = result + addend -- a skip connection's gradient joining a data gradient (mg_wino_tiles.add), added in
// float32 AFTER the float16 rounding of an autocast result, exactly where the separate add launch put it
__global__ void splitk_epilogue_kernel(const float* __restrict__ part, int S, size_t n, int N,
                                       const float* __restrict__ bias, int act, float* __restrict__ out,
                                       int round_f16 = 0, const float* __restrict__ addend = nullptr) {
    const size_t n4 = n / 4;   // launcher guarantees N % 4 == 0
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 s = zero4();
        int z = 0;
        for (; z + 3 < S; z += 4) {          // four slabs per trip in flight; added in slab order (the same bits)
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = ld4(part + (size_t)(z + u) * n + 4 * i);
#pragma unroll
            for (int u = 0; u < 4; ++u) add4(s, v[u]);
        }
        for (; z < S; ++z) add4(s, ld4(part + (size_t)z * n + 4 * i));
        if (bias) add4(s, ld4(bias + (4 * i) % N));
        s.x = apply_act(s.x, act); s.y = apply_act(s.y, act); s.z = apply_act(s.z, act); s.w = apply_act(s.w, act);
        if (round_f16) { s.x = round_h(s.x); s.y = round_h(s.y); s.z = round_h(s.z); s.w = round_h(s.w); }
        if (addend) add4(s, ld4(addend + 4 * i));
        *reinterpret_cast<float4*>(out + 4 * i) = s;
    }
}

// column sums of a [M, C] matrix.  part[blockIdx.y][c] = sum over this block's row slice; with final != 0 (single
// slice) the result goes straight to out[c] (+= when accumulate).
__global__ void colsum_partial_kernel(const float* __restrict__ a, long long M, int C, long long rows_per_split,
                                      float* __restrict__ part, int final, int accumulate) {
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
    const long long m_begin = (long long)blockIdx.y * rows_per_split;
    const long long m_end = min(M, m_begin + rows_per_split);
    float s = 0.0f;
    if (c < C) {
        // eight rows per trip: their loads are in flight together (one 4-byte load per thread and trip is pure latency); the
        // additions keep the row order -- the same bits
        long long m = m_begin + rg;
        for (; m + 28 < m_end; m += 32) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = a[(m + 4 * u) * C + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; m < m_end; m += 4) s += a[m * C + c];
    }
    red[rg][threadIdx.x & 63] = s;
    __syncthreads();
    if (rg == 0 && c < C) {
        const float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (final) part[c] = accumulate ? part[c] + v : v;
        else part[(size_t)blockIdx.y * C + c] = v;
    }
}

// The split-K combine launches.  blocks: the caller's grid rule over the n / 4 float4s of the result (conv_grid, wino_grid,
// h16_grid); the kernels walk grid strides, so any count >= 1 gives the same bits.
inline unsigned conv_grid(size_t n4) {
    const size_t b = (n4 + 255) / 256;
    return (unsigned)(b > 4096 ? 4096 : b);
}
inline void splitk_epilogue(unsigned blocks, const float* part, int splits, size_t n, int N, const float* bias, int act, float* out,
                            int round_f16, hipStream_t st, const float* addend = nullptr) {
    hipLaunchKernelGGL(splitk_epilogue_kernel, dim3(blocks), dim3(256), 0, st, part, splits, n, N, bias, act, out, round_f16, addend);
}
inline void splitk_reduce(unsigned blocks, const float* part, int splits, size_t n, float* out, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, part, splits, n, out, accumulate);
}

}  // namespace
