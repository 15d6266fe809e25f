// Winograd F(2x2, 3x3) with two-byte images for the forward passes of half-precision inference (opt-in:
// MG_PRECISION_F16_INFER).  The arithmetic is the float16 branch of wino.h's -- U = G w G^T and V = B^T d B rounded to float16
// once (U from float32 sums, V from exact ones: wh_input_image), exact products on v_mfma_f32_32x32x16_f16, float32
// accumulation, the convolution output rounded through float16 -- but the rounded images are what lives in HBM:
//   U16[16][Co][Ci], V16[16][T][Ci] (float16), M[16][T][Co] (float32), T = B * H/2 * W/2 tiles.
// Three launches per trunk layer: the image transform (skipped when the layer in front handed its image over), one batched
// 16-position GEMM on LDS-DMA staging (winoh_gemm_kernel: hgemm_kernel's loop with the position on the grid), and
// winoh_out_norm_kernel, the float16 counterpart of wino_out_norm_kernel (inverse transform, InstanceNorm, activation, residual,
// the next layer's V16).  Forward only: no gradient pass exists for these images.
// Needs: wino.h (bt4, f4add ...), dense_gemm.h (dg_dma16, dg_wait_vmcnt), dense_gemm_h.h (HG_BK), conv_plan.h (mg_launch).
#pragma once

namespace {

typedef _Float16 wh_h4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ wh_h4 wh_pack(const float4 v) { return wh_h4{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w}; }
__device__ __forceinline__ float4 wh_round4(float4 v) { return make_float4(round_h(v.x), round_h(v.y), round_h(v.z), round_h(v.w)); }

__device__ __forceinline__ float wh_comp(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
// out[4 r + c] = float16(B^T d B)[r][c] of four channels.  The two passes of bt4 run in double, where these sums of four float32
// values are exact, so the image is the correctly rounded float16 of the exact transform: a float32 transform leaves up to 2^-22 of
// the patch's magnitude on an element that cancels to almost nothing, several float16 ulps of such an element.
__device__ __forceinline__ void wh_input_image(const float4 (&d)[4][4], wh_h4 (&out)[16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double t[4][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double d0 = wh_comp(d[0][c], j), d1 = wh_comp(d[1][c], j), d2 = wh_comp(d[2][c], j), d3 = wh_comp(d[3][c], j);
            t[0][c] = d0 - d2; t[1][c] = d1 + d2; t[2][c] = d2 - d1; t[3][c] = d1 - d3;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            out[4 * r + 0][j] = (_Float16)(t[r][0] - t[r][2]);
            out[4 * r + 1][j] = (_Float16)(t[r][1] + t[r][2]);
            out[4 * r + 2][j] = (_Float16)(t[r][2] - t[r][1]);
            out[4 * r + 3][j] = (_Float16)(t[r][1] - t[r][3]);
        }
    }
}

// U16[16][Co][Ci] = float16(G g G^T) from OHWI weights [Co][3][3][Ci]: wino_weight_xform_kernel's arithmetic, rounded once
__global__ void winoh_weight_xform_kernel(const float* __restrict__ w, int Co, int Ci, _Float16* __restrict__ U) {
    const int C4 = Ci / 4;
    const size_t total = (size_t)Co * C4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4), co = (int)(i / C4);
        float4 g[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) g[r][c] = ld4(w + ((size_t)(co * 3 + r) * 3 + c) * Ci + 4 * c4);
        float4 tmp[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            tmp[0][c] = g[0][c];
            tmp[1][c] = f4scale(f4add(f4add(g[0][c], g[1][c]), g[2][c]), 0.5f);
            tmp[2][c] = f4scale(f4add(f4sub(g[0][c], g[1][c]), g[2][c]), 0.5f);
            tmp[3][c] = g[2][c];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float4 o[4];
            o[0] = tmp[r][0];
            o[1] = f4scale(f4add(f4add(tmp[r][0], tmp[r][1]), tmp[r][2]), 0.5f);
            o[2] = f4scale(f4add(f4sub(tmp[r][0], tmp[r][1]), tmp[r][2]), 0.5f);
            o[3] = tmp[r][2];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                *reinterpret_cast<wh_h4*>(U + ((size_t)(r * 4 + c) * Co + co) * Ci + 4 * c4) = wh_pack(o[c]);
        }
    }
}

// V16[16][T][C] = float16(B^T d B), patch origin (2 ty - 1, 2 tx - 1): wino_input_xform_kernel's gather, wh_input_image's sums
__global__ void winoh_input_xform_kernel(const float* __restrict__ x, int B, int H, int W, int C, int TH, int TW, int reflect,
                                         _Float16* __restrict__ V) {
    const int C4 = C / 4;
    const size_t T = (size_t)B * TH * TW, total = T * C4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const size_t t = i / C4;
        const int tx = (int)(t % TW), ty = (int)((t / TW) % TH), b = (int)(t / ((size_t)TW * TH));
        float4 d[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int iy = 2 * ty - 1 + r;
            bool oky = true;
            if (reflect) iy = reflect_idx(iy, H); else oky = (iy >= 0 && iy < H);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                int ix = 2 * tx - 1 + c;
                bool ok = oky;
                if (reflect) ix = reflect_idx(ix, W); else ok = ok && (ix >= 0 && ix < W);
                d[r][c] = ok ? ld4(x + ((size_t)(b * H + iy) * W + ix) * C + 4 * c4) : zero4();
            }
        }
        wh_h4 o[16];
        wh_input_image(d, o);
#pragma unroll
        for (int p = 0; p < 16; ++p) *reinterpret_cast<wh_h4*>(V + ((size_t)p * T + t) * C + 4 * c4) = o[p];
    }
}

// ---- the 16 position GEMMs as one launch: M[p][T][Co] (float32) = V16[p][T][K] * U16[p][Co][K]^T -----------------------------
// hgemm_kernel's loop (dense_gemm_h.h): 64-deep chunks = 128-byte rows, XOR-swizzled unpadded LDS images filled by
// buffer_load ... lds with counted vmcnt, NBUF buffers, one barrier per chunk, one ds_read_b128 per MFMA operand.  The position is
// part of the flat grid (as in dgemm32g_kernel), every position has its own buffer descriptors, the k order is fixed and nothing
// is split or atomically added: the result is a function of the operands alone.  Rows of a ragged last tile load a clamped row
// (never stored); K % 64 == 0, N % 64 == 0, and one position's operand stays below 2 GiB (winoh_ok).
struct WhArgs {
    const _Float16* A;       // V16 [P][M][K]
    const _Float16* B;       // U16 [P][N][K]
    float* C;                // [P][M][N]
    int M, N, K, P;
    int tiles_m, tiles_n;
};

template <int BM, int BN, int WGM, int WGN, int NBUF>
__global__ __launch_bounds__(64 * WGM * WGN) void winoh_gemm_kernel(WhArgs g) {
#if defined(__HIP_DEVICE_COMPILE__)
    using Cfg = HgCfg<BM, BN, WGM, WGN, false, NBUF>;
    constexpr int MB = Cfg::MB, NB = Cfg::NB, PA = Cfg::PA, PB = Cfg::PB;
    extern __shared__ __attribute__((aligned(1024))) float wh_smem[];
    float* As0 = wh_smem;
    float* Bs0 = wh_smem + NBUF * Cfg::ASZ;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles = g.tiles_m * g.tiles_n;
    const int L = xcd_remap(blockIdx.x, tiles * g.P);
    // consecutive L share the position and the n tile: an XCD streams one [BN][K] panel of U16 through its L2 for all m tiles
    const int z = L / tiles;
    const int rem = L - z * tiles;
    const int tn = rem / g.tiles_m, tm = rem - tn * g.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int chunks = g.K / HG_BK;

    auto make_rsrc = [](const void* p, unsigned bytes) -> dg_v4i {
        const unsigned long long a = (unsigned long long)p;
        dg_v4i r;
        r[0] = (int)(unsigned)a;
        r[1] = (int)((unsigned)(a >> 32) & 0xffffu);
        r[2] = (int)bytes;
        r[3] = 0x00020000;
        return r;
    };
    const dg_v4i ra = make_rsrc(g.A + (size_t)z * g.M * g.K, (unsigned)g.M * (unsigned)g.K * 2u);
    const dg_v4i rb = make_rsrc(g.B + (size_t)z * g.N * g.K, (unsigned)g.N * (unsigned)g.K * 2u);
    unsigned va[PA], vb[PB];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int row = 8 * (wave * PA + i) + (lane >> 3), q = (lane & 7) ^ ((row >> 1) & 7);
        va[i] = (unsigned)min(m0 + row, g.M - 1) * (unsigned)g.K * 2u + 16u * q;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int row = 8 * (wave * PB + i) + (lane >> 3), q = (lane & 7) ^ ((row >> 1) & 7);
        vb[i] = (unsigned)min(n0 + row, g.N - 1) * (unsigned)g.K * 2u + 16u * q;
    }
    const unsigned lds_a0 = (unsigned)(size_t)(dg_lds_ptr)As0 + (unsigned)(wave * PA) * 1024u;
    const unsigned lds_b0 = (unsigned)(size_t)(dg_lds_ptr)Bs0 + (unsigned)(wave * PB) * 1024u;
    auto issue = [&](int c, int buf) {
        const unsigned off = (unsigned)c * (HG_BK * 2u);
        const unsigned la = lds_a0 + (unsigned)buf * (unsigned)(Cfg::ASZ * 4), lb = lds_b0 + (unsigned)buf * (unsigned)(Cfg::BSZ * 4);
#pragma unroll
        for (int i = 0; i < PA; ++i) dg_dma16(va[i], ra, la + 1024u * i, off);
#pragma unroll
        for (int i = 0; i < PB; ++i) dg_dma16(vb[i], rb, lb + 1024u * i, off);
    };

    f32x16 acc[MB][NB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) acc[mi][ni] = f32x16{0};
    const int wm0 = (wave / WGN) * (BM / WGM), wn0 = (wave % WGN) * (BN / WGN);
    const int r = lane & 31, kh = lane >> 5;

    constexpr int AHEAD = NBUF - 1, PER = PA + PB;         // chunks in flight, DMA instructions per chunk and lane
#pragma unroll
    for (int i = 0; i < AHEAD; ++i)
        if (i < chunks) issue(i, i);
    int cur = 0, nxt = AHEAD % NBUF;
    for (int c = 0; c < chunks; ++c) {
        // chunk c has landed when at most the younger chunks' instructions are outstanding (fewer near the tail: wait for all)
        if (NBUF == 2 || c + AHEAD > chunks) dg_wait_vmcnt<0>();
        else dg_wait_vmcnt<(AHEAD - 1) * PER>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (c + AHEAD < chunks) issue(c + AHEAD, nxt);
        const float* As = As0 + cur * Cfg::ASZ;
        const float* Bs = Bs0 + cur * Cfg::BSZ;
        f16x8 a[2][MB], b[2][NB];
        auto fetch = [&](int s, int buf) {
#pragma unroll
            for (int mi = 0; mi < MB; ++mi) a[buf][mi] = cd_frag_kc(As, wm0 + 32 * mi + r, s, kh);
#pragma unroll
            for (int ni = 0; ni < NB; ++ni) b[buf][ni] = cd_frag_kc(Bs, wn0 + 32 * ni + r, s, kh);
        };
        fetch(0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s + 1 < 4) fetch(s + 1, (s + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = 0; mi < MB; ++mi)
#pragma unroll
                for (int ni = 0; ni < NB; ++ni) acc[mi][ni] = mfma32x32x16h(a[s & 1][mi], b[s & 1][ni], acc[mi][ni]);
            __builtin_amdgcn_sched_barrier(0);
        }
        cur = cur + 1 == NBUF ? 0 : cur + 1;
        nxt = nxt + 1 == NBUF ? 0 : nxt + 1;
    }

    float* o = g.C + (size_t)z * g.M * g.N;
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int ni = 0; ni < NB; ++ni) {
            const int col = n0 + wn0 + 32 * ni + (lane & 31);
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int row = m0 + wm0 + 32 * mi + mfma32_row(rr, lane);
                if (row < g.M && col < g.N) o[(size_t)row * g.N + col] = acc[mi][ni][rr];
            }
        }
#endif
}

// 128 x 128 tiles (8 waves, two buffers: two workgroups per CU) where they still give every CU a workgroup, else 64 x 64 (4 waves,
// three buffers).  The one choice the launch and mg_conv_plan_name share.
inline bool winoh_big_tiles(long long T, int Co) {
    return Co % 128 == 0 && ((T + 127) / 128) * (Co / 128) * 16 >= 256;
}
template <int BM, int BN, int WGM, int WGN, int NBUF>
inline void winoh_gemm_go(WhArgs a, hipStream_t st) {
    using Cfg = HgCfg<BM, BN, WGM, WGN, false, NBUF>;
    a.tiles_m = (a.M + BM - 1) / BM;
    a.tiles_n = (a.N + BN - 1) / BN;
    static bool once = false;
    if (!once) {
        hipFuncSetAttribute((const void*)winoh_gemm_kernel<BM, BN, WGM, WGN, NBUF>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)Cfg::LDS_BYTES);
        once = true;
    }
    const unsigned grid = (unsigned)((long long)a.tiles_m * a.tiles_n * a.P);
    mg_launch(winoh_gemm_kernel<BM, BN, WGM, WGN, NBUF>, dim3(grid), dim3(Cfg::NT), Cfg::LDS_BYTES, st, a);
}
// (the 128 x 128 tile as 2 x 2 waves of 64 x 64 results -- a third fewer LDS bytes per MFMA -- measured 112.5 us against the 4 x 2
// layout's 109.0 on the 2048-tile 1024-channel trunk layer, alternating: LDS reads are not what bounds it)
inline void winoh_gemm_launch(const _Float16* V, const _Float16* U, float* Mx, long long T, int Co, int Ci, hipStream_t st) {
    const WhArgs a{V, U, Mx, (int)T, Co, Ci, 16, 0, 0};
    if (winoh_big_tiles(T, Co)) winoh_gemm_go<128, 128, 4, 2, 2>(a, st);
    else winoh_gemm_go<64, 64, 2, 2, 3>(a, st);
}
inline const char* winoh_gemm_name(long long T, int Co) {
    return winoh_big_tiles(T, Co) ? "winoh_gemm_kernel<128, 128, 4, 2, 2>" : "winoh_gemm_kernel<64, 64, 2, 2, 3>";
}

// ---- output transform + InstanceNorm2d(affine=False) (+ activation, + residual) (+ the next layer's V16) ----------------------
// wino_out_norm_kernel's scheme (a workgroup owns a sample's 32-channel slab; thread = (channel quad, tile lane), NT tiles in
// registers between the statistics and the apply; double sums, fixed-order LDS reduction) on the float16 route's values: per
// element A^T M A + bias, rounded through float16 (the convolution's output, as wino_output_xform_kernel(round_f16 = 1) leaves it),
// then the InstanceNorm of those values, activation, float32 residual add, float32 y.  y16 (optional): the float16 copy of y an
// ineligible consumer stages its operand from (what mg_instnorm_fwd_h writes).  NEXT: V16' = float16(B^T y B) for a following 3x3
// stride-1 pad-1 layer, from the plane in LDS -- winoh_input_xform_kernel's arithmetic on the same float32 values, the same bits.
struct WinohNorm {
    float eps;
    int act;
    const float* residual;
    float* y;
    float* mean;
    float* rstd;
    _Float16* y16;
    _Float16* v_next;
    int next_reflect;
};
template <int NT, bool NEXT = false>
__global__ __launch_bounds__(256) void winoh_out_norm_kernel(const float* __restrict__ Mx, int B, int TH, int TW, int C,
                                                             const float* __restrict__ bias, WinohNorm nrm,
                                                             float* __restrict__ y_raw) {
    __shared__ double red[2][32][32];
    __shared__ __attribute__((aligned(16))) float plane[NEXT ? NT * 32 * 4 * 32 : 4];      // [pixel][32 channels]
    const int cq = threadIdx.x & 7, tl = threadIdx.x >> 3;
    const int b = blockIdx.y, c0 = blockIdx.x * 32 + 4 * cq;
    const int Ts = TH * TW;
    const size_t T = (size_t)B * Ts;
    float4 v[NT][4];
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const float4 bv = bias ? ld4(bias + c0) : zero4();
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int tile = tl + 32 * i;
        if (tile < Ts) {
            const size_t t = (size_t)b * Ts + tile;
            float4 m[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) m[r][c] = ld4(Mx + ((size_t)(r * 4 + c) * T + t) * C + c0);
            float4 tmp[2][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                tmp[0][c] = f4add(f4add(m[0][c], m[1][c]), m[2][c]);
                tmp[1][c] = f4sub(f4sub(m[1][c], m[2][c]), m[3][c]);
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                v[i][2 * r] = wh_round4(f4add(f4add(f4add(tmp[r][0], tmp[r][1]), tmp[r][2]), bv));
                v[i][2 * r + 1] = wh_round4(f4add(f4sub(f4sub(tmp[r][1], tmp[r][2]), tmp[r][3]), bv));
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s1[0] += (double)v[i][q].x; s2[0] += (double)v[i][q].x * (double)v[i][q].x;
                s1[1] += (double)v[i][q].y; s2[1] += (double)v[i][q].y * (double)v[i][q].y;
                s1[2] += (double)v[i][q].z; s2[2] += (double)v[i][q].z * (double)v[i][q].z;
                s1[3] += (double)v[i][q].w; s2[3] += (double)v[i][q].w * (double)v[i][q].w;
            }
        }
    }
    // red[0/1][tile lane][channel] -> 8 partials per channel -> totals in every thread of the channel quad
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[0][tl][4 * cq + j] = s1[j];
        red[1][tl][4 * cq + j] = s2[j];
    }
    __syncthreads();
    {
        const int c = threadIdx.x & 31, part = threadIdx.x >> 5;
        double a = 0.0, bsum = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a += red[0][4 * part + i][c];
            bsum += red[1][4 * part + i][c];
        }
        __syncthreads();
        red[0][part][c] = a;
        red[1][part][c] = bsum;
    }
    __syncthreads();
    const int HW = 4 * Ts;
    float mu[4], rs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double x1 = 0.0, x2 = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            x1 += red[0][i][4 * cq + j];
            x2 += red[1][i][4 * cq + j];
        }
        const double mval = x1 / HW;
        double var = x2 / HW - mval * mval;
        if (var < 0.0) var = 0.0;
        mu[j] = (float)mval;
        rs[j] = (float)(1.0 / sqrt(var + (double)nrm.eps));
    }
    if (tl == 0) {
        *reinterpret_cast<float4*>(nrm.mean + (size_t)b * C + c0) = make_float4(mu[0], mu[1], mu[2], mu[3]);
        *reinterpret_cast<float4*>(nrm.rstd + (size_t)b * C + c0) = make_float4(rs[0], rs[1], rs[2], rs[3]);
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int tile = tl + 32 * i;
        if (tile < Ts) {
            const int ty = tile / TW, tx = tile - ty * TW;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const size_t off = ((size_t)(b * 2 * TH + 2 * ty + (q >> 1)) * (2 * TW) + 2 * tx + (q & 1)) * C + c0;
                if (y_raw) *reinterpret_cast<float4*>(y_raw + off) = v[i][q];      // (inference: nobody reads the raw output again)
                float4 o;
                o.x = apply_act((v[i][q].x - mu[0]) * rs[0], nrm.act);
                o.y = apply_act((v[i][q].y - mu[1]) * rs[1], nrm.act);
                o.z = apply_act((v[i][q].z - mu[2]) * rs[2], nrm.act);
                o.w = apply_act((v[i][q].w - mu[3]) * rs[3], nrm.act);
                if (nrm.residual) {
                    const float4 rr = ld4(nrm.residual + off);
                    o.x += rr.x; o.y += rr.y; o.z += rr.z; o.w += rr.w;
                }
                *reinterpret_cast<float4*>(nrm.y + off) = o;
                if (nrm.y16) *reinterpret_cast<wh_h4*>(nrm.y16 + off) = wh_pack(o);
                if (NEXT) *reinterpret_cast<float4*>(plane + ((2 * ty + (q >> 1)) * (2 * TW) + 2 * tx + (q & 1)) * 32 + 4 * cq) = o;
            }
        }
    }
    if (NEXT) {
        __syncthreads();
        const int H = 2 * TH, W = 2 * TW;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int tile = tl + 32 * i;
            if (tile < Ts) {
                const int ty = tile / TW, tx = tile - ty * TW;
                const size_t t = (size_t)b * Ts + tile;
                float4 d[4][4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int iy = 2 * ty - 1 + r;
                    bool oky = true;
                    if (nrm.next_reflect) iy = reflect_idx(iy, H); else oky = (iy >= 0 && iy < H);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        int ix = 2 * tx - 1 + c;
                        bool ok = oky;
                        if (nrm.next_reflect) ix = reflect_idx(ix, W); else ok = ok && (ix >= 0 && ix < W);
                        d[r][c] = ok ? *reinterpret_cast<const float4*>(plane + (iy * W + ix) * 32 + 4 * cq) : zero4();
                    }
                }
                wh_h4 o[16];
                wh_input_image(d, o);
#pragma unroll
                for (int p = 0; p < 16; ++p) *reinterpret_cast<wh_h4*>(nrm.v_next + ((size_t)p * T + t) * C + c0) = o[p];
            }
        }
    }
}

}  // namespace
