// What the frame kernels of the multi-resolution STFT loss (stft_loss_rows.hip) and of the mel-spectrogram loss (mel_loss_rows.hip)
// share: the clamp of the magnitudes, the tile of SD_TILE complex double points per workgroup, the transform of lsd_fft.h restated
// for a vector type (double2 forward, float2 for the inverse), the staging of the windowed, reflected frames in double, the split
// into "the float32 spectrum of the definition", the sum of a frame's lanes (sd_frame_sum), the whole tail of the backward frames
// kernels from the Hermitian spectrum in registers to the windowed frames in the workspace (sd_inverse_tail) and the test of a
// row's frame range.  Each statement stands here once so that the two losses cannot drift apart; stft_loss_rows.hip's head says why
// the forward transform runs in double.  Beneath this header, frames_common.h holds what the LSD backward shares as well.
// Deliberately NOT shared between the two losses: the seeded upstream gradient (the STFT loss uses the double quotient unrounded,
// the mel loss rounds it to float32 first; both are asserted bit for bit) and the two finish kernels (different formulas).
#pragma once
#include <math.h>

#include "frames_common.h"

namespace {

constexpr double kStftClamp = 1e-7;
constexpr int SD_TILE = 2048;       // complex double points of frame data per workgroup: 32 KiB

// ---- the transform of lsd_fft.h restated for a vector type V (double2 forward, float2 for the inverse): the same Stockham stages,
// split and roots; a stage may have fewer butterflies than the workgroup has threads, and the roots exp(-2 pi i t / N) are kept
// as doubles for t < N/2 only (root[t + N/2] = -root[t]), rounded to float32 once where the float32 inverse reads them ----
__device__ __forceinline__ float2 sd_mk(float a, float b) { return make_float2(a, b); }
__device__ __forceinline__ double2 sd_mk(double a, double b) { return make_double2(a, b); }
__device__ __forceinline__ void sd_cvt(double2 a, double2& o) { o = a; }
__device__ __forceinline__ void sd_cvt(double2 a, float2& o) { o = make_float2((float)a.x, (float)a.y); }

template <typename V>
__device__ __forceinline__ V sd_cmul(V a, V b) { return sd_mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

template <int N, typename V>
__device__ __forceinline__ V sd_root(const double2* __restrict__ root, int t) {
    const double2 r = root[t & (N / 2 - 1)];
    V o;
    sd_cvt((t & (N / 2)) ? make_double2(-r.x, -r.y) : r, o);
    return o;
}

template <int N>
__device__ __forceinline__ void sd_roots(double2* __restrict__ root, int tid) {
    for (int t = tid; t < N / 2; t += LSD_NT) {
        double sn, cs;
        sincospi(-2.0 * (double)t / (double)N, &sn, &cs);
        root[t] = make_double2(cs, sn);
    }
}

template <int R, typename V>
__device__ __forceinline__ void sd_butterfly(V (&v)[R]) {
    if (R == 2) {
        const V a = v[0], b = v[1];
        v[0] = sd_mk(a.x + b.x, a.y + b.y);
        v[1] = sd_mk(a.x - b.x, a.y - b.y);
    } else if (R == 4) {
        const V a0 = sd_mk(v[0].x + v[2].x, v[0].y + v[2].y), a1 = sd_mk(v[0].x - v[2].x, v[0].y - v[2].y);
        const V a2 = sd_mk(v[1].x + v[3].x, v[1].y + v[3].y), a3 = sd_mk(v[1].x - v[3].x, v[1].y - v[3].y);
        v[0] = sd_mk(a0.x + a2.x, a0.y + a2.y);
        v[2] = sd_mk(a0.x - a2.x, a0.y - a2.y);
        v[1] = sd_mk(a1.x + a3.y, a1.y - a3.x);      // a1 - i a3
        v[3] = sd_mk(a1.x - a3.y, a1.y + a3.x);      // a1 + i a3
    } else {
        V e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
        sd_butterfly<4>(e);
        sd_butterfly<4>(o);
        const decltype(v[0].x) H = (decltype(v[0].x))0.70710678118654752440;
        const V t0 = o[0];
        const V t1 = sd_mk((o[1].x + o[1].y) * H, (o[1].y - o[1].x) * H);        // (1 - i) / sqrt 2
        const V t2 = sd_mk(o[2].y, -o[2].x);                                      // -i
        const V t3 = sd_mk((o[3].y - o[3].x) * H, (-o[3].x - o[3].y) * H);       // (-1 - i) / sqrt 2
        v[0] = sd_mk(e[0].x + t0.x, e[0].y + t0.y); v[4] = sd_mk(e[0].x - t0.x, e[0].y - t0.y);
        v[1] = sd_mk(e[1].x + t1.x, e[1].y + t1.y); v[5] = sd_mk(e[1].x - t1.x, e[1].y - t1.y);
        v[2] = sd_mk(e[2].x + t2.x, e[2].y + t2.y); v[6] = sd_mk(e[2].x - t2.x, e[2].y - t2.y);
        v[3] = sd_mk(e[3].x + t3.x, e[3].y + t3.y); v[7] = sd_mk(e[3].x - t3.x, e[3].y - t3.y);
    }
}

// lsd_stage over the TILE / P transforms of P points in buf; root: the half table of N = 2 P.  Both barriers inside.
template <int P, int R, int NS, int TILE, typename V>
__device__ __forceinline__ void sd_stage(V* __restrict__ buf, const double2* __restrict__ root, int tid) {
    constexpr int NB = P / R, TOT = (TILE / P) * NB, IT = (TOT + LSD_NT - 1) / LSD_NT;
    V v[IT][R];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * LSD_NT, fr = idx / NB, j = idx % NB;
        if (idx < TOT) {
#pragma unroll
            for (int r = 0; r < R; ++r) v[it][r] = buf[fr * P + j + r * NB];
            if (NS > 1) {
                const int k = j % NS;
#pragma unroll
                for (int r = 1; r < R; ++r) v[it][r] = sd_cmul(v[it][r], sd_root<2 * P, V>(root, 2 * (r * k * (P / (NS * R)))));
            }
            sd_butterfly<R>(v[it]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * LSD_NT, fr = idx / NB, j = idx % NB;
        const int d = (j / NS) * NS * R + j % NS;
        if (idx < TOT) {
#pragma unroll
            for (int r = 0; r < R; ++r) buf[fr * P + d + r * NS] = v[it][r];
        }
    }
    __syncthreads();
}

template <int P, int NS, int TILE, typename V>
__device__ __forceinline__ void sd_stages8(V* buf, const double2* root, int tid) {
    sd_stage<P, 8, NS, TILE>(buf, root, tid);
    if constexpr (NS * 8 < P) sd_stages8<P, NS * 8, TILE>(buf, root, tid);
}

// Stage radices as lsd_fft: P = 256: 4 8 8;  P = 512: 8 8 8;  P = 1024: 2 8 8 8.
template <int P, int TILE, typename V>
__device__ __forceinline__ void sd_fft(V* buf, const double2* root, int tid) {
    constexpr int REM = lsd_log2(P) % 3;
    if constexpr (REM == 0) {
        sd_stages8<P, 1, TILE>(buf, root, tid);
    } else {
        sd_stage<P, 1 << REM, 1, TILE>(buf, root, tid);
        sd_stages8<P, 1 << REM, TILE>(buf, root, tid);
    }
}

// lsd_real_bin in double, rounded to float32 once: THE float32 spectrum of the definition
template <int M>
__device__ __forceinline__ float2 sd_real_bin(const double2* __restrict__ Z, int k, const double2* __restrict__ root) {
    const double2 zk = Z[k & (M - 1)], zm = Z[(M - k) & (M - 1)], w = sd_root<2 * M, double2>(root, k);
    const double2 e = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));          // (Z[k] + conj Z[M-k]) / 2
    const double2 o = make_double2(0.5 * (zk.y + zm.y), 0.5 * (zm.x - zk.x));          // (Z[k] - conj Z[M-k]) / 2i
    const double2 t = sd_cmul(w, o);
    return make_float2((float)(e.x + t.x), (float)(e.y + t.y));
}

// lsd_load_tile for SD_TILE points in double: the product of the float32 sample and the float32 window is exact
template <int N>
__device__ __forceinline__ void sd_load_tile(double2* __restrict__ buf, const LsdFrame* __restrict__ info,
                                             const float* __restrict__ hr, long long hr_total, const float* __restrict__ sr,
                                             long long sr_total, const float* __restrict__ window, int center, int tid) {
    constexpr int M = N / 2;
#pragma unroll 4
    for (int i = tid; i < SD_TILE; i += LSD_NT) {
        const int fr = i / N, is_sr = (i / M) & 1, m = i % M;
        const LsdFrame fi = info[fr];
        const float* __restrict__ x = is_sr ? sr : hr;
        const long long at = is_sr ? fi.sr_at : fi.hr_at, total = is_sr ? sr_total : hr_total;
        double e[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            long long t = fi.first + 2 * m + q;
            if (center) {
                if (t < 0) t = -t;
                if (t >= fi.len) t = 2 * (fi.len - 1) - t;
            }
            float v = 0.0f;
            if (fi.live && t >= 0 && t < fi.len) {
                const long long p = at + t;
                if (p >= 0 && p < total) v = x[p];
            }
            e[q] = (double)v * (double)window[2 * m + q];
        }
        buf[i] = make_double2(e[0], e[1]);
    }
}

// acc[q], q < Q, summed over the TPF lanes of frame fr (lane j of the frame): a wave's tree, then for a frame of several waves
// the hand-off through red and the ascending sum on lane j == 0, which alone ends with the sums.  One barrier where TPF > 64.
template <int Q, int TPF>
__device__ __forceinline__ void sd_frame_sum(double (&acc)[Q], double (*red)[Q], int tid, int fr, int j) {
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = wave_sum_d(acc[q]);
    if (TPF > 64) {
        if ((tid & 63) == 0) {
#pragma unroll
            for (int q = 0; q < Q; ++q) red[tid >> 6][q] = acc[q];
        }
        __syncthreads();
        if (j == 0) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                acc[q] = red[fr * (TPF / 64)][q];
                for (int w = 1; w < TPF / 64; ++w) acc[q] += red[fr * (TPF / 64) + w][q];
            }
        }
    }
}

// The tail of a backward frames kernel, from "the Hermitian spectrum H_k (G_k / 2 for 0 < k < N/2, Re G_k for k = 0, N/2, rounded
// to float32) of bins k = j + i TPF of frame fr = tid / TPF is in h[i]" to "y[n] window[n] of the tile's frames is in frames_out
// [total_frames][N]".  The caller's barrier comes first: every lane has read what lies in fbuf, the tile's SD_TILE double2 seen as
// float2.  H_k goes to fbuf[fr N + k] (the frames' regions fill half of the buffer); the inverse real transform is the adjoint of
// the forward's pack-and-split (lsd_rows_grad.hip's head has the algebra): conj Zt of every frame is held in registers until all H
// are read, packed densely as [FT][M], the forward stages run on it in float32, and the result is stored in 16-byte stores.
template <int N, int BPL>
__device__ __forceinline__ void sd_inverse_tail(const float2 (&h)[BPL], float2* fbuf, const double2* root, const float* window,
                                                float* frames_out, long long tile, long long total_frames, int tid) {
    constexpr int M = N / 2, FT = SD_TILE / N, TPF = LSD_NT / FT, NBINS = N / 2 + 1, HALF = SD_TILE / 2;
    static_assert(BPL == (NBINS + TPF - 1) / TPF, "h holds the lane's bins");
    static_assert(HALF % LSD_NT == 0 && (HALF / 2) % LSD_NT == 0 && M % 2 == 0, "whole points and whole point pairs per thread");
    const int fr = tid / TPF, j = tid % TPF;
#pragma unroll
    for (int i = 0; i < BPL; ++i) {
        const int k = j + i * TPF;
        if (k < NBINS) fbuf[fr * N + k] = h[i];
    }
    __syncthreads();
    float2 zt[HALF / LSD_NT];
#pragma unroll
    for (int it = 0; it < HALF / LSD_NT; ++it) {
        const int idx = tid + it * LSD_NT, f2 = idx / M, k = idx % M;
        zt[it] = frames_conj_zt(fbuf[f2 * N + k], fbuf[f2 * N + M - k], sd_root<N, float2>(root, k));
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < HALF / LSD_NT; ++it) fbuf[tid + it * LSD_NT] = zt[it];
    __syncthreads();
    sd_fft<M, HALF>(fbuf, root, tid);
    // y[2m] = Re, y[2m+1] = -Im of the transform; two points = four samples per store
#pragma unroll
    for (int it = 0; it < HALF / 2 / LSD_NT; ++it) {
        const int idx = tid + it * LSD_NT, f2 = idx / (M / 2), n = 4 * (idx % (M / 2));
        const long long g = tile * FT + f2;
        if (g < total_frames) {
            const float4 v = *reinterpret_cast<const float4*>(fbuf + f2 * M + n / 2);
            *reinterpret_cast<float4*>(frames_out + g * N + n) =
                make_float4(v.x * window[n], -v.y * window[n + 1], v.z * window[n + 2], -v.w * window[n + 3]);
        }
    }
}

// a row whose frames [f0, f0 + nf) the frame kernels served
__device__ __forceinline__ bool stft_row_frames(const mg_metric_row* __restrict__ rows, const long long* __restrict__ frame_start,
                                                long long total_frames, int u, long long& f0, long long& nf) {
    f0 = frame_start[u];
    nf = frame_start[u + 1] - f0;
    return lsd_row_ok(rows[u]) && f0 >= 0 && nf > 0 && nf - 1 <= INT_MAX && f0 + nf <= total_frames;
}

}  // namespace
