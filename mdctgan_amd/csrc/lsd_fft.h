// What lsd_rows_kernel (metrics_rows.hip), its backward (lsd_rows_grad.hip) and the STFT loss (stft_loss_rows.hip) share: the tile of LSD_TILE complex points per
// workgroup of LSD_NT threads, the search of a frame's row, the staging of the windowed, reflected frames as packed complex
// points, the Stockham stages in LDS and the split of a packed transform into the bins of the real one.  The comments at the
// head of metrics_rows.hip describe all of it; each statement stands here once so that the kernels cannot drift apart.
// ONE restated copy exists: stft_loss_rows.hip and mel_loss_rows.hip need these stages, the split and the staging for double2 on a
// smaller tile (their sign and clamp decisions want a spectrum that is accurate per bin) and share them as the sd_* templates of
// stft_frames.h, so that
// nothing here -- and no bit of the LSD -- changes.  A change to the statements below belongs there as well.
// What the LSD backward shares with those two losses all the same stands in frames_common.h: the conj Zt of the inverse tail (the
// root value is the caller's) and the host side -- operand checks, grid, n_fft dispatch, the backward's epilogue.  Deliberately NOT
// shared: this transform (float2, LSD_TILE, the N-entry root table) and with it the rest of lsd_rows_grad_frames_kernel's tail,
// its windowed store included -- stated through a shared function the store compiles to other instructions at N = 512 and 2048
// (same arithmetic, other registers and order), and the LSD metric's kernels are not to change at all; the LSD kernel's reduction,
// in which every lane ends with the sum; and every loss's own expression for the seeded upstream gradient.
#pragma once
#include <limits.h>

#include "rows.h"

constexpr int LSD_NT = 256;
constexpr int LSD_TILE = 4096;      // complex points of frame data per workgroup

inline bool lsd_size_ok(int n_fft) { return n_fft == 512 || n_fft == 1024 || n_fft == 2048; }

__device__ __forceinline__ float2 lsd_cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

template <int R>
__device__ __forceinline__ void lsd_butterfly(float2 (&v)[R]) {
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
        lsd_butterfly<4>(e);
        lsd_butterfly<4>(o);
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

// One Stockham stage over the TILE / P transforms of P points in the tile.  buf: [TILE / P][P] complex; NS = size of the
// sub-transforms done so far; root[t] = exp(-2 pi i t / 2P).  Butterfly j of a transform reads points j + r P / R and writes
// (j / NS) NS R + j % NS + r NS.  Contains both barriers: on entry every earlier write to buf must already be fenced by the
// caller's barrier.
template <int P, int R, int NS, int TILE = LSD_TILE>
__device__ __forceinline__ void lsd_stage(float2* __restrict__ buf, const float2* __restrict__ root, int tid) {
    constexpr int NB = P / R, FT = TILE / P, IT = FT * NB / LSD_NT;
    static_assert(FT * NB % LSD_NT == 0, "whole butterflies per thread");
    float2 v[IT][R];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * LSD_NT, fr = idx / NB, j = idx % NB;
#pragma unroll
        for (int r = 0; r < R; ++r) v[it][r] = buf[fr * P + j + r * NB];
        if (NS > 1) {
            const int k = j % NS;
#pragma unroll
            for (int r = 1; r < R; ++r) v[it][r] = lsd_cmul(v[it][r], root[2 * (r * k * (P / (NS * R)))]);
        }
        lsd_butterfly<R>(v[it]);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * LSD_NT, fr = idx / NB, j = idx % NB;
        const int d = (j / NS) * NS * R + j % NS;
#pragma unroll
        for (int r = 0; r < R; ++r) buf[fr * P + d + r * NS] = v[it][r];
    }
    __syncthreads();
}

template <int P, int NS, int TILE = LSD_TILE>
__device__ __forceinline__ void lsd_stages8(float2* buf, const float2* root, int tid) {
    lsd_stage<P, 8, NS, TILE>(buf, root, tid);
    if constexpr (NS * 8 < P) lsd_stages8<P, NS * 8, TILE>(buf, root, tid);
}

constexpr int lsd_log2(int n) { int l = 0; while (n > 1) { n >>= 1; ++l; } return l; }

// Stage radices: P = 256: 4 8 8;  P = 512: 8 8 8;  P = 1024: 2 8 8 8.
template <int P, int TILE = LSD_TILE>
__device__ __forceinline__ void lsd_fft(float2* buf, const float2* root, int tid) {
    constexpr int REM = lsd_log2(P) % 3;
    if constexpr (REM == 0) {
        lsd_stages8<P, 1, TILE>(buf, root, tid);
    } else {
        lsd_stage<P, 1 << REM, 1, TILE>(buf, root, tid);
        lsd_stages8<P, 1 << REM, TILE>(buf, root, tid);
    }
}

// X[k] of the real transform whose packed M-point transform is Z, k = 0 .. M; w = exp(-2 pi i k / 2M)
template <int M>
__device__ __forceinline__ float2 lsd_real_bin(const float2* __restrict__ Z, int k, float2 w) {
    const float2 zk = Z[k & (M - 1)], zm = Z[(M - k) & (M - 1)];
    const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));          // (Z[k] + conj Z[M-k]) / 2
    const float2 o = make_float2(0.5f * (zk.y + zm.y), 0.5f * (zm.x - zk.x));          // (Z[k] - conj Z[M-k]) / 2i
    const float2 t = lsd_cmul(w, o);
    return make_float2(e.x + t.x, e.y + t.y);
}

// root[t] = exp(-2 pi i t / N), evaluated in double (sincospi of an exactly representable argument) and rounded once
template <int N>
__device__ __forceinline__ void lsd_roots(float2* __restrict__ root, int tid) {
    for (int t = tid; t < N; t += LSD_NT) {
        double s, c;
        sincospi(-2.0 * (double)t / (double)N, &s, &c);
        root[t] = make_float2((float)c, (float)s);
    }
}

// a metric row that the frame kernels serve (a table that does not agree with itself gives silent frames, never a read outside
// the row)
__device__ __forceinline__ bool lsd_row_ok(const mg_metric_row& rw) {
    return rw.len > 0 && rw.len <= INT_MAX && rw.hr_pos > -kFar && rw.hr_pos < kFar && rw.sr_pos > -kFar && rw.sr_pos < kFar;
}

struct LsdFrame { long long hr_at, sr_at, len, first; float shift; int live; };     // `first`: sample of the row under window tap 0

// The row of frame g of the flattened frame index: the last u with frame_start[u] <= g (rows without frames share a start and
// lose).  -> the frame's place (live == 0: a silent frame) and its row.
template <bool SHIFT>
__device__ __forceinline__ LsdFrame lsd_locate(long long g, const mg_metric_row* __restrict__ rows, int n_rows,
                                               const long long* __restrict__ frame_start, long long total_frames,
                                               const float* __restrict__ shift, int n_fft, int hop, int center, int& row) {
    LsdFrame fi = {0, 0, 0, 0, 0.0f, 0};
    row = 0;
    if (g < total_frames) {
        int lo = 0, hi = n_rows;                       // invariant: the answer is in [lo, hi)
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (frame_start[mid] <= g) lo = mid; else hi = mid;
        }
        const mg_metric_row rw = rows[lo];
        const long long f = g - frame_start[lo];
        if (rw.len > 0 && rw.len <= INT_MAX && f >= 0 && f < frame_start[lo + 1] - frame_start[lo] && f <= INT_MAX &&
            rw.hr_pos > -kFar && rw.hr_pos < kFar && rw.sr_pos > -kFar && rw.sr_pos < kFar) {      // (lsd_row_ok, f in its row)
            fi.hr_at = rw.hr_pos;
            fi.sr_at = rw.sr_pos;
            fi.len = rw.len;
            fi.first = f * hop - (center ? n_fft / 2 : 0);
            fi.shift = SHIFT ? shift[lo] : 0.0f;
            fi.live = 1;
            row = lo;
        }
    }
    return fi;
}

// buf [LSD_TILE / N][hr, sr][N / 2]: z[m] = x_w[2m] + i x_w[2m+1] for hr, then for sr, of every frame of the tile.  x_w[n] =
// x[reflect(first + n)] window[n] (center; the reflection is at the row's own [0, len)) or x[first + n] window[n], one float32
// product; a sample outside the row or its buffer enters as 0.  `info` must be fenced by the caller's barrier.
template <int N, bool SHIFT>
__device__ __forceinline__ void lsd_load_tile(float2* __restrict__ buf, const LsdFrame* __restrict__ info,
                                              const float* __restrict__ hr, long long hr_total, const float* __restrict__ sr,
                                              long long sr_total, const float* __restrict__ window, int center, int tid) {
    constexpr int M = N / 2;
#pragma unroll 4
    for (int i = tid; i < LSD_TILE; i += LSD_NT) {
        const int fr = i / N, is_sr = (i / M) & 1, m = i % M;
        const LsdFrame fi = info[fr];
        const float* __restrict__ x = is_sr ? sr : hr;
        const long long at = is_sr ? fi.sr_at : fi.hr_at, total = is_sr ? sr_total : hr_total;
        float e[2];
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
                if (p >= 0 && p < total) v = (SHIFT && !is_sr) ? x[p] + fi.shift : x[p];
            }
            e[q] = v * window[2 * m + q];
        }
        buf[i] = make_float2(e[0], e[1]);
    }
}
