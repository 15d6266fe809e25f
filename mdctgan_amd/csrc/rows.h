// What the packed-rows kernels share (resample.hip, resample_rows.hip, train_rows.hip, metrics_rows.hip): many waveforms sit at
// aligned starts of one float32 buffer and device row tables (mg_seg_row, mg_resample_row, mg_train_row, mg_metric_row of
// include/mdctgan_hip.h, taken as they are) say where every row reads and writes.  The two loops below carry the project's
// bit-for-bit guarantees, so each is stated once:
//   tap_range + fir_chain          the polyphase tap chain of mg_resample: the taps inside the window, fmaf in ascending tap order.
//                                  A row has the same bits through every kernel that calls the pair.
//   block_sum_store + sum_chunks   the two-level double sum: per chunk quads -> wave -> red[4][N] -> ((r0 + r1) + r2) + r3, then
//                                  the chunks of a row in ascending order.  Pack-invariance of every moment and metric rests on it.
#pragma once
#include "common.h"
#include "mdctgan_hip.h"

constexpr int kChunk = MG_MOMENTS_CHUNK;
constexpr long long kFar = 1LL << 62;            // positions beyond this are a broken table: the row is dropped before any sum overflows

// x blocks per row for a launch over n_rows rows of at most max_len samples, `per_block` samples per block and pass: enough
// blocks to fill the chip, few enough that a table of thousands of rows does not launch mostly empty ones
inline dim3 rows_grid(int n_rows, long long max_len, int per_block) {
    const unsigned gy = (unsigned)(n_rows < 65535 ? n_rows : 65535);
    long long bx = (max_len + per_block - 1) / per_block;
    const long long cap = 8192 / gy > 8 ? 8192 / gy : 8;
    bx = bx < cap ? bx : cap;
    return dim3((unsigned)(bx < 1 ? 1 : (bx > 1024 ? 1024 : bx)), gy);
}

// The taps [k_lo, k_hi) of a K-tap filter, whose tap 0 sits at sample t0, that fall inside the window [j_lo, j_hi)
template <typename T>
__device__ __forceinline__ void tap_range(T j_lo, T j_hi, T t0, int K, int& k_lo, int& k_hi) {
    k_lo = (int)(j_lo - t0 > 0 ? (j_lo - t0 < K ? j_lo - t0 : K) : 0);
    k_hi = (int)(j_hi - t0 < K ? (j_hi - t0 > 0 ? j_hi - t0 : 0) : K);
}

// mg_resample's chain over those taps (only [k_lo, k_hi) of xt and kp is read); SHIFT: every sample enters as xt[k] + s
template <bool SHIFT>
__device__ __forceinline__ float fir_chain(const float* xt, const float* kp, int k_lo, int k_hi, float s) {
    float acc = 0.0f;
    for (int k = k_lo; k < k_hi; ++k) acc = fmaf(SHIFT ? xt[k] + s : xt[k], kp[k], acc);
    return acc;
}

// The chunks of MG_MOMENTS_CHUNK samples that a row of `len` samples has partial sums for
__device__ __forceinline__ int row_chunks(long long len, int max_chunks) {
    const long long all = len > 0 ? (len + kChunk - 1) / kChunk : 0;
    return (int)(all < max_chunks ? all : max_chunks);
}

// The N sums of one chunk over a workgroup of 256: every wave, then the four waves in a fixed tree, stored to dst[0 .. N).
// Both barriers are inside: red is free again on return.
template <int N>
__device__ __forceinline__ void block_sum_store(const double (&acc)[N], double (&red)[4][N], double* __restrict__ dst) {
    double s[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = wave_sum_d(acc[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int w = threadIdx.x;
        dst[w] = ((red[0][w] + red[1][w]) + red[2][w]) + red[3][w];
    }
    __syncthreads();
}

// out[0 .. N) = the chunk sums partial[c][0 .. N) of one row, c ascending
template <int N>
__device__ __forceinline__ void sum_chunks(const double* __restrict__ partial, int n_chunks, double* __restrict__ out) {
    double s[N] = {};
    for (int c = 0; c < n_chunks; ++c)
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] += partial[(size_t)c * N + k];
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = s[k];
}
