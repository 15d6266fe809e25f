// The front end of the reference's data path for MANY utterances in shared launches (data/audio_dataset.py:66-78, 141-186):
// every utterance sits at its own place of one packed buffer and device row tables say where each row reads and writes, as the
// mg_seg_row kernels of mdct.hip do for the generator's batches.
//   resample_rows_kernel    resample_kernel (resample.hip) with a row table in place of [B, L]: per output sample the same fmaf
//                           chain in ascending tap order, so a row has mg_resample's bits whatever else shares the launch.  An
//                           optional per-row shift enters every sample of the row (not the zero padding around it) as a float32
//                           add: read_audio's `raw += 1e-4 - mean(raw)` (:146).
//   rows_moments_*          per row {sum x, sum x^2} in double: chunks of MG_MOMENTS_CHUNK samples counted from the row's first sample,
//                           each summed by one workgroup in a fixed tree, then the chunks of a row in ascending order.
//   add_noise_rows_kernel   :73-78 / :179-184 per row, in place: y = lr + a (n - m), a and m from the double moments on the device.
// All windows are cut to their buffers, a row of length 0 is dead, there are no atomics.
#include <limits.h>
#include <math.h>

#include "rows.h"

namespace {

template <bool BANK_IN_LDS, bool SHIFT>
__global__ __launch_bounds__(256) void resample_rows_kernel(const float* __restrict__ x, long long x_total,
                                                            const mg_resample_row* __restrict__ rows, int n_rows,
                                                            const float* __restrict__ shift, const float* __restrict__ kern,
                                                            int orig, int new_, int width, float* __restrict__ out,
                                                            long long out_total) {
    extern __shared__ float kl_s[];                // [new][K]
    const int K = 2 * width + orig;
    if (BANK_IN_LDS) {
        for (int i = threadIdx.x; i < new_ * K; i += blockDim.x) kl_s[i] = kern[i];
        __syncthreads();
    }
    const float* kl = BANK_IN_LDS ? kl_s : kern;
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const mg_resample_row rw = rows[r];
        if (rw.in_len <= 0 || rw.out_len <= 0 || rw.in_len > INT_MAX || rw.out_len > INT_MAX) continue;
        if (rw.in_pos <= -kFar || rw.in_pos >= x_total || rw.out_pos <= -kFar || rw.out_pos >= out_total) continue;
        // samples [j_lo, j_hi) of the row exist in x, samples [o_lo, o_hi) of its output in out (all of them for a sound table)
        const long long j_lo = rw.in_pos < 0 ? -rw.in_pos : 0;
        const long long j_hi = rw.in_len < x_total - rw.in_pos ? rw.in_len : x_total - rw.in_pos;
        const long long o_lo = rw.out_pos < 0 ? -rw.out_pos : 0;
        const long long o_hi = rw.out_len < out_total - rw.out_pos ? rw.out_len : out_total - rw.out_pos;
        const float s = SHIFT ? shift[r] : 0.0f;
        for (long long o = o_lo + blockIdx.x * blockDim.x + threadIdx.x; o < o_hi; o += (long long)gridDim.x * blockDim.x) {
            const int n = (int)o / new_, p = (int)o - n * new_;
            const long long t0 = (long long)n * orig - width;          // sample index of tap 0
            int k_lo, k_hi;
            tap_range(j_lo, j_hi, t0, K, k_lo, k_hi);
            out[rw.out_pos + o] = fir_chain<SHIFT>(x + (rw.in_pos + t0), kl + p * K, k_lo, k_hi, s);
        }
    }
}

// One workgroup = one chunk of one row.  Thread t owns samples 4t .. 4t+3 (+ 1024 i) of the chunk, whatever the row's alignment;
// 16-byte loads where the quad is aligned and whole (VEC: a 16-byte aligned x), scalar loads of the same samples otherwise.
template <bool VEC>
__global__ __launch_bounds__(256) void rows_moments_chunks_kernel(const float* __restrict__ x, long long total,
                                                                  const SegRow* __restrict__ rows, int n_rows, int max_chunks,
                                                                  double* __restrict__ partial) {
    __shared__ double red[4][2];
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const SegRow rw = seg_row_clamped(rows, r, total);
        const long long len = rw.hi - rw.lo;
        if (len <= 0) continue;
        const int n_chunks = row_chunks(len, max_chunks);
        for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
            const long long base = rw.lo + (long long)c * kChunk;
            const int n = (int)(rw.hi - base < kChunk ? rw.hi - base : kChunk);
            double acc[2] = {0.0, 0.0};                                  // sum x, sum x^2
            for (int i = 4 * threadIdx.x; i < n; i += 4 * 256) {
                float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (VEC && ((base + i) & 3) == 0 && i + 3 < n) {
                    const float4 v = *reinterpret_cast<const float4*>(x + base + i);
                    e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (i + k < n) e[k] = x[base + i + k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) { const double d = (double)e[k]; acc[0] += d; acc[1] += d * d; }   // (missing: adds 0)
            }
            block_sum_store<2>(acc, red, partial + ((size_t)r * max_chunks + c) * 2);
        }
    }
}

__global__ __launch_bounds__(256) void rows_moments_final_kernel(const SegRow* __restrict__ rows, long long total, int n_rows,
                                                                 int max_chunks, const double* __restrict__ partial,
                                                                 double* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const SegRow rw = seg_row_clamped(rows, r, total);
    sum_chunks<2>(partial + (size_t)r * max_chunks * 2, row_chunks(rw.hi - rw.lo, max_chunks), out + 2 * (size_t)r);
}

template <bool VEC>
__global__ __launch_bounds__(256) void add_noise_rows_kernel(float* __restrict__ lr, const float* __restrict__ noise, long long total,
                                                             const SegRow* __restrict__ rows, int n_rows,
                                                             const double* __restrict__ lr_moments,
                                                             const double* __restrict__ noise_moments, double snr_gain,
                                                             double segment_length) {
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const SegRow rw = seg_row_clamped(rows, r, total);
        const long long len = rw.hi - rw.lo;
        if (len < 2) continue;                      // (no standard deviation: the host refuses such a row before the launch)
        const double N = (double)len;
        const double sum_n = noise_moments[2 * (size_t)r], sum_n2 = noise_moments[2 * (size_t)r + 1];
        const double mean = sum_n / N;
        const double var = (sum_n2 - sum_n * mean) / (N - 1.0);                     // torch.std: unbiased
        const double noise_var = (lr_moments[2 * (size_t)r + 1] / segment_length) / snr_gain;
        const float a = (float)(sqrt(noise_var) / sqrt(var)), m = (float)mean;
        // quads at absolute multiples of 4, so that a 16-byte access is aligned wherever the row starts
        const long long q0 = rw.lo & ~3LL;
        for (long long p = q0 + 4 * (long long)(blockIdx.x * blockDim.x + threadIdx.x); p < rw.hi;
             p += 4 * (long long)gridDim.x * blockDim.x) {
            if (VEC && p >= rw.lo && p + 3 < rw.hi) {
                float4 v = *reinterpret_cast<const float4*>(lr + p);
                const float4 z = *reinterpret_cast<const float4*>(noise + p);
                v.x = v.x + a * (z.x - m); v.y = v.y + a * (z.y - m); v.z = v.z + a * (z.z - m); v.w = v.w + a * (z.w - m);
                *reinterpret_cast<float4*>(lr + p) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p + k >= rw.lo && p + k < rw.hi) lr[p + k] = lr[p + k] + a * (noise[p + k] - m);
            }
        }
    }
}

}  // namespace

extern "C" {

// See include/mdctgan_hip.h.
int mg_resample_rows(const float* x, long long x_total, const mg_resample_row* rows, int n_rows, long long max_out_len,
                     const float* shift, const float* kern, int orig, int new_, int width, float* out, long long out_total,
                     void* stream) {
    if (!x || !rows || !kern || !out || n_rows <= 0 || x_total <= 0 || out_total <= 0 || max_out_len <= 0) return MG_ERR_ARG;
    if (orig <= 0 || new_ <= 0 || width < 0) return MG_ERR_ARG;
    if ((long long)new_ * (2LL * width + orig) > INT_MAX / 4) return MG_ERR_ARG;
    const size_t lds = (size_t)new_ * (2 * width + orig) * sizeof(float);
    const dim3 grid = rows_grid(n_rows, max_out_len, 256);
    hipStream_t st = (hipStream_t)stream;
#define MG_RR_LAUNCH(LDS, SH, BYTES)                                                                                          \
    hipLaunchKernelGGL((resample_rows_kernel<LDS, SH>), grid, dim3(256), BYTES, st, x, x_total, rows, n_rows, shift, kern, orig, \
                       new_, width, out, out_total)
    if (lds <= 48 * 1024) {
        if (shift) MG_RR_LAUNCH(true, true, lds); else MG_RR_LAUNCH(true, false, lds);
    } else {
        if (shift) MG_RR_LAUNCH(false, true, 0); else MG_RR_LAUNCH(false, false, 0);
    }
#undef MG_RR_LAUNCH
    MG_CHECK_LAUNCH();
    return MG_OK;
}

size_t mg_rows_moments_workspace(int n_rows, long long max_len) {
    if (n_rows <= 0 || max_len <= 0) return 0;
    return (size_t)n_rows * (size_t)((max_len + kChunk - 1) / kChunk) * 2 * sizeof(double);
}

int mg_rows_moments(const float* x, long long total, const mg_seg_row* rows, int n_rows, long long max_len, double* out,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !rows || !out || !workspace || n_rows <= 0 || total <= 0 || max_len <= 0) return MG_ERR_ARG;
    const long long max_chunks = (max_len + kChunk - 1) / kChunk;
    if (max_chunks > INT_MAX || workspace_bytes < mg_rows_moments_workspace(n_rows, max_len)) return MG_ERR_ARG;
    const SegRow* rt = reinterpret_cast<const SegRow*>(rows);
    double* partial = static_cast<double*>(workspace);
    const dim3 grid = rows_grid(n_rows, max_len, kChunk);
    hipStream_t st = (hipStream_t)stream;
    if (al16(x))
        hipLaunchKernelGGL(rows_moments_chunks_kernel<true>, grid, dim3(256), 0, st, x, total, rt, n_rows, (int)max_chunks, partial);
    else
        hipLaunchKernelGGL(rows_moments_chunks_kernel<false>, grid, dim3(256), 0, st, x, total, rt, n_rows, (int)max_chunks, partial);
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(rows_moments_final_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, rt, total, n_rows,
                       (int)max_chunks, partial, out);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_add_noise_rows(float* lr, const float* noise, long long total, const mg_seg_row* rows, int n_rows, long long max_len,
                      const double* lr_moments, const double* noise_moments, double snr, long long segment_length, void* stream) {
    if (!lr || !noise || !rows || !lr_moments || !noise_moments || n_rows <= 0 || total <= 0 || max_len <= 0) return MG_ERR_ARG;
    if (segment_length <= 0 || !(snr == snr) || snr > 3000.0 || snr < -3000.0) return MG_ERR_ARG;
    const double snr_gain = pow(10.0, snr / 10.0);
    const SegRow* rt = reinterpret_cast<const SegRow*>(rows);
    const dim3 grid = rows_grid(n_rows, max_len, 1024);
    hipStream_t st = (hipStream_t)stream;
    if (al16(lr) && al16(noise))
        hipLaunchKernelGGL(add_noise_rows_kernel<true>, grid, dim3(256), 0, st, lr, noise, total, rt, n_rows, lr_moments,
                           noise_moments, snr_gain, (double)segment_length);
    else
        hipLaunchKernelGGL(add_noise_rows_kernel<false>, grid, dim3(256), 0, st, lr, noise, total, rt, n_rows, lr_moments,
                           noise_moments, snr_gain, (double)segment_length);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"
