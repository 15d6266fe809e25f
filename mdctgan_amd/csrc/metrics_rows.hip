// The metrics of util/util.py:132-177 (compute_matrics) for MANY utterances in shared launches: the last step of the reference's
// generate_audio.py:57-67, which metrics.hip serves one clip at a time.  Every utterance sits at its own place of three packed
// float32 buffers (ground truth hr, low-rate lr, super-resolved sr; each with its own total), a device row table
// (mg_metric_row = hr_pos, lr_pos, sr_pos, len) says where: sample t < len of row u is hr[hr_pos + t], lr[lr_pos + t],
// sr[sr_pos + t].  An optional shift [n_rows] enters every hr sample as one float32 add, hr[p] + shift[u] -- the operand
// resample_rows_kernel<., true> forms, so the un-materialised `raw += 1e-4 - mean(raw)` of read_audio is the ground truth.
//   metrics_rows_packed_*   per row {sum hr^2, sum (sr - hr)^2, sum (lr - hr)^2} in double (metrics_rows_kernel's arithmetic) with
//                           the two-level sums of rows_moments_* (resample_rows.hip): chunks of MG_MOMENTS_CHUNK samples counted
//                           from the row's first sample, one workgroup per chunk in a fixed tree, then the chunks in ascending order.
//   lsd_rows_kernel         the per-frame log-spectral distance of every frame of every utterance, straight from the waveforms:
//                           neither the windowed frames nor the spectra of metrics.hip's three-launch chain exist in HBM.
//   lsd_mean_loss_kernel    scale * the mean of that per-frame array as a float32 [1] loss (the training term of --lambda_lsd).
// Windows are cut to their buffers (a sample outside one is not read: it is skipped by the sums and enters a frame as 0), a row
// with len <= 0 is dead, there are no atomics, every sum has one fixed order: a row has the same bits alone as inside any pack.
//
// lsd_rows_kernel.  A tile is LSD_TILE / N consecutive frames of the flattened frame index (8 / 4 / 2 at N = 512 / 1024 / 2048), so
// it may hold the end of one utterance and the start of the next; frame_start [n_rows + 1] (a device prefix array) places the
// utterances, and one lane per frame of the tile searches it and leaves the frame's row in LDS.  Frame f of a row is
// x[reflect(f hop + n - N/2)] window[n] (center) or x[f hop + n] window[n], reflected at the row's own [0, len), one float32
// product as stft_frames_kernel forms it.  TWO REAL transforms per frame, each through one complex transform of M = N/2 points:
//     z[m] = x_w[2m] + i x_w[2m+1],   Z = DFT_M(z),   E[k] = (Z[k] + conj Z[M-k]) / 2,   O[k] = (Z[k] - conj Z[M-k]) / 2i,
//     X[k] = E[k] + exp(-2 pi i k / N) O[k],   k = 0 .. N/2   (indices of Z mod M),
// the same statements for hr and for sr, so sr == hr gives exactly 0 and a quiet sr is as accurate as a loud one.  (One N-point
// transform of hr_w + i sr_w costs the same and was tried first: its float32 error is relative to the LOUDER signal, and for
// sr == hr a near-null bin of a mirror-symmetric edge frame left 1.07e-5 where the tests allow 1e-5.)
// The DFT is mdct_pow2.hip's Stockham autosort FFT restated for M complex points per signal: plain float32 on the VALU, radix-8
// stages with one radix-4 (N = 512) or radix-2 (N = 2048) stage first, every stage in place in LDS (all butterflies of the tile
// are read into registers, a barrier, then written to their autosort positions: natural order out).  Roots exp(-2 pi i t / N) are
// evaluated in double by the workgroup (sincospi of an exactly representable argument) and rounded once; the stages use the even
// ones.  Epilogue per bin in double as lsd_frames_kernel: p = re^2 + im^2, d = log10(p_hr + 1e-6) - log10(p_sr + 1e-6), sum d^2
// over the N/2 + 1 bins by the 256 / frames-per-tile lanes of the frame in a fixed tree, sqrt(sum / (N/2 + 1)) rounded once to
// float32 and stored once.
// LDS: 32 KiB of frame data + 8 N bytes of roots (4 / 8 / 16 KiB): three workgroups per CU.
// The row search, the staging, the stages and the split are stated in lsd_fft.h, which the backward (lsd_rows_grad.hip) shares.
#include <math.h>

#include "lsd_fft.h"

namespace {

// samples [lo, hi) of a row of `len` samples at `pos` exist in a buffer of `total` samples
__device__ __forceinline__ void cut_to(long long pos, long long total, long long& lo, long long& hi) {
    if (pos <= -kFar || pos >= total) { hi = lo; return; }
    if (-pos > lo) lo = -pos;
    if (total - pos < hi) hi = total - pos;
}

// One workgroup = one chunk of one row.  Thread t owns samples 4t .. 4t+3 (+ 1024 i) of the chunk, whatever the row's alignment;
// 16-byte loads where the quad is aligned and whole in all three buffers (VEC: 16-byte aligned bases), scalar loads otherwise.
template <bool VEC, bool SHIFT>
__global__ __launch_bounds__(256) void metrics_rows_packed_chunks_kernel(const float* __restrict__ hr, long long hr_total,
                                                                         const float* __restrict__ lr, long long lr_total,
                                                                         const float* __restrict__ sr, long long sr_total,
                                                                         const mg_metric_row* __restrict__ rows, int n_rows,
                                                                         const float* __restrict__ shift, int max_chunks,
                                                                         double* __restrict__ partial) {
    __shared__ double red[4][3];
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const mg_metric_row rw = rows[r];
        if (rw.len <= 0) continue;
        long long lo = 0, hi = rw.len;
        cut_to(rw.hr_pos, hr_total, lo, hi);
        cut_to(rw.lr_pos, lr_total, lo, hi);
        cut_to(rw.sr_pos, sr_total, lo, hi);
        if (hi <= lo) continue;
        const int n_chunks = row_chunks(rw.len, max_chunks);
        const float s = SHIFT ? shift[r] : 0.0f;
        for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
            const long long t0 = (long long)c * kChunk;
            // samples [a, b) of the chunk exist in all three buffers (all of them for a sound table)
            const int a = (int)(lo - t0 > 0 ? (lo - t0 < kChunk ? lo - t0 : kChunk) : 0);
            const int b = (int)(hi - t0 < kChunk ? (hi - t0 > 0 ? hi - t0 : 0) : kChunk);
            const float* h = hr + (rw.hr_pos + t0);                    // (only [a, b) of each is read)
            const float* l = lr + (rw.lr_pos + t0);
            const float* q = sr + (rw.sr_pos + t0);
            const bool quads = VEC && (((rw.hr_pos + t0) | (rw.lr_pos + t0) | (rw.sr_pos + t0)) & 3) == 0;
            double acc[3] = {0.0, 0.0, 0.0};                              // sum hr^2, sum (sr - hr)^2, sum (lr - hr)^2
            for (int i = 4 * threadIdx.x; i < b; i += 4 * 256) {
                float eh[4], el[4], es[4];
                bool on[4];
                if (quads && i >= a && i + 3 < b) {
                    const float4 vh = *reinterpret_cast<const float4*>(h + i);
                    const float4 vl = *reinterpret_cast<const float4*>(l + i);
                    const float4 vs = *reinterpret_cast<const float4*>(q + i);
                    eh[0] = vh.x; eh[1] = vh.y; eh[2] = vh.z; eh[3] = vh.w;
                    el[0] = vl.x; el[1] = vl.y; el[2] = vl.z; el[3] = vl.w;
                    es[0] = vs.x; es[1] = vs.y; es[2] = vs.z; es[3] = vs.w;
                    on[0] = on[1] = on[2] = on[3] = true;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        on[k] = i + k >= a && i + k < b;
                        eh[k] = on[k] ? h[i + k] : 0.0f;
                        el[k] = on[k] ? l[i + k] : 0.0f;
                        es[k] = on[k] ? q[i + k] : 0.0f;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // (a missing sample adds 0 to all three sums: its shift stays out as well)
                    const double hv = on[k] ? (double)(SHIFT ? eh[k] + s : eh[k]) : 0.0;
                    const double ds = (double)es[k] - hv, dl = (double)el[k] - hv;
                    acc[0] += hv * hv;
                    acc[1] += ds * ds;
                    acc[2] += dl * dl;
                }
            }
            block_sum_store<3>(acc, red, partial + ((size_t)r * max_chunks + c) * 3);
        }
    }
}

__global__ __launch_bounds__(256) void metrics_rows_packed_final_kernel(const mg_metric_row* __restrict__ rows, long long hr_total,
                                                                        long long lr_total, long long sr_total, int n_rows,
                                                                        int max_chunks, const double* __restrict__ partial,
                                                                        double* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const mg_metric_row rw = rows[r];
    long long lo = 0, hi = rw.len > 0 ? rw.len : 0;
    cut_to(rw.hr_pos, hr_total, lo, hi);
    cut_to(rw.lr_pos, lr_total, lo, hi);
    cut_to(rw.sr_pos, sr_total, lo, hi);
    const int n_chunks = row_chunks(hi > lo ? rw.len : 0, max_chunks);         // (the chunks the first kernel wrote)
    sum_chunks<3>(partial + (size_t)r * max_chunks * 3, n_chunks, out + 3 * (size_t)r);
}

// ------------------------------------------------------------------------------------------------------------------
// lsd_rows_kernel
// ------------------------------------------------------------------------------------------------------------------
template <int N, bool SHIFT>
__global__ __launch_bounds__(LSD_NT) void lsd_rows_kernel(const float* __restrict__ hr, long long hr_total,
                                                          const float* __restrict__ sr, long long sr_total,
                                                          const mg_metric_row* __restrict__ rows, int n_rows,
                                                          const long long* __restrict__ frame_start, long long total_frames,
                                                          const float* __restrict__ shift, const float* __restrict__ window,
                                                          int hop, int center, long long n_tiles, float* __restrict__ out) {
    constexpr int M = N / 2, FT = LSD_TILE / N, TPF = LSD_NT / FT, NBINS = N / 2 + 1;
    static_assert(TPF >= 32 && M % LSD_NT == 0, "a frame's lanes fill whole half-waves, a load pass stays inside one signal of a frame");
    __shared__ __attribute__((aligned(16))) float2 buf[LSD_TILE];          // [FT][hr, sr][M]
    __shared__ __attribute__((aligned(16))) float2 root[N];
    __shared__ double red[LSD_NT / 64];
    __shared__ LsdFrame info[FT];
    const int tid = threadIdx.x;
    lsd_roots<N>(root, tid);
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (tid < FT) {
            int row;
            info[tid] = lsd_locate<SHIFT>(tile * FT + tid, rows, n_rows, frame_start, total_frames, shift, N, hop, center, row);
        }
        __syncthreads();
        lsd_load_tile<N, SHIFT>(buf, info, hr, hr_total, sr, sr_total, window, center, tid);
        __syncthreads();
        lsd_fft<M>(buf, root, tid);
        // bins k = j, j + TPF, ... of frame fr on lane j of the frame's TPF lanes
        const int fr = tid / TPF, j = tid % TPF;
        const float2* Zh = buf + fr * N;
        const float2* Zs = Zh + M;
        double acc = 0.0;
        for (int k = j; k < NBINS; k += TPF) {
            const float2 w = root[k];
            const float2 a = lsd_real_bin<M>(Zh, k, w), b = lsd_real_bin<M>(Zs, k, w);
            const double pa = (double)a.x * a.x + (double)a.y * a.y, pb = (double)b.x * b.x + (double)b.y * b.y;
            const double d = log10(pa + 1e-6) - log10(pb + 1e-6);
            acc += d * d;
        }
#pragma unroll
        for (int o = (TPF < 64 ? TPF : 64) / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (TPF > 64) {
            if ((tid & 63) == 0) red[tid >> 6] = acc;
            __syncthreads();
            if (j == 0) {
                acc = red[fr * (TPF / 64)];
                for (int w = 1; w < TPF / 64; ++w) acc += red[fr * (TPF / 64) + w];
            }
        }
        if (j == 0) {
            const long long g = tile * FT + fr;
            if (g < total_frames) out[g] = info[fr].live ? (float)sqrt(acc / NBINS) : 0.0f;
        }
        __syncthreads();                                    // buf, info and red are free for the next tile
    }
}

// ------------------------------------------------------------------------------------------------------------------
// lsd_mean_loss_kernel: the loss node's reduction over lsd_rows_kernel's per-frame array, one workgroup.  Tiles of 256 consecutive
// frames, one per thread; a tile is summed in block_sum_store's tree (rows.h), the tiles are added in ascending order by thread 0;
// loss[0] = float32(scale * sum / total_frames), rounded once.  A training batch has a few hundred frames: one or two tiles.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lsd_mean_loss_kernel(const float* __restrict__ per_frame, long long total_frames, double scale,
                                                            float* __restrict__ loss) {
    __shared__ double red[4][1];
    __shared__ double tile_sum[1];
    double sum = 0.0;                                       // (thread 0's)
    for (long long base = 0; base < total_frames; base += 256) {
        const long long i = base + threadIdx.x;
        const double acc[1] = {i < total_frames ? (double)per_frame[i] : 0.0};
        block_sum_store<1>(acc, red, tile_sum);             // (both barriers inside: tile_sum is thread 0's to read and to rewrite)
        if (threadIdx.x == 0) sum += tile_sum[0];
    }
    if (threadIdx.x == 0) loss[0] = (float)(scale * sum / (double)total_frames);
}

}  // namespace

extern "C" {

// See include/mdctgan_hip.h.
size_t mg_metrics_rows_packed_workspace(int n_rows, long long max_len) {
    if (n_rows <= 0 || max_len <= 0) return 0;
    return (size_t)n_rows * (size_t)((max_len + kChunk - 1) / kChunk) * 3 * sizeof(double);
}

int mg_metrics_rows_packed(const float* hr, long long hr_total, const float* lr, long long lr_total, const float* sr,
                           long long sr_total, const mg_metric_row* rows, int n_rows, long long max_len, const float* hr_shift,
                           double* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!hr || !lr || !sr || !rows || !out || !workspace || n_rows <= 0 || max_len <= 0) return MG_ERR_ARG;
    if (hr_total <= 0 || lr_total <= 0 || sr_total <= 0) return MG_ERR_ARG;
    const long long max_chunks = (max_len + kChunk - 1) / kChunk;
    if (max_chunks > INT_MAX || workspace_bytes < mg_metrics_rows_packed_workspace(n_rows, max_len)) return MG_ERR_ARG;
    double* partial = static_cast<double*>(workspace);
    const dim3 grid = rows_grid(n_rows, max_len, kChunk);
    hipStream_t st = (hipStream_t)stream;
#define MG_MRP_LAUNCH(V, S)                                                                                                       \
    hipLaunchKernelGGL((metrics_rows_packed_chunks_kernel<V, S>), grid, dim3(256), 0, st, hr, hr_total, lr, lr_total, sr, sr_total, \
                       rows, n_rows, hr_shift, (int)max_chunks, partial)
    if (al16(hr) && al16(lr) && al16(sr)) {
        if (hr_shift) MG_MRP_LAUNCH(true, true); else MG_MRP_LAUNCH(true, false);
    } else {
        if (hr_shift) MG_MRP_LAUNCH(false, true); else MG_MRP_LAUNCH(false, false);
    }
#undef MG_MRP_LAUNCH
    MG_CHECK_LAUNCH();
    hipLaunchKernelGGL(metrics_rows_packed_final_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, rows, hr_total,
                       lr_total, sr_total, n_rows, (int)max_chunks, partial, out);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_lsd_rows(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows, int n_rows,
                const long long* frame_start, long long total_frames, const float* hr_shift, const float* window, int n_fft,
                int hop, int center, float* out, void* stream) {
    if (!hr || !sr || !rows || !frame_start || !window || !out || n_rows <= 0 || total_frames <= 0) return MG_ERR_ARG;
    if (hr_total <= 0 || sr_total <= 0 || hop <= 0 || !lsd_size_ok(n_fft)) return MG_ERR_ARG;
    const long long ft = LSD_TILE / n_fft, n_tiles = (total_frames + ft - 1) / ft;
    const unsigned blocks = (unsigned)(n_tiles < 3 * 256 * 4 ? n_tiles : 3 * 256 * 4);    // a few waves of three workgroups per CU
    hipStream_t st = (hipStream_t)stream;
#define MG_LSD_LAUNCH(NN, S)                                                                                                  \
    hipLaunchKernelGGL((lsd_rows_kernel<NN, S>), dim3(blocks), dim3(LSD_NT), 0, st, hr, hr_total, sr, sr_total, rows, n_rows, \
                       frame_start, total_frames, hr_shift, window, hop, center != 0, n_tiles, out)
#define MG_LSD_SIZE(NN) do { if (hr_shift) MG_LSD_LAUNCH(NN, true); else MG_LSD_LAUNCH(NN, false); } while (0)
    if (n_fft == 512) MG_LSD_SIZE(512);
    else if (n_fft == 1024) MG_LSD_SIZE(1024);
    else MG_LSD_SIZE(2048);
#undef MG_LSD_SIZE
#undef MG_LSD_LAUNCH
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int mg_lsd_mean_loss(const float* per_frame, long long total_frames, double scale, float* loss, void* stream) {
    if (!per_frame || !loss || total_frames <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(lsd_mean_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, per_frame, total_frames, scale, loss);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"
