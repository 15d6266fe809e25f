// The multi-resolution STFT loss of many utterances in shared launches (Python: metrics.mrstft_many / mrstft_loss /
// mrstft_loss_term; the training term of --lambda_mrstft), on the frame machinery of lsd_fft.h: the row search, the staging with
// the reflection at the row's own ends, the Stockham stages and the split of lsd_rows_kernel (metrics_rows.hip).  The FORWARD
// transform runs in double (sd_* of stft_frames.h, shared with mel_loss_rows.hip: lsd_fft.h's statements for double2, on a tile of 2048 points) and every bin is rounded to
// float32 once: the sign of ln m_hr - ln m_sr and the clamp are DECISIONS, each weighted with 1/m^2 in the gradient, and a float32
// transform errs relative to the frame's largest bin -- on a tone whose peak lies eleven decades of power above the clamp that is
// percents of a bin near the clamp, so a float32 transform (this one or a CPU's) takes some of those decisions differently from
// float64 and from one build to the next.  A spectrum that is accurate per bin takes them as float64 does wherever the bins are
// 1e-6 apart.  The inverse transform of the gradient has no decisions and stays in float32.
//
// One resolution r = (N, hop), window [N] (the host passes the periodic Hann window), K = N/2 + 1 bins, F_u frames of row u.  With
// p = re^2 + im^2 of the float32 spectrum (the double transform rounded once; p formed in double) and m = sqrt(max(p, 1e-7)):
//     A_u = sum_{f,k} (m_hr - m_sr)^2     B_u = sum_{f,k} m_hr^2     C_u = sum_{f,k} |ln m_hr - ln m_sr|
//     loss_u = sqrt(A_u / B_u) + C_u / (F_u K)                (spectral convergence + log-magnitude L1, per utterance)
// Gradient with respect to sr only.  At the non-smooth points, by definition: A_u == 0 gives a spectral-convergence term of exactly
// 0 (value and gradient), a bin with ln m_hr == ln m_sr contributes 0 (sign(0) = 0), a bin with p_sr < 1e-7 contributes 0 (the
// clamp); B_u >= F_u K 1e-7 > 0 for a live row.  So silence against silence, an all-zero sr and sr == hr (the same statements on
// both operands) have gradient exactly 0, and the first and last have loss exactly 0.
//
//   stft_loss_frames_kernel   forward, one launch over all frames of the pack: lsd_rows_kernel up to the split, then per bin in
//       double d = m_hr - m_sr; the lanes of a frame sum {d^2, m_hr^2, |ln m_hr - ln m_sr|} in lsd_rows_kernel's tree and lane 0
//       stores the three doubles of the frame to partial [total_frames][3] (a frame outside every live row: zeros).  Frames and
//       spectra are never written.  LDS: 32 KiB of frame data (4 / 2 / 1 frames per workgroup at N = 512 / 1024 / 2048) + 8 N bytes
//       of roots (the half circle in double).
//   stft_loss_finish_kernel   one thread per row: the row's frames in ascending order in double -> row_out[u] = {A_u, B_u, C_u,
//       loss_u}; a dead row (or one whose frame range does not fit the table) gives four zeros.
//   stft_loss_grad_frames_kernel   backward, phase one: the two spectra of every frame again, then per bin, in double, from the
//       row's A_u, B_u, F_u (row_out) and the row's upstream gradient g_u
//           c_k = (g_u (m_sr - m_hr) / sqrt(A_u B_u) - g_u sign(ln m_hr - ln m_sr) / (F_u K m_sr)) / m_sr     (0 where clamped;
//                                                                                     the first term 0 where A_u == 0)
//       i.e. G_k = (dL/dm_k / m_k) X_sr[k] and y = Re sum_{k=0..N/2} G_k exp(+2 pi i k n / N): the Hermitian spectrum H_k = G_k / 2
//       (0 < k < N/2), Re G_k (k = 0, N/2) is rounded to float32, kept in registers until every lane has read its bins (a barrier),
//       written as float2 over the dead doubles and inverted in float32 through lsd_rows_grad_frames_kernel's adjoint of the
//       pack-and-split and the forward stages.  y[n] window[n] goes to the workspace [total_frames][N] (float32) in 16-byte stores.  No reduction:
//       the row sums come from the forward.
//   lsd_rows_grad_gather_kernel   phase two, lsd_gather.h (shared with the LSD backward): every sample of a live row sums its taps
//       in double in one fixed order and is written (ACC == false) or added to (ACC == true: the second and later resolutions) by
//       exactly one thread.
//   stft_loss_mean_kernel   the dense batch's loss node: loss[0] = float32(scale * mean_u mean_r loss_{r,u}), one workgroup, double.
// Static LDS only, no atomics, no host read-back, launch counts independent of the number of rows; no arithmetic for a row depends
// on where the row sits, so a row has the same value and gradient bits alone and in any pack.  Tables that do not agree with
// themselves lose samples; nothing is read or written outside a buffer, and only samples of live rows are written.
// Shared with mel_loss_rows.hip through stft_frames.h: everything up to the float32 spectrum, the sum of a frame's lanes
// (sd_frame_sum) and the backward's tail from H_k on (sd_inverse_tail); with lsd_rows_grad.hip as well, through frames_common.h:
// the conj Zt of that tail and the host side (operand checks, grid, n_fft dispatch, the backward's epilogue with the gather).
// Deliberately this file's own: the seeded gradient ((go * up_scale) / n_rows) / n_res in double, UNROUNDED (the mel loss rounds it
// to float32, the LSD divides by the row's frame count and rounds: each is asserted bit for bit), and stft_loss_finish_kernel.
#include "stft_frames.h"

namespace {

template <int N>
__global__ __launch_bounds__(LSD_NT) void stft_loss_frames_kernel(const float* __restrict__ hr, long long hr_total,
                                                                  const float* __restrict__ sr, long long sr_total,
                                                                  const mg_metric_row* __restrict__ rows, int n_rows,
                                                                  const long long* __restrict__ frame_start, long long total_frames,
                                                                  const float* __restrict__ window, int hop, int center,
                                                                  long long n_tiles, double* __restrict__ partial) {
    constexpr int M = N / 2, FT = SD_TILE / N, TPF = LSD_NT / FT, NBINS = N / 2 + 1;
    static_assert(TPF >= 64 && M % LSD_NT == 0, "a frame's lanes fill whole waves, a load pass stays inside one signal of a frame");
    __shared__ __attribute__((aligned(16))) double2 buf[SD_TILE];          // [FT][hr, sr][M]
    __shared__ __attribute__((aligned(16))) double2 root[N / 2];
    __shared__ double red[LSD_NT / 64][3];
    __shared__ LsdFrame info[FT];
    const int tid = threadIdx.x;
    sd_roots<N>(root, tid);
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (tid < FT) {
            int row;
            info[tid] = lsd_locate<false>(tile * FT + tid, rows, n_rows, frame_start, total_frames, nullptr, N, hop, center, row);
        }
        __syncthreads();
        sd_load_tile<N>(buf, info, hr, hr_total, sr, sr_total, window, center, tid);
        __syncthreads();
        sd_fft<M, SD_TILE>(buf, root, tid);
        // bins k = j, j + TPF, ... of frame fr on lane j of the frame's TPF lanes
        const int fr = tid / TPF, j = tid % TPF;
        const double2* Zh = buf + fr * N;
        const double2* Zs = Zh + M;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int k = j; k < NBINS; k += TPF) {
            const float2 a = sd_real_bin<M>(Zh, k, root), b = sd_real_bin<M>(Zs, k, root);
            const double pa = fmax((double)a.x * a.x + (double)a.y * a.y, kStftClamp);
            const double pb = fmax((double)b.x * b.x + (double)b.y * b.y, kStftClamp);
            const double d = sqrt(pa) - sqrt(pb);
            acc[0] += d * d;
            acc[1] += pa;
            acc[2] += fabs(0.5 * (log(pa) - log(pb)));
        }
        sd_frame_sum<3, TPF>(acc, red, tid, fr, j);
        if (j == 0) {
            const long long g = tile * FT + fr;
            if (g < total_frames) {
                const bool live = info[fr].live != 0;
#pragma unroll
                for (int q = 0; q < 3; ++q) partial[g * 3 + q] = live ? acc[q] : 0.0;
            }
        }
        __syncthreads();                                    // buf, info and red are free for the next tile
    }
}

__global__ __launch_bounds__(256) void stft_loss_finish_kernel(const double* __restrict__ partial, const mg_metric_row* __restrict__ rows,
                                                               int n_rows, const long long* __restrict__ frame_start,
                                                               long long total_frames, int n_bins, double* __restrict__ row_out) {
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < n_rows; u += (long long)gridDim.x * 256) {
        long long f0, nf;
        double s[3] = {0.0, 0.0, 0.0}, loss = 0.0;
        if (stft_row_frames(rows, frame_start, total_frames, (int)u, f0, nf)) {
            for (long long f = f0; f < f0 + nf; ++f) {
#pragma unroll
                for (int q = 0; q < 3; ++q) s[q] += partial[f * 3 + q];
            }
            loss = ((s[0] > 0.0 && s[1] > 0.0) ? sqrt(s[0] / s[1]) : 0.0) + s[2] / ((double)nf * (double)n_bins);
        }
        row_out[u * 4 + 0] = s[0];
        row_out[u * 4 + 1] = s[1];
        row_out[u * 4 + 2] = s[2];
        row_out[u * 4 + 3] = loss;
    }
}

// SEEDED: `up` is not the per-row gradient but the loss node's upstream scalar go [1], and every row's gradient is formed here, in
// double, as ((go[0] * up_scale) / n_rows) / n_res -- d (scale * mean_u mean_r loss_{r,u}) / d loss_{r,u} times go[0] -- when the
// kernel runs, so a captured step follows a loss scale that changes between replays.
template <int N, bool SEEDED>
__global__ __launch_bounds__(LSD_NT) void stft_loss_grad_frames_kernel(const float* __restrict__ hr, long long hr_total,
                                                                       const float* __restrict__ sr, long long sr_total,
                                                                       const mg_metric_row* __restrict__ rows, int n_rows,
                                                                       const long long* __restrict__ frame_start,
                                                                       long long total_frames, const float* __restrict__ window,
                                                                       const double* __restrict__ row_sums,
                                                                       const float* __restrict__ up, double up_scale, int n_res,
                                                                       int hop, int center, long long n_tiles,
                                                                       float* __restrict__ frames_out) {
    constexpr int M = N / 2, FT = SD_TILE / N, TPF = LSD_NT / FT, NBINS = N / 2 + 1, BPL = (NBINS + TPF - 1) / TPF;
    static_assert(TPF >= 64 && M % LSD_NT == 0, "a frame's lanes fill whole waves, a load pass stays inside one signal of a frame");
    __shared__ __attribute__((aligned(16))) double2 buf[SD_TILE];          // [FT][hr, sr][M] double; then, as float2: [FT][N] holding
    __shared__ __attribute__((aligned(16))) double2 root[N / 2];           //   H_k, k = 0 .. M, of every frame; then [FT][M]
    __shared__ LsdFrame info[FT];
    __shared__ double coef[FT][2];                                         // g / sqrt(A B) (0: A == 0),  g / (F K)
    float2* fbuf = reinterpret_cast<float2*>(buf);
    const int tid = threadIdx.x;
    sd_roots<N>(root, tid);
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (tid < FT) {
            int row;
            const LsdFrame fi = lsd_locate<false>(tile * FT + tid, rows, n_rows, frame_start, total_frames, nullptr, N, hop, center, row);
            info[tid] = fi;
            double c_sc = 0.0, c_l1 = 0.0;
            if (fi.live) {
                const double g = SEEDED ? (((double)up[0] * up_scale) / (double)n_rows) / (double)n_res : (double)up[row];
                const double A = row_sums[(long long)row * 4], B = row_sums[(long long)row * 4 + 1];
                if (A > 0.0 && B > 0.0) c_sc = g / sqrt(A * B);
                c_l1 = g / ((double)(frame_start[row + 1] - frame_start[row]) * (double)NBINS);
            }
            coef[tid][0] = c_sc;
            coef[tid][1] = c_l1;
        }
        __syncthreads();
        sd_load_tile<N>(buf, info, hr, hr_total, sr, sr_total, window, center, tid);
        __syncthreads();
        sd_fft<M, SD_TILE>(buf, root, tid);
        // pass one: H_k of bins k = j, j + TPF, ... of frame fr on lane j of the frame's TPF lanes, in registers
        const int fr = tid / TPF, j = tid % TPF;
        const double2* Zh = buf + fr * N;
        const double2* Zs = Zh + M;
        const double c_sc = coef[fr][0], c_l1 = coef[fr][1];
        float2 h[BPL];
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int k = j + i * TPF;
            h[i] = make_float2(0.0f, 0.0f);
            if (k < NBINS) {
                const float2 a = sd_real_bin<M>(Zh, k, root), b = sd_real_bin<M>(Zs, k, root);
                const double pa = fmax((double)a.x * a.x + (double)a.y * a.y, kStftClamp);
                const double pb = (double)b.x * b.x + (double)b.y * b.y;
                if (pb >= kStftClamp) {
                    const double ma = sqrt(pa), mb = sqrt(pb), dl = log(pa) - log(pb);
                    const double sg = dl > 0.0 ? 1.0 : (dl < 0.0 ? -1.0 : 0.0);
                    const double c = (c_sc * (mb - ma) - c_l1 * sg / mb) / mb;
                    h[i] = (k == 0 || k == M) ? make_float2((float)(c * (double)b.x), 0.0f)
                                              : make_float2((float)(0.5 * c * (double)b.x), (float)(0.5 * c * (double)b.y));
                }
            }
        }
        __syncthreads();                                    // every lane has read its Z[k] and Z[M-k]: the doubles are dead
        sd_inverse_tail<N>(h, fbuf, root, window, frames_out, tile, total_frames, tid);
        __syncthreads();                                    // buf, info and coef are free for the next tile
    }
}

// One workgroup.  Tiles of 256 consecutive rows, one per thread: a row's losses are added in resolution order and divided by n_res,
// a tile is summed in block_sum_store's tree (rows.h), the tiles are added in ascending order by thread 0.
__global__ __launch_bounds__(256) void stft_loss_mean_kernel(const double* __restrict__ row_out, int n_rows, int n_res, double scale,
                                                             float* __restrict__ loss) {
    __shared__ double red[4][1];
    __shared__ double tile_sum[1];
    double sum = 0.0;                                       // (thread 0's)
    for (long long base = 0; base < n_rows; base += 256) {
        const long long u = base + threadIdx.x;
        double v = 0.0;
        if (u < n_rows) {
            for (int r = 0; r < n_res; ++r) v += row_out[((long long)r * n_rows + u) * 4 + 3];
            v /= (double)n_res;
        }
        const double acc[1] = {v};
        block_sum_store<1>(acc, red, tile_sum);             // (both barriers inside: tile_sum is thread 0's to read and to rewrite)
        if (threadIdx.x == 0) sum += tile_sum[0];
    }
    if (threadIdx.x == 0) loss[0] = (float)(scale * sum / (double)n_rows);
}

}  // namespace

extern "C" {

// See include/mdctgan_hip.h.
size_t mg_stft_loss_rows_workspace(long long total_frames) {
    if (total_frames <= 0 || total_frames > kFar / (3 * (long long)sizeof(double))) return 0;
    return (size_t)total_frames * 3 * sizeof(double);
}

size_t mg_stft_loss_rows_backward_workspace(long long total_frames, int n_fft) {
    if (total_frames <= 0 || !lsd_size_ok(n_fft) || total_frames > kFar / (n_fft * (long long)sizeof(float))) return 0;
    return (size_t)total_frames * (size_t)n_fft * sizeof(float);
}

int mg_stft_loss_rows(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows, int n_rows,
                      const long long* frame_start, long long total_frames, const float* window, int n_fft, int hop, int center,
                      double* row_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!frames_args_ok(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop) || !row_out ||
        !frames_workspace_ok(mg_stft_loss_rows_workspace(total_frames), workspace, workspace_bytes))
        return MG_ERR_ARG;
    double* partial = static_cast<double*>(workspace);
    const FramesGrid grid = frames_grid(total_frames, n_fft, SD_TILE, 3);
    hipStream_t st = (hipStream_t)stream;
    frames_with_n_fft(n_fft, [&](auto nn) {
        hipLaunchKernelGGL((stft_loss_frames_kernel<decltype(nn)::value>), dim3(grid.blocks), dim3(LSD_NT), 0, st, hr, hr_total, sr,
                           sr_total, rows, n_rows, frame_start, total_frames, window, hop, center != 0, grid.n_tiles, partial);
    });
    MG_CHECK_LAUNCH();
    const unsigned fblocks = (unsigned)((n_rows + 255) / 256 < 1024 ? (n_rows + 255) / 256 : 1024);
    hipLaunchKernelGGL(stft_loss_finish_kernel, dim3(fblocks), dim3(256), 0, st, partial, rows, n_rows, frame_start, total_frames,
                       n_fft / 2 + 1, row_out);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"

namespace {

// both entry points: `up` is grad_rows [n_rows] (seeded == false) or go [1] with up_scale and n_res
int stft_loss_rows_backward(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                            int n_rows, const long long* frame_start, long long total_frames, const float* window, int n_fft, int hop,
                            int center, const double* row_sums, const float* up, double up_scale, int n_res, bool seeded,
                            int accumulate, float* grad_sr, void* workspace, size_t workspace_bytes, void* stream) {
    if (!frames_args_ok(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop) || !row_sums || !up ||
        !grad_sr || n_res <= 0)
        return MG_ERR_ARG;
    const FramesGrid grid = frames_grid(total_frames, n_fft, SD_TILE, 3);
    hipStream_t st = (hipStream_t)stream;
    return frames_backward(rows, n_rows, frame_start, total_frames, n_fft, hop, center, sr_total,
                           mg_stft_loss_rows_backward_workspace(total_frames, n_fft), workspace, workspace_bytes, accumulate != 0,
                           grad_sr, st, [&](float* frames) {
        frames_with_n_fft(n_fft, [&](auto nn) { frames_with_flag(seeded, [&](auto g) {
            hipLaunchKernelGGL((stft_loss_grad_frames_kernel<decltype(nn)::value, decltype(g)::value>), dim3(grid.blocks),
                               dim3(LSD_NT), 0, st, hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window,
                               row_sums, up, up_scale, n_res, hop, center != 0, grid.n_tiles, frames);
        }); });
    });
}

}  // namespace

extern "C" {

int mg_stft_loss_rows_backward(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                               int n_rows, const long long* frame_start, long long total_frames, const float* window, int n_fft,
                               int hop, int center, const double* row_sums, const float* grad_rows, int accumulate, float* grad_sr,
                               void* workspace, size_t workspace_bytes, void* stream) {
    return stft_loss_rows_backward(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop, center,
                                   row_sums, grad_rows, 0.0, 1, false, accumulate, grad_sr, workspace, workspace_bytes, stream);
}

int mg_stft_loss_rows_backward_seeded(const float* hr, long long hr_total, const float* sr, long long sr_total,
                                      const mg_metric_row* rows, int n_rows, const long long* frame_start, long long total_frames,
                                      const float* window, int n_fft, int hop, int center, const double* row_sums, const float* go,
                                      double scale, int n_res, int accumulate, float* grad_sr, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    return stft_loss_rows_backward(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop, center,
                                   row_sums, go, scale, n_res, true, accumulate, grad_sr, workspace, workspace_bytes, stream);
}

int mg_stft_loss_mean(const double* row_out, int n_rows, int n_res, double scale, float* loss, void* stream) {
    if (!row_out || !loss || n_rows <= 0 || n_res <= 0) return MG_ERR_ARG;
    hipLaunchKernelGGL(stft_loss_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_out, n_rows, n_res, scale, loss);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"
