// The backward pass of lsd_rows_kernel (metrics_rows.hip): the gradient of every utterance's log-spectral distance with respect to
// its super-resolved waveform sr, for any pack of utterances, in two launches without atomics.  hr is a constant.
//
// For one frame, with NB = N/2 + 1 bins, p = |X|^2, d_k = log10(p_hr[k] + 1e-6) - log10(p_sr[k] + 1e-6), L = sqrt(sum d_k^2 / NB)
// and the upstream g (the row's gradient, already divided by the row's frame count):
//     dL/dx_w[n] = sum_k c_k 2 Re(X_sr[k] exp(+2 pi i k n / N)),   c_k = -g d_k / (L NB ln 10 (p_sr[k] + 1e-6)),
// i.e. y = Re sum_{k=0..N/2} G_k exp(+2 pi i k n / N) with G_k = 2 c_k X_sr[k]: the unnormalised inverse real transform of the
// Hermitian spectrum H_k = G_k / 2 (0 < k < N/2), Re G_k (k = 0, N/2).  A frame with L == 0 (sr == hr, silence) contributes 0
// by definition.  Then dL/dx = the adjoint of framing and reflection applied to y[n] window[n].
//
//   lsd_rows_grad_frames_kernel   the forward's tile, row search, staging and Stockham stages (lsd_fft.h); the epilogue in double
//       as the forward's: pass one keeps d_k / (p_sr[k] + 1e-6) and X_sr[k] of the lane's 9 bins in registers and sums d_k^2 in
//       the forward's tree (every lane of the frame ends with the sum); pass two writes H_k, k = 0 .. N/2, over the frame's own
//       LDS region (after a barrier: lsd_real_bin read Z[k] and Z[M-k] from other lanes).  The inverse real transform is the
//       adjoint of the forward's pack-and-split, M = N/2:
//           A_k = H_k + conj H_{M-k},   B_k = (H_k - conj H_{M-k}) exp(+2 pi i k / N),   Zt_k = A_k + i B_k,   k = 0 .. M-1,
//           y[2m] + i y[2m+1] = sum_k Zt_k exp(+2 pi i k m / M) = conj DFT_M(conj Zt)[m],
//       so the forward stages run once more, on conj Zt, over the half tile that the Zt of all frames fill when packed densely.
//       y[n] window[n] goes to the workspace [total_frames][N] (float32) in 16-byte stores.
//       LDS: the forward's 32 KiB of frame data + 8 N bytes of roots, which would admit three workgroups per CU; the 206-232
//       VGPRs (no scratch) admit two.
//   lsd_rows_grad_gather_kernel   (lsd_gather.h, shared with stft_loss_rows.hip) one thread per sample: the taps that framing and
//       reflection mapped to it, summed in double in one fixed order, rounded once and stored once to grad_sr[sr_pos + t].
// Neither kernel's arithmetic for a row depends on where the row sits: a row has the same gradient bits alone and in any pack.
// mg_lsd_rows_backward_seeded is the same two launches for the loss node of a training step (metrics.lsd_loss_term): phase one
// forms every row's upstream gradient itself from the node's upstream scalar on the device (SEEDED below).
// Shared with stft_loss_rows.hip and mel_loss_rows.hip through frames_common.h: the conj Zt of the tail and the host side (operand
// checks, grid, n_fft and flag dispatch, the backward's epilogue with the gather).  Deliberately this file's own (lsd_fft.h's head
// says why): the float2 transform on LSD_TILE points with its N-entry root table, the rest of the tail around it, the reduction in
// which every lane ends with the sum, and the seeded gradient divided by the row's frame count and rounded.
#include <math.h>

#include "frames_common.h"

namespace {

// SEEDED: `up` is not the per-row gradient but the loss node's upstream scalar go [1], and row u's gradient is formed here, in double,
// as ((go[0] * up_scale) / n_rows) / frames_u, rounded to float32 once -- the statements autograd runs around the unseeded entry
// point for scale * mean_u(row u's mean), so a power-of-two scale gives that path's bits, and a captured step reads go at run time.
template <int N, bool SHIFT, bool SEEDED>
__global__ __launch_bounds__(LSD_NT) void lsd_rows_grad_frames_kernel(const float* __restrict__ hr, long long hr_total,
                                                                      const float* __restrict__ sr, long long sr_total,
                                                                      const mg_metric_row* __restrict__ rows, int n_rows,
                                                                      const long long* __restrict__ frame_start,
                                                                      long long total_frames, const float* __restrict__ shift,
                                                                      const float* __restrict__ window,
                                                                      const float* __restrict__ up, double up_scale, int hop,
                                                                      int center, long long n_tiles,
                                                                      float* __restrict__ frames_out) {
    constexpr int M = N / 2, FT = LSD_TILE / N, TPF = LSD_NT / FT, NBINS = N / 2 + 1, BPL = (NBINS + TPF - 1) / TPF;
    constexpr int HALF = LSD_TILE / 2;                                      // the Zt of the tile's frames, densely: [FT][M]
    static_assert(TPF >= 32 && M % LSD_NT == 0, "a frame's lanes fill whole half-waves, a load pass stays inside one signal of a frame");
    static_assert(HALF % LSD_NT == 0 && (HALF / 2) % LSD_NT == 0 && M % 2 == 0, "whole points and whole point pairs per thread");
    __shared__ __attribute__((aligned(16))) float2 buf[LSD_TILE];          // [FT][hr, sr][M], then [FT][H: M + 1], then [FT][M]
    __shared__ __attribute__((aligned(16))) float2 root[N];
    __shared__ double red[LSD_NT / 64];
    __shared__ LsdFrame info[FT];
    __shared__ float upstream[FT];
    const int tid = threadIdx.x;
    lsd_roots<N>(root, tid);
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (tid < FT) {
            int row;
            const LsdFrame fi = lsd_locate<SHIFT>(tile * FT + tid, rows, n_rows, frame_start, total_frames, shift, N, hop, center, row);
            info[tid] = fi;
            float g = 0.0f;
            if (fi.live) {
                if (SEEDED) g = (float)((((double)up[0] * up_scale) / (double)n_rows) / (double)(frame_start[row + 1] - frame_start[row]));
                else g = up[row];
            }
            upstream[tid] = g;
        }
        __syncthreads();
        lsd_load_tile<N, SHIFT>(buf, info, hr, hr_total, sr, sr_total, window, center, tid);
        __syncthreads();
        lsd_fft<M>(buf, root, tid);
        // pass one: bins k = j, j + TPF, ... of frame fr on lane j of the frame's TPF lanes
        const int fr = tid / TPF, j = tid % TPF;
        float2* Zh = buf + fr * N;
        const float2* Zs = Zh + M;
        double e[BPL];                                      // d_k / (p_sr[k] + 1e-6)
        float2 xs[BPL];                                     // X_sr[k]
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int k = j + i * TPF;
            e[i] = 0.0;
            xs[i] = make_float2(0.0f, 0.0f);
            if (k < NBINS) {
                const float2 w = root[k];
                const float2 a = lsd_real_bin<M>(Zh, k, w), b = lsd_real_bin<M>(Zs, k, w);
                const double pa = (double)a.x * a.x + (double)a.y * a.y, pb = (double)b.x * b.x + (double)b.y * b.y;
                const double d = log10(pa + 1e-6) - log10(pb + 1e-6);
                acc += d * d;
                e[i] = d / (pb + 1e-6);
                xs[i] = b;
            }
        }
#pragma unroll
        for (int o = (TPF < 64 ? TPF : 64) / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (TPF > 64) {
            if ((tid & 63) == 0) red[tid >> 6] = acc;
            __syncthreads();
            acc = red[fr * (TPF / 64)];
            for (int w = 1; w < TPF / 64; ++w) acc += red[fr * (TPF / 64) + w];
        }
        __syncthreads();                                    // every lane has read its Z[k] and Z[M-k]
        // pass two: H_k over the frame's region, k = 0 .. M (one point into the sr half)
        const double L = sqrt(acc / NBINS);
        const double scale = (info[fr].live && acc > 0.0) ? -2.0 * (double)upstream[fr] / (L * NBINS * 2.302585092994045684) : 0.0;
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int k = j + i * TPF;
            if (k < NBINS) {
                const double c = scale * e[i];
                Zh[k] = (k == 0 || k == M) ? make_float2((float)(c * (double)xs[i].x), 0.0f)
                                           : make_float2((float)(0.5 * c * (double)xs[i].x), (float)(0.5 * c * (double)xs[i].y));
            }
        }
        __syncthreads();
        // conj Zt of every frame, held in registers until all H are read, then packed densely
        float2 zt[HALF / LSD_NT];
#pragma unroll
        for (int it = 0; it < HALF / LSD_NT; ++it) {
            const int idx = tid + it * LSD_NT, f2 = idx / M, k = idx % M;
            zt[it] = frames_conj_zt(buf[f2 * N + k], buf[f2 * N + M - k], root[k]);
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < HALF / LSD_NT; ++it) buf[tid + it * LSD_NT] = zt[it];
        __syncthreads();
        lsd_fft<M, HALF>(buf, root, tid);
        // y[2m] = Re, y[2m+1] = -Im of the transform; two points = four samples per store
#pragma unroll
        for (int it = 0; it < HALF / 2 / LSD_NT; ++it) {
            const int idx = tid + it * LSD_NT, f2 = idx / (M / 2), n = 4 * (idx % (M / 2));
            const long long g = tile * FT + f2;
            if (g < total_frames) {
                const float4 v = *reinterpret_cast<const float4*>(buf + f2 * M + n / 2);
                *reinterpret_cast<float4*>(frames_out + g * N + n) =
                    make_float4(v.x * window[n], -v.y * window[n + 1], v.z * window[n + 2], -v.w * window[n + 3]);
            }
        }
        __syncthreads();                                    // buf, info, upstream and red are free for the next tile
    }
}

}  // namespace

extern "C" {

// See include/mdctgan_hip.h.
size_t mg_lsd_rows_backward_workspace(long long total_frames, int n_fft) {
    if (total_frames <= 0 || !lsd_size_ok(n_fft) || total_frames > kFar / (n_fft * (long long)sizeof(float))) return 0;
    return (size_t)total_frames * (size_t)n_fft * sizeof(float);
}

}  // extern "C"

namespace {

// both entry points: `up` is grad_rows [n_rows] (seeded == false) or go [1] with up_scale
int lsd_rows_backward(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                      int n_rows, const long long* frame_start, long long total_frames, const float* hr_shift,
                      const float* window, int n_fft, int hop, int center, const float* up, double up_scale, bool seeded,
                      float* grad_sr, void* workspace, size_t workspace_bytes, void* stream) {
    if (!frames_args_ok(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop) || !up || !grad_sr)
        return MG_ERR_ARG;
    const FramesGrid grid = frames_grid(total_frames, n_fft, LSD_TILE, 2);     // two workgroups per CU (VGPR-bound)
    hipStream_t st = (hipStream_t)stream;
    return frames_backward(rows, n_rows, frame_start, total_frames, n_fft, hop, center, sr_total,
                           mg_lsd_rows_backward_workspace(total_frames, n_fft), workspace, workspace_bytes, false, grad_sr, st,
                           [&](float* frames) {
        frames_with_n_fft(n_fft, [&](auto nn) { frames_with_flag(hr_shift != nullptr, [&](auto s) { frames_with_flag(seeded, [&](auto g) {
            hipLaunchKernelGGL((lsd_rows_grad_frames_kernel<decltype(nn)::value, decltype(s)::value, decltype(g)::value>),
                               dim3(grid.blocks), dim3(LSD_NT), 0, st, hr, hr_total, sr, sr_total, rows, n_rows, frame_start,
                               total_frames, hr_shift, window, up, up_scale, hop, center != 0, grid.n_tiles, frames);
        }); }); });
    });
}

}  // namespace

extern "C" {

int mg_lsd_rows_backward(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                         int n_rows, const long long* frame_start, long long total_frames, const float* hr_shift,
                         const float* window, int n_fft, int hop, int center, const float* grad_rows, float* grad_sr,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return lsd_rows_backward(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, hr_shift, window, n_fft, hop, center,
                             grad_rows, 0.0, false, grad_sr, workspace, workspace_bytes, stream);
}

int mg_lsd_rows_backward_seeded(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                                int n_rows, const long long* frame_start, long long total_frames, const float* hr_shift,
                                const float* window, int n_fft, int hop, int center, const float* go, double scale, float* grad_sr,
                                void* workspace, size_t workspace_bytes, void* stream) {
    return lsd_rows_backward(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, hr_shift, window, n_fft, hop, center,
                             go, scale, true, grad_sr, workspace, workspace_bytes, stream);
}

}  // extern "C"
