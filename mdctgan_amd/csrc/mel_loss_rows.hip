// The multi-scale mel-spectrogram L1 loss of many utterances in shared launches (Python: metrics.mel_many / mel_loss / mel_loss_term;
// the training term of --lambda_mel), on the frame machinery of the multi-resolution STFT loss: stft_frames.h's staging with the
// reflection at the row's own ends, the double transform rounded to float32 once per bin, the clamp of the magnitudes, and the
// float32 inverse, window store and gather of its backward.  What is new here is what happens between the magnitudes and the sums.
//
// One resolution r = (N, hop, J), window [N] (the host passes the periodic Hann window), K = N/2 + 1 bins, F_u frames of row u, a
// float32 filterbank W [J][K] (the host passes the HTK triangles of metrics.mel_fbank) widened to double.  With p = re^2 + im^2 of
// the float32 spectrum (p formed in double) and m = sqrt(max(p, 1e-7)), per frame f and filter j
//     E_j = sum_k W[j][k] m_k  (double, k ascending)     l_j = ln max(E_j, 1e-5)
//     loss_u = sum_{f,j} |l_hr - l_sr| / (F_u J)
// Gradient with respect to sr only.  At the non-smooth points, by definition: a filter with l_hr == l_sr contributes 0 (sign(0) =
// 0), a filter with E_sr <= 1e-5 contributes 0 (the floor of the log), a bin with p_sr < 1e-7 contributes 0 (the clamp).  So silence
// against silence, an all-zero sr and sr == hr (the same statements on both operands) have gradient exactly 0, and the first and
// last have loss exactly 0.
//
// The filterbank comes with two int32 tables that the host derives from it: band_k [J][2], filter j's support [k_lo, k_hi), and
// band_j [K][2], the filters [j_lo, j_hi) that contain bin k.  W is read inside those bands only, and the kernels clip every band to
// the matrix, so tables that do not agree with W lose terms and nothing is read outside a buffer.
//
//   mel_loss_frames_kernel   forward, one launch over all frames of the pack: stft_loss_frames_kernel up to the magnitudes, which
//       every lane keeps in registers until all lanes of the workgroup have read their Z[k] and Z[M-k] (a barrier) and then writes
//       over the dead frame data as doubles, frame fr at [fr 2N .. ): m_hr [K], m_sr [K].  Then lane j of the frame's lanes owns
//       filters j, j + TPF, ... and walks each band in ascending k (both operands share the W read); the lanes of a frame sum |l_hr -
//       l_sr| in stft_loss_frames_kernel's tree and lane 0 stores the frame's double to partial [total_frames] (a frame outside
//       every live row: 0).  LDS as the STFT loss: 32 KiB of frame data + 8 N bytes of roots; the filter walk adds none.
//   mel_loss_finish_kernel   one thread per row: the row's frames in ascending order -> row_out[u] = {sum, 0, 0, loss_u}: the layout
//       of mg_stft_loss_rows, so that mg_stft_loss_mean is the loss node of a dense batch unchanged.
//   mel_loss_grad_frames_kernel   backward, phase one: both spectra, both m arrays and E of both operands again (no per-frame
//       state is kept from the forward), then per filter, in double, with g_u the row's upstream gradient
//           dE_j = -g_u sign(l_hr - l_sr) / (F_u J E_sr)     (0 where E_sr <= 1e-5)
//       to LDS behind the m arrays (J <= 256 doubles: K + K + J <= 2 N), then per bin, on the lane that holds X_sr[k] in registers,
//           dm_k = sum_{j in band_j[k]} W[j][k] dE_j  (j ascending)     c_k = dm_k / m_sr   (0 where p_sr < 1e-7)     G_k = c_k X_sr[k]
//       and from G_k on stft_loss_grad_frames_kernel's statements: the Hermitian halves rounded to float32 once, the float32 inverse
//       through the same stages, y[n] window[n] to the workspace [total_frames][N].  SEEDED: g_u is formed here from the loss node's
//       upstream scalar go [1] as ((go[0] * up_scale) / n_rows) / n_res in double and rounded to float32 -- the float32 row gradient
//       that autograd hands the unseeded form for scale * the mean over a dense batch -- when the kernel runs, so a captured step
//       follows a loss scale that changes between replays.
//   lsd_rows_grad_gather_kernel   phase two, lsd_gather.h.
// Static LDS only, no atomics, no host read-back, launch counts independent of the number of rows; no arithmetic for a row depends
// on where the row sits, so a row has the same value and gradient bits alone and in any pack.
// Shared with stft_loss_rows.hip through stft_frames.h: everything up to the float32 spectrum, the sum of a frame's lanes
// (sd_frame_sum) and the backward's tail from H_k on (sd_inverse_tail); the host side (operand checks, grid, n_fft dispatch, the
// backward's epilogue with the gather) is frames_common.h's, shared with lsd_rows_grad.hip too.  Deliberately this file's own:
// the seeded gradient ROUNDED to float32 (the STFT loss keeps the double; each is asserted bit for bit) and mel_loss_finish_kernel.
#include "stft_frames.h"

namespace {

constexpr double kMelFloor = 1e-5;
constexpr int MEL_MAX_FILTERS = 256;

// [lo, hi) of a band table entry, clipped to [0, n)
__device__ __forceinline__ void mel_band(const int* __restrict__ band, int i, int n, int& lo, int& hi) {
    lo = band[2 * i];
    hi = band[2 * i + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
}

// E_j of both operands: filter j's band of the frame's m arrays (LDS) in ascending k
template <int NBINS>
__device__ __forceinline__ void mel_energies(const float* __restrict__ fbank, const int* __restrict__ band_k, int j,
                                             const double* __restrict__ mh, const double* __restrict__ ms, double& eh, double& es) {
    int lo, hi;
    mel_band(band_k, j, NBINS, lo, hi);
    const float* __restrict__ w = fbank + (long long)j * NBINS;
    eh = 0.0;
    es = 0.0;
    for (int k = lo; k < hi; ++k) {
        const double wk = (double)w[k];
        eh += wk * mh[k];
        es += wk * ms[k];
    }
}

template <int N>
__global__ __launch_bounds__(LSD_NT) void mel_loss_frames_kernel(const float* __restrict__ hr, long long hr_total,
                                                                 const float* __restrict__ sr, long long sr_total,
                                                                 const mg_metric_row* __restrict__ rows, int n_rows,
                                                                 const long long* __restrict__ frame_start, long long total_frames,
                                                                 const float* __restrict__ window, const float* __restrict__ fbank,
                                                                 const int* __restrict__ band_k, int n_mels, int hop, int center,
                                                                 long long n_tiles, double* __restrict__ partial) {
    constexpr int M = N / 2, FT = SD_TILE / N, TPF = LSD_NT / FT, NBINS = N / 2 + 1, BPL = (NBINS + TPF - 1) / TPF;
    static_assert(TPF >= 64 && M % LSD_NT == 0, "a frame's lanes fill whole waves, a load pass stays inside one signal of a frame");
    static_assert(2 * NBINS <= 2 * N, "a frame's two m arrays fit its dead frame data");
    __shared__ __attribute__((aligned(16))) double2 buf[SD_TILE];          // [FT][hr, sr][M]; then, as double: [FT][2 N] holding m_hr, m_sr
    __shared__ __attribute__((aligned(16))) double2 root[N / 2];
    __shared__ double red[LSD_NT / 64][1];
    __shared__ LsdFrame info[FT];
    double* mbuf = reinterpret_cast<double*>(buf);
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
        double mh[BPL], ms[BPL];
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int k = j + i * TPF;
            mh[i] = ms[i] = 0.0;
            if (k < NBINS) {
                const float2 a = sd_real_bin<M>(Zh, k, root), b = sd_real_bin<M>(Zs, k, root);
                mh[i] = sqrt(fmax((double)a.x * a.x + (double)a.y * a.y, kStftClamp));
                ms[i] = sqrt(fmax((double)b.x * b.x + (double)b.y * b.y, kStftClamp));
            }
        }
        __syncthreads();                                    // every lane has read its Z[k] and Z[M-k]: the frame data is dead
        double* Mh = mbuf + fr * 2 * N;
        double* Ms = Mh + NBINS;
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int k = j + i * TPF;
            if (k < NBINS) {
                Mh[k] = mh[i];
                Ms[k] = ms[i];
            }
        }
        __syncthreads();
        double acc[1] = {0.0};
        for (int f = j; f < n_mels; f += TPF) {
            double eh, es;
            mel_energies<NBINS>(fbank, band_k, f, Mh, Ms, eh, es);
            acc[0] += fabs(log(fmax(eh, kMelFloor)) - log(fmax(es, kMelFloor)));
        }
        sd_frame_sum<1, TPF>(acc, red, tid, fr, j);
        if (j == 0) {
            const long long g = tile * FT + fr;
            if (g < total_frames) partial[g] = info[fr].live != 0 ? acc[0] : 0.0;
        }
        __syncthreads();                                    // buf, info and red are free for the next tile
    }
}

__global__ __launch_bounds__(256) void mel_loss_finish_kernel(const double* __restrict__ partial, const mg_metric_row* __restrict__ rows,
                                                              int n_rows, const long long* __restrict__ frame_start,
                                                              long long total_frames, int n_mels, double* __restrict__ row_out) {
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < n_rows; u += (long long)gridDim.x * 256) {
        long long f0, nf;
        double s = 0.0, loss = 0.0;
        if (stft_row_frames(rows, frame_start, total_frames, (int)u, f0, nf)) {
            for (long long f = f0; f < f0 + nf; ++f) s += partial[f];
            loss = s / ((double)nf * (double)n_mels);
        }
        row_out[u * 4 + 0] = s;
        row_out[u * 4 + 1] = 0.0;
        row_out[u * 4 + 2] = 0.0;
        row_out[u * 4 + 3] = loss;
    }
}

template <int N, bool SEEDED>
__global__ __launch_bounds__(LSD_NT) void mel_loss_grad_frames_kernel(const float* __restrict__ hr, long long hr_total,
                                                                      const float* __restrict__ sr, long long sr_total,
                                                                      const mg_metric_row* __restrict__ rows, int n_rows,
                                                                      const long long* __restrict__ frame_start,
                                                                      long long total_frames, const float* __restrict__ window,
                                                                      const float* __restrict__ fbank, const int* __restrict__ band_k,
                                                                      const int* __restrict__ band_j, int n_mels,
                                                                      const float* __restrict__ up, double up_scale, int n_res,
                                                                      int hop, int center, long long n_tiles,
                                                                      float* __restrict__ frames_out) {
    constexpr int M = N / 2, FT = SD_TILE / N, TPF = LSD_NT / FT, NBINS = N / 2 + 1, BPL = (NBINS + TPF - 1) / TPF;
    static_assert(TPF >= 64 && M % LSD_NT == 0, "a frame's lanes fill whole waves, a load pass stays inside one signal of a frame");
    static_assert(2 * NBINS + MEL_MAX_FILTERS <= 2 * N, "a frame's m arrays and dE fit its dead frame data");
    __shared__ __attribute__((aligned(16))) double2 buf[SD_TILE];          // [FT][hr, sr][M] double; then, as double: [FT][2 N] holding
    __shared__ __attribute__((aligned(16))) double2 root[N / 2];           //   m_hr, m_sr, dE; then, as float2: [FT][N] holding H_k; then [FT][M]
    __shared__ LsdFrame info[FT];
    __shared__ double coef[FT];                                            // g / (F J)
    float2* fbuf = reinterpret_cast<float2*>(buf);
    double* mbuf = reinterpret_cast<double*>(buf);
    const int tid = threadIdx.x;
    sd_roots<N>(root, tid);
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (tid < FT) {
            int row;
            const LsdFrame fi = lsd_locate<false>(tile * FT + tid, rows, n_rows, frame_start, total_frames, nullptr, N, hop, center, row);
            info[tid] = fi;
            double c = 0.0;
            if (fi.live) {
                const double g = SEEDED ? (double)(float)((((double)up[0] * up_scale) / (double)n_rows) / (double)n_res) : (double)up[row];
                c = g / ((double)(frame_start[row + 1] - frame_start[row]) * (double)n_mels);
            }
            coef[tid] = c;
        }
        __syncthreads();
        sd_load_tile<N>(buf, info, hr, hr_total, sr, sr_total, window, center, tid);
        __syncthreads();
        sd_fft<M, SD_TILE>(buf, root, tid);
        // pass one: the magnitudes and X_sr of bins k = j, j + TPF, ... of frame fr on lane j of the frame's TPF lanes, in registers
        const int fr = tid / TPF, j = tid % TPF;
        const double2* Zh = buf + fr * N;
        const double2* Zs = Zh + M;
        const double c_l1 = coef[fr];
        double mh[BPL], ms[BPL];                            // ms < 0: the bin is clamped (p_sr < 1e-7)
        float2 xs[BPL];
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int k = j + i * TPF;
            mh[i] = ms[i] = 0.0;
            xs[i] = make_float2(0.0f, 0.0f);
            if (k < NBINS) {
                const float2 a = sd_real_bin<M>(Zh, k, root), b = sd_real_bin<M>(Zs, k, root);
                const double pb = (double)b.x * b.x + (double)b.y * b.y;
                mh[i] = sqrt(fmax((double)a.x * a.x + (double)a.y * a.y, kStftClamp));
                ms[i] = pb >= kStftClamp ? sqrt(pb) : -1.0;
                xs[i] = b;
            }
        }
        __syncthreads();                                    // every lane has read its Z[k] and Z[M-k]: the doubles are dead
        double* Mh = mbuf + fr * 2 * N;
        double* Ms = Mh + NBINS;
        double* dE = Ms + NBINS;
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int k = j + i * TPF;
            if (k < NBINS) {
                Mh[k] = mh[i];
                Ms[k] = ms[i] < 0.0 ? sqrt(kStftClamp) : ms[i];
            }
        }
        __syncthreads();
        // pass two: dL/dE_sr of filters j, j + TPF, ...
        for (int f = j; f < n_mels; f += TPF) {
            double eh, es, d = 0.0;
            mel_energies<NBINS>(fbank, band_k, f, Mh, Ms, eh, es);
            if (es > kMelFloor) {
                const double dl = log(fmax(eh, kMelFloor)) - log(es);
                const double sg = dl > 0.0 ? 1.0 : (dl < 0.0 ? -1.0 : 0.0);
                d = -(c_l1 * sg) / es;
            }
            dE[f] = d;
        }
        __syncthreads();
        // pass three: H_k of the lane's bins
        float2 h[BPL];
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int k = j + i * TPF;
            h[i] = make_float2(0.0f, 0.0f);
            if (k < NBINS && ms[i] > 0.0) {
                int lo, hi;
                mel_band(band_j, k, n_mels, lo, hi);
                double dm = 0.0;
                for (int f = lo; f < hi; ++f) dm += (double)fbank[(long long)f * NBINS + k] * dE[f];
                const double c = dm / ms[i];
                h[i] = (k == 0 || k == M) ? make_float2((float)(c * (double)xs[i].x), 0.0f)
                                          : make_float2((float)(0.5 * c * (double)xs[i].x), (float)(0.5 * c * (double)xs[i].y));
            }
        }
        __syncthreads();                                    // every lane has read its dE: the doubles are dead
        sd_inverse_tail<N>(h, fbuf, root, window, frames_out, tile, total_frames, tid);
        __syncthreads();                                    // buf, info and coef are free for the next tile
    }
}

bool mel_args_ok(const void* hr, long long hr_total, const void* sr, long long sr_total, const void* rows, int n_rows,
                 const void* frame_start, long long total_frames, const void* window, const void* fbank, const void* band_k,
                 const void* band_j, int n_mels, int n_fft, int hop) {
    if (!frames_args_ok(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop)) return false;
    if (!fbank || !band_k || !band_j || n_mels < 1 || n_mels > MEL_MAX_FILTERS) return false;
    return ((uintptr_t)fbank & 3) == 0 && ((uintptr_t)band_k & 3) == 0 && ((uintptr_t)band_j & 3) == 0;
}

}  // namespace

extern "C" {

// See include/mdctgan_hip.h.
size_t mg_mel_loss_rows_workspace(long long total_frames) {
    if (total_frames <= 0 || total_frames > kFar / (long long)sizeof(double)) return 0;
    return (size_t)total_frames * sizeof(double);
}

size_t mg_mel_loss_rows_backward_workspace(long long total_frames, int n_fft) {
    return mg_stft_loss_rows_backward_workspace(total_frames, n_fft);
}

int mg_mel_loss_rows(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows, int n_rows,
                     const long long* frame_start, long long total_frames, const float* window, int n_fft, int hop, int center,
                     const float* fbank, const int* band_k, const int* band_j, int n_mels, double* row_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (!mel_args_ok(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, fbank, band_k, band_j, n_mels, n_fft,
                     hop) || !row_out || !frames_workspace_ok(mg_mel_loss_rows_workspace(total_frames), workspace, workspace_bytes))
        return MG_ERR_ARG;
    double* partial = static_cast<double*>(workspace);
    const FramesGrid grid = frames_grid(total_frames, n_fft, SD_TILE, 3);                 // as mg_stft_loss_rows
    hipStream_t st = (hipStream_t)stream;
    frames_with_n_fft(n_fft, [&](auto nn) {
        hipLaunchKernelGGL((mel_loss_frames_kernel<decltype(nn)::value>), dim3(grid.blocks), dim3(LSD_NT), 0, st, hr, hr_total, sr,
                           sr_total, rows, n_rows, frame_start, total_frames, window, fbank, band_k, n_mels, hop, center != 0,
                           grid.n_tiles, partial);
    });
    MG_CHECK_LAUNCH();
    const unsigned fblocks = (unsigned)((n_rows + 255) / 256 < 1024 ? (n_rows + 255) / 256 : 1024);
    hipLaunchKernelGGL(mel_loss_finish_kernel, dim3(fblocks), dim3(256), 0, st, partial, rows, n_rows, frame_start, total_frames,
                       n_mels, row_out);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"

namespace {

// both entry points: `up` is grad_rows [n_rows] (seeded == false) or go [1] with up_scale and n_res
int mel_loss_rows_backward(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                           int n_rows, const long long* frame_start, long long total_frames, const float* window, int n_fft, int hop,
                           int center, const float* fbank, const int* band_k, const int* band_j, int n_mels, const float* up,
                           double up_scale, int n_res, bool seeded, int accumulate, float* grad_sr, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!mel_args_ok(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, fbank, band_k, band_j, n_mels, n_fft,
                     hop) || !up || !grad_sr || n_res <= 0)
        return MG_ERR_ARG;
    const FramesGrid grid = frames_grid(total_frames, n_fft, SD_TILE, 3);
    hipStream_t st = (hipStream_t)stream;
    return frames_backward(rows, n_rows, frame_start, total_frames, n_fft, hop, center, sr_total,
                           mg_mel_loss_rows_backward_workspace(total_frames, n_fft), workspace, workspace_bytes, accumulate != 0,
                           grad_sr, st, [&](float* frames) {
        frames_with_n_fft(n_fft, [&](auto nn) { frames_with_flag(seeded, [&](auto g) {
            hipLaunchKernelGGL((mel_loss_grad_frames_kernel<decltype(nn)::value, decltype(g)::value>), dim3(grid.blocks),
                               dim3(LSD_NT), 0, st, hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window,
                               fbank, band_k, band_j, n_mels, up, up_scale, n_res, hop, center != 0, grid.n_tiles, frames);
        }); });
    });
}

}  // namespace

extern "C" {

int mg_mel_loss_rows_backward(const float* hr, long long hr_total, const float* sr, long long sr_total, const mg_metric_row* rows,
                              int n_rows, const long long* frame_start, long long total_frames, const float* window, int n_fft,
                              int hop, int center, const float* fbank, const int* band_k, const int* band_j, int n_mels,
                              const float* grad_rows, int accumulate, float* grad_sr, void* workspace, size_t workspace_bytes,
                              void* stream) {
    return mel_loss_rows_backward(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop, center,
                                  fbank, band_k, band_j, n_mels, grad_rows, 0.0, 1, false, accumulate, grad_sr, workspace,
                                  workspace_bytes, stream);
}

int mg_mel_loss_rows_backward_seeded(const float* hr, long long hr_total, const float* sr, long long sr_total,
                                     const mg_metric_row* rows, int n_rows, const long long* frame_start, long long total_frames,
                                     const float* window, int n_fft, int hop, int center, const float* fbank, const int* band_k,
                                     const int* band_j, int n_mels, const float* go, double scale, int n_res, int accumulate,
                                     float* grad_sr, void* workspace, size_t workspace_bytes, void* stream) {
    return mel_loss_rows_backward(hr, hr_total, sr, sr_total, rows, n_rows, frame_start, total_frames, window, n_fft, hop, center,
                                  fbank, band_k, band_j, n_mels, go, scale, n_res, true, accumulate, grad_sr, workspace,
                                  workspace_bytes, stream);
}

}  // extern "C"
