// The adjoint of framing and reflection, shared by every backward pass that leaves one window-weighted float32 gradient frame per
// STFT frame in a workspace [total_frames][N]: lsd_rows_grad.hip (the log-spectral distance), stft_loss_rows.hip (the
// multi-resolution STFT loss) and mel_loss_rows.hip (the mel-spectrogram loss).  Stated once so that they cannot drift apart.
//   lsd_rows_grad_gather_kernel   one thread per sample slot; row u owns the slots [S_u, S_u + frames_u hop + N), S_u =
//       frame_start[u] hop + u N (its len never exceeds that), found by binary search.  Sample t sums the workspace taps that
//       framing mapped to it -- the direct position t, on a centred transform the left reflection -t (1 <= t <= N/2) and the
//       right reflection 2 (len - 1) - t (t < len - 1, inside the right padding); for each, every frame whose span covers the
//       position, ascending -- in double in that order, rounds once and stores once to grad_sr[sr_pos + t].  ACC: the rounded sum
//       is added to what grad_sr[sr_pos + t] holds (one float32 add by the one thread that owns the sample: the second and later
//       resolutions of a multi-resolution loss, launched in resolution order on one stream).  Samples outside the rows, dead rows,
//       samples outside the sr buffer and centred rows of at most N/2 samples (the forward's staging would reflect them twice;
//       plan_metrics refuses them) are never written.
#pragma once
#include "lsd_fft.h"

namespace {

template <bool ACC>
__global__ __launch_bounds__(256) void lsd_rows_grad_gather_kernel(const float* __restrict__ frames, const mg_metric_row* __restrict__ rows,
                                                                   int n_rows, const long long* __restrict__ frame_start,
                                                                   long long total_frames, int n_fft, int hop, int center,
                                                                   long long sr_total, long long n_slots,
                                                                   float* __restrict__ grad_sr) {
    const long long N = n_fft, H = hop, off = center ? N / 2 : 0;
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < n_slots; s += (long long)gridDim.x * 256) {
        int lo = 0, hi = n_rows;                           // the last u with S_u <= s
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (frame_start[mid] * H + mid * N <= s) lo = mid; else hi = mid;
        }
        const mg_metric_row rw = rows[lo];
        const long long f0 = frame_start[lo], nf = frame_start[lo + 1] - f0, t = s - (f0 * H + lo * N);
        // (the frames kernel's rules: a table that does not agree with itself loses samples, it reads nothing outside the workspace)
        if (!lsd_row_ok(rw) || f0 < 0 || nf <= 0 || nf - 1 > INT_MAX || f0 + nf > total_frames || t < 0 || t >= rw.len) continue;
        // a centred row of at most N/2 samples is reflected twice by the staging (the planner refuses it): it gets no gradient
        if (center && rw.len <= N / 2) continue;
        const long long p = rw.sr_pos + t;
        if (p < 0 || p >= sr_total) continue;
        double acc = 0.0;
        // the taps at position q of the padded row (tap 0 of frame 0 = position 0), frames ascending
        auto take = [&](long long q) {
            const long long f_lo = q - N + 1 <= 0 ? 0 : (q - N + H) / H;
            const long long f_hi = q / H < nf - 1 ? q / H : nf - 1;
            for (long long f = f_lo; f <= f_hi; ++f) acc += (double)frames[(f0 + f) * N + (q - f * H)];
        };
        take(t + off);
        if (center) {
            if (t >= 1 && t <= N / 2) take(off - t);
            const long long r = 2 * (rw.len - 1) - t;
            if (t < rw.len - 1 && r <= rw.len - 1 + N / 2) take(r + off);
        }
        grad_sr[p] = ACC ? grad_sr[p] + (float)acc : (float)acc;
    }
}

// The gather's launch over the frames of `workspace`; the caller has checked that the slot count does not overflow
// (total_frames <= (kFar - n_rows n_fft) / hop).  -> the launch's status.
inline int lsd_launch_gather(const float* frames, const mg_metric_row* rows, int n_rows, const long long* frame_start,
                             long long total_frames, int n_fft, int hop, int center, long long sr_total, bool accumulate,
                             float* grad_sr, hipStream_t st) {
    const long long n_slots = total_frames * hop + (long long)n_rows * n_fft;
    const long long want = (n_slots + 255) / 256;
    const unsigned gblocks = (unsigned)(want < 256 * 64 ? want : 256 * 64);
    if (accumulate)
        hipLaunchKernelGGL(lsd_rows_grad_gather_kernel<true>, dim3(gblocks), dim3(256), 0, st, frames, rows, n_rows, frame_start,
                           total_frames, n_fft, hop, center != 0, sr_total, n_slots, grad_sr);
    else
        hipLaunchKernelGGL(lsd_rows_grad_gather_kernel<false>, dim3(gblocks), dim3(256), 0, st, frames, rows, n_rows, frame_start,
                           total_frames, n_fft, hop, center != 0, sr_total, n_slots, grad_sr);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // namespace
