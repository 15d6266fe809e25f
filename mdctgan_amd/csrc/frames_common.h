// What the three spectral losses' files (lsd_rows_grad.hip, stft_loss_rows.hip, mel_loss_rows.hip) share whatever transform they
// run, each statement once: on the device the conj Zt of the adjoint pack-and-split in the backward tail (the root value is the
// caller's), and on the host the operand checks, the grid of a frames launch, the n_fft and flag dispatch, and the backward's
// epilogue.  stft_frames.h builds the whole inverse tail of the STFT and mel losses on it; lsd_rows_grad_frames_kernel calls it
// inside a tail of its own around lsd_fft.h's float2 transform (lsd_fft.h's head says what is deliberately not shared, and why).
#pragma once
#include <type_traits>

#include "lsd_gather.h"

namespace {

// conj Zt_k of the adjoint of the pack-and-split: Zt_k = A_k + i B_k, A_k = H_k + conj H_{M-k}, B_k = (H_k - conj H_{M-k}) conj w,
// h1 = H_k, h2 = H_{M-k}, w = exp(-2 pi i k / N)
__device__ __forceinline__ float2 frames_conj_zt(float2 h1, float2 h2, float2 w) {
    const float2 a = make_float2(h1.x + h2.x, h1.y - h2.y);                         // H_k + conj H_{M-k}
    const float2 b = lsd_cmul(make_float2(h1.x - h2.x, h1.y + h2.y), make_float2(w.x, -w.y));
    return make_float2(a.x - b.y, -(a.y + b.x));                                    // conj (a + i b)
}

// ---- host ----
// the operands every frames entry point takes
inline bool frames_args_ok(const void* hr, long long hr_total, const void* sr, long long sr_total, const void* rows, int n_rows,
                           const void* frame_start, long long total_frames, const void* window, int n_fft, int hop) {
    return hr && sr && rows && frame_start && window && n_rows > 0 && total_frames > 0 && hr_total > 0 && sr_total > 0 && hop > 0 &&
           lsd_size_ok(n_fft);
}

inline bool frames_workspace_ok(size_t need, const void* workspace, size_t workspace_bytes) {
    return need != 0 && workspace && workspace_bytes >= need && al16(workspace);
}

// tiles of `tile` complex points and the grid that walks them: at most a few waves of `wg_per_cu` workgroups per CU
struct FramesGrid { long long n_tiles; unsigned blocks; };
inline FramesGrid frames_grid(long long total_frames, int n_fft, int tile, int wg_per_cu) {
    const long long ft = tile / n_fft, n_tiles = (total_frames + ft - 1) / ft, cap = wg_per_cu * 256 * 4;
    return {n_tiles, (unsigned)(n_tiles < cap ? n_tiles : cap)};
}

// f(std::integral_constant<int, n_fft>) for the sizes of lsd_size_ok; f(std::bool_constant<flag>)
template <typename F>
inline void frames_with_n_fft(int n_fft, F&& f) {
    if (n_fft == 512) f(std::integral_constant<int, 512>{});
    else if (n_fft == 1024) f(std::integral_constant<int, 1024>{});
    else f(std::integral_constant<int, 2048>{});
}
template <typename F>
inline void frames_with_flag(bool flag, F&& f) {
    if (flag) f(std::true_type{}); else f(std::false_type{});
}

// A backward pass after its operand checks: the workspace [total_frames][n_fft] and the gather's slot count are checked, then
// launch_frames(frames) fills the workspace (phase one) and the gather writes (or adds to) grad_sr (phase two).
template <typename Launch>
inline int frames_backward(const mg_metric_row* rows, int n_rows, const long long* frame_start, long long total_frames, int n_fft,
                           int hop, int center, long long sr_total, size_t need, void* workspace, size_t workspace_bytes,
                           bool accumulate, float* grad_sr, hipStream_t st, Launch&& launch_frames) {
    if (!frames_workspace_ok(need, workspace, workspace_bytes)) return MG_ERR_ARG;
    if (total_frames > (kFar - (long long)n_rows * n_fft) / hop) return MG_ERR_ARG;          // the gather's slot count
    float* frames = static_cast<float*>(workspace);
    launch_frames(frames);
    MG_CHECK_LAUNCH();
    return lsd_launch_gather(frames, rows, n_rows, frame_start, total_frames, n_fft, hop, center, sr_total, accumulate, grad_sr, st);
}

}  // namespace
