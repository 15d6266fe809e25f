// The training side of the reference's data path (data/audio_dataset.py:34-82, AudioDataset.readaudio + __getitem__) for a whole
// batch in shared launches: the corpus sits packed in one device buffer, a device row table says which window of it every batch
// row is, and (LR_audio, HR_audio) come out as two dense [B, seg_len] tensors.
//   train_hr_rows_kernel   resample_rows_kernel (resample_rows.hip) writing dense rows: hr[out_row][t] = resample(window, fs -> hr)[t]
//                          for t < min(seg_len, ceil(hr L / fs)), zero after (seg_pad_audio, :102-110).
//   train_lr_rows_kernel   both resampling steps of the low-rate leg in one kernel: a workgroup owns one tile of output samples of one
//                          row, computes the lr-rate intermediate samples that tile's taps touch into LDS (each by mg_resample's fmaf
//                          chain and rounded to float32 once, as the tensor between the reference's two aF.resample calls is), then
//                          runs the up-sampling chain from LDS.  The halo is recomputed per tile (48 -> 8 -> 48 kHz: 14 intermediates
//                          beside 171 per 1024 outputs).  FULL: the whole low-rate signal goes to the row's window of a packed buffer
//                          instead (--add_noise takes its power before the crop).
// A row's window [in_pos, in_pos + in_len) is the whole signal in both legs: taps outside it contribute nothing, whatever the
// corpus holds next to it.  Per output sample the chains are mg_resample's in ascending tap order, so a row has the bits of
// make_training_pair on its window alone.  No atomics; every store is guarded; the loops a workgroup runs depend on its row alone.
#include <limits.h>

#include "rows.h"

namespace {

struct Bank { const float* kern; int orig, new_, width; };          // kern == nullptr: equal rates, the step is a copy

constexpr int kThreads = 256;
constexpr int kTile = 1024;                      // output samples of one workgroup pass (the host may shrink it, see tile_for)
constexpr int kMidCap = 4096;                    // lr-rate intermediates of one tile held in LDS
constexpr int kBankCap = 2048;                   // floats of one filter bank held in LDS (rows padded to an odd stride)
constexpr int kMaxLen = 1 << 30;                 // rows of more output samples are refused / dropped: every index below stays an int

__host__ __device__ inline int bank_stride(int K) { return K | 1; }       // odd: the phases of neighbouring outputs sit on different banks
inline bool bank_fits(const Bank& b) {
    return b.kern && (long long)b.new_ * bank_stride(2 * b.width + b.orig) <= kBankCap;
}

__device__ __forceinline__ void stage_bank(float* dst, const Bank& b) {
    const int K = 2 * b.width + b.orig, S = bank_stride(K);
    for (int i = threadIdx.x; i < b.new_ * K; i += kThreads) dst[(i / K) * S + (i % K)] = b.kern[i];
}

// Sample o of resample(window) for the bank (kl, stride S): sample j of the window is x[pos + j] and exists for j in [j_lo, j_hi)
// -- the row's samples already cut to the corpus, or the intermediates a tile holds in LDS
__device__ __forceinline__ float chain_at(const float* x, long long pos, long long j_lo, long long j_hi, const float* kl, int S,
                                          int orig, int new_, int width, int o) {
    const int n = o / new_, p = o - n * new_;
    const long long t0 = (long long)n * orig - width;                      // sample index of tap 0
    int k_lo, k_hi;
    tap_range(j_lo, j_hi, t0, 2 * width + orig, k_lo, k_hi);
    return fir_chain<false>(x + (pos + t0), kl + p * S, k_lo, k_hi, 0.0f);
}

// The window of a row cut to the corpus; false: a dead or broken row
__device__ __forceinline__ bool row_window(const mg_train_row& rw, long long x_total, long long* j_lo, long long* j_hi) {
    if (rw.in_len <= 0 || rw.in_len > INT_MAX || rw.in_pos <= -kFar || rw.in_pos >= x_total) return false;
    *j_lo = rw.in_pos < 0 ? -rw.in_pos : 0;
    *j_hi = rw.in_len < x_total - rw.in_pos ? rw.in_len : x_total - rw.in_pos;
    return *j_lo < *j_hi;
}

template <bool BANK_IN_LDS>
__global__ __launch_bounds__(kThreads) void train_hr_rows_kernel(const float* __restrict__ x, long long x_total,
                                                                 const mg_train_row* __restrict__ rows, int n_rows, int seg_len,
                                                                 Bank bank, float* __restrict__ hr, long long out_rows) {
    __shared__ float bank_s[kBankCap];
    if (BANK_IN_LDS) {
        stage_bank(bank_s, bank);
        __syncthreads();
    }
    const int K = 2 * bank.width + bank.orig;
    const float* kl = BANK_IN_LDS ? bank_s : bank.kern;
    const int S = BANK_IN_LDS ? bank_stride(K) : K;
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const mg_train_row rw = rows[r];
        long long j_lo, j_hi;
        if (!row_window(rw, x_total, &j_lo, &j_hi) || rw.out_row < 0 || rw.out_row >= out_rows) continue;
        const long long len = bank.kern ? ((long long)bank.new_ * rw.in_len + bank.orig - 1) / bank.orig : rw.in_len;
        const int n_sig = (int)(len < seg_len ? len : seg_len);
        float* dst = hr + rw.out_row * (long long)seg_len;
        for (int o = blockIdx.x * kThreads + threadIdx.x; o < seg_len; o += gridDim.x * kThreads) {
            float v = 0.0f;
            if (o < n_sig) {
                if (bank.kern) v = chain_at(x, rw.in_pos, j_lo, j_hi, kl, S, bank.orig, bank.new_, bank.width, o);
                else if (o >= j_lo && o < j_hi) v = x[rw.in_pos + o];
            }
            dst[o] = v;
        }
    }
}

template <bool DOWN_IN_LDS, bool UP_IN_LDS, bool FULL>
__global__ __launch_bounds__(kThreads) void train_lr_rows_kernel(const float* __restrict__ x, long long x_total,
                                                                 const mg_train_row* __restrict__ rows, int n_rows, int seg_len,
                                                                 Bank down, Bank up, int tile_len, float* __restrict__ lr,
                                                                 long long out_rows, float* __restrict__ lr_full,
                                                                 long long full_total) {
    __shared__ float down_s[kBankCap];
    __shared__ float up_s[kBankCap];
    __shared__ float mid_s[kMidCap];
    if (DOWN_IN_LDS) stage_bank(down_s, down);
    if (UP_IN_LDS) stage_bank(up_s, up);
    if (DOWN_IN_LDS || UP_IN_LDS) __syncthreads();
    const int Kd = 2 * down.width + down.orig, Ku = 2 * up.width + up.orig;
    const float* kd = DOWN_IN_LDS ? down_s : down.kern;
    const float* ku = UP_IN_LDS ? up_s : up.kern;
    const int Sd = DOWN_IN_LDS ? bank_stride(Kd) : Kd, Su = UP_IN_LDS ? bank_stride(Ku) : Ku;

    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const mg_train_row rw = rows[r];
        long long j_lo, j_hi;
        if (!row_window(rw, x_total, &j_lo, &j_hi)) continue;
        // the intermediate exists for 0 <= i < mid_len, the low-rate signal for 0 <= o < lr_len
        const long long mid_len = down.kern ? ((long long)down.new_ * rw.in_len + down.orig - 1) / down.orig : rw.in_len;
        const long long lr_len = up.kern ? ((long long)up.new_ * mid_len + up.orig - 1) / up.orig : mid_len;
        if (mid_len > INT_MAX || lr_len > INT_MAX) continue;
        int n_out;
        float* dst;
        if (FULL) {
            if (rw.full_len <= 0 || rw.full_len > kMaxLen || rw.full_pos < 0 || rw.full_pos >= full_total ||
                rw.full_len > full_total - rw.full_pos) continue;
            n_out = (int)rw.full_len;
            dst = lr_full + rw.full_pos;
        } else {
            if (rw.out_row < 0 || rw.out_row >= out_rows) continue;
            n_out = seg_len;
            dst = lr + rw.out_row * (long long)seg_len;
        }
        const int n_sig = (int)(lr_len < n_out ? lr_len : n_out);
        const int n_tiles = (n_out + tile_len - 1) / tile_len;
        for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
            const int o0 = tile * tile_len;
            const int o1 = o0 + tile_len < n_out ? o0 + tile_len : n_out;
            const int s1 = o1 < n_sig ? o1 : n_sig;                       // [o0, s1): signal, [s1, o1): zero padding
            long long c_lo = 0, c_hi = 0;                                   // the intermediates this tile's taps touch
            if (up.kern && s1 > o0) {
                c_lo = (long long)(o0 / up.new_) * up.orig - up.width;
                c_hi = (long long)((s1 - 1) / up.new_) * up.orig - up.width + Ku;
                c_lo = c_lo < 0 ? 0 : c_lo;
                c_hi = c_hi > mid_len ? mid_len : c_hi;
                if (c_hi - c_lo > kMidCap) continue;                        // (the host's tile_len rules this out)
                for (long long i = c_lo + threadIdx.x; i < c_hi; i += kThreads)
                    mid_s[i - c_lo] = down.kern ? chain_at(x, rw.in_pos, j_lo, j_hi, kd, Sd, down.orig, down.new_, down.width, (int)i)
                                                : (i >= j_lo && i < j_hi ? x[rw.in_pos + i] : 0.0f);
            }
            __syncthreads();
            for (int o = o0 + threadIdx.x; o < o1; o += kThreads) {
                float v = 0.0f;
                if (o < s1) {
                    if (up.kern) {
                        v = chain_at(mid_s, -c_lo, c_lo, c_hi, ku, Su, up.orig, up.new_, up.width, o);
                    } else if (down.kern) {
                        v = chain_at(x, rw.in_pos, j_lo, j_hi, kd, Sd, down.orig, down.new_, down.width, o);
                    } else if (o >= j_lo && o < j_hi) {
                        v = x[rw.in_pos + o];
                    }
                }
                dst[o] = v;
            }
            __syncthreads();                                                // mid_s is rewritten by the next tile
        }
    }
}

inline bool bank_ok(const mg_resample_bank* b) {
    if (!b) return false;
    if (!b->kern) return true;
    return b->orig > 0 && b->new_ > 0 && b->width >= 0 && (long long)b->new_ * (2LL * b->width + b->orig) <= INT_MAX / 4;
}

inline Bank bank_of(const mg_resample_bank* b) { return Bank{b->kern, b->kern ? b->orig : 1, b->kern ? b->new_ : 1, b->kern ? b->width : 0}; }

// The longest tile whose intermediates fit kMidCap: (floor((T - 1) / new) + 1) * orig + K <= kMidCap; 0: none does
inline int tile_for(const Bank& up) {
    if (!up.kern) return kTile;
    const long long m = ((long long)kMidCap - (2LL * up.width + up.orig)) / up.orig - 1;
    if (m < 0) return 0;
    const long long t = (m + 1) * up.new_;
    return (int)(t < kTile ? t : kTile);
}

// The two legs' checks and launches, shared by the three entry points below
inline bool pair_args_ok(const float* corpus, long long corpus_total, const mg_train_row* rows, int n_rows, int seg_len,
                         long long out_rows) {
    return corpus && rows && n_rows > 0 && seg_len > 0 && seg_len <= kMaxLen && corpus_total > 0 && out_rows > 0 &&
           out_rows <= LLONG_MAX / seg_len;
}

int launch_hr(const float* corpus, long long corpus_total, const mg_train_row* rows, int n_rows, int seg_len, const Bank& bh,
              float* hr, long long out_rows, hipStream_t st) {
    const dim3 gh = rows_grid(n_rows, seg_len, kThreads);
    if (bank_fits(bh))
        hipLaunchKernelGGL(train_hr_rows_kernel<true>, gh, dim3(kThreads), 0, st, corpus, corpus_total, rows, n_rows, seg_len, bh, hr,
                           out_rows);
    else
        hipLaunchKernelGGL(train_hr_rows_kernel<false>, gh, dim3(kThreads), 0, st, corpus, corpus_total, rows, n_rows, seg_len, bh, hr,
                           out_rows);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

int launch_lr(const float* corpus, long long corpus_total, const mg_train_row* rows, int n_rows, int seg_len, const Bank& bd,
              const Bank& bu, float* lr, long long out_rows, float* lr_full, long long lr_full_total, long long max_full_len,
              hipStream_t st) {
    const int tile_len = tile_for(bu);
    if (tile_len <= 0) return MG_ERR_UNSUPPORTED;
    const dim3 gl = rows_grid(n_rows, lr_full ? max_full_len : (long long)seg_len, tile_len);
#define MG_TL_LAUNCH(D, U, F)                                                                                                     \
    hipLaunchKernelGGL((train_lr_rows_kernel<D, U, F>), gl, dim3(kThreads), 0, st, corpus, corpus_total, rows, n_rows, seg_len, bd, \
                       bu, tile_len, lr, out_rows, lr_full, lr_full_total)
#define MG_TL_FULL(D, U) do { if (lr_full) MG_TL_LAUNCH(D, U, true); else MG_TL_LAUNCH(D, U, false); } while (0)
    if (bank_fits(bd)) {
        if (bank_fits(bu)) MG_TL_FULL(true, true); else MG_TL_FULL(true, false);
    } else {
        if (bank_fits(bu)) MG_TL_FULL(false, true); else MG_TL_FULL(false, false);
    }
#undef MG_TL_FULL
#undef MG_TL_LAUNCH
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // namespace

extern "C" {

// See include/mdctgan_hip.h.
int mg_train_pair_rows(const float* corpus, long long corpus_total, const mg_train_row* rows, int n_rows, int seg_len,
                       const mg_resample_bank* to_hr, const mg_resample_bank* to_lr, const mg_resample_bank* lr_to_hr, float* lr,
                       float* hr, long long out_rows, float* lr_full, long long lr_full_total, long long max_full_len,
                       void* stream) {
    if (!hr || !pair_args_ok(corpus, corpus_total, rows, n_rows, seg_len, out_rows)) return MG_ERR_ARG;
    if (!bank_ok(to_hr) || !bank_ok(to_lr) || !bank_ok(lr_to_hr)) return MG_ERR_ARG;
    if (lr_full ? (lr_full_total <= 0 || max_full_len <= 0) : !lr) return MG_ERR_ARG;
    if (tile_for(bank_of(lr_to_hr)) <= 0) return MG_ERR_UNSUPPORTED;
    const int rc = launch_hr(corpus, corpus_total, rows, n_rows, seg_len, bank_of(to_hr), hr, out_rows, (hipStream_t)stream);
    if (rc != MG_OK) return rc;
    return launch_lr(corpus, corpus_total, rows, n_rows, seg_len, bank_of(to_lr), bank_of(lr_to_hr), lr, out_rows, lr_full,
                     lr_full_total, max_full_len, (hipStream_t)stream);
}

int mg_train_hr_rows(const float* corpus, long long corpus_total, const mg_train_row* rows, int n_rows, int seg_len,
                     const mg_resample_bank* to_hr, float* hr, long long out_rows, void* stream) {
    if (!hr || !pair_args_ok(corpus, corpus_total, rows, n_rows, seg_len, out_rows) || !bank_ok(to_hr)) return MG_ERR_ARG;
    return launch_hr(corpus, corpus_total, rows, n_rows, seg_len, bank_of(to_hr), hr, out_rows, (hipStream_t)stream);
}

int mg_train_lr_rows(const float* corpus, long long corpus_total, const mg_train_row* rows, int n_rows, int seg_len,
                     const mg_resample_bank* to_lr, const mg_resample_bank* lr_to_hr, float* lr, long long out_rows, float* lr_full,
                     long long lr_full_total, long long max_full_len, void* stream) {
    if (!pair_args_ok(corpus, corpus_total, rows, n_rows, seg_len, out_rows)) return MG_ERR_ARG;
    if (!bank_ok(to_lr) || !bank_ok(lr_to_hr)) return MG_ERR_ARG;
    if (lr_full ? (lr_full_total <= 0 || max_full_len <= 0) : !lr) return MG_ERR_ARG;
    return launch_lr(corpus, corpus_total, rows, n_rows, seg_len, bank_of(to_lr), bank_of(lr_to_hr), lr, out_rows, lr_full,
                     lr_full_total, max_full_len, (hipStream_t)stream);
}

}  // extern "C"
