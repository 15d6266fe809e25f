// A cascade of second-order sections (an IIR low-pass: Butterworth, Chebyshev) over the rows of a packed buffer, one pass or
// forward-backward (zero phase), for filter-diverse low-rate training inputs (lowpass.py, train_data.training_batch_many).
// Every row has its own window (mg_sos_row) and its own MG_SOS_MAX_SECTIONS x 6 coefficients; the recursion runs in double.
//
// The recursion is serial along time, so a row is cut into chunks of MG_SOS_CHUNK samples, one lane per chunk.  The cascade is a
// linear system with a state of 2 x 6 doubles (transposed direct form II, s1 / s2 per section), hence per pass
//   sos_pass_kernel<., false>   every chunk from a zero state -> its end state e_c; in the forward pass one more workgroup per row
//                               runs MG_SOS_CHUNK zero-input steps from each unit state: the columns of the chunk transition
//                               matrix T (the same for both passes: same filter, same chunk length)
//   sos_carry_kernel            s_0 = 0, s_{c+1} = T s_c + e_c along the row in ascending chunk order; 12 lanes hold a row of T each
//                               and read the state out of one another's registers; the start states replace the end states
//   sos_pass_kernel<., true>    every chunk again from its true start state, storing
// Chunks are counted from the row's first sample (forward) or from its last sample (reverse), never from the buffer, and the sums
// of the carry have one fixed order: a row has the same bits alone, in any pack, in any order and from run to run.  No atomics.
// The value between the two passes stays double: the forward pass writes sample t to the place the reverse pass reads it from,
// mid[j][c] with (c, j) the reverse chunk and offset of t, so that both sides coalesce across lanes.  A lane walking its chunk
// of the float32 input (or output) would touch one cache line per lane; the 64 chunks of a workgroup go through LDS instead,
// 16 samples of every chunk at a time, rows padded to 17 floats, the next tile's loads in flight during the
// recursion of this one.  The input window is cut to its buffer and the signal is zero outside it; every store is guarded.
// LDS is static (9 KB / 13 KB), no function attribute is set, nothing synchronises with the host: the launches can be captured.
#include <limits.h>

#include "rows.h"

namespace {

constexpr int kC = MG_SOS_CHUNK;                 // samples of one chunk = of one lane
constexpr int kSub = 16;                         // samples of every chunk that a workgroup stages at a time (measured: DESIGN.md)
constexpr int kLanes = 64;                       // chunks of one workgroup: one wave
constexpr int kPad = kSub + 1;                   // LDS row stride in floats, odd: lane l reads bank (17 l + j) % 32
constexpr int kSec = MG_SOS_MAX_SECTIONS;
constexpr int kState = 2 * kSec;
constexpr int kCarry = 128;                      // chunks whose states the carry holds in LDS at a time
constexpr long long kMaxLen = 1LL << 30;         // longer rows are refused: every index inside a row stays an int

static_assert(kC % kSub == 0, "a chunk is a whole number of staged tiles");

struct Coef { double b0[kSec], b1[kSec], b2[kSec], a1[kSec], a2[kSec]; };

__device__ __forceinline__ Coef load_coef(const double* __restrict__ sos) {
    Coef c;
#pragma unroll
    for (int k = 0; k < kSec; ++k) {
        c.b0[k] = sos[6 * k]; c.b1[k] = sos[6 * k + 1]; c.b2[k] = sos[6 * k + 2];
        c.a1[k] = sos[6 * k + 4]; c.a2[k] = sos[6 * k + 5];                 // (a0 == 1: the caller normalises)
    }
    return c;
}

// One sample through the cascade, transposed direct form II per section
__device__ __forceinline__ double cascade_step(const Coef& c, double (&s)[kState], double x) {
#pragma unroll
    for (int k = 0; k < kSec; ++k) {
        const double y = fma(c.b0[k], x, s[2 * k]);
        s[2 * k] = fma(-c.a1[k], y, fma(c.b1[k], x, s[2 * k + 1]));
        s[2 * k + 1] = fma(-c.a2[k], y, c.b2[k] * x);
        x = y;
    }
    return x;
}

// The workspace: per row the double signal between the passes [kC][nc_max], the chunk states [kState][nc_max] and T [kState][kState]
struct Work { double* mid; double* st; double* T; };
__host__ __device__ inline size_t work_doubles_per_row(long long nc_max) { return (size_t)(kC + kState) * nc_max + kState * kState; }
__device__ __forceinline__ Work work_of(double* ws, int r, int nc_max) {
    double* base = ws + (size_t)r * work_doubles_per_row(nc_max);
    return Work{base, base + (size_t)kC * nc_max, base + (size_t)(kC + kState) * nc_max};
}

// A live row: at least one sample, no more than the launch was sized for
__device__ __forceinline__ bool row_live(const mg_sos_row& rw, int max_len) {
    return rw.len > 0 && rw.len <= max_len && rw.in_pos > -kFar && rw.in_pos < kFar && rw.out_pos > -kFar && rw.out_pos < kFar;
}

// REV: the reverse pass (sample i of the pass is sample len - 1 - i of the row, read from mid).  APPLY: start from the carried
// states and store; otherwise from zero, keeping the end states.  FINAL: the stores are the float32 output, otherwise mid.
// with_T: the last x block of every row computes T instead.
template <bool REV, bool APPLY, bool FINAL>
__global__ __launch_bounds__(kLanes) void sos_pass_kernel(const float* __restrict__ x, long long x_total,
                                                          const mg_sos_row* __restrict__ rows, const double* __restrict__ sos,
                                                          int n_rows, int max_len, int nc_max, double* __restrict__ ws,
                                                          float* __restrict__ out, long long out_total, int with_T) {
    __shared__ float in_s[REV ? 1 : kLanes * kPad];
    __shared__ float out_s[APPLY && FINAL ? kLanes * kPad : 1];
    const int lane = threadIdx.x;
    const int n_blk = with_T ? gridDim.x - 1 : gridDim.x;
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const mg_sos_row rw = rows[r];
        if (!row_live(rw, max_len)) continue;
        const int len = (int)rw.len, nc = (len + kC - 1) / kC;
        const Coef cf = load_coef(sos + (size_t)r * (kSec * 6));
        const Work w = work_of(ws, r, nc_max);

        if (with_T && (int)blockIdx.x == n_blk) {                          // column `lane` of T: kC zero-input steps from unit state
            if (lane < kState) {
                double s[kState];
#pragma unroll
                for (int k = 0; k < kState; ++k) s[k] = k == lane ? 1.0 : 0.0;
                for (int j = 0; j < kC; ++j) cascade_step(cf, s, 0.0);
#pragma unroll
                for (int k = 0; k < kState; ++k) w.T[k * kState + lane] = s[k];
            }
            continue;
        }

        for (int cb = blockIdx.x; cb * kLanes < nc; cb += n_blk) {
            const int c = cb * kLanes + lane;                               // this lane's chunk; its samples are i0 + [0, kC)
            const int i0 = c * kC, blk0 = cb * kLanes * kC;
            const int left = len - blk0;                                    // > 0
            const int n_sub = left < kC ? (left + kSub - 1) / kSub : kC / kSub;   // tiles in which the block's first chunk has samples
            double s[kState];
#pragma unroll
            for (int k = 0; k < kState; ++k) s[k] = APPLY && c < nc ? w.st[(size_t)k * nc_max + c] : 0.0;

            float pre_f[REV ? 1 : kSub];
            double pre_d[REV ? kSub : 1];
            // tile q of the block: element e = lc * kSub + j is sample blk0 + lc * kC + q * kSub + j (cooperative, coalesced);
            // mid[j][c] is this lane's own sample already
            auto fetch = [&](int q) {
                if constexpr (REV) {
#pragma unroll
                    for (int j = 0; j < kSub; ++j) {
                        const int jj = q * kSub + j;
                        pre_d[j] = i0 + jj < len ? w.mid[(size_t)jj * nc_max + c] : 0.0;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < kSub; ++i) {
                        const int e = i * kLanes + lane, lc = e / kSub, j = e % kSub;
                        const int idx = blk0 + lc * kC + q * kSub + j;
                        const long long p = rw.in_pos + idx;
                        pre_f[i] = idx < len && p >= 0 && p < x_total ? x[p] : 0.0f;
                    }
                }
            };
            fetch(0);
            for (int q = 0; q < n_sub; ++q) {
                double xin[kSub];
                if constexpr (REV) {
#pragma unroll
                    for (int j = 0; j < kSub; ++j) xin[j] = pre_d[j];
                } else {
#pragma unroll
                    for (int i = 0; i < kSub; ++i) {
                        const int e = i * kLanes + lane;
                        in_s[(e / kSub) * kPad + e % kSub] = pre_f[i];
                    }
                    __syncthreads();
#pragma unroll
                    for (int j = 0; j < kSub; ++j) xin[j] = (double)in_s[lane * kPad + j];
                }
                if (q + 1 < n_sub) fetch(q + 1);
#pragma unroll
                for (int j = 0; j < kSub; ++j) {
                    const double y = cascade_step(cf, s, xin[j]);
                    if constexpr (APPLY && FINAL) out_s[lane * kPad + j] = (float)y;
                    if constexpr (APPLY && !FINAL) {
                        const int idx = i0 + q * kSub + j;
                        if (idx < len) {
                            const int rr = len - 1 - idx;                   // where the reverse pass reads this sample
                            w.mid[(size_t)(rr % kC) * nc_max + rr / kC] = y;
                        }
                    }
                }
                if constexpr (APPLY && FINAL) {
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < kSub; ++i) {
                        const int e = i * kLanes + lane, lc = e / kSub, j = e % kSub;
                        const int idx = blk0 + lc * kC + q * kSub + j;
                        if (idx < len) {
                            const long long p = rw.out_pos + (REV ? len - 1 - idx : idx);
                            if (p >= 0 && p < out_total) out[p] = out_s[lc * kPad + j];
                        }
                    }
                }
                __syncthreads();                                            // in_s / out_s are rewritten by the next tile
            }
            if (!APPLY && c < nc) {
#pragma unroll
                for (int k = 0; k < kState; ++k) w.st[(size_t)k * nc_max + c] = s[k];
            }
        }
    }
}

// v of lane `src` (a constant), read from its registers
__device__ __forceinline__ double lane_value(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// st[.][c]: the end state of chunk c from a zero state -> its true start state; one wave per row, lane i < 12 owns state i
__global__ __launch_bounds__(kLanes) void sos_carry_kernel(const mg_sos_row* __restrict__ rows, int n_rows, int max_len,
                                                           int nc_max, double* __restrict__ ws) {
    __shared__ double e_s[kState][kCarry + 1];                              // (odd stride: the 12 lanes sit on 12 banks)
    const int lane = threadIdx.x, i = lane < kState ? lane : 0;
    for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const mg_sos_row rw = rows[r];
        if (!row_live(rw, max_len)) continue;
        const int nc = ((int)rw.len + kC - 1) / kC;
        const Work w = work_of(ws, r, nc_max);
        double Trow[kState];
#pragma unroll
        for (int j = 0; j < kState; ++j) Trow[j] = lane < kState ? w.T[i * kState + j] : 0.0;
        double s = 0.0;
        for (int c0 = 0; c0 < nc; c0 += kCarry) {
            const int nb = nc - c0 < kCarry ? nc - c0 : kCarry;
            for (int e = lane; e < kState * kCarry; e += kLanes) {
                const int k = e / kCarry, cc = e % kCarry;
                if (cc < nb) e_s[k][cc] = w.st[(size_t)k * nc_max + c0 + cc];
            }
            __syncthreads();
            for (int cc = 0; cc < nb; ++cc) {
                const double e_i = e_s[i][cc];
                if (lane < kState) e_s[i][cc] = s;
                double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int j = 0; j < kState; ++j) acc[j & 3] = fma(Trow[j], lane_value(s, j), acc[j & 3]);
                s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + e_i;
            }
            __syncthreads();
            for (int e = lane; e < kState * kCarry; e += kLanes) {
                const int k = e / kCarry, cc = e % kCarry;
                if (cc < nb) w.st[(size_t)k * nc_max + c0 + cc] = e_s[k][cc];
            }
            __syncthreads();
        }
    }
}

inline long long chunks_of(long long max_len) { return (max_len + kC - 1) / kC; }

}  // namespace

extern "C" {

// See include/mdctgan_hip.h.
size_t mg_sos_rows_workspace(int n_rows, long long max_len) {
    if (n_rows <= 0 || max_len <= 0 || max_len > kMaxLen) return 0;
    const size_t per_row = work_doubles_per_row(chunks_of(max_len)) * sizeof(double);
    if (per_row > SIZE_MAX / (size_t)n_rows) return 0;
    return per_row * (size_t)n_rows;
}

int mg_sos_rows(const float* x, long long x_total, const mg_sos_row* rows, const double* sos, int n_rows, long long max_len,
                int zero_phase, float* out, long long out_total, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !rows || !sos || !out || !workspace || n_rows <= 0 || x_total <= 0 || out_total <= 0) return MG_ERR_ARG;
    const size_t need = mg_sos_rows_workspace(n_rows, max_len);
    if (need == 0 || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7)) return MG_ERR_ARG;
    if (x < out + out_total && out < x + x_total) return MG_ERR_ARG;       // the reverse pass would read what it has overwritten
    hipStream_t st = (hipStream_t)stream;
    const int nc_max = (int)chunks_of(max_len), L = (int)max_len;
    double* ws = (double*)workspace;
    const unsigned gy = (unsigned)(n_rows < 65535 ? n_rows : 65535);
    const int bx = (nc_max + kLanes - 1) / kLanes;
    const unsigned gx = (unsigned)(bx < 4096 ? bx : 4096);
    const dim3 block(kLanes);
#define MG_SOS_PASS(REV, APPLY, FINAL, GX, WITH_T)                                                                                \
    hipLaunchKernelGGL((sos_pass_kernel<REV, APPLY, FINAL>), dim3(GX, gy), block, 0, st, x, x_total, rows, sos, n_rows, L, nc_max, \
                       ws, out, out_total, WITH_T)
    MG_SOS_PASS(false, false, false, gx + 1, 1);
    hipLaunchKernelGGL(sos_carry_kernel, dim3(gy), block, 0, st, rows, n_rows, L, nc_max, ws);
    if (zero_phase) {
        MG_SOS_PASS(false, true, false, gx, 0);
        MG_SOS_PASS(true, false, false, gx, 0);
        hipLaunchKernelGGL(sos_carry_kernel, dim3(gy), block, 0, st, rows, n_rows, L, nc_max, ws);
        MG_SOS_PASS(true, true, true, gx, 0);
    } else {
        MG_SOS_PASS(false, true, true, gx, 0);
    }
#undef MG_SOS_PASS
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // extern "C"
