// K11: LSGAN / BCE / L1 loss reductions and their gradients, over a LIST of tensors in one launch per stage (the feature-matching
// loss sums an L1 term per discriminator layer: 8-12 tensors -> 3 launches instead of 3 per tensor).  A single tensor is a list of
// one.  Stage 1 block partials (double), stage 2 fixed-order sum -> deterministic.
//
// Replaces (reference): MSELoss / BCELoss / L1Loss networks.py:106-109, :127-137, pix2pixHD_model.py:443-451.
#include "common.h"
#include "mdctgan_hip.h"

namespace {

enum { LOSS_MSE_CONST = 0, LOSS_L1 = 1, LOSS_BCE_CONST = 2 };      // `kind` of mg_loss_multi_*, KIND of the kernels

// Every tensor has min(ceil(n / 1024), 1024) partial blocks and its own grid stride whatever else is in the list, and the terms are
// added in list order, so a list gives the bits of its tensors' one-item calls accumulated in place.
struct LossList {
    const float* a[MG_LOSS_MAX_ITEMS];
    const float* b[MG_LOSS_MAX_ITEMS];
    float* grad[MG_LOSS_MAX_ITEMS];
    unsigned long long n[MG_LOSS_MAX_ITEMS];
    unsigned long long zero_tail[MG_LOSS_MAX_ITEMS];   // backward: elements after grad[i][n) to clear (the stacked batch's other half)
    unsigned first_block[MG_LOSS_MAX_ITEMS + 1];       // forward: partial blocks of item i are [first_block[i], first_block[i + 1])
    float coef[MG_LOSS_MAX_ITEMS];                     // backward: scale / n, divided on the host
    int count;
};
template <int KIND>
__global__ __launch_bounds__(256) void loss_partial_multi_kernel(LossList L, float target, double* __restrict__ part) {
    __shared__ double red[4];
    int it = 0;
    while (it + 1 < L.count && blockIdx.x >= L.first_block[it + 1]) ++it;
    const unsigned blk = blockIdx.x - L.first_block[it], nblk = L.first_block[it + 1] - L.first_block[it];
    const float* __restrict__ a = L.a[it];
    const float* __restrict__ b = L.b[it];
    const size_t n = (size_t)L.n[it];
    double s = 0.0;
    for (size_t i = (size_t)blk * blockDim.x + threadIdx.x; i < n; i += (size_t)nblk * blockDim.x) {
        if (KIND == 2) {      // nn.BCELoss against a constant label: log terms clamped at -100 like torch's
            const float pv = a[i];
            s += (double)((target - 1.0f) * fmaxf(logf(1.0f - pv), -100.0f) - target * fmaxf(logf(pv), -100.0f));
            continue;
        }
        const float d = a[i] - (KIND == 0 ? target : b[i]);
        s += (KIND == 0) ? (double)d * (double)d : (double)fabsf(d);
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// one wave per item (a fixed lane-strided order, then a fixed butterfly: deterministic), then thread 0 adds the terms in list order
__global__ __launch_bounds__(64 * MG_LOSS_MAX_ITEMS) void loss_final_multi_kernel(LossList L, const double* __restrict__ part,
                                                                                  float scale, float* __restrict__ loss,
                                                                                  int accumulate) {
    __shared__ float term[MG_LOSS_MAX_ITEMS];
    const int it = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (it < L.count) {
        const int nb = (int)(L.first_block[it + 1] - L.first_block[it]);
        const double* p = part + L.first_block[it];
        double s = 0.0;
        for (int i = lane; i < nb; i += 64) s += p[i];
        s = wave_sum_d(s);
        if (lane == 0) term[it] = (float)(s * (1.0 / (double)L.n[it])) * scale;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = accumulate ? loss[0] : 0.0f;
        for (int i = 0; i < L.count; ++i) acc = (i == 0 && !accumulate) ? term[0] : acc + term[i];
        loss[0] = acc;
    }
}
template <int KIND>
__global__ void loss_grad_multi_kernel(LossList L, float target, const float* __restrict__ go) {
    const int it = blockIdx.y;
    const float* __restrict__ a = L.a[it];
    const float* __restrict__ b = L.b[it];
    float* __restrict__ grad = L.grad[it];
    const size_t n = (size_t)L.n[it], nz = (size_t)L.zero_tail[it];
    const float gsc = L.coef[it] * (go ? go[0] : 1.0f);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n + nz; i += (size_t)gridDim.x * blockDim.x) {
        if (i >= n) { grad[i] = 0.0f; continue; }
        if (KIND == 2) {      // binary_cross_entropy_backward: (p - t) / max((1 - p) p, 1e-12)
            const float pv = a[i];
            grad[i] = (pv - target) / fmaxf((1.0f - pv) * pv, 1e-12f) * gsc;
            continue;
        }
        const float d = a[i] - (KIND == 0 ? target : b[i]);
        if (KIND == 0) grad[i] = 2.0f * d * gsc;
        else grad[i] = (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f)) * gsc;
    }
}

// the host side of both stages, for every entry point below
bool loss_list(const mg_loss_item* items, int count, bool need_b, bool need_grad, LossList* L) {
    if (!items || count < 1 || count > MG_LOSS_MAX_ITEMS) return false;
    L->count = count;
    unsigned fb = 0;
    for (int i = 0; i < count; ++i) {
        if (!items[i].a || items[i].n <= 0 || (need_b && !items[i].b) || (need_grad && !items[i].grad) || items[i].zero_tail < 0)
            return false;
        L->a[i] = items[i].a; L->b[i] = items[i].b; L->grad[i] = items[i].grad;
        L->n[i] = (unsigned long long)items[i].n; L->zero_tail[i] = (unsigned long long)items[i].zero_tail;
        L->first_block[i] = fb;
        size_t nb = ((size_t)items[i].n + 1023) / 1024;
        if (nb > 1024) nb = 1024;
        fb += (unsigned)nb;
    }
    L->first_block[count] = fb;
    return true;
}
// workspace: 1024 doubles per item (the callers check its size: they state it differently)
int loss_fwd(int kind, const mg_loss_item* items, int count, float target, float scale, float* loss, int accumulate,
             void* workspace, void* stream) {
    LossList L;
    if (kind < 0 || kind > 2 || !loss || !workspace) return MG_ERR_ARG;
    if (!loss_list(items, count, kind == 1, false, &L)) return MG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(L.first_block[count]);
    double* part = (double*)workspace;
    if (kind == 0) hipLaunchKernelGGL(loss_partial_multi_kernel<0>, grid, dim3(256), 0, st, L, target, part);
    else if (kind == 1) hipLaunchKernelGGL(loss_partial_multi_kernel<1>, grid, dim3(256), 0, st, L, target, part);
    else hipLaunchKernelGGL(loss_partial_multi_kernel<2>, grid, dim3(256), 0, st, L, target, part);
    hipLaunchKernelGGL(loss_final_multi_kernel, dim3(1), dim3(64 * MG_LOSS_MAX_ITEMS), 0, st, L, (const double*)part, scale, loss,
                       accumulate);
    MG_CHECK_LAUNCH();
    return MG_OK;
}
// grad_out == nullptr: a factor of 1
int loss_bwd(int kind, const mg_loss_item* items, int count, float target, float scale, const float* grad_out, void* stream) {
    LossList L;
    if (kind < 0 || kind > 2) return MG_ERR_ARG;
    if (!loss_list(items, count, kind == 1, true, &L)) return MG_ERR_ARG;
    size_t nmax = 0;
    for (int i = 0; i < count; ++i) {
        const size_t ni = (size_t)(items[i].n + items[i].zero_tail);
        if (ni > nmax) nmax = ni;
        L.coef[i] = scale / (float)items[i].n;
    }
    const dim3 grid(grid_for(nmax), count);
    hipStream_t st = (hipStream_t)stream;
    if (kind == 0) hipLaunchKernelGGL(loss_grad_multi_kernel<0>, grid, dim3(256), 0, st, L, target, grad_out);
    else if (kind == 1) hipLaunchKernelGGL(loss_grad_multi_kernel<1>, grid, dim3(256), 0, st, L, target, grad_out);
    else hipLaunchKernelGGL(loss_grad_multi_kernel<2>, grid, dim3(256), 0, st, L, target, grad_out);
    MG_CHECK_LAUNCH();
    return MG_OK;
}

}  // namespace

extern "C" {

// The single-tensor entry points: a list of one (at most 1024 partials, so mg_loss_workspace() bytes are enough for it)
size_t mg_loss_workspace(void) { return 1024 * sizeof(double); }

int mg_mse_const_fwd(const float* pred, long long n, float target, float scale, float* loss, int accumulate,
                     void* workspace, void* stream) {
    const mg_loss_item one{pred, nullptr, nullptr, n, 0};
    return loss_fwd(LOSS_MSE_CONST, &one, 1, target, scale, loss, accumulate, workspace, stream);
}
int mg_mse_const_bwd(const float* pred, long long n, float target, float scale, const float* grad_out, float* grad,
                     void* stream) {
    const mg_loss_item one{pred, nullptr, grad, n, 0};
    return loss_bwd(LOSS_MSE_CONST, &one, 1, target, scale, grad_out, stream);
}
int mg_bce_const_fwd(const float* pred, long long n, float target, float scale, float* loss, int accumulate,
                     void* workspace, void* stream) {
    const mg_loss_item one{pred, nullptr, nullptr, n, 0};
    return loss_fwd(LOSS_BCE_CONST, &one, 1, target, scale, loss, accumulate, workspace, stream);
}
int mg_bce_const_bwd(const float* pred, long long n, float target, float scale, const float* grad_out, float* grad,
                     void* stream) {
    const mg_loss_item one{pred, nullptr, grad, n, 0};
    return loss_bwd(LOSS_BCE_CONST, &one, 1, target, scale, grad_out, stream);
}
int mg_l1_fwd(const float* a, const float* b, long long n, float scale, float* loss, int accumulate, void* workspace,
              void* stream) {
    const mg_loss_item one{a, b, nullptr, n, 0};
    return loss_fwd(LOSS_L1, &one, 1, 0.0f, scale, loss, accumulate, workspace, stream);
}
int mg_l1_bwd(const float* a, const float* b, long long n, float scale, const float* grad_out, float* grad_a,
              void* stream) {
    const mg_loss_item one{a, b, grad_a, n, 0};
    return loss_bwd(LOSS_L1, &one, 1, 0.0f, scale, grad_out, stream);
}

size_t mg_loss_multi_workspace(void) { return (size_t)MG_LOSS_MAX_ITEMS * 1024 * sizeof(double); }

int mg_loss_multi_fwd(int kind, const mg_loss_item* items, int count, float target, float scale, float* loss, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (workspace_bytes < mg_loss_multi_workspace()) return MG_ERR_ARG;
    return loss_fwd(kind, items, count, target, scale, loss, accumulate, workspace, stream);
}
int mg_loss_multi_bwd(int kind, const mg_loss_item* items, int count, float target, float scale, const float* grad_out,
                      void* stream) {
    return loss_bwd(kind, items, count, target, scale, grad_out, stream);
}

}  // extern "C"
