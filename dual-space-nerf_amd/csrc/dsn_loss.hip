// dsn_loss.hip - the trainer's loss on the device (dsn_train_loss / dsn_train_loss_grad; the rule is in include/dsnerf.h):
// utils/loss.py's MSELoss / SmoothL1Loss with the optional LOSSwMask term, its in-place acc_map[occupancy == 1] = 1, and the
// mse / psnr the trainer takes of the same batch, in one pass over the rays; the two seed arrays of the backward in another.
// Forward: workgroup b owns rays [b DSN_LOSS_SHARE, (b + 1) DSN_LOSS_SHARE) - a function of R alone - and leaves three fp64
// partials {sum term, sum d d, sum |a' - occ|} in the workspace; k_loss_final (one workgroup) adds the partials in index order
// and writes out4.  Every partial has one writer and every sum a fixed order: the same bits on every call, whatever the
// workspace held.  No atomics, no matrix instructions.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"

#define LOSS_THREADS DSN_LOSS_SHARE      // one thread per ray of the share; three colour elements per thread

static_assert(LOSS_THREADS == 256, "the block sums below assume four waves");

// the sum over the workgroup in a fixed order: butterfly within each wave, then the waves in index order (every thread returns it)
__device__ __forceinline__ double loss_block_sum(double v, double* s) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    const int wave = threadIdx.x >> 6;
    __syncthreads();                      // (s is reused by the next sum)
    if ((threadIdx.x & 63) == 0) s[wave] = v;
    __syncthreads();
    return ((s[0] + s[1]) + s[2]) + s[3];
}

__device__ __forceinline__ double loss_target(const float* t32, const double* t64, int64_t i) {
    return t64 ? t64[i] : (double)t32[i];
}

__device__ __forceinline__ double loss_occ(const uint8_t* o8, const float* o32, int64_t r) {
    return o8 ? (double)o8[r] : (double)o32[r];
}

__global__ void __launch_bounds__(LOSS_THREADS) k_loss_partial(const float* __restrict__ color, const float* __restrict__ t32,
                                                               const double* __restrict__ t64, float* acc,
                                                               const uint8_t* __restrict__ o8, const float* __restrict__ o32,
                                                               int64_t R, int kind, int overwrite, double* __restrict__ part) {
    __shared__ double s[4];
    const int64_t r0 = (int64_t)blockIdx.x * DSN_LOSS_SHARE;
    const int64_t e0 = 3 * r0, n = 3 * R;
    double term = 0.0, sq = 0.0, mask = 0.0;
    for (int k = 0; k < 3; ++k) {          // elements e0 + t, e0 + 256 + t, e0 + 512 + t of the share: whole-wave contiguous loads
        const int64_t i = e0 + (int64_t)k * LOSS_THREADS + threadIdx.x;
        if (i < n) {
            const double d = (double)color[i] - loss_target(t32, t64, i);
            const double dd = d * d;
            sq += dd;
            if (kind == DSN_LOSS_L2) term += dd;
            else { const double a = fabs(d); term += a < 1.0 ? 0.5 * dd : a - 0.5; }      // NaN: a < 1 is false, a - 0.5 is NaN
        }
    }
    const int64_t r = r0 + threadIdx.x;
    if ((o8 || o32) && r < R) {
        const double occ = loss_occ(o8, o32, r);
        if (occ == 1.0) {
            if (overwrite) acc[r] = 1.0f;
            // (a' = 1 = occ: the ray adds exactly 0)
        } else {
            mask = fabs((double)acc[r] - occ);
        }
    }
    term = loss_block_sum(term, s);
    sq = loss_block_sum(sq, s);
    mask = loss_block_sum(mask, s);
    if (threadIdx.x == 0) {
        part[3 * (size_t)blockIdx.x + 0] = term;
        part[3 * (size_t)blockIdx.x + 1] = sq;
        part[3 * (size_t)blockIdx.x + 2] = mask;
    }
}

// out4 = {loss_rgb, loss_mask, mse, psnr}: thread t adds partials t, t + 256, ... in index order, then the fixed block sum
__global__ void __launch_bounds__(LOSS_THREADS) k_loss_final(const double* __restrict__ part, int64_t nblocks, int64_t R, int mask_on,
                                                             double* __restrict__ out4) {
    __shared__ double s[4];
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t b = threadIdx.x; b < nblocks; b += LOSS_THREADS)
        for (int k = 0; k < 3; ++k) v[k] += part[3 * b + k];
    for (int k = 0; k < 3; ++k) v[k] = loss_block_sum(v[k], s);
    if (threadIdx.x == 0) {
        const double n = 3.0 * (double)R;              // R = 0: 0 / 0, NaN in every mean, as torch's mean of nothing
        const double mse = v[1] / n;
        out4[0] = v[0] / n;
        out4[1] = mask_on ? 0.1 * (v[2] / (double)R) : 0.0;
        out4[2] = mse;
        out4[3] = -10.0 * log10(mse);                  // +inf at mse = 0
    }
}

// one thread per colour element; thread r < R also writes g_acc[r]
__global__ void __launch_bounds__(LOSS_THREADS) k_loss_grad(const float* __restrict__ color, const float* __restrict__ t32,
                                                            const double* __restrict__ t64, const float* __restrict__ acc,
                                                            const uint8_t* __restrict__ o8, const float* __restrict__ o32, int64_t R,
                                                            int kind, const float* __restrict__ up_rgb, const float* __restrict__ up_mask,
                                                            double s, double m, float* __restrict__ g_color, float* __restrict__ g_acc) {
    const int64_t i = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (i >= 3 * R) return;
    const double d = (double)color[i] - loss_target(t32, t64, i);
    double e;
    if (kind == DSN_LOSS_L2) e = 2.0 * d;
    else e = fabs(d) < 1.0 ? d : (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d));       // NaN stays NaN
    const double us = (double)(up_rgb ? *up_rgb : 0.0f) * s;
    g_color[i] = (float)(us * e);
    if (g_acc && i < R) {
        float g = 0.0f;
        if (o8 || o32) {
            const double occ = loss_occ(o8, o32, i);
            if (!(occ == 1.0)) {
                const double x = (double)acc[i] - occ;
                const double sign = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x));      // sign(0) = +0, NaN stays NaN
                g = (float)(((double)(up_mask ? *up_mask : 0.0f) * m) * sign);
            }
        }
        g_acc[i] = g;
    }
}

static int64_t loss_blocks(int64_t R) { return (R + DSN_LOSS_SHARE - 1) / DSN_LOSS_SHARE; }

size_t dsn_train_loss_workspace_size(int64_t R) { return dsn_align256(sizeof(double) * 3 * (size_t)loss_blocks(R)) + 256; }

void dsn_launch_train_loss(const float* color, const float* t32, const double* t64, float* acc, const uint8_t* o8, const float* o32,
                           int64_t R, int kind, int overwrite, double* out4, void* workspace, hipStream_t st) {
    const int64_t nb = loss_blocks(R);
    double* part = (double*)workspace;
    if (nb > 0)
        hipLaunchKernelGGL(k_loss_partial, dim3((unsigned)nb), dim3(LOSS_THREADS), 0, st, color, t32, t64, acc, o8, o32, R, kind, overwrite,
                           part);
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(LOSS_THREADS), 0, st, part, nb, R, (o8 || o32) ? 1 : 0, out4);
}

void dsn_launch_train_loss_grad(const float* color, const float* t32, const double* t64, const float* acc, const uint8_t* o8,
                                const float* o32, int64_t R, int kind, const float* up_rgb, const float* up_mask, float* g_color,
                                float* g_acc, hipStream_t st) {
    if (R <= 0) return;
    const double s = 1.0 / (3.0 * (double)R), m = 0.1 / (double)R;
    const int64_t nb = (3 * R + LOSS_THREADS - 1) / LOSS_THREADS;
    hipLaunchKernelGGL(k_loss_grad, dim3((unsigned)nb), dim3(LOSS_THREADS), 0, st, color, t32, t64, acc, o8, o32, R, kind, up_rgb, up_mask, s,
                       m, g_color, g_acc);
}
