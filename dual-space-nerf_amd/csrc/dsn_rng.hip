// dsn_rng.hip - the training step's random draws on the device (dsn_train_draws; the rule is in include/dsnerf.h): the stratified
// jitter and the density noise of R rays x S samples from Philox4x32-10, addressed by (seed, step, ray id, quad of samples, kind).
// A thread owns one (ray, quad): up to two generator calls, four jitter values by integer shifts, four noise values by a float64
// Box-Muller rounded to float32 once.  The kernel is bound by its stores (8 bytes per (ray, sample) with both arrays): consecutive
// threads own consecutive quads of a ray, so a wave's 16-byte stores cover 1 KB of consecutive addresses.  One writer per word, no
// atomics, no LDS, no workspace.  The integer part is plain C++; -ffp-contract=off keeps the float64 part one rounding per operation.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include "dsn_philox.h"
#include <cmath>

#define DRAW_THREADS 256
#define DRAW_KIND_JITTER 0u
#define DRAW_KIND_NOISE 1u

// one word pair -> two normal deviates, float64 throughout, each rounded to float32 once
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const double u1 = ((double)a + 1.0) * 0x1p-32;       // (0, 1], exact
    const double u2 = (double)b * 0x1p-32;               // [0, 1), exact
    const double r = sqrt(-2.0 * log(u1));
    const double t = 6.283185307179586 * u2;
    z0 = (float)(r * cos(t));
    z1 = (float)(r * sin(t));
}

// VEC (S % 4 == 0 and a 16-byte aligned base: n == 4 and `at` is a multiple of 4 floats) is a template argument: as a run-time branch
// the compiler merges the two paths' last words into a 12-byte and a 4-byte store
template <bool VEC>
__device__ __forceinline__ void store_quad(float* out, int64_t at, const float* v, int n) {
    if (VEC) {
        *reinterpret_cast<float4*>(out + at) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < n) out[at + j] = v[j];
}

template <bool VEC_J, bool VEC_N>
__global__ void __launch_bounds__(DRAW_THREADS) k_train_draws(uint32_t k0, uint32_t k1, uint32_t step, uint32_t ray_base,
                                                               const int32_t* __restrict__ ray_ids, int R, int S, int nq, float noise_std,
                                                               float* __restrict__ jitter, float* __restrict__ noise) {
    const int64_t t = (int64_t)blockIdx.x * DRAW_THREADS + threadIdx.x;
    if (t >= (int64_t)R * nq) return;
    const int r = (int)(t / nq);
    const int q = (int)(t - (int64_t)r * nq);
    const uint32_t id = ray_ids ? (uint32_t)ray_ids[r] : ray_base + (uint32_t)r;
    const int s0 = 4 * q;
    const int n = S - s0 < 4 ? S - s0 : 4;               // the words past S are dropped
    const int64_t at = (int64_t)r * S + s0;
    float v[4];
    if (jitter) {
        const DsnPhiloxOut w = dsn_philox4x32_10((uint32_t)q, id, step, DRAW_KIND_JITTER, k0, k1);
        for (int j = 0; j < 4; ++j) v[j] = (float)(w.x[j] >> 8) * 0x1p-24f;      // 24 bits: exact in float32
        store_quad<VEC_J>(jitter, at, v, n);
    }
    if (noise) {
        const DsnPhiloxOut w = dsn_philox4x32_10((uint32_t)q, id, step, DRAW_KIND_NOISE, k0, k1);
        box_muller(w.x[0], w.x[1], v[0], v[1]);
        box_muller(w.x[2], w.x[3], v[2], v[3]);
        for (int j = 0; j < 4; ++j) v[j] = v[j] * noise_std;
        store_quad<VEC_N>(noise, at, v, n);
    }
}

// R, S > 0 and R * S <= INT_MAX (the entry point checks): at most 2^23 workgroups
void dsn_launch_train_draws(uint64_t seed, uint32_t step, uint32_t ray_base, const int32_t* ray_ids, int R, int S, float noise_std,
                            float* jitter, float* noise, hipStream_t st) {
    const int nq = (S + 3) / 4;
    const int64_t threads = (int64_t)R * nq;
    const bool whole = S % 4 == 0;
    const bool vec_j = whole && ((uintptr_t)jitter & 15) == 0, vec_n = whole && ((uintptr_t)noise & 15) == 0;
    auto k = vec_j ? (vec_n ? k_train_draws<true, true> : k_train_draws<true, false>)
                   : (vec_n ? k_train_draws<false, true> : k_train_draws<false, false>);
    hipLaunchKernelGGL(k, dim3((unsigned)((threads + DRAW_THREADS - 1) / DRAW_THREADS)), dim3(DRAW_THREADS), 0, st, (uint32_t)seed,
                       (uint32_t)(seed >> 32), step, ray_base, ray_ids, R, S, nq, noise_std, jitter, noise);
}
