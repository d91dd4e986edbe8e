// dsn_optim.hip - the optimizer step on the device (dsn_adam_step; the rule is in include/dsnerf.h): torch.optim.Adam's
// _single_tensor_adam over every tensor of the call in ONE launch.  The tensors travel as a table of segments in the kernel
// arguments (as DsnParamPtrs does for the packer): a workgroup owns DSN_ADAM_BLOCK consecutive elements of one segment and finds
// the segment by its index in the table's prefix of workgroup counts.  Elementwise: one writer per word, no atomics, no LDS, no
// matrix instructions.  float32 with one rounding per operation (-ffp-contract=off, `/` and sqrtf correctly rounded): a numpy
// restatement reproduces every bit.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include <cmath>

#define ADAM_THREADS 256
#define ADAM_PER_THREAD 4
#define ADAM_MAX_BLOCKS ((1u << 24) - 1)      // workgroups per launch: x 256 threads < 2^32

static_assert(ADAM_THREADS * ADAM_PER_THREAD == DSN_ADAM_BLOCK, "a thread owns four consecutive elements: one 16-byte access per array");

struct DsnAdamSeg {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    float ss, c2, wd;      // lr / (1 - beta1^t), sqrt(1 - beta2^t), weight decay: they differ between param groups
    uint32_t first;        // the segment's first workgroup
};
struct DsnAdamTable {
    DsnAdamSeg seg[DSN_ADAM_TABLE];
    float w1, w2, b2, eps;
    int nseg;
};
static_assert(sizeof(DsnAdamTable) <= 3072, "the table travels in the kernel arguments (4 KB)");
static_assert(DSN_ADAM_TABLE >= DSN_NUM_PARAMS_INTERNAL, "the model's tensors take one launch");
static_assert((DSN_ADAM_MAX_N + DSN_ADAM_BLOCK - 1) / DSN_ADAM_BLOCK <= ADAM_MAX_BLOCKS, "the longest tensor fits one launch");

struct DsnAdamConst { float w1, w2, b2, eps, ss, c2, wd; };

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const DsnAdamConst& c) {
    if (c.wd != 0.0f) g = g + c.wd * p;
    m = m + c.w1 * (g - m);
    v = c.b2 * v + c.w2 * (g * g);
    p = p - c.ss * dsn_div(m, dsn_div(sqrtf(v), c.c2) + c.eps);
}

__global__ void __launch_bounds__(ADAM_THREADS) k_adam_step(const DsnAdamTable T) {
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = T.nseg - 1;           // the last segment whose first workgroup is <= b (uniform: scalar loads of the arguments)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (T.seg[mid].first <= b) lo = mid; else hi = mid - 1;
    }
    float* const p = T.seg[lo].p;
    const float* const g = T.seg[lo].g;
    float* const m = T.seg[lo].m;
    float* const v = T.seg[lo].v;
    const int64_t n = T.seg[lo].n;
    const DsnAdamConst c = {T.w1, T.w2, T.b2, T.eps, T.seg[lo].ss, T.seg[lo].c2, T.seg[lo].wd};
    const int64_t i0 = (int64_t)(b - T.seg[lo].first) * DSN_ADAM_BLOCK + ADAM_PER_THREAD * (int64_t)threadIdx.x;
    if (i0 >= n) return;
    const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    if (aligned && i0 + ADAM_PER_THREAD <= n) {
        float4 p4 = *reinterpret_cast<const float4*>(p + i0);
        const float4 g4 = *reinterpret_cast<const float4*>(g + i0);
        float4 m4 = *reinterpret_cast<const float4*>(m + i0);
        float4 v4 = *reinterpret_cast<const float4*>(v + i0);
        adam_element(p4.x, g4.x, m4.x, v4.x, c);
        adam_element(p4.y, g4.y, m4.y, v4.y, c);
        adam_element(p4.z, g4.z, m4.z, v4.z, c);
        adam_element(p4.w, g4.w, m4.w, v4.w, c);
        *reinterpret_cast<float4*>(m + i0) = m4;
        *reinterpret_cast<float4*>(v + i0) = v4;
        *reinterpret_cast<float4*>(p + i0) = p4;
        return;
    }
    // the segment's tail, and every element of a segment with a pointer off the 16-byte grid (a view into a larger buffer)
    for (int j = 0; j < ADAM_PER_THREAD; ++j) {
        const int64_t i = i0 + j;
        if (i >= n) break;
        float pe = p[i], me = m[i], ve = v[i];
        adam_element(pe, g[i], me, ve, c);
        m[i] = me;
        v[i] = ve;
        p[i] = pe;
    }
}

void dsn_adam_scalars(double lr, double weight_decay, double beta1, double beta2, double eps, double t, float* out7) {
    out7[0] = (float)(1.0 - beta1);
    out7[1] = (float)(1.0 - beta2);
    out7[2] = (float)beta2;
    out7[3] = (float)eps;
    out7[4] = (float)weight_decay;
    out7[5] = (float)(lr / (1.0 - std::pow(beta1, t)));
    out7[6] = (float)std::sqrt(1.0 - std::pow(beta2, t));
}

// Tensors without a gradient or without elements take no segment.  A launch ends when the table is full or its workgroups would pass
// ADAM_MAX_BLOCKS (grid x block threads stays below 2^32, the runtime's limit; one tensor of DSN_ADAM_MAX_N elements fits): the next
// one starts behind it on the same stream.  Returns the number of launches.
int dsn_launch_adam_step(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                         const int64_t* n, int count, const double* lr, const double* weight_decay, double beta1, double beta2, double eps,
                         double t, hipStream_t st) {
    DsnAdamTable T = {};
    float s[7];
    dsn_adam_scalars(0.0, 0.0, beta1, beta2, eps, t, s);
    T.w1 = s[0]; T.w2 = s[1]; T.b2 = s[2]; T.eps = s[3];
    T.nseg = 0;
    uint32_t blocks = 0;
    int launches = 0;
    const uint32_t max_blocks = ADAM_MAX_BLOCKS;
    for (int i = 0; i <= count; ++i) {
        uint32_t need = 0;
        if (i < count) {
            if (!grads[i] || n[i] <= 0) continue;
            need = (uint32_t)((n[i] + DSN_ADAM_BLOCK - 1) / DSN_ADAM_BLOCK);      // (n <= 2^33: at most 2^23)
        }
        if (T.nseg > 0 && (i == count || T.nseg == DSN_ADAM_TABLE || blocks + need > max_blocks)) {
            hipLaunchKernelGGL(k_adam_step, dim3(blocks), dim3(ADAM_THREADS), 0, st, T);
            ++launches;
            T.nseg = 0;
            blocks = 0;
        }
        if (i == count) break;
        dsn_adam_scalars(lr[i], weight_decay[i], beta1, beta2, eps, t, s);
        DsnAdamSeg& g = T.seg[T.nseg++];
        g.p = params[i]; g.g = grads[i]; g.m = exp_avgs[i]; g.v = exp_avg_sqs[i];
        g.n = n[i];
        g.wd = s[4]; g.ss = s[5]; g.c2 = s[6];
        g.first = blocks;
        blocks += need;
    }
    return launches;
}
