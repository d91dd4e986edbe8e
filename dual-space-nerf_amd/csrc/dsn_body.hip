// dsn_body.hip - the SMPL forward pass for a whole clip (dsn_body_shape / dsn_body_pose, the rule of include/dsnerf.h; numpy
// restatement: tests/body_pose_restate.py).  The file is compiled with -ffp-contract=off like the rest of the library: every `a * b + c`
// below is two roundings, and every sum runs in ascending index order whatever the launch geometry.
//   k_body_chain    one wave per pose, float64: 25 lanes do the Rodrigues rotations (24 joints + Rh), 16 lanes walk the joints in index
//                   order (one lane per element of the 4 x 4 product), then A, Rh_mat and the 207 pose features are rounded to float32
//   k_body_verts    a workgroup owns 256 consecutive vertices (768 consecutive floats of the 3V axis: every posedirs row is read coalesced)
//                   and a block of 8 poses: their features sit in LDS as [k][pose] and are read as two 16-byte broadcasts per k, one
//                   accumulator per pose and float in registers - a posedirs element is loaded once per pose block.  The three coordinates
//                   of a vertex meet through LDS; blend, rigid part and Rh / Th run one thread per vertex with the block's joint
//                   transforms in LDS (broadcast reads).  Per-workgroup min / max keys for the bounds.
//   k_body_bounds   one wave per pose reduces the partial keys, pads, writes [2,3]
// No atomics; every output word has one writer.
#include "dsn_common.h"
#include "dsn_kernels.h"

#define BODY_J 24
#define BODY_PF 207
#define BODY_PB 8            // poses per block of k_body_verts
#define BODY_TV 256          // vertices per workgroup of k_body_verts (= its thread count)

struct DsnBodyParents { int p[BODY_J]; };

// ---- workspace: [P][208] pose features, [P][24][16] A, [P][12] Rh_mat, [P][tiles][8] partial bounds (6 keys, NaN mask, pad) --------------
__host__ __device__ inline int dsn_body_tiles(int V) { return (V + BODY_TV - 1) / BODY_TV; }
struct DsnBodyWs { float* pf; float* A; float* Rh; uint32_t* part; };
__host__ __device__ inline DsnBodyWs dsn_body_ws(void* base, int V, int P) {
    DsnBodyWs w;
    char* p = (char*)base;
    w.pf = (float*)p;      p += dsn_align256(sizeof(float) * 208 * (size_t)P);
    w.A = (float*)p;       p += dsn_align256(sizeof(float) * 384 * (size_t)P);
    w.Rh = (float*)p;      p += dsn_align256(sizeof(float) * 12 * (size_t)P);
    w.part = (uint32_t*)p;
    return w;
}
size_t dsn_body_pose_workspace_size(int V, int P) {
    return dsn_align256(sizeof(float) * 208 * (size_t)P) + dsn_align256(sizeof(float) * 384 * (size_t)P) +
           dsn_align256(sizeof(float) * 12 * (size_t)P) + dsn_align256(sizeof(uint32_t) * 8 * (size_t)P * (size_t)dsn_body_tiles(V));
}

// utils/h36m_utils.py:210-229 batch_rodrigues for one axis-angle vector, float64: R[9] row-major
__device__ __forceinline__ void body_rodrigues(const float* p32, double* R) {
    const double px = (double)p32[0], py = (double)p32[1], pz = (double)p32[2];
    const double qx = px + 1e-8, qy = py + 1e-8, qz = pz + 1e-8;
    const double angle = sqrt((qx * qx + qy * qy) + qz * qz);
    const double rx = px / angle, ry = py / angle, rz = pz / angle;
    const double c = cos(angle), s = sin(angle);
    const double K[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
    const double omc = 1.0 - c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double kk = (K[i * 3 + 0] * K[0 * 3 + j] + K[i * 3 + 1] * K[1 * 3 + j]) + K[i * 3 + 2] * K[2 * 3 + j];
            R[i * 3 + j] = ((i == j ? 1.0 : 0.0) + s * K[i * 3 + j]) + omc * kk;
        }
}

__global__ __launch_bounds__(64) void k_body_chain(const float* __restrict__ joints, DsnBodyParents par, const float* __restrict__ poses,
                                                   const float* __restrict__ Rh, int P, float* __restrict__ wsA, float* __restrict__ wsRh,
                                                   float* __restrict__ wsPf, float* __restrict__ outA, float* __restrict__ outRh) {
    __shared__ double sT[BODY_J][16];      // [R | rel joint; 0 0 0 1] per joint
    __shared__ double sG[BODY_J][16];      // the product down the parents
    __shared__ double sRh[9];
    __shared__ double sJ[BODY_J][3];
    const int p = blockIdx.x, l = threadIdx.x;
    if (p >= P) return;
    for (int i = l; i < BODY_J * 3; i += 64) sJ[i / 3][i % 3] = (double)joints[i];
    __syncthreads();
    if (l < BODY_J) {
        double R[9];
        body_rodrigues(poses + ((size_t)p * BODY_J + l) * 3, R);
        const int pa = l == 0 ? 0 : par.p[l];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) sT[l][r * 4 + c] = R[r * 3 + c];
            sT[l][r * 4 + 3] = l == 0 ? sJ[0][r] : sJ[l][r] - sJ[pa][r];
        }
        sT[l][12] = 0.0; sT[l][13] = 0.0; sT[l][14] = 0.0; sT[l][15] = 1.0;
    } else if (l == BODY_J) {
        double R[9];
        if (Rh) body_rodrigues(Rh + (size_t)p * 3, R);
        else for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        for (int i = 0; i < 9; ++i) sRh[i] = R[i];
    }
    __syncthreads();
    if (l < 16) sG[0][l] = sT[0][l];
    __syncthreads();
    for (int i = 1; i < BODY_J; ++i) {
        if (l < 16) {
            const int r = l >> 2, c = l & 3;
            const double* a = sG[par.p[i]];
            const double* b = sT[i];
            sG[i][l] = ((a[r * 4 + 0] * b[0 * 4 + c] + a[r * 4 + 1] * b[1 * 4 + c]) + a[r * 4 + 2] * b[2 * 4 + c]) + a[r * 4 + 3] * b[3 * 4 + c];
        }
        __syncthreads();
    }
    // A = G [I | -J]: column 3 minus the row's product with (J, 0)
    for (int i = l; i < BODY_J * 4; i += 64) {
        const int j = i >> 2, r = i & 3;
        const double* g = sG[j] + r * 4;
        const double rel = ((g[0] * sJ[j][0] + g[1] * sJ[j][1]) + g[2] * sJ[j][2]) + g[3] * 0.0;
        const float row[4] = {(float)g[0], (float)g[1], (float)g[2], (float)(g[3] - rel)};
        const size_t o = ((size_t)p * BODY_J + j) * 16 + r * 4;
        for (int c = 0; c < 4; ++c) wsA[o + c] = row[c];
        if (outA) for (int c = 0; c < 4; ++c) outA[o + c] = row[c];
    }
    for (int i = l; i < 208; i += 64) {
        float f = 0.0f;
        if (i < BODY_PF) { const int j = 1 + i / 9, e = i % 9; f = (float)(sT[j][(e / 3) * 4 + e % 3] - ((e % 4 == 0) ? 1.0 : 0.0)); }
        wsPf[(size_t)p * 208 + i] = f;
    }
    if (l < 12) {
        const float f = l < 9 ? (float)sRh[l] : 0.0f;
        wsRh[(size_t)p * 12 + l] = f;
        if (outRh && l < 9) outRh[(size_t)p * 9 + l] = f;
    }
}

// float bits -> an unsigned key with the order of the values and -0 < +0 (NaN is kept out by the caller)
__device__ __forceinline__ uint32_t body_key(float x) { const uint32_t b = __float_as_uint(x); return (b >> 31) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float body_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }

__global__ __launch_bounds__(BODY_TV) void k_body_verts(const float* __restrict__ v_shaped, const float* __restrict__ weights,
                                                        const float* __restrict__ posedirs, int V, int P, const float* __restrict__ wsPf,
                                                        const float* __restrict__ wsA, const float* __restrict__ wsRh,
                                                        const float* __restrict__ Th, float* __restrict__ xyz, float* __restrict__ xyz_smpl,
                                                        uint32_t* __restrict__ part, int want_bounds) {
    __shared__ __attribute__((aligned(16))) float sPf[BODY_PF * BODY_PB];       // [k][pose]
    __shared__ __attribute__((aligned(16))) float sA[BODY_PB][BODY_J * 12];      // rows 0-2 of every joint transform
    __shared__ float sRT[BODY_PB][12];                                           // Rh_mat, Th
    __shared__ float sV[BODY_PB][3 * BODY_TV];                                   // v_posed of the tile
    __shared__ uint32_t sRed[BODY_TV / 64][7];
    const int tid = threadIdx.x, tile = blockIdx.x, p0 = blockIdx.y * BODY_PB;
    const int np = min(BODY_PB, P - p0);
    const int n3 = 3 * V, f0 = tile * 3 * BODY_TV;
    for (int i = tid; i < BODY_PF * BODY_PB; i += BODY_TV) {
        const int k = i / BODY_PB, q = i % BODY_PB;
        sPf[i] = q < np ? wsPf[(size_t)(p0 + q) * 208 + k] : 0.0f;
    }
    for (int i = tid; i < BODY_PB * BODY_J * 12; i += BODY_TV) {
        const int q = i / (BODY_J * 12), e = i % (BODY_J * 12), j = e / 12, c = e % 12;
        sA[q][e] = q < np ? wsA[((size_t)(p0 + q) * BODY_J + j) * 16 + c] : 0.0f;
    }
    if (tid < BODY_PB * 12) {
        const int q = tid / 12, e = tid % 12;
        float f = 0.0f;
        if (q < np) f = e < 9 ? wsRh[(size_t)(p0 + q) * 12 + e] : (Th ? Th[(size_t)(p0 + q) * 3 + (e - 9)] : 0.0f);
        sRT[q][e] = f;
    }
    __syncthreads();
    // ---- v_posed = v_shaped + sum_k pf[k] posedirs[k]: three floats of the tile per thread, 256 apart
    {
        float acc[3][BODY_PB];
        int idx[3];
        bool ok[3];
        for (int e = 0; e < 3; ++e) {
            idx[e] = f0 + e * BODY_TV + tid;
            ok[e] = idx[e] < n3;
            for (int q = 0; q < BODY_PB; ++q) acc[e][q] = 0.0f;
        }
        if (posedirs) {
            const float4* pf4 = (const float4*)sPf;
#pragma unroll 3
            for (int k = 0; k < BODY_PF; ++k) {
                const float* row = posedirs + (size_t)k * n3;
                float d[3];
                for (int e = 0; e < 3; ++e) d[e] = ok[e] ? row[idx[e]] : 0.0f;
                const float4 a = pf4[k * 2], b = pf4[k * 2 + 1];
                const float f[BODY_PB] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                for (int e = 0; e < 3; ++e)
                    for (int q = 0; q < BODY_PB; ++q) acc[e][q] = acc[e][q] + f[q] * d[e];
            }
        }
        for (int e = 0; e < 3; ++e) {
            const float vs = ok[e] ? v_shaped[idx[e]] : 0.0f;
            for (int q = 0; q < BODY_PB; ++q) sV[q][e * BODY_TV + tid] = posedirs ? vs + acc[e][q] : vs;
        }
    }
    __syncthreads();
    // ---- blend, rigid part, Rh / Th: one thread per vertex
    const int v = tile * BODY_TV + tid;
    const bool live = v < V;
    float w[BODY_J];
    for (int j = 0; j < BODY_J; ++j) w[j] = live ? weights[(size_t)v * BODY_J + j] : 0.0f;
    for (int q = 0; q < np; ++q) {
        float T[12];
        for (int c = 0; c < 12; ++c) T[c] = 0.0f;
        const float4* A4 = (const float4*)sA[q];
        for (int j = 0; j < BODY_J; ++j) {
            const float4 r0 = A4[j * 3], r1 = A4[j * 3 + 1], r2 = A4[j * 3 + 2];
            const float a[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
            for (int c = 0; c < 12; ++c) T[c] = T[c] + w[j] * a[c];
        }
        const float vx = sV[q][3 * tid], vy = sV[q][3 * tid + 1], vz = sV[q][3 * tid + 2];
        float xs[3], xw[3];
        for (int r = 0; r < 3; ++r) xs[r] = ((T[r * 4] * vx + T[r * 4 + 1] * vy) + T[r * 4 + 2] * vz) + T[r * 4 + 3];
        const float* R = sRT[q];
        for (int r = 0; r < 3; ++r) xw[r] = ((R[r * 3] * xs[0] + R[r * 3 + 1] * xs[1]) + R[r * 3 + 2] * xs[2]) + R[9 + r];
        if (live) {
            const size_t o = ((size_t)(p0 + q) * V + v) * 3;
            for (int r = 0; r < 3; ++r) xyz[o + r] = xw[r];
            if (xyz_smpl) for (int r = 0; r < 3; ++r) xyz_smpl[o + r] = xs[r];
        }
        if (want_bounds) {      // (uniform: every thread of the workgroup takes part)
            uint32_t red[7];
            for (int r = 0; r < 3; ++r) {
                const bool use = live && !(xw[r] != xw[r]);
                const uint32_t k = use ? body_key(xw[r]) : 0u;
                red[r] = use ? k : 0xFFFFFFFFu;
                red[3 + r] = k;
            }
            red[6] = live ? ((xw[0] != xw[0]) ? 1u : 0u) | ((xw[1] != xw[1]) ? 2u : 0u) | ((xw[2] != xw[2]) ? 4u : 0u) : 0u;
            for (int o = 32; o >= 1; o >>= 1) {
                for (int r = 0; r < 3; ++r) {
                    red[r] = min(red[r], (uint32_t)__shfl_xor((int)red[r], o));
                    red[3 + r] = max(red[3 + r], (uint32_t)__shfl_xor((int)red[3 + r], o));
                }
                red[6] |= (uint32_t)__shfl_xor((int)red[6], o);
            }
            __syncthreads();      // (the previous pose's sRed has been read)
            if ((tid & 63) == 0) for (int r = 0; r < 7; ++r) sRed[tid >> 6][r] = red[r];
            __syncthreads();
            if (tid < 8) {
                uint32_t o = 0u;
                if (tid < 7) {
                    o = sRed[0][tid];
                    for (int wv = 1; wv < BODY_TV / 64; ++wv)
                        o = tid < 3 ? min(o, sRed[wv][tid]) : tid < 6 ? max(o, sRed[wv][tid]) : (o | sRed[wv][tid]);
                }
                part[((size_t)(p0 + q) * gridDim.x + tile) * 8 + tid] = o;
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_body_bounds(const uint32_t* __restrict__ part, int tiles, int P, int pad_mode, float* __restrict__ bounds) {
    const int p = blockIdx.x, l = threadIdx.x;
    if (p >= P) return;
    uint32_t red[7] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u};
    for (int t = l; t < tiles; t += 64) {
        const uint32_t* s = part + ((size_t)p * tiles + t) * 8;
        for (int r = 0; r < 3; ++r) { red[r] = min(red[r], s[r]); red[3 + r] = max(red[3 + r], s[3 + r]); }
        red[6] |= s[6];
    }
    for (int o = 32; o >= 1; o >>= 1) {
        for (int r = 0; r < 3; ++r) {
            red[r] = min(red[r], (uint32_t)__shfl_xor((int)red[r], o));
            red[3 + r] = max(red[3 + r], (uint32_t)__shfl_xor((int)red[3 + r], o));
        }
        red[6] |= (uint32_t)__shfl_xor((int)red[6], o);
    }
    if (l < 6) {
        const int c = l % 3, hi = l / 3;
        uint32_t k = 0u;
        for (int r = 0; r < 6; ++r) if (r == l) k = red[r];
        float x = ((red[6] >> c) & 1u) ? __uint_as_float(0x7FC00000u) : body_unkey(k);
        // utils/zju_mocap_dataset.py:60-65, utils/h36m_utils.py:372-379: float32 padding
        float pad = 0.0f;
        if (pad_mode == 1) pad = 0.1f;
        else if (pad_mode == 2) pad = c == 2 ? 0.05f : 0.0f;
        else if (pad_mode == 3) pad = 0.05f;
        if (pad != 0.0f) x = hi ? x + pad : x - pad;
        bounds[(size_t)p * 6 + l] = x;
    }
}

// ---- dsn_body_shape ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_body_shape(const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                    const float* __restrict__ betas, int B, int n3, float* __restrict__ v_shaped) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    const float vt = v_template[i];
    if (!shapedirs || !betas || B <= 0) { v_shaped[i] = vt; return; }
    float s = 0.0f;
    const float* row = shapedirs + (size_t)i * B;
    for (int b = 0; b < B; ++b) s = s + row[b] * betas[b];
    v_shaped[i] = vt + s;
}
// one thread per (joint, coordinate): the sum over the vertices is a chain in ascending order
__global__ __launch_bounds__(64) void k_body_joints(const float* __restrict__ J_regressor, const float* __restrict__ v_shaped, int V,
                                                    float* __restrict__ joints) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= BODY_J * 3) return;
    const int j = i / 3, c = i % 3;
    const float* row = J_regressor + (size_t)j * V;
    float s = 0.0f;
    for (int v = 0; v < V; ++v) s = s + row[v] * v_shaped[(size_t)v * 3 + c];
    joints[i] = s;
}

void dsn_launch_body_shape(const float* v_template, const float* shapedirs, const float* betas, int B, const float* J_regressor, int V,
                           float* v_shaped, float* joints, hipStream_t st) {
    const int n3 = 3 * V;
    hipLaunchKernelGGL(k_body_shape, dim3((n3 + 255) / 256), dim3(256), 0, st, v_template, shapedirs, betas, B, n3, v_shaped);
    if (joints) hipLaunchKernelGGL(k_body_joints, dim3(2), dim3(64), 0, st, J_regressor, v_shaped, V, joints);
}

void dsn_launch_body_pose(const float* v_shaped, const float* joints, const int* parents24, const float* weights, const float* posedirs, int V,
                          const float* poses, const float* Rh, const float* Th, int P, int pad_mode, float* xyz, float* xyz_smpl, float* A,
                          float* bounds, float* Rh_mat, void* workspace, hipStream_t st) {
    DsnBodyParents par;
    for (int i = 0; i < BODY_J; ++i) par.p[i] = i == 0 ? 0 : parents24[i];
    const DsnBodyWs w = dsn_body_ws(workspace, V, P);
    const int tiles = dsn_body_tiles(V);
    hipLaunchKernelGGL(k_body_chain, dim3(P), dim3(64), 0, st, joints, par, poses, Rh, P, w.A, w.Rh, w.pf, A, Rh_mat);
    hipLaunchKernelGGL(k_body_verts, dim3(tiles, (P + BODY_PB - 1) / BODY_PB), dim3(BODY_TV), 0, st, v_shaped, weights, posedirs, V, P, w.pf,
                       w.A, w.Rh, Th, xyz, xyz_smpl, w.part, bounds ? 1 : 0);
    if (bounds) hipLaunchKernelGGL(k_body_bounds, dim3(P), dim3(64), 0, st, w.part, tiles, P, pad_mode, bounds);
}
