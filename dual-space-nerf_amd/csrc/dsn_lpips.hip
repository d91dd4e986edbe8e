// dsn_lpips.hip - the LPIPS distance of test.py:18-23, 77-91 (lpips v0.1, net = alex | vgg, lpips=True, spatial=False, eval) on the
// device; the rule is in include/dsnerf.h.
//   k_lpips_prep    pixels -> the scaling layer's output, split, [n,H,W,3]; flags non-finite pixels
//   k_lpips_conv    every convolution: implicit GEMM on the split-fp16 scheme of dsn_field16.hip (three K = 16 f16 MFMA products per
//                   operand pair, fp32 accumulation), bias + ReLU + range check + split in the epilogue, the tap's float32 copy too
//   k_lpips_pool    floor-mode max pooling on the split words
//   k_lpips_head    per tap: unit-normalise over channels, lin-weighted squared difference, float64, one partial per share
//   k_lpips_final   partials in index order -> out, out_layers, status
//   k_lpips_nchw    a tap as float32 [n,C,h,w] (dsn_lpips_features)
// Activations live between layers as [n,h,w,C] words: fp16 hi in the low half, fp16 lo = (v - hi) * 2^12 in the high half - the four
// bytes a float takes, so the consumer's eight k values per lane are one 32-byte load and two permutes per pair, no split.  Weights are
// split once by dsn_lpips_pack, in B-operand order.  Every output element has one writer, every sum a fixed order, and an image's
// values depend on that image alone (grid z = image): the same bits on every call, alone or in any batch.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

#define LP_THREADS 256
#define LP_TILE_M DSN_LPIPS_TILE_M      // output pixels per wave: two 32-row MFMA tiles
#define LP_TILE_N 64                    // output channels per wave: two 32-column MFMA tiles (every Cout is a multiple of 64)
#define LP_MAX_OPS 20
#define LP_HEAD_SHARES 1024             // most partials per (frame, tap): a share is at least 64 pixels, 16 per wave

// ---- the two backbones ---------------------------------------------------------------------------------------------------------
struct LpOp { int conv, cin, cout, k, s, p, tap; };     // conv = 0: max pooling k / s
static const LpOp LP_ALEX[] = {{1, 3, 64, 11, 4, 2, 0}, {0, 0, 0, 3, 2, 0, -1}, {1, 64, 192, 5, 1, 2, 1}, {0, 0, 0, 3, 2, 0, -1},
                               {1, 192, 384, 3, 1, 1, 2}, {1, 384, 256, 3, 1, 1, 3}, {1, 256, 256, 3, 1, 1, 4}};
static const LpOp LP_VGG[] = {{1, 3, 64, 3, 1, 1, -1}, {1, 64, 64, 3, 1, 1, 0}, {0, 0, 0, 2, 2, 0, -1},
                              {1, 64, 128, 3, 1, 1, -1}, {1, 128, 128, 3, 1, 1, 1}, {0, 0, 0, 2, 2, 0, -1},
                              {1, 128, 256, 3, 1, 1, -1}, {1, 256, 256, 3, 1, 1, -1}, {1, 256, 256, 3, 1, 1, 2}, {0, 0, 0, 2, 2, 0, -1},
                              {1, 256, 512, 3, 1, 1, -1}, {1, 512, 512, 3, 1, 1, -1}, {1, 512, 512, 3, 1, 1, 3}, {0, 0, 0, 2, 2, 0, -1},
                              {1, 512, 512, 3, 1, 1, -1}, {1, 512, 512, 3, 1, 1, -1}, {1, 512, 512, 3, 1, 1, 4}};
static const LpOp* lp_ops(int net, int& n) {
    if (net == DSN_LPIPS_ALEX) { n = (int)(sizeof(LP_ALEX) / sizeof(LpOp)); return LP_ALEX; }
    n = (int)(sizeof(LP_VGG) / sizeof(LpOp));
    return LP_VGG;
}
static int lp_k16(const LpOp& o) { return (o.k * o.k * o.cin + 15) / 16; }
static size_t lp_wimg_bytes(const LpOp& o) { return (size_t)lp_k16(o) * (o.cout / 32) * 64 * 32; }

// packed image: [256 B header: int32 word 0 = weights outside the split's range] then per convolution {B-operand image, bias}, then
// the five lin vectors; every piece 256-byte aligned
struct LpPackedView { size_t w[LP_MAX_OPS], b[LP_MAX_OPS], lin[5], total; };
static LpPackedView lp_packed_view(int net) {
    LpPackedView v;
    int n;
    const LpOp* ops = lp_ops(net, n);
    size_t p = 256;
    int tap_c[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        v.w[i] = v.b[i] = 0;
        if (!ops[i].conv) continue;
        v.w[i] = p; p += dsn_align256(lp_wimg_bytes(ops[i]));
        v.b[i] = p; p += dsn_align256(sizeof(float) * ops[i].cout);
        if (ops[i].tap >= 0) tap_c[ops[i].tap] = ops[i].cout;
    }
    for (int l = 0; l < 5; ++l) { v.lin[l] = p; p += dsn_align256(sizeof(float) * tap_c[l]); }
    v.total = p;
    return v;
}
size_t dsn_lpips_packed_size(int net) { return lp_packed_view(net).total; }

// ---- split words ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lp_split(float v) {
    const _Float16 hi = (_Float16)v;
    const float res = fmaf((float)hi, -1.0f, v);            // exact
    const _Float16 lo = (_Float16)(res * DSN_LO_SCALE);
    return (uint32_t)__builtin_bit_cast(uint16_t, hi) | ((uint32_t)__builtin_bit_cast(uint16_t, lo) << 16);
}
__device__ __forceinline__ float lp_join(uint32_t w) {
    const float hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
    const float lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
    return fmaf(lo, DSN_LO_INV, hi);
}
__device__ __forceinline__ bool lp_in_range(float v) { return fabsf(v) < DSN_LPIPS_RANGE_MAX; }      // false for NaN

// ---- weights -> B-operand image --------------------------------------------------------------------------------------------------
// k = (ky kw + kx) Cin + ci, zero beyond kh kw Cin; image [k-step t][32-column tile j][lane l][hi 8 halves | lo 8 halves], lane l holds
// column 32 j + (l & 31), k = 16 t + 8 (l >> 5) + i
__global__ void __launch_bounds__(LP_THREADS) k_lpips_pack(const float* __restrict__ w, const float* __restrict__ b, int cin, int cout, int ksz,
                                                           int k16, uint16_t* __restrict__ wimg, float* __restrict__ bias,
                                                           int32_t* __restrict__ unsafe) {
    const size_t n = (size_t)k16 * (cout / 32) * 64 * 8;
    const size_t e = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;
    bool bad = false;
    if (e < n) {
        const int i = (int)(e & 7), l = (int)((e >> 3) & 63);
        const size_t tj = e >> 9;
        const int j = (int)(tj % (cout / 32)), t = (int)(tj / (cout / 32));
        const int k = 16 * t + 8 * (l >> 5) + i, co = 32 * j + (l & 31);
        float v = 0.0f;
        if (k < ksz * ksz * cin) {
            const int tap = k / cin, ci = k - tap * cin;
            v = w[((size_t)co * cin + ci) * ksz * ksz + tap];
        }
        bad = !lp_in_range(v);
        const uint32_t s = lp_split(v);
        const size_t base = (tj * 64 + l) * 16;
        wimg[base + i] = (uint16_t)(s & 0xffffu);
        wimg[base + 8 + i] = (uint16_t)(s >> 16);
    }
    if (e < (size_t)cout) {
        const float v = b[e];
        bad = bad || !lp_in_range(v);
        bias[e] = v;
    }
    if (bad) atomicOr(unsafe, 1);
}
__global__ void __launch_bounds__(LP_THREADS) k_lpips_pack_lin(const float* __restrict__ src, int c, float* __restrict__ dst,
                                                               int32_t* __restrict__ unsafe) {
    const int i = blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= c) return;
    const float v = src[i];
    dst[i] = v;
    if (!(fabsf(v) <= 3.4e38f)) atomicOr(unsafe, 1);
}

int dsn_launch_lpips_pack(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, void* packed,
                          hipStream_t st) {
    const LpPackedView pv = lp_packed_view(net);
    int n;
    const LpOp* ops = lp_ops(net, n);
    char* base = (char*)packed;
    if (hipMemsetAsync(packed, 0, 256, st) != hipSuccess) return 1;
    int c = 0, tap_c[5];
    for (int i = 0; i < n; ++i) {
        if (!ops[i].conv) continue;
        const LpOp& o = ops[i];
        const size_t ne = (size_t)lp_k16(o) * (o.cout / 32) * 64 * 8;
        hipLaunchKernelGGL(k_lpips_pack, dim3((unsigned)((ne + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0, st, conv_w[c], conv_b[c],
                           o.cin, o.cout, o.k, lp_k16(o), (uint16_t*)(base + pv.w[i]), (float*)(base + pv.b[i]), (int32_t*)base);
        if (o.tap >= 0) tap_c[o.tap] = o.cout;
        ++c;
    }
    for (int l = 0; l < 5; ++l)
        hipLaunchKernelGGL(k_lpips_pack_lin, dim3((tap_c[l] + LP_THREADS - 1) / LP_THREADS), dim3(LP_THREADS), 0, st, lin_w[l], tap_c[l],
                           (float*)(base + pv.lin[l]), (int32_t*)base);
    return 0;
}

// ---- pixels -> the scaling layer's output ------------------------------------------------------------------------------------------
// image i < n_a comes from `a` (float32), the others from b64 / b32 (cast to float32 first); out [n,H,W,3] split words, RGB
__global__ void __launch_bounds__(LP_THREADS) k_lpips_prep(const float* __restrict__ a, const double* __restrict__ b64,
                                                           const float* __restrict__ b32, int n_a, size_t per_image, int rgb_pm1,
                                                           uint32_t* __restrict__ out, int32_t* __restrict__ flags) {
    const size_t e = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;      // element of image blockIdx.y: pixel e / 3, output channel e % 3
    if (e >= per_image) return;
    const int img = blockIdx.y;
    const size_t px = e / 3;
    const int c = (int)(e - 3 * px);
    const size_t src = px * 3 + (rgb_pm1 ? c : 2 - c);                   // flip(1): BGR -> RGB
    float v;
    if (img < n_a) v = a[(size_t)img * per_image + src];
    else if (b64) v = (float)b64[(size_t)(img - n_a) * per_image + src];
    else v = b32[(size_t)(img - n_a) * per_image + src];
    if (!(fabsf(v) <= 3.4e38f)) { atomicOr(flags + img, DSN_LPIPS_NONFINITE); v = 0.0f; }
    const float x = rgb_pm1 ? v : 2.0f * v - 1.0f;
    const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
    const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
    out[(size_t)img * per_image + e] = lp_split(dsn_div(x - shift, scale));
}

// ---- convolution -------------------------------------------------------------------------------------------------------------------
struct LpConvArgs {
    const uint32_t* in;      // [n,hi,wi,cin] split words
    const uint4* wimg;       // B-operand image
    const float* bias;
    uint32_t* out;           // [n,ho,wo,cout] split words
    float* tap;              // the same as float32, or NULL
    int32_t* flags;          // [n]
    int hi, wi, cin, ho, wo, cout, k, s, p, k16;
};

struct LpOperands { u32x4 a[2][2]; uint4 b[2][2]; };      // a[m tile][first / second four words], b[n tile][hi / lo]

// GATHER: Cin is no multiple of 16 (the two first layers, Cin = 3): every k of a lane's eight is looked up on its own
template <bool GATHER>
__device__ __forceinline__ void lp_load(const LpConvArgs& g, const uint32_t* __restrict__ in_img, const int (&iy0)[2], const int (&ix0)[2],
                                        const bool (&valid)[2], int t, int ky, int kx, int c0, int n64, int lane, LpOperands& o) {
    const int kh = lane >> 5;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        u32x4 lo4 = {0u, 0u, 0u, 0u}, hi4 = {0u, 0u, 0u, 0u};
        if (!GATHER) {
            const int iy = iy0[m] + ky, ix = ix0[m] + kx;
            if (valid[m] && iy >= 0 && iy < g.hi && ix >= 0 && ix < g.wi) {
                const u32x4* p = (const u32x4*)(in_img + ((size_t)iy * g.wi + ix) * g.cin + c0 + 8 * kh);
                lo4 = p[0]; hi4 = p[1];
            }
        } else {
            uint32_t w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = 16 * t + 8 * kh + i;
                const int tap = k / g.cin, ci = k - tap * g.cin;
                const int dy = tap / g.k, dx = tap - dy * g.k;
                const int iy = iy0[m] + dy, ix = ix0[m] + dx;
                w[i] = 0u;
                if (valid[m] && dy < g.k && iy >= 0 && iy < g.hi && ix >= 0 && ix < g.wi) w[i] = in_img[((size_t)iy * g.wi + ix) * g.cin + ci];
            }
            lo4 = u32x4{w[0], w[1], w[2], w[3]}; hi4 = u32x4{w[4], w[5], w[6], w[7]};
        }
        o.a[m][0] = lo4; o.a[m][1] = hi4;
    }
    const int nt32 = g.cout >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint4* p = g.wimg + (((size_t)t * nt32 + 2 * n64 + j) * 64 + lane) * 2;
        o.b[j][0] = p[0]; o.b[j][1] = p[1];
    }
}
// eight split words -> the eight hi halves and the eight lo halves
__device__ __forceinline__ void lp_unzip(const u32x4& w0, const u32x4& w1, half8& h, half8& l) {
    u32x4 hh, ll;
    hh[0] = (w0[0] & 0xffffu) | (w0[1] << 16); ll[0] = (w0[0] >> 16) | (w0[1] & 0xffff0000u);
    hh[1] = (w0[2] & 0xffffu) | (w0[3] << 16); ll[1] = (w0[2] >> 16) | (w0[3] & 0xffff0000u);
    hh[2] = (w1[0] & 0xffffu) | (w1[1] << 16); ll[2] = (w1[0] >> 16) | (w1[1] & 0xffff0000u);
    hh[3] = (w1[2] & 0xffffu) | (w1[3] << 16); ll[3] = (w1[2] >> 16) | (w1[3] & 0xffff0000u);
    h = __builtin_bit_cast(half8, hh);
    l = __builtin_bit_cast(half8, ll);
}

// one wave per LP_TILE_M x LP_TILE_N output tile of image blockIdx.y; the four waves of a workgroup take neighbouring channel tiles
// of the same pixels where there are any (their activation loads meet in the L1)
template <bool GATHER>
__global__ void __launch_bounds__(LP_THREADS) k_lpips_conv(const LpConvArgs g) {
    DSN_OWN_SIMD();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt64 = g.cout / LP_TILE_N, npix = g.ho * g.wo;
    const int tile = blockIdx.x * (LP_THREADS / 64) + wave;
    if (tile >= nt64 * ((npix + LP_TILE_M - 1) / LP_TILE_M)) return;
    const int n64 = tile % nt64, m64 = tile / nt64;
    const int img = blockIdx.y;
    const uint32_t* in_img = g.in + (size_t)img * g.hi * g.wi * g.cin;

    int iy0[2], ix0[2];
    bool valid[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int p = m64 * LP_TILE_M + 32 * m + (lane & 31);
        valid[m] = p < npix;
        const int oy = p / g.wo, ox = p - oy * g.wo;
        iy0[m] = oy * g.s - g.p; ix0[m] = ox * g.s - g.p;
    }
    f32x16 accM[2][2], accC[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { accM[m][j][r] = 0.0f; accC[m][j][r] = 0.0f; }

    int ky = 0, kx = 0, c0 = 0;
    LpOperands cur, nxt;
    lp_load<GATHER>(g, in_img, iy0, ix0, valid, 0, ky, kx, c0, n64, lane, cur);
    for (int t = 0; t < g.k16; ++t) {
        if (!GATHER) {
            c0 += 16;
            if (c0 == g.cin) { c0 = 0; if (++kx == g.k) { kx = 0; ++ky; } }
        }
        nxt = cur;
        if (t + 1 < g.k16) lp_load<GATHER>(g, in_img, iy0, ix0, valid, t + 1, ky, kx, c0, n64, lane, nxt);
        half8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) lp_unzip(cur.a[m][0], cur.a[m][1], ah[m], al[m]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            bh[j] = __builtin_bit_cast(half8, cur.b[j][0]);
            bl[j] = __builtin_bit_cast(half8, cur.b[j][1]);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                accM[m][j] = MFMA16(ah[m], bh[j], accM[m][j]);
                accC[m][j] = MFMA16(ah[m], bl[j], accC[m][j]);
            }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j) accC[m][j] = MFMA16(al[m], bh[j], accC[m][j]);
        cur = nxt;
    }

    // accumulator layout: lane l, register r holds output pixel row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the tile, channel column l & 31
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ch = n64 * LP_TILE_N + 32 * j + (lane & 31);
        const float bias = g.bias[ch];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = m64 * LP_TILE_M + 32 * m + dsn_crow(r, lane >> 5);
                if (p >= npix) continue;
                float v = (accM[m][j][r] + accC[m][j][r] * DSN_LO_INV) + bias;
                v = v > 0.0f ? v : (v <= 0.0f ? 0.0f : v);      // ReLU; NaN stays NaN for the range check
                bad = bad || !lp_in_range(v);
                const size_t o = ((size_t)img * npix + p) * g.cout + ch;
                g.out[o] = lp_split(v);
                if (g.tap) g.tap[o] = v;
            }
    }
    if (bad) atomicOr(g.flags + img, DSN_LPIPS_RANGE);
}

// ---- max pooling, floor mode ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LP_THREADS) k_lpips_pool(const uint32_t* __restrict__ in, int hi, int wi, int c, int k, int s, int ho, int wo,
                                                           uint32_t* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (e >= (size_t)ho * wo * c) return;
    const int img = blockIdx.y;
    const int ch = (int)(e % c);
    const size_t px = e / c;
    const int ox = (int)(px % wo), oy = (int)(px / wo);
    const uint32_t* p = in + (size_t)img * hi * wi * c;
    uint32_t best = p[((size_t)(oy * s) * wi + ox * s) * c + ch];
    float bv = lp_join(best);
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const uint32_t w = p[((size_t)(oy * s + dy) * wi + ox * s + dx) * c + ch];      // floor mode: every window lies inside
            const float v = lp_join(w);
            if (v > bv || v != v) { bv = v; best = w; }
        }
    out[(size_t)img * ho * wo * c + e] = best;
}

// ---- the head ------------------------------------------------------------------------------------------------------------------------
static int lp_head_shares(int npix) {
    const int n = (npix + 63) / 64;
    return n < LP_HEAD_SHARES ? n : LP_HEAD_SHARES;
}
__device__ __forceinline__ double lp_wave_sum(double v) {      // butterfly: every lane ends with the same bits
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// tap [n,npix,c] float32; frame f pairs images f and F + f.  Workgroup (share b, frame f): pixels [b npix / nb, (b + 1) npix / nb),
// wave w takes every fourth of them in order, one pixel at a time with the channels across its lanes.
__global__ void __launch_bounds__(LP_THREADS) k_lpips_head(const float* __restrict__ tap, int F, int npix, int c, const float* __restrict__ lin,
                                                           double* __restrict__ part) {
    const int f = blockIdx.y, b = blockIdx.x, nb = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = (int)((long long)b * npix / nb), p1 = (int)((long long)(b + 1) * npix / nb);
    const int nc = c >> 6;
    double w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = j < nc ? (double)lin[lane + 64 * j] : 0.0;
    double acc = 0.0;
    for (int p = p0 + wave; p < p1; p += LP_THREADS / 64) {
        const float* x0 = tap + ((size_t)f * npix + p) * c;
        const float* x1 = tap + ((size_t)(F + f) * npix + p) * c;
        double a0[8], a1[8], s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a0[j] = j < nc ? (double)x0[lane + 64 * j] : 0.0;
            a1[j] = j < nc ? (double)x1[lane + 64 * j] : 0.0;
            s0 += a0[j] * a0[j];
            s1 += a1[j] * a1[j];
        }
        const double n0 = sqrt(lp_wave_sum(s0)) + 1e-10, n1 = sqrt(lp_wave_sum(s1)) + 1e-10;      // the eps sits outside the root
        double d = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double e = a0[j] / n0 - a1[j] / n1;
            d += w[j] * (e * e);
        }
        acc += lp_wave_sum(d);
    }
    __shared__ double s[LP_THREADS / 64];
    if (lane == 0) s[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)f * LP_HEAD_SHARES + b] = ((s[0] + s[1]) + s[2]) + s[3];
}

// part [5][F][LP_HEAD_SHARES]; one thread per frame
__global__ void __launch_bounds__(64) k_lpips_final(const double* __restrict__ part, int F, int nb0, int nb1, int nb2, int nb3, int nb4, int np0,
                                                    int np1, int np2, int np3, int np4, const int32_t* __restrict__ flags,
                                                    const int32_t* __restrict__ unsafe, double* __restrict__ out,
                                                    double* __restrict__ out_layers, int32_t* __restrict__ status) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    const int nb[5] = {nb0, nb1, nb2, nb3, nb4}, np[5] = {np0, np1, np2, np3, np4};
    const int st = flags[f] | flags[F + f] | (unsafe[0] ? DSN_LPIPS_RANGE : 0);
    double total = 0.0;
    for (int l = 0; l < 5; ++l) {
        double t = 0.0;
        for (int b = 0; b < nb[l]; ++b) t += part[((size_t)l * F + f) * LP_HEAD_SHARES + b];
        t /= (double)np[l];
        if (st) t = __builtin_nan("");
        out_layers[5 * f + l] = t;
        total += t;
    }
    out[f] = total;
    status[f] = st;
}
__global__ void __launch_bounds__(64) k_lpips_too_small(int F, double* __restrict__ out, double* __restrict__ out_layers,
                                                        int32_t* __restrict__ status) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    out[f] = __builtin_nan("");
    for (int l = 0; l < 5; ++l) out_layers[5 * f + l] = __builtin_nan("");
    status[f] = DSN_LPIPS_TOO_SMALL;
}
__global__ void __launch_bounds__(64) k_lpips_status(int n, int too_small, const int32_t* __restrict__ flags, const int32_t* __restrict__ unsafe,
                                                     int32_t* __restrict__ status) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) status[i] = too_small ? DSN_LPIPS_TOO_SMALL : (flags[i] | (unsafe[0] ? DSN_LPIPS_RANGE : 0));
}

// tap [n,npix,c] -> [n,c,npix]; NaN for an image whose status is set
__global__ void __launch_bounds__(LP_THREADS) k_lpips_nchw(const float* __restrict__ tap, int npix, int c, const int32_t* __restrict__ flags,
                                                           const int32_t* __restrict__ unsafe, float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * LP_THREADS + threadIdx.x;      // element of the output: channel e / npix, pixel e % npix
    if (e >= (size_t)npix * c) return;
    const int img = blockIdx.y;
    const size_t ch = e / npix, p = e - ch * npix;
    const bool bad = flags[img] != 0 || unsafe[0] != 0;
    out[(size_t)img * npix * c + e] = bad ? __builtin_nanf("") : tap[((size_t)img * npix + p) * c + ch];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static int lp_out_side(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }
int dsn_lpips_min_side(int net) { return net == DSN_LPIPS_ALEX ? 31 : 16; }

struct LpPlan {
    int nops;
    const LpOp* ops;
    int h[LP_MAX_OPS + 1], w[LP_MAX_OPS + 1], c[LP_MAX_OPS + 1];      // sizes before op i (index nops: the last output)
    int tap_h[5], tap_w[5], tap_c[5];
    size_t flags, part, x0, buf[2], tap[5], total;                    // workspace offsets for N images
};
static LpPlan lp_plan(int net, int N, int H, int W) {
    LpPlan pl;
    pl.ops = lp_ops(net, pl.nops);
    pl.h[0] = H; pl.w[0] = W; pl.c[0] = 3;
    size_t biggest = 0;
    for (int i = 0; i < pl.nops; ++i) {
        const LpOp& o = pl.ops[i];
        pl.h[i + 1] = lp_out_side(pl.h[i], o.k, o.s, o.p);
        pl.w[i + 1] = lp_out_side(pl.w[i], o.k, o.s, o.p);
        pl.c[i + 1] = o.conv ? o.cout : pl.c[i];
        const size_t words = (size_t)pl.h[i + 1] * pl.w[i + 1] * pl.c[i + 1];
        biggest = words > biggest ? words : biggest;
        if (o.conv && o.tap >= 0) { pl.tap_h[o.tap] = pl.h[i + 1]; pl.tap_w[o.tap] = pl.w[i + 1]; pl.tap_c[o.tap] = o.cout; }
    }
    size_t p = 0;
    pl.flags = p; p += dsn_align256(sizeof(int32_t) * (size_t)N);
    pl.part = p;  p += dsn_align256(sizeof(double) * 5 * (size_t)N * LP_HEAD_SHARES);
    pl.x0 = p;    p += dsn_align256(sizeof(uint32_t) * 3 * (size_t)N * H * W);
    for (int b = 0; b < 2; ++b) { pl.buf[b] = p; p += dsn_align256(sizeof(uint32_t) * (size_t)N * biggest); }
    for (int l = 0; l < 5; ++l) { pl.tap[l] = p; p += dsn_align256(sizeof(float) * (size_t)N * pl.tap_h[l] * pl.tap_w[l] * pl.tap_c[l]); }
    pl.total = p;
    return pl;
}
size_t dsn_lpips_workspace_size(int net, int N, int H, int W) {
    if (H < dsn_lpips_min_side(net) || W < dsn_lpips_min_side(net)) return 256;
    return lp_plan(net, N, H, W).total;
}

// the backbone on N images: a (the first n_a, float32) and b (the others); the taps end in the workspace as float32 [N,h,w,C]
static void lp_backbone(const LpPlan& pl, int net, const void* packed, const float* a, const double* b64, const float* b32, int n_a, int N,
                        int H, int W, int rgb_pm1, char* ws, hipStream_t st) {
    const LpPackedView pv = lp_packed_view(net);
    const char* pk = (const char*)packed;
    int32_t* flags = (int32_t*)(ws + pl.flags);
    (void)hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)N, st);
    const size_t per_image = (size_t)H * W * 3;
    hipLaunchKernelGGL(k_lpips_prep, dim3((unsigned)((per_image + LP_THREADS - 1) / LP_THREADS), N), dim3(LP_THREADS), 0, st, a, b64, b32, n_a,
                       per_image, rgb_pm1, (uint32_t*)(ws + pl.x0), flags);
    const uint32_t* in = (const uint32_t*)(ws + pl.x0);
    int which = 0;
    for (int i = 0; i < pl.nops; ++i) {
        const LpOp& o = pl.ops[i];
        uint32_t* out = (uint32_t*)(ws + pl.buf[which]);
        if (o.conv) {
            LpConvArgs g;
            g.in = in; g.wimg = (const uint4*)(pk + pv.w[i]); g.bias = (const float*)(pk + pv.b[i]); g.out = out;
            g.tap = o.tap >= 0 ? (float*)(ws + pl.tap[o.tap]) : nullptr;
            g.flags = flags;
            g.hi = pl.h[i]; g.wi = pl.w[i]; g.cin = o.cin; g.ho = pl.h[i + 1]; g.wo = pl.w[i + 1]; g.cout = o.cout;
            g.k = o.k; g.s = o.s; g.p = o.p; g.k16 = lp_k16(o);
            const int tiles = (o.cout / LP_TILE_N) * ((g.ho * g.wo + LP_TILE_M - 1) / LP_TILE_M);
            const dim3 grid((tiles + LP_THREADS / 64 - 1) / (LP_THREADS / 64), N);
            if (o.cin % 16) hipLaunchKernelGGL(k_lpips_conv<true>, grid, dim3(LP_THREADS), 0, st, g);
            else hipLaunchKernelGGL(k_lpips_conv<false>, grid, dim3(LP_THREADS), 0, st, g);
        } else {
            const size_t ne = (size_t)pl.h[i + 1] * pl.w[i + 1] * pl.c[i];
            hipLaunchKernelGGL(k_lpips_pool, dim3((unsigned)((ne + LP_THREADS - 1) / LP_THREADS), N), dim3(LP_THREADS), 0, st, in, pl.h[i], pl.w[i],
                               pl.c[i], o.k, o.s, pl.h[i + 1], pl.w[i + 1], out);
        }
        in = out;
        which ^= 1;
    }
}

void dsn_launch_lpips_features(const void* packed, int net, const float* stack, int N, int H, int W, int rgb_pm1, float* const* out_taps,
                               int32_t* status, void* workspace, hipStream_t st) {
    const int32_t* unsafe = (const int32_t*)packed;
    if (H < dsn_lpips_min_side(net) || W < dsn_lpips_min_side(net)) {
        hipLaunchKernelGGL(k_lpips_status, dim3((N + 63) / 64), dim3(64), 0, st, N, 1, (const int32_t*)nullptr, unsafe, status);
        return;
    }
    const LpPlan pl = lp_plan(net, N, H, W);
    char* ws = (char*)workspace;
    lp_backbone(pl, net, packed, stack, nullptr, nullptr, N, N, H, W, rgb_pm1, ws, st);
    const int32_t* flags = (const int32_t*)(ws + pl.flags);
    for (int l = 0; l < 5; ++l) {
        const int npix = pl.tap_h[l] * pl.tap_w[l];
        const size_t ne = (size_t)npix * pl.tap_c[l];
        hipLaunchKernelGGL(k_lpips_nchw, dim3((unsigned)((ne + LP_THREADS - 1) / LP_THREADS), N), dim3(LP_THREADS), 0, st,
                           (const float*)(ws + pl.tap[l]), npix, pl.tap_c[l], flags, unsafe, out_taps[l]);
    }
    hipLaunchKernelGGL(k_lpips_status, dim3((N + 63) / 64), dim3(64), 0, st, N, 0, flags, unsafe, status);
}

void dsn_launch_lpips(const void* packed, int net, const float* img, const double* gt64, const float* gt32, int F, int H, int W, int rgb_pm1,
                      double* out, double* out_layers, int32_t* status, void* workspace, hipStream_t st) {
    if (H < dsn_lpips_min_side(net) || W < dsn_lpips_min_side(net)) {
        hipLaunchKernelGGL(k_lpips_too_small, dim3((F + 63) / 64), dim3(64), 0, st, F, out, out_layers, status);
        return;
    }
    const LpPlan pl = lp_plan(net, 2 * F, H, W);
    const LpPackedView pv = lp_packed_view(net);
    char* ws = (char*)workspace;
    lp_backbone(pl, net, packed, img, gt64, gt32, F, 2 * F, H, W, rgb_pm1, ws, st);
    double* part = (double*)(ws + pl.part);
    int nb[5], np[5];
    for (int l = 0; l < 5; ++l) {
        np[l] = pl.tap_h[l] * pl.tap_w[l];
        nb[l] = lp_head_shares(np[l]);
        hipLaunchKernelGGL(k_lpips_head, dim3(nb[l], F), dim3(LP_THREADS), 0, st, (const float*)(ws + pl.tap[l]), F, np[l], pl.tap_c[l],
                           (const float*)((const char*)packed + pv.lin[l]), part + (size_t)l * F * LP_HEAD_SHARES);
    }
    hipLaunchKernelGGL(k_lpips_final, dim3((F + 63) / 64), dim3(64), 0, st, part, F, nb[0], nb[1], nb[2], nb[3], nb[4], np[0], np[1], np[2], np[3],
                       np[4], (const int32_t*)(ws + pl.flags), (const int32_t*)packed, out, out_layers, status);
}
