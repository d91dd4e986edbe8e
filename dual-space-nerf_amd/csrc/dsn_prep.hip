// dsn_prep.hip - the datasets' image preparation on the device (dsn_image_undistort, dsn_image_morph, dsn_image_resize and the fused
// ZJU item dsn_image_prep; the rule is in include/dsnerf.h): the undistortion map per destination pixel in float64 (one rounding per
// operation: -ffp-contract=off), fixed-point bilinear taps with a zero border, box erode / dilate through an LDS tile with halo, row
// pass then column pass, and the integer-factor resizes.  One writer per output element, no atomics, no workspace.
// All four kernels work on full-resolution tiles of PREP_TW x PREP_TH pixels with PREP_THREADS threads.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include <climits>
#include <cmath>

#define PREP_TW 64
#define PREP_TH 16
#define PREP_THREADS 256
#define PREP_KMAX 15
#define PREP_RW (PREP_TW + PREP_KMAX - 1)          // region = tile + halo
#define PREP_RH (PREP_TH + PREP_KMAX - 1)
#define PREP_OUTSIDE INT_MIN

static_assert(PREP_TW == DSN_PREP_TILE_W && PREP_TH == DSN_PREP_TILE_H, "the header documents the tile");

struct DsnCam { double fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6; };

__device__ __forceinline__ DsnCam load_cam(const double* __restrict__ K, const double* __restrict__ D, int nd, int n) {
    const double* k = K + (size_t)n * 9;
    const double* d = D + (size_t)n * nd;
    DsnCam c;
    c.fx = k[0]; c.cx = k[2]; c.fy = k[4]; c.cy = k[5];
    c.k1 = d[0]; c.k2 = d[1]; c.p1 = d[2]; c.p2 = d[3];
    c.k3 = nd > 4 ? d[4] : 0.0;
    c.k4 = nd > 5 ? d[5] : 0.0; c.k5 = nd > 5 ? d[6] : 0.0; c.k6 = nd > 5 ? d[7] : 0.0;
    return c;
}

// the map of destination pixel (i, j) in 1/32 pixel: false = an outside pixel (not finite, or 2^30 or more in magnitude)
__device__ __forceinline__ bool prep_map(const DsnCam& c, int i, int j, int& iu, int& iv) {
    const double x = ((double)j - c.cx) / c.fx, y = ((double)i - c.cy) / c.fy;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, t = (2.0 * x) * y;
    const double num = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double den = 1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2;
    const double kr = num / den;
    const double xd = (x * kr + c.p1 * t) + c.p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + c.p1 * (r2 + 2.0 * y2)) + c.p2 * t;
    const double us = (c.fx * xd + c.cx) * 32.0, vs = (c.fy * yd + c.cy) * 32.0;
    if (!(fabs(us) < 1073741824.0) || !(fabs(vs) < 1073741824.0)) return false;          // NaN fails both comparisons
    iu = (int)rint(us);          // half to even
    iv = (int)rint(vs);
    return true;
}

struct DsnTaps { int sx, sy; int w00, w01, w10, w11; bool x0, x1, y0, y1; };

__device__ __forceinline__ DsnTaps prep_taps(int iu, int iv, int H, int W) {
    DsnTaps t;
    t.sx = iu >> 5; t.sy = iv >> 5;
    const int ax = iu & 31, ay = iv & 31;
    t.w00 = (32 - ay) * (32 - ax); t.w01 = (32 - ay) * ax; t.w10 = ay * (32 - ax); t.w11 = ay * ax;
    t.x0 = t.sx >= 0 && t.sx < W; t.x1 = t.sx >= -1 && t.sx < W - 1;
    t.y0 = t.sy >= 0 && t.sy < H; t.y1 = t.sy >= -1 && t.sy < H - 1;
    return t;
}

// ---- dsn_image_undistort ---------------------------------------------------------------------------------------------------------------
template <typename T, int C>
__global__ void __launch_bounds__(PREP_THREADS) k_image_undistort(const T* __restrict__ src, T* __restrict__ dst, const double* __restrict__ K,
                                                                  const double* __restrict__ D, int nd, int H, int W) {
    const int n = blockIdx.z;
    const int j = blockIdx.x * PREP_TW + (threadIdx.x & (PREP_TW - 1));
    const int i0 = blockIdx.y * PREP_TH + (threadIdx.x / PREP_TW);
    const DsnCam cam = load_cam(K, D, nd, n);
    const T* im = src + (size_t)n * H * W * C;
#pragma unroll
    for (int r = 0; r < PREP_TH; r += PREP_THREADS / PREP_TW) {
        const int i = i0 + r;
        if (i >= H || j >= W) continue;
        T out[C];
        for (int ch = 0; ch < C; ++ch) out[ch] = (T)0;
        int iu, iv;
        if (prep_map(cam, i, j, iu, iv)) {
            const DsnTaps t = prep_taps(iu, iv, H, W);
            const size_t base = ((size_t)((int64_t)t.sy * W + t.sx)) * C;          // (used only where the tap is inside)
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const T s00 = t.y0 && t.x0 ? im[base + ch] : (T)0;
                const T s01 = t.y0 && t.x1 ? im[base + C + ch] : (T)0;
                const T s10 = t.y1 && t.x0 ? im[base + (size_t)W * C + ch] : (T)0;
                const T s11 = t.y1 && t.x1 ? im[base + (size_t)W * C + C + ch] : (T)0;
                if constexpr (sizeof(T) == 1) {
                    out[ch] = (T)(((int)s00 * t.w00 + (int)s01 * t.w01 + (int)s10 * t.w10 + (int)s11 * t.w11 + 512) >> 10);
                } else {
                    const float f00 = (float)t.w00 * 0x1p-10f, f01 = (float)t.w01 * 0x1p-10f, f10 = (float)t.w10 * 0x1p-10f,
                                f11 = (float)t.w11 * 0x1p-10f;
                    out[ch] = ((s00 * f00 + s01 * f01) + s10 * f10) + s11 * f11;
                }
            }
        }
        T* o = dst + (((size_t)n * H + i) * W + j) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) o[ch] = out[ch];
    }
}

void dsn_launch_image_undistort(const void* src, void* dst, const double* K, const double* D, int nd, int N, int H, int W, int channels,
                                int dtype, hipStream_t st) {
    const dim3 grid((W + PREP_TW - 1) / PREP_TW, (H + PREP_TH - 1) / PREP_TH, N), block(PREP_THREADS);
    if (dtype == DSN_PREP_U8) {
        if (channels == 1) hipLaunchKernelGGL((k_image_undistort<uint8_t, 1>), grid, block, 0, st, (const uint8_t*)src, (uint8_t*)dst, K, D, nd, H, W);
        else hipLaunchKernelGGL((k_image_undistort<uint8_t, 3>), grid, block, 0, st, (const uint8_t*)src, (uint8_t*)dst, K, D, nd, H, W);
    } else {
        if (channels == 1) hipLaunchKernelGGL((k_image_undistort<float, 1>), grid, block, 0, st, (const float*)src, (float*)dst, K, D, nd, H, W);
        else hipLaunchKernelGGL((k_image_undistort<float, 3>), grid, block, 0, st, (const float*)src, (float*)dst, K, D, nd, H, W);
    }
}

// ---- box morphology on an LDS tile with halo ---------------------------------------------------------------------------------------------
// region[r][q]: the pixel (tile row0 - k/2 + r, tile col0 - k/2 + q), the operation's neutral value outside the image.  Row pass into
// rows[r][x] = op over region[r][x .. x + k - 1], column pass out(y, x) = op over rows[y .. y + k - 1][x].
template <bool DILATE>
__device__ __forceinline__ uint8_t prep_op(uint8_t a, uint8_t b) { return DILATE ? (a > b ? a : b) : (a < b ? a : b); }

template <bool DILATE>
__device__ __forceinline__ void prep_row_pass(const uint8_t (*region)[PREP_RW + 1], uint8_t (*rows)[PREP_TW], int k) {
    const int rh = PREP_TH + k - 1;
    for (int e = threadIdx.x; e < rh * PREP_TW; e += PREP_THREADS) {
        const int r = e / PREP_TW, x = e - r * PREP_TW;
        uint8_t v = region[r][x];
        for (int d = 1; d < k; ++d) v = prep_op<DILATE>(v, region[r][x + d]);
        rows[r][x] = v;
    }
}

template <bool DILATE>
__device__ __forceinline__ uint8_t prep_col_pass(const uint8_t (*rows)[PREP_TW], int y, int x, int k) {
    uint8_t v = rows[y][x];
    for (int d = 1; d < k; ++d) v = prep_op<DILATE>(v, rows[y + d][x]);
    return v;
}

template <bool DILATE>
__global__ void __launch_bounds__(PREP_THREADS) k_image_morph(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int k) {
    __shared__ uint8_t region[PREP_RH][PREP_RW + 1];
    __shared__ uint8_t rows[PREP_RH][PREP_TW];
    const int n = blockIdx.z, x0 = blockIdx.x * PREP_TW, y0 = blockIdx.y * PREP_TH, a = k / 2;
    const int rh = PREP_TH + k - 1, rw = PREP_TW + k - 1;
    const uint8_t* im = src + (size_t)n * H * W;
    for (int e = threadIdx.x; e < rh * rw; e += PREP_THREADS) {
        const int r = e / rw, q = e - r * rw;
        const int i = y0 - a + r, j = x0 - a + q;
        region[r][q] = (i >= 0 && i < H && j >= 0 && j < W) ? im[(size_t)i * W + j] : (DILATE ? (uint8_t)0 : (uint8_t)255);
    }
    __syncthreads();
    prep_row_pass<DILATE>(region, rows, k);
    __syncthreads();
    for (int e = threadIdx.x; e < PREP_TH * PREP_TW; e += PREP_THREADS) {
        const int y = e / PREP_TW, x = e - y * PREP_TW;
        if (y0 + y < H && x0 + x < W) dst[((size_t)n * H + y0 + y) * W + x0 + x] = prep_col_pass<DILATE>(rows, y, x, k);
    }
}

void dsn_launch_image_morph(const uint8_t* src, uint8_t* dst, int N, int H, int W, int k, int op, hipStream_t st) {
    const dim3 grid((W + PREP_TW - 1) / PREP_TW, (H + PREP_TH - 1) / PREP_TH, N), block(PREP_THREADS);
    if (op == DSN_PREP_DILATE) hipLaunchKernelGGL(k_image_morph<true>, grid, block, 0, st, src, dst, H, W, k);
    else hipLaunchKernelGGL(k_image_morph<false>, grid, block, 0, st, src, dst, H, W, k);
}

// ---- dsn_image_resize --------------------------------------------------------------------------------------------------------------------
// the area rule of a c x c block of uint8 levels: c = 2 rounds half up, c = 4 half to even, c = 1 copies
__device__ __forceinline__ int prep_area_u8(int s, int c) {
    return c == 1 ? s : c == 2 ? (s + 2) >> 2 : (s + 7 + ((s >> 4) & 1)) >> 4;
}

// a thread per output element (pixel, channel); Ho = H / c, Wo = W / c
template <typename T>
__global__ void __launch_bounds__(PREP_THREADS) k_image_resize(const T* __restrict__ src, T* __restrict__ dst, int64_t total, int H, int W, int C,
                                                               int c, int area) {
    const int64_t e = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x;
    if (e >= total) return;
    const int Ho = H / c, Wo = W / c;
    const int ch = (int)(e % C);
    int64_t p = e / C;
    const int x = (int)(p % Wo);
    p /= Wo;
    const int y = (int)(p % Ho);
    const int64_t n = p / Ho;
    const T* at = src + (((size_t)n * H + (size_t)y * c) * W + (size_t)x * c) * C + ch;
    if (!area || c == 1) { dst[e] = at[0]; return; }
    if constexpr (sizeof(T) == 1) {
        int s = 0;
        for (int dy = 0; dy < c; ++dy)
            for (int dx = 0; dx < c; ++dx) s += at[((size_t)dy * W + dx) * C];
        dst[e] = (T)prep_area_u8(s, c);
    } else {
        float s = at[0];
        for (int q = 1; q < c * c; ++q) s = s + at[((size_t)(q / c) * W + (q % c)) * C];          // row-major
        dst[e] = s * (c == 2 ? 0.25f : 0.0625f);
    }
}

void dsn_launch_image_resize(const void* src, void* dst, int N, int H, int W, int channels, int dtype, int c, int mode, hipStream_t st) {
    const int64_t total = (int64_t)N * (H / c) * (W / c) * channels;
    const dim3 grid((unsigned)((total + PREP_THREADS - 1) / PREP_THREADS)), block(PREP_THREADS);
    if (dtype == DSN_PREP_U8)
        hipLaunchKernelGGL(k_image_resize<uint8_t>, grid, block, 0, st, (const uint8_t*)src, (uint8_t*)dst, total, H, W, channels, c,
                           mode == DSN_PREP_AREA);
    else
        hipLaunchKernelGGL(k_image_resize<float>, grid, block, 0, st, (const float*)src, (float*)dst, total, H, W, channels, c,
                           mode == DSN_PREP_AREA);
}

// ---- dsn_image_prep: the ZJU item in one launch --------------------------------------------------------------------------------------------
// the area rule on the c x c block of output element `idx` (pixel idx / 3, channel idx % 3) of output row oy of the tile's masked plane
__device__ __forceinline__ int prep_block_level(const uint8_t (*masked)[PREP_TW * 3], int oy, int idx, int c) {
    const int ox = idx / 3, ch = idx - ox * 3;
    int s = 0;
    for (int dy = 0; dy < c; ++dy)
        for (int dx = 0; dx < c; ++dx) s += masked[oy * c + dy][(ox * c + dx) * 3 + ch];
    return prep_area_u8(s, c);
}

template <typename OUT>
__global__ void __launch_bounds__(PREP_THREADS) k_image_prep(const uint8_t* __restrict__ img, const uint8_t* __restrict__ cihp,
                                                             const double* __restrict__ K, const double* __restrict__ D, int nd, int H0, int W0,
                                                             int c, int border, OUT* __restrict__ out_img, uint8_t* __restrict__ out_u8,
                                                             uint8_t* __restrict__ out_fg, uint8_t* __restrict__ out_cihp) {
    __shared__ uint8_t region[PREP_RH][PREP_RW + 1];          // phase A: the undistorted foreground bit of tile and halo
    __shared__ uint8_t rows[PREP_RH][PREP_TW];                // the row pass of the dilation
    __shared__ int2 maps[PREP_TH][PREP_TW];                   // the tile's own map, kept from phase A
    __shared__ __attribute__((aligned(16))) uint8_t masked[PREP_TH][PREP_TW * 3];          // undistort(img) * msk_fg at full resolution
    __shared__ __attribute__((aligned(16))) uint8_t fgt[PREP_TH][PREP_TW];                 // msk_fg at full resolution
    __shared__ __attribute__((aligned(16))) OUT lut[256];                                  // level / 255.0
    const int n = blockIdx.z, x0 = blockIdx.x * PREP_TW, y0 = blockIdx.y * PREP_TH, a = border / 2;
    const int rh = PREP_TH + border - 1, rw = PREP_TW + border - 1;
    const DsnCam cam = load_cam(K, D, nd, n);
    const uint8_t* im = img + (size_t)n * H0 * W0 * 3;
    const uint8_t* ci = cihp + (size_t)n * H0 * W0;
    lut[threadIdx.x] = (OUT)((double)threadIdx.x / 255.0);

    // phase A: map and foreground bit of tile and halo; pixels outside the image do not take part in the dilation
    for (int e = threadIdx.x; e < rh * rw; e += PREP_THREADS) {
        const int r = e / rw, q = e - r * rw;
        const int i = y0 - a + r, j = x0 - a + q;
        uint8_t bit = 0;
        int iu = PREP_OUTSIDE, iv = 0;
        if (i >= 0 && i < H0 && j >= 0 && j < W0) {
            if (prep_map(cam, i, j, iu, iv)) {
                const DsnTaps t = prep_taps(iu, iv, H0, W0);
                const size_t base = (size_t)((int64_t)t.sy * W0 + t.sx);
                const int s = (t.y0 && t.x0 && ci[base] ? t.w00 : 0) + (t.y0 && t.x1 && ci[base + 1] ? t.w01 : 0) +
                              (t.y1 && t.x0 && ci[base + W0] ? t.w10 : 0) + (t.y1 && t.x1 && ci[base + W0 + 1] ? t.w11 : 0);
                bit = (uint8_t)((s + 512) >> 10);
            } else {
                iu = PREP_OUTSIDE;
            }
        }
        region[r][q] = bit;
        const int ty = r - a, tx = q - a;
        if (ty >= 0 && ty < PREP_TH && tx >= 0 && tx < PREP_TW) maps[ty][tx] = make_int2(iu, iv);
    }
    __syncthreads();
    prep_row_pass<true>(region, rows, border);
    __syncthreads();

    // phase B: the dilated mask, the image's taps, the product - at full resolution into LDS
    for (int e = threadIdx.x; e < PREP_TH * PREP_TW; e += PREP_THREADS) {
        const int y = e / PREP_TW, x = e - y * PREP_TW;
        const uint8_t m = prep_col_pass<true>(rows, y, x, border);
        fgt[y][x] = m;
        const int2 uv = maps[y][x];
        int v[3] = {0, 0, 0};
        if (m && uv.x != PREP_OUTSIDE) {
            const DsnTaps t = prep_taps(uv.x, uv.y, H0, W0);
            const size_t base = ((size_t)((int64_t)t.sy * W0 + t.sx)) * 3;
            const bool b00 = t.y0 && t.x0, b01 = t.y0 && t.x1, b10 = t.y1 && t.x0, b11 = t.y1 && t.x1;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int s00 = b00 ? im[base + ch] : 0, s01 = b01 ? im[base + 3 + ch] : 0;
                const int s10 = b10 ? im[base + (size_t)W0 * 3 + ch] : 0, s11 = b11 ? im[base + (size_t)W0 * 3 + 3 + ch] : 0;
                v[ch] = ((s00 * t.w00 + s01 * t.w01 + s10 * t.w10 + s11 * t.w11 + 512) >> 10) * m;
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) masked[y][x * 3 + ch] = (uint8_t)v[ch];
    }
    __syncthreads();

    // phase C: c x c blocks.  An output row of the tile is a flat run of n3 = 3 tw values; a thread owns 16 bytes of it (two float64,
    // four float32 or - img_u8 - four levels) and stores them at once where the row starts on that grid, value by value otherwise.
    const int H = H0 / c, W = W0 / c;
    const int oy0 = y0 / c, ox0 = x0 / c;
    const int tw = min(PREP_TW / c, W - ox0), th = min(PREP_TH / c, H - oy0);
    const int n3 = tw * 3;
    constexpr int PER = 16 / (int)sizeof(OUT);
    const int groups = (n3 + PER - 1) / PER;
    for (int e = threadIdx.x; e < th * groups; e += PREP_THREADS) {
        const int oy = e / groups, e0 = (e - oy * groups) * PER;
        OUT* dst = out_img + (((size_t)n * H + oy0 + oy) * W + ox0) * 3 + e0;
        __attribute__((aligned(16))) OUT v[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) v[q] = e0 + q < n3 ? lut[prep_block_level(masked, oy, e0 + q, c)] : (OUT)0;
        if (e0 + PER <= n3 && ((uintptr_t)dst & 15) == 0) {
            *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(v);
        } else {
#pragma unroll
            for (int q = 0; q < PER; ++q)
                if (e0 + q < n3) dst[q] = v[q];
        }
    }
    if (out_u8) {
        const int groups8 = (n3 + 3) / 4;
        for (int e = threadIdx.x; e < th * groups8; e += PREP_THREADS) {
            const int oy = e / groups8, e0 = (e - oy * groups8) * 4;
            uint8_t* dst = out_u8 + (((size_t)n * H + oy0 + oy) * W + ox0) * 3 + e0;
            uint32_t word = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (e0 + q < n3) word |= (uint32_t)prep_block_level(masked, oy, e0 + q, c) << (8 * q);
            if (e0 + 4 <= n3 && ((uintptr_t)dst & 3) == 0) {
                *reinterpret_cast<uint32_t*>(dst) = word;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (e0 + q < n3) dst[q] = (uint8_t)(word >> (8 * q));
            }
        }
    }
    // the masks: nearest = the block's first pixel; msk_cihp from the raw mask
    for (int e = threadIdx.x; e < th * tw; e += PREP_THREADS) {
        const int oy = e / tw, ox = e - oy * tw;
        const size_t pix = ((size_t)n * H + oy0 + oy) * W + ox0 + ox;
        if (out_fg) out_fg[pix] = fgt[oy * c][ox * c];
        if (out_cihp) out_cihp[pix] = ci[(size_t)(y0 + oy * c) * W0 + x0 + ox * c];
    }
}

void dsn_launch_image_prep(const uint8_t* img, const uint8_t* msk_cihp, const double* K, const double* D, int nd, int N, int H0, int W0, int c,
                           int border, int out_dtype, void* out_img, uint8_t* out_img_u8, uint8_t* out_msk_fg, uint8_t* out_msk_cihp,
                           hipStream_t st) {
    const dim3 grid((W0 + PREP_TW - 1) / PREP_TW, (H0 + PREP_TH - 1) / PREP_TH, N), block(PREP_THREADS);
    if (out_dtype == DSN_PREP_F64)
        hipLaunchKernelGGL(k_image_prep<double>, grid, block, 0, st, img, msk_cihp, K, D, nd, H0, W0, c, border, (double*)out_img, out_img_u8,
                           out_msk_fg, out_msk_cihp);
    else
        hipLaunchKernelGGL(k_image_prep<float>, grid, block, 0, st, img, msk_cihp, K, D, nd, H0, W0, c, border, (float*)out_img, out_img_u8,
                           out_msk_fg, out_msk_cihp);
}
