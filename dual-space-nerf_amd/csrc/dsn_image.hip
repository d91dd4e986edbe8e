// dsn_image.hip - the step AFTER the hot path, on the device:
//   post_process (utils/render_utils.py:466-472): rows of the compacted per-ray outputs go, in order, to the pixels
//   where mask_at_box is set; every other pixel is zero; optional clamp of the colour image (test.py:62-63);
//   mse / psnr with and without the mask (metrics.py:8-21, test.py:70-71) accumulated in float64 like the reference
//   (its ground-truth image is float64).
// Integer / byte work is exact: the rank of a masked pixel is its exclusive prefix count over the mask.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include <climits>

#define IMG_THREADS 256

// per-block popcount of the mask
__global__ void __launch_bounds__(IMG_THREADS) k_img_count(const uint8_t* __restrict__ mask, int n, int32_t* __restrict__ counts) {
    const int i = blockIdx.x * IMG_THREADS + threadIdx.x;
    const bool m = i < n && mask[i] != 0;
    const unsigned long long b = __ballot(m);
    __shared__ int s[IMG_THREADS / 64];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

// exclusive scan of the block counts (single workgroup, chunks of 1024 with a carry)
__global__ void __launch_bounds__(1024) k_img_scan(int32_t* __restrict__ counts, int nblocks) {
    __shared__ int s[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nblocks ? counts[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int t = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nblocks) counts[i] = carry + s[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += s[1023];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(IMG_THREADS) k_img_scatter(const float* __restrict__ rgb, const float* __restrict__ disp,
                                                              const float* __restrict__ acc, const float* __restrict__ depth,
                                                              int R, const uint8_t* __restrict__ mask, int n,
                                                              const int32_t* __restrict__ offs, int clamp_rgb,
                                                              float* __restrict__ img_rgb, float* __restrict__ img_disp,
                                                              float* __restrict__ img_acc, float* __restrict__ img_depth) {
    const int i = blockIdx.x * IMG_THREADS + threadIdx.x;
    const bool m = i < n && mask[i] != 0;
    const unsigned long long b = __ballot(m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int s[IMG_THREADS / 64];
    if (lane == 0) s[wave] = __popcll(b);
    __syncthreads();
    int before = offs[blockIdx.x];
    for (int w = 0; w < wave; ++w) before += s[w];
    const int rank = before + __popcll(b & ((1ull << lane) - 1ull));
    if (i >= n) return;
    const bool take = m && rank < R;
    float c[3] = {0.f, 0.f, 0.f};
    if (take) {
        for (int k = 0; k < 3; ++k) {
            float v = rgb[3 * rank + k];
            if (clamp_rgb) v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);   // torch.clamp keeps NaN; so does this
            c[k] = v;
        }
    }
    for (int k = 0; k < 3; ++k) img_rgb[3 * i + k] = c[k];
    if (img_disp) img_disp[i] = take ? disp[rank] : 0.0f;
    if (img_acc) img_acc[i] = take ? acc[rank] : 0.0f;
    if (img_depth) img_depth[i] = take ? depth[rank] : 0.0f;
}

// sums of squared differences: out[0] over all pixels, out[1] over masked pixels, out[2] number of masked pixels
__global__ void __launch_bounds__(IMG_THREADS) k_img_sqerr(const float* __restrict__ img, const double* __restrict__ gt64,
                                                            const float* __restrict__ gt32, const uint8_t* __restrict__ mask,
                                                            int n, double* __restrict__ sums) {
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = blockIdx.x * IMG_THREADS + threadIdx.x; i < n; i += gridDim.x * IMG_THREADS) {
        double e = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double g = gt64 ? gt64[3 * i + k] : (double)gt32[3 * i + k];
            const double d = (double)img[3 * i + k] - g;
            e += d * d;
        }
        a += e;
        if (mask && mask[i]) { b += e; c += 1.0; }
    }
    __shared__ double s[3][IMG_THREADS];
    s[0][threadIdx.x] = a; s[1][threadIdx.x] = b; s[2][threadIdx.x] = c;
    __syncthreads();
    for (int off = IMG_THREADS / 2; off >= 1; off >>= 1) {
        if (threadIdx.x < off)
            for (int k = 0; k < 3; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) atomicAdd(sums + k, s[k][0]);
}

// out4 = {mse_all, mse_masked, psnr_all, psnr_masked}   (metrics.py:8-21)
__global__ void k_img_psnr(const double* __restrict__ sums, int n, double* __restrict__ out4) {
    const double mse_all = sums[0] / (3.0 * (double)n);
    const double mse_m = sums[1] / (3.0 * sums[2]);
    out4[0] = mse_all;
    out4[1] = mse_m;
    out4[2] = -10.0 * log10(mse_all);
    out4[3] = -10.0 * log10(mse_m);
}

size_t dsn_image_workspace_size(int H, int W) {
    const size_t nblocks = ((size_t)H * W + IMG_THREADS - 1) / IMG_THREADS;
    return dsn_align256(sizeof(int32_t) * nblocks) + 256;
}

void dsn_launch_image_scatter(const float* rgb, const float* disp, const float* acc, const float* depth, int R,
                              const uint8_t* mask, int H, int W, int clamp_rgb, float* img_rgb, float* img_disp,
                              float* img_acc, float* img_depth, void* workspace, hipStream_t st) {
    const int n = H * W;
    const int nblocks = (n + IMG_THREADS - 1) / IMG_THREADS;
    int32_t* counts = (int32_t*)workspace;
    hipLaunchKernelGGL(k_img_count, dim3(nblocks), dim3(IMG_THREADS), 0, st, mask, n, counts);
    hipLaunchKernelGGL(k_img_scan, dim3(1), dim3(1024), 0, st, counts, nblocks);
    hipLaunchKernelGGL(k_img_scatter, dim3(nblocks), dim3(IMG_THREADS), 0, st, rgb, disp, acc, depth, R, mask, n, counts,
                       clamp_rgb, img_rgb, img_disp, img_acc, img_depth);
}

void dsn_launch_image_psnr(const float* img_rgb, const double* gt64, const float* gt32, const uint8_t* mask, int H, int W,
                           double* out4, void* workspace, hipStream_t st) {
    const int n = H * W;
    double* sums = (double*)((char*)workspace + dsn_image_workspace_size(H, W) - 256);
    (void)hipMemsetAsync(sums, 0, 3 * sizeof(double), st);
    int blocks = (n + IMG_THREADS - 1) / IMG_THREADS;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_img_sqerr, dim3(blocks), dim3(IMG_THREADS), 0, st, img_rgb, gt64, gt32, mask, n, sums);
    hipLaunchKernelGGL(k_img_psnr, dim3(1), dim3(1), 0, st, sums, n, out4);
}

// ---- SSIM: metrics.py:23-38 ssim_metric = scikit-image 0.15 compare_ssim(pred, gt, multichannel=True) ---------------------
// on the float64 images that are zero outside mask_at_box, cropped to cv2.boundingRect(mask).  Per channel: 7 x 7 uniform
// window, data range 2 (float64's dtype range (-1, 1)), sample covariance (49/48); the channel value is the mean of S over the
// crop without its 3-pixel border (the centres of whole windows only, so the filter's border mode never enters); the result
// is the mean over the three channels.  A crop side below 7 (an empty mask included) has no value: status, NaN.
// Three launches, no host synchronisation and no atomics: row-band partial rectangles (integer min / max), one workgroup
// per output tile (staged with its halo in LDS, window sums and S in fp64, one partial per channel), one workgroup per frame
// summing its tiles' partials in tile order.  Every partial depends on its own frame only: a frame's value is the same bits
// in any batch and on every call.
#define SSIM_TH 16                      // output tile: rows
#define SSIM_TW 32                      //              columns
#define SSIM_HH (SSIM_TH + 6)           // staged tile: the output tile and its 3-pixel halo
#define SSIM_HW (SSIM_TW + 6)
#define SSIM_THREADS 256
#define SSIM_BANDS 64                   // row bands of the rectangle kernel (H of them when H < 64)

static int ssim_bands(int H) { return H < SSIM_BANDS ? H : SSIM_BANDS; }
static int ssim_tiles_x(int W) { return (W + SSIM_TW - 1) / SSIM_TW; }
static int ssim_tiles_y(int H) { return (H + SSIM_TH - 1) / SSIM_TH; }

// per (frame, band) {xmin, xmax, ymin, ymax} of the set mask pixels; {INT_MAX, -1, INT_MAX, -1} for a band without any
__global__ void __launch_bounds__(SSIM_THREADS) k_ssim_rect(const uint8_t* __restrict__ mask, int H, int W, int4* __restrict__ rect_part) {
    const int band = blockIdx.x, nb = gridDim.x, f = blockIdx.y;
    const int y0 = (int)((long long)band * H / nb), y1 = (int)((long long)(band + 1) * H / nb);
    const uint8_t* m = mask + (size_t)f * H * W;
    int xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
    for (int y = y0; y < y1; ++y)
        for (int x = threadIdx.x; x < W; x += SSIM_THREADS)
            if (m[(size_t)y * W + x]) {
                xmin = min(xmin, x); xmax = max(xmax, x);
                ymin = min(ymin, y); ymax = max(ymax, y);
            }
    for (int o = 32; o >= 1; o >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, o)); xmax = max(xmax, __shfl_xor(xmax, o));
        ymin = min(ymin, __shfl_xor(ymin, o)); ymax = max(ymax, __shfl_xor(ymax, o));
    }
    __shared__ int4 s[SSIM_THREADS / 64];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = make_int4(xmin, xmax, ymin, ymax);
    __syncthreads();
    if (threadIdx.x == 0) {
        int4 r = s[0];
        for (int w = 1; w < SSIM_THREADS / 64; ++w) {
            r.x = min(r.x, s[w].x); r.y = max(r.y, s[w].y); r.z = min(r.z, s[w].z); r.w = max(r.w, s[w].w);
        }
        rect_part[(size_t)f * SSIM_BANDS + band] = r;
    }
}

// the frame's cv2.boundingRect {x, y, w, h} ({0, 0, 0, 0} for an empty mask) from its band partials; called by whole waves
// (each wave reduces on its own, so the value is wave-uniform without LDS or a barrier)
__device__ inline int4 ssim_frame_rect(const int4* __restrict__ part, int nb) {
    const int l = threadIdx.x & 63;
    int4 v = l < nb ? part[l] : make_int4(INT_MAX, -1, INT_MAX, -1);
    for (int o = 32; o >= 1; o >>= 1) {
        v.x = min(v.x, __shfl_xor(v.x, o)); v.y = max(v.y, __shfl_xor(v.y, o));
        v.z = min(v.z, __shfl_xor(v.z, o)); v.w = max(v.w, __shfl_xor(v.w, o));
    }
    if (v.y < 0) return make_int4(0, 0, 0, 0);
    return make_int4(v.x, v.z, v.y - v.x + 1, v.w - v.z + 1);
}

// one workgroup per (tile, frame): sum over the tile's outputs inside the crop interior of S, per channel -> part[f][tile][3]
__global__ void __launch_bounds__(SSIM_THREADS) k_ssim_tile(const float* __restrict__ img, const double* __restrict__ gt64,
                                                             const float* __restrict__ gt32, const uint8_t* __restrict__ mask,
                                                             int H, int W, int clamp_rgb, const int4* __restrict__ rect_part, int nb,
                                                             double* __restrict__ part) {
    const int f = blockIdx.z;
    const int4 r = ssim_frame_rect(rect_part + (size_t)f * SSIM_BANDS, nb);
    // the crop interior [iy0, iy1) x [ix0, ix1): the centres of whole 7 x 7 windows
    const int iy0 = r.y + 3, iy1 = r.y + r.w - 3, ix0 = r.x + 3, ix1 = r.x + r.z - 3;
    const int ty0 = blockIdx.y * SSIM_TH, tx0 = blockIdx.x * SSIM_TW;
    if (r.z < 7 || r.w < 7 || ty0 >= iy1 || ty0 + SSIM_TH <= iy0 || tx0 >= ix1 || tx0 + SSIM_TW <= ix0) return;

    __shared__ float sx[3][SSIM_HH * SSIM_HW];       // pred (float32, optionally clamped), zero outside the mask
    __shared__ double sy[3][SSIM_HH * SSIM_HW];      // gt, zero outside the mask
    __shared__ double sv[5][SSIM_TH * SSIM_HW];      // vertical 7-sums of x, y, x^2, y^2, xy (then the block reduction)
    const uint8_t* m = mask + (size_t)f * H * W;
    const size_t base = (size_t)f * H * W * 3;
    for (int p = threadIdx.x; p < SSIM_HH * SSIM_HW; p += SSIM_THREADS) {
        const int gy = ty0 - 3 + p / SSIM_HW, gx = tx0 - 3 + p % SSIM_HW;
        float x[3] = {0.f, 0.f, 0.f};
        double y[3] = {0.0, 0.0, 0.0};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t i = (size_t)gy * W + gx;
            if (m[i]) {
                for (int k = 0; k < 3; ++k) {
                    float v = img[base + 3 * i + k];
                    if (clamp_rgb) v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);   // torch.clamp keeps NaN; so does this
                    x[k] = v;
                    y[k] = gt64 ? gt64[base + 3 * i + k] : (double)gt32[base + 3 * i + k];
                }
            }
        }
        for (int k = 0; k < 3; ++k) { sx[k][p] = x[k]; sy[k][p] = y[k]; }
    }
    __syncthreads();

    const double C1 = (0.01 * 2.0) * (0.01 * 2.0), C2 = (0.03 * 2.0) * (0.03 * 2.0), cov = 49.0 / 48.0;
    double acc[3];
    for (int c = 0; c < 3; ++c) {
        for (int q = threadIdx.x; q < SSIM_TH * SSIM_HW; q += SSIM_THREADS) {
            const int rr = q / SSIM_HW, cc = q % SSIM_HW;
            double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
            for (int k = 0; k < 7; ++k) {
                const double xv = sx[c][(rr + k) * SSIM_HW + cc], yv = sy[c][(rr + k) * SSIM_HW + cc];
                a += xv; b += yv; aa += xv * xv; bb += yv * yv; ab += xv * yv;
            }
            sv[0][q] = a; sv[1][q] = b; sv[2][q] = aa; sv[3][q] = bb; sv[4][q] = ab;
        }
        __syncthreads();
        double t = 0.0;
        for (int q = threadIdx.x; q < SSIM_TH * SSIM_TW; q += SSIM_THREADS) {
            const int rr = q / SSIM_TW, cc = q % SSIM_TW;
            const int gy = ty0 + rr, gx = tx0 + cc;
            if (gy < iy0 || gy >= iy1 || gx < ix0 || gx >= ix1) continue;
            double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (int k = 0; k < 7; ++k)
                for (int j = 0; j < 5; ++j) s[j] += sv[j][rr * SSIM_HW + cc + k];
            const double ux = s[0] / 49.0, uy = s[1] / 49.0, uxx = s[2] / 49.0, uyy = s[3] / 49.0, uxy = s[4] / 49.0;
            const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
            t += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
        }
        acc[c] = t;
        __syncthreads();                               // sv is rewritten by the next channel / the reduction
    }
    double* red = &sv[0][0];                           // [3][SSIM_THREADS]
    for (int c = 0; c < 3; ++c) red[c * SSIM_THREADS + threadIdx.x] = acc[c];
    __syncthreads();
    for (int off = SSIM_THREADS / 2; off >= 1; off >>= 1) {
        if (threadIdx.x < off)
            for (int c = 0; c < 3; ++c) red[c * SSIM_THREADS + threadIdx.x] += red[c * SSIM_THREADS + threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        const size_t tile = ((size_t)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[tile * 3 + threadIdx.x] = red[threadIdx.x * SSIM_THREADS];
    }
}

// one workgroup per frame: the tiles that met the crop interior (exactly those k_ssim_tile did not leave early), in tile order
__global__ void __launch_bounds__(SSIM_THREADS) k_ssim_finish(const int4* __restrict__ rect_part, int nb, const double* __restrict__ part,
                                                               int ntx, int nty, double* __restrict__ out_ssim,
                                                               int32_t* __restrict__ out_rect, int32_t* __restrict__ out_status) {
    const int f = blockIdx.x;
    const int4 r = ssim_frame_rect(rect_part + (size_t)f * SSIM_BANDS, nb);
    const int status = r.z == 0 ? DSN_SSIM_EMPTY_MASK : (r.z < 7 || r.w < 7 ? DSN_SSIM_CROP_TOO_SMALL : DSN_SSIM_OK);
    __shared__ double s[SSIM_THREADS];
    double t = 0.0;
    if (status == DSN_SSIM_OK) {
        const int iy0 = r.y + 3, iy1 = r.y + r.w - 3, ix0 = r.x + 3, ix1 = r.x + r.z - 3;
        const int bx0 = ix0 / SSIM_TW, nbx = (ix1 - 1) / SSIM_TW - bx0 + 1;
        const int by0 = iy0 / SSIM_TH, nby = (iy1 - 1) / SSIM_TH - by0 + 1;
        for (int k = threadIdx.x; k < nbx * nby; k += SSIM_THREADS) {
            const double* p = part + (((size_t)f * nty + by0 + k / nbx) * ntx + bx0 + k % nbx) * 3;
            t += p[0] + p[1] + p[2];
        }
    }
    s[threadIdx.x] = t;
    __syncthreads();
    for (int off = SSIM_THREADS / 2; off >= 1; off >>= 1) {
        if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out_ssim[f] = status == DSN_SSIM_OK ? s[0] / (3.0 * (double)(r.z - 6) * (double)(r.w - 6)) : __builtin_nan("");
        out_rect[4 * f + 0] = r.x; out_rect[4 * f + 1] = r.y; out_rect[4 * f + 2] = r.z; out_rect[4 * f + 3] = r.w;
        out_status[f] = status;
    }
}

size_t dsn_image_ssim_workspace_size(int F, int H, int W) {
    return dsn_align256(sizeof(int4) * SSIM_BANDS * (size_t)F) +
           dsn_align256(sizeof(double) * 3 * (size_t)F * ssim_tiles_x(W) * ssim_tiles_y(H));
}

void dsn_launch_image_ssim(const float* img_rgb, const double* gt64, const float* gt32, const uint8_t* mask, int F, int H, int W,
                           int clamp_rgb, double* out_ssim, int32_t* out_rect, int32_t* out_status, void* workspace, hipStream_t st) {
    int4* rect_part = (int4*)workspace;
    double* part = (double*)((char*)workspace + dsn_align256(sizeof(int4) * SSIM_BANDS * (size_t)F));
    const int nb = ssim_bands(H), ntx = ssim_tiles_x(W), nty = ssim_tiles_y(H);
    hipLaunchKernelGGL(k_ssim_rect, dim3(nb, F), dim3(SSIM_THREADS), 0, st, mask, H, W, rect_part);
    hipLaunchKernelGGL(k_ssim_tile, dim3(ntx, nty, F), dim3(SSIM_THREADS), 0, st, img_rgb, gt64, gt32, mask, H, W, clamp_rgb,
                       rect_part, nb, part);
    hipLaunchKernelGGL(k_ssim_finish, dim3(F), dim3(SSIM_THREADS), 0, st, rect_part, nb, part, ntx, nty, out_ssim, out_rect,
                       out_status);
}
