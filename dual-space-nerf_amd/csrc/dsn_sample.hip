// dsn_sample.hip - a training batch drawn on the device (dsn_train_rays / dsn_bound_mask; the rule is in include/dsnerf.h):
// utils/rays_utils.py:104-172 my_sample_ray and utils/h36m_utils.py:78-146 sample_ray_h36m without the host.
//   classes : one thread per pixel - the box mask (six integer polygon tests inside the corners' bounding rectangle, or the caller's
//             mask), the three class predicates as 64-pixel ballot words, per-tile counts (TS_TILE pixels = 4 words);
//   scan    : one workgroup, the tiles' counts -> exclusive prefixes per class, [tiles] = the class total;
//   draw    : round 0, one thread per slot: hash -> list entry -> rank-select (binary search over the tile prefixes, popcount select
//             inside the tile's words) -> the pixel's ray and box test (dsn_rays.h);
//   finish  : one workgroup compacts round 0 in slot order (workgroup scan), then runs the later rounds - a small remainder - in a
//             loop inside the kernel, and writes the status word and the round count;
//   gather  : one thread per ray of the batch: the pixel's ray again (the same text: dsn_camera_rays' bits), rgb, occupancy, coord.
// No atomics, nothing read back by the host, nothing whose order depends on arrival.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include "dsn_rays.h"

#define TS_TILE 256            // pixels per tile = threads of the class kernel = 4 ballot words
#define TS_WORDS 4
#define TS_WG 1024             // threads of the one-workgroup kernels
#define TS_CORNER_LIMIT ((int64_t)1 << 29)     // |rounded corner| below this: every cross product below stays inside int64
static_assert(TS_TILE == 64 * TS_WORDS, "a tile is whole ballot words");

static int64_t ts_tiles(int64_t hw) { return (hw + TS_TILE - 1) / TS_TILE; }
static size_t ts_up(size_t n) { return (n + 255) / 256 * 256; }
// info int32 [64] ([0] camera usable, [1] rays accepted) | words uint64 [3][tiles * 4] | prefix int32 [3][tiles + 1] |
// cand int32 [nrays] | sel int32 [nrays]
struct TsWs { int32_t* info; unsigned long long* words; int32_t* prefix; int32_t* cand; int32_t* sel; size_t bytes; };
static TsWs ts_ws(void* ws, int64_t hw, int nrays) {
    const int64_t tiles = ts_tiles(hw);
    char* p = (char*)ws;
    size_t o = 0;
    TsWs r;
    r.info = (int32_t*)(p + o); o += 256;
    r.words = (unsigned long long*)(p + o); o += ts_up((size_t)8 * 3 * tiles * TS_WORDS);
    r.prefix = (int32_t*)(p + o); o += ts_up((size_t)4 * 3 * (tiles + 1));
    r.cand = (int32_t*)(p + o); o += ts_up((size_t)4 * nrays);
    r.sel = (int32_t*)(p + o); o += ts_up((size_t)4 * nrays);
    r.bytes = o;
    return r;
}
size_t dsn_train_rays_workspace_size(int64_t hw, int nrays) { return ts_ws(nullptr, hw, nrays).bytes; }

// ---- the box mask ------------------------------------------------------------------------------------------------------------
// s_c[16] = the eight rounded corners (x, y), s_c[16..19] = their bounding rectangle cut to the image (x0, y0, x1, y1, inclusive),
// s_c[20] = 1 when every corner is usable.  Threads 0..7 project; the caller synchronises after the call.
__device__ __forceinline__ void ts_corners(const double* __restrict__ K, const double* __restrict__ Rm, const double* __restrict__ T,
                                           const double* __restrict__ bounds, int H, int W, int64_t* s_c) {
    const int t = threadIdx.x;
    if (t < 8) {   // get_bound_corners' order: x from bit 2, y from bit 1, z from bit 0
        const double x = bounds[(t & 4) ? 3 : 0], y = bounds[(t & 2) ? 4 : 1], z = bounds[(t & 1) ? 5 : 2];
        double cam[3], pix[3];
        for (int c = 0; c < 3; ++c) cam[c] = ((x * Rm[3 * c] + y * Rm[3 * c + 1]) + z * Rm[3 * c + 2]) + T[c];
        for (int c = 0; c < 3; ++c) pix[c] = (cam[0] * K[3 * c] + cam[1] * K[3 * c + 1]) + cam[2] * K[3 * c + 2];
        const double u = rint(pix[0] / pix[2]), v = rint(pix[1] / pix[2]);      // np.round: half to even
        const double lim = (double)TS_CORNER_LIMIT;
        const bool ok = pix[2] > 0.0 && cam[2] > 0.0 && u > -lim && u < lim && v > -lim && v < lim;    // (NaN fails every comparison)
        s_c[2 * t] = ok ? (int64_t)u : 0;
        s_c[2 * t + 1] = ok ? (int64_t)v : 0;
        s_c[24 + t] = ok ? 1 : 0;
    }
    __syncthreads();
    if (t == 0) {
        int64_t x0 = s_c[0], x1 = s_c[0], y0 = s_c[1], y1 = s_c[1], ok = 1;
        for (int k = 0; k < 8; ++k) {
            const int64_t cx = s_c[2 * k], cy = s_c[2 * k + 1];
            x0 = cx < x0 ? cx : x0; x1 = cx > x1 ? cx : x1;
            y0 = cy < y0 ? cy : y0; y1 = cy > y1 ? cy : y1;
            ok &= s_c[24 + k];
        }
        s_c[16] = x0 > 0 ? x0 : 0; s_c[17] = y0 > 0 ? y0 : 0;
        s_c[18] = x1 < W - 1 ? x1 : W - 1; s_c[19] = y1 < H - 1 ? y1 : H - 1;
        s_c[20] = ok;
    }
}
#define TS_CORNER_WORDS 32

// pixel (x, y) against one loop: on one of its segments, or winding number non-zero; exact in int64
__device__ __forceinline__ bool ts_in_loop(const int64_t* s_c, const int* idx, int n, int64_t x, int64_t y) {
    int wn = 0;
    bool on = false;
    for (int e = 0; e < n; ++e) {
        const int a = idx[e], b = idx[e + 1 == n ? 0 : e + 1];
        const int64_t ax = s_c[2 * a], ay = s_c[2 * a + 1], bx = s_c[2 * b], by = s_c[2 * b + 1];
        const int64_t cross = (bx - ax) * (y - ay) - (by - ay) * (x - ax);
        const int64_t lx = ax < bx ? ax : bx, hx = ax < bx ? bx : ax, ly = ay < by ? ay : by, hy = ay < by ? by : ay;
        on = on || (cross == 0 && x >= lx && x <= hx && y >= ly && y <= hy);
        if (ay <= y) { if (by > y && cross > 0) ++wn; }
        else if (by <= y && cross < 0) --wn;
    }
    return on || wn != 0;
}
// the union of the six loops as the reference writes them (the second keeps its closing typo: triangle 5-7-6 plus segment 4-5)
__device__ __forceinline__ bool ts_box_pixel(const int64_t* s_c, int64_t x, int64_t y) {
    if (!s_c[20] || x < s_c[16] || x > s_c[18] || y < s_c[17] || y > s_c[19]) return false;
    const int l0[4] = {0, 1, 3, 2}, l1[5] = {4, 5, 7, 6, 5}, l2[4] = {0, 1, 5, 4}, l3[4] = {2, 3, 7, 6}, l4[4] = {0, 2, 6, 4},
              l5[4] = {1, 3, 7, 5};
    return ts_in_loop(s_c, l0, 4, x, y) || ts_in_loop(s_c, l1, 5, x, y) || ts_in_loop(s_c, l2, 4, x, y) ||
           ts_in_loop(s_c, l3, 4, x, y) || ts_in_loop(s_c, l4, 4, x, y) || ts_in_loop(s_c, l5, 4, x, y);
}

__global__ void __launch_bounds__(TS_TILE) k_ts_bound_mask(const double* __restrict__ K, const double* __restrict__ Rm,
                                                            const double* __restrict__ T, const double* __restrict__ bounds, int H, int W,
                                                            uint8_t* __restrict__ mask_out) {
    __shared__ int64_t s_c[TS_CORNER_WORDS];
    ts_corners(K, Rm, T, bounds, H, W, s_c);
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * TS_TILE + threadIdx.x;
    if (p < (int64_t)H * W) mask_out[p] = ts_box_pixel(s_c, p % W, p / W) ? 1 : 0;
}

// ---- classes -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TS_TILE) k_ts_classes(const double* __restrict__ K, const double* __restrict__ Rm,
                                                         const double* __restrict__ T, const double* __restrict__ bounds, int H, int W,
                                                         int convention, const uint8_t* __restrict__ mask_a,
                                                         const uint8_t* __restrict__ mask_b, const uint8_t* __restrict__ bound_in,
                                                         uint8_t* __restrict__ mask_out, int64_t tiles,
                                                         unsigned long long* __restrict__ words, int32_t* __restrict__ prefix,
                                                         int32_t* __restrict__ info) {
    __shared__ int64_t s_c[TS_CORNER_WORDS];
    __shared__ int s_n[3][TS_WORDS];
    if (!bound_in) {
        ts_corners(K, Rm, T, bounds, H, W, s_c);
        __syncthreads();
    }
    const int64_t p = (int64_t)blockIdx.x * TS_TILE + threadIdx.x;
    const bool in = p < (int64_t)H * W;
    uint8_t b = 0, a = 0, a2 = 0;
    if (in) {
        b = bound_in ? bound_in[p] : (ts_box_pixel(s_c, p % W, p / W) ? 1 : 0);
        mask_out[p] = b;
        a = mask_a[p];
        a2 = mask_b ? mask_b[p] : 0;
    }
    const bool b1 = b == 1;
    bool cls[3];
    if (convention == DSN_RAYS_H36M) { cls[0] = in && b1 && a == 1; cls[1] = in && a2 == 2; cls[2] = in && b1 && a != 100; }
    else { cls[0] = in && a != 0; cls[1] = in && a == 2; cls[2] = in && b1; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long w = __ballot(cls[c]);
        if (lane == 0) {
            words[((int64_t)c * tiles + blockIdx.x) * TS_WORDS + wave] = w;
            s_n[c][wave] = __popcll(w);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        prefix[(int64_t)c * (tiles + 1) + blockIdx.x] = (s_n[c][0] + s_n[c][1]) + (s_n[c][2] + s_n[c][3]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = bound_in ? 1 : (int32_t)s_c[20];
}

// exclusive scan of v over the workgroup in thread order (every thread calls); total = the sum
__device__ __forceinline__ int ts_block_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    __syncthreads();          // (the previous call's readers are done with s_w)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int i = 0; i < nw; ++i) { const int t = s_w[i]; if (i < wave) base += t; total += t; }
    return base + inc - v;
}

// one workgroup: the tiles' counts of each class -> exclusive prefixes in place, [tiles] = the class total
__global__ void __launch_bounds__(TS_WG) k_ts_scan(int32_t* __restrict__ prefix, int64_t tiles) {
    __shared__ int s_w[TS_WG / 64];
    const int64_t per = (tiles + TS_WG - 1) / TS_WG;
    const int64_t b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < tiles ? b0 + per : tiles;
    for (int c = 0; c < 3; ++c) {
        int32_t* pc = prefix + (int64_t)c * (tiles + 1);
        int sum = 0;
        for (int64_t k = b0; k < b1; ++k) sum += pc[k];
        int total;
        int run = ts_block_scan(sum, s_w, total);
        for (int64_t k = b0; k < b1; ++k) { const int n = pc[k]; pc[k] = run; run += n; }
        if (threadIdx.x == 0) pc[tiles] = total;
    }
}

// ---- draws -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ts_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
// the header's h(seed, r, c, k)
__device__ __forceinline__ uint32_t ts_hash(uint32_t seed, int r, int c, uint32_t k) {
    return ts_mix(ts_mix(seed + 0x9E3779B9u * (uint32_t)(3 * r + c)) ^ k);
}
// pixel of entry `rank` (0-based, < the class total) of class c's row-major list
__device__ __forceinline__ int ts_select(const unsigned long long* __restrict__ words, const int32_t* __restrict__ prefix, int64_t tiles,
                                         int c, int rank) {
    const int32_t* pc = prefix + (int64_t)c * (tiles + 1);
    int64_t lo = 0, hi = tiles - 1;          // the last tile whose prefix is <= rank (tiles of count 0 share a prefix: the last one wins,
    while (lo < hi) {                        //  and only the last of them can hold the entry)
        const int64_t mid = (lo + hi + 1) >> 1;
        if (pc[mid] <= rank) lo = mid; else hi = mid - 1;
    }
    int n = rank - pc[lo];
    const unsigned long long* w = words + ((int64_t)c * tiles + lo) * TS_WORDS;
    int word = 0;
    unsigned long long bits = w[0];
    for (; word < TS_WORDS - 1; ++word) {
        const int pcnt = __popcll(bits);
        if (n < pcnt) break;
        n -= pcnt;
        bits = w[word + 1];
    }
    int pos = 0;                              // the n-th set bit of `bits`
    for (int sh = 32; sh; sh >>= 1) {
        const unsigned long long low = bits & ((1ull << sh) - 1);
        const int pcnt = __popcll(low);
        if (n >= pcnt) { n -= pcnt; bits >>= sh; pos += sh; } else bits = low;
    }
    return (int)(lo * TS_TILE + word * 64 + pos);      // (a set bit: a pixel of the image)
}

struct TsRound { int n_body, n_face, n_rand, draws; };
__device__ __forceinline__ TsRound ts_round(int rem, int face_count) {
    TsRound q;
    q.n_body = rem * 6 / 10;
    const int nf = rem * 5 / 100;
    q.n_rand = rem - q.n_body - nf;
    q.n_face = face_count > 0 ? nf : 0;       // an empty face class leaves its draws out of the round
    q.draws = q.n_body + q.n_face + q.n_rand;
    return q;
}
struct TsDrawArgs {
    const double *K, *R, *T, *bounds;
    int W, convention, hw;
    uint32_t seed;
    const unsigned long long* words;
    const int32_t* prefix;
    int64_t tiles;
};
// slot of round r: its pixel when the ray passes the convention's box test, -1 otherwise
__device__ __forceinline__ int ts_draw(const TsDrawArgs& a, const TsRound& q, const int count[3], int r, int slot) {
    int c = 0, k = slot;
    if (slot >= q.n_body + q.n_face) { c = 2; k = slot - q.n_body - q.n_face; }
    else if (slot >= q.n_body) { c = 1; k = slot - q.n_body; }
    const int rank = (int)(((unsigned long long)ts_hash(a.seed, r, c, (uint32_t)k) * (unsigned long long)count[c]) >> 32);
    int p = ts_select(a.words, a.prefix, a.tiles, c, rank);
    p = p < a.hw ? p : a.hw - 1;               // (never taken: the words hold no bit beyond the image)
    const DsnPixelRay ray = a.convention == DSN_RAYS_H36M ? dsn_pixel_ray_h36m(a.K, a.R, a.T, a.bounds, a.W, p)
                                                           : dsn_pixel_ray_zju(a.K, a.R, a.T, a.bounds, a.W, p);
    return ray.hit ? p : -1;
}

__global__ void __launch_bounds__(256) k_ts_draw0(TsDrawArgs a, int nrays, const int32_t* __restrict__ info, int32_t* __restrict__ cand) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= nrays) return;
    int count[3];
    for (int c = 0; c < 3; ++c) count[c] = a.prefix[(int64_t)c * (a.tiles + 1) + a.tiles];
    int v = -1;
    if (info[0] && count[0] > 0 && count[2] > 0) {
        const TsRound q = ts_round(nrays, count[1]);
        if (slot < q.draws) v = ts_draw(a, q, count, 0, slot);
    }
    cand[slot] = v;
}

__global__ void __launch_bounds__(TS_WG) k_ts_finish(TsDrawArgs a, int nrays, int32_t* __restrict__ info, const int32_t* __restrict__ cand,
                                                      int32_t* __restrict__ sel, int32_t* __restrict__ status, int32_t* __restrict__ rounds) {
    __shared__ int s_w[TS_WG / 64];
    int count[3];
    for (int c = 0; c < 3; ++c) count[c] = a.prefix[(int64_t)c * (a.tiles + 1) + a.tiles];
    const int cam_ok = info[0];
    if (!cam_ok || count[0] <= 0 || count[2] <= 0) {          // (uniform: every thread leaves)
        if (threadIdx.x == 0) { *status = cam_ok ? DSN_TRAIN_RAYS_EMPTY_CLASS : DSN_TRAIN_RAYS_BAD_CAMERA; *rounds = 0; info[1] = 0; }
        return;
    }
    int got = 0, r = 0;
    for (; got < nrays && r < DSN_TRAIN_RAYS_MAX_ROUNDS; ++r) {
        const TsRound q = ts_round(nrays - got, count[1]);
        const int draws = r == 0 ? nrays : q.draws;            // (round 0: the draw kernel's slots; those beyond q.draws hold -1)
        for (int base = 0; base < draws; base += TS_WG) {
            const int slot = base + threadIdx.x;
            int p = -1;
            if (slot < draws) p = r == 0 ? cand[slot] : ts_draw(a, q, count, r, slot);
            int total;
            const int pos = ts_block_scan(p >= 0 ? 1 : 0, s_w, total);
            if (p >= 0) sel[got + pos] = p;
            got += total;
        }
    }
    if (threadIdx.x == 0) { *status = got == nrays ? DSN_TRAIN_RAYS_OK : DSN_TRAIN_RAYS_SHORT; *rounds = r; info[1] = got; }
}

__global__ void __launch_bounds__(256) k_ts_gather(TsDrawArgs a, int nrays, const int32_t* __restrict__ info, const int32_t* __restrict__ sel,
                                                    const double* __restrict__ img64, const float* __restrict__ img32,
                                                    const uint8_t* __restrict__ bound, const uint8_t* __restrict__ occ_src,
                                                    float* __restrict__ ray_o, float* __restrict__ ray_d, float* __restrict__ near,
                                                    float* __restrict__ far, int64_t* __restrict__ coord, float* __restrict__ rgb,
                                                    uint8_t* __restrict__ occupancy, uint8_t* __restrict__ mask_at_box) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nrays) return;
    if (i >= info[1]) {          // a batch that came up short (status says so): zeros behind what was accepted
        for (int c = 0; c < 3; ++c) { ray_o[3 * i + c] = 0.f; ray_d[3 * i + c] = 0.f; rgb[3 * i + c] = 0.f; }
        near[i] = 0.f; far[i] = 0.f; coord[2 * i] = 0; coord[2 * i + 1] = 0; mask_at_box[i] = 0;
        if (occupancy) occupancy[i] = 0;
        return;
    }
    const int p = sel[i];
    const DsnPixelRay ray = a.convention == DSN_RAYS_H36M ? dsn_pixel_ray_h36m(a.K, a.R, a.T, a.bounds, a.W, p)
                                                           : dsn_pixel_ray_zju(a.K, a.R, a.T, a.bounds, a.W, p);
    for (int c = 0; c < 3; ++c) { ray_o[3 * i + c] = ray.o[c]; ray_d[3 * i + c] = ray.d[c]; }
    near[i] = ray.near;
    far[i] = ray.far;
    coord[2 * i] = p / a.W;
    coord[2 * i + 1] = p % a.W;
    const bool keep = a.convention != DSN_RAYS_H36M || bound[p] == 1;      // h36m_utils.py:85: img[bound_mask != 1] = 0
    for (int c = 0; c < 3; ++c) {
        const float v = img64 ? (float)img64[(int64_t)3 * p + c] : img32[(int64_t)3 * p + c];
        rgb[3 * i + c] = keep ? v : 0.f;
    }
    if (occupancy) occupancy[i] = occ_src[p];
    mask_at_box[i] = 1;
}

void dsn_launch_bound_mask(const double* K, const double* R, const double* T, const double* bounds, int H, int W, uint8_t* mask_out,
                           hipStream_t st) {
    const int64_t tiles = ts_tiles((int64_t)H * W);
    hipLaunchKernelGGL(k_ts_bound_mask, dim3((unsigned)tiles), dim3(TS_TILE), 0, st, K, R, T, bounds, H, W, mask_out);
}

void dsn_launch_train_rays(const DsnTrainRaysArgs& g, hipStream_t st) {
    const int64_t hw = (int64_t)g.H * g.W, tiles = ts_tiles(hw);
    const TsWs w = ts_ws(g.workspace, hw, g.nrays);
    hipLaunchKernelGGL(k_ts_classes, dim3((unsigned)tiles), dim3(TS_TILE), 0, st, g.K, g.R, g.T, g.bounds, g.H, g.W, g.convention, g.mask_a,
                       g.mask_b, g.bound_in, g.bound_out, tiles, w.words, w.prefix, w.info);
    hipLaunchKernelGGL(k_ts_scan, dim3(1), dim3(TS_WG), 0, st, w.prefix, tiles);
    TsDrawArgs a;
    a.K = g.K; a.R = g.R; a.T = g.T; a.bounds = g.bounds; a.W = g.W; a.convention = g.convention; a.hw = (int)hw; a.seed = g.seed;
    a.words = w.words; a.prefix = w.prefix; a.tiles = tiles;
    const unsigned blocks = (unsigned)((g.nrays + 255) / 256);
    hipLaunchKernelGGL(k_ts_draw0, dim3(blocks), dim3(256), 0, st, a, g.nrays, w.info, w.cand);
    hipLaunchKernelGGL(k_ts_finish, dim3(1), dim3(TS_WG), 0, st, a, g.nrays, w.info, w.cand, w.sel, g.status, g.rounds);
    hipLaunchKernelGGL(k_ts_gather, dim3(blocks), dim3(256), 0, st, a, g.nrays, w.info, w.sel, g.img64, g.img32, g.bound_out, g.occ_src,
                       g.ray_o, g.ray_d, g.near, g.far, g.coord, g.rgb, g.occupancy, g.mask_at_box);
}
