// dsn_jpeg.hip - baseline JPEG on the device (dsn_jpeg_coefficients, dsn_jpeg_scan, dsn_jpeg_encode; the rule is in
// include/dsnerf.h and restated in tests/jpeg_restate.py).  Integer arithmetic throughout; the only atomics are 32-bit ORs into the
// cleared unstuffed stream and the frames' status words.
//   k_jpeg_zero_status : clears the frames' status words (k_jpeg_coef ORs DSN_JPEG_NONFINITE into them)
//   k_jpeg_coef    : a workgroup per MCU, a wave per block, a lane per sample -> int16 coef [F][block][64 zigzag], dummy DCs resolved
//   k_jpeg_bits    : a wave per block, a lane per coefficient -> the block's bit length
//   k_jpeg_tile / k_jpeg_tiles : the tile scan (per tile of JPEG_TILE entries, then one workgroup over a frame's tile totals)
//   k_jpeg_clear   : zeroes the words of the unstuffed stream the frame will use
//   k_jpeg_emit    : the lanes' words again, placed by the wave's prefix sum, OR-ed into the stream
//   k_jpeg_ffcount : 0xFF bytes per 16-byte chunk (the last byte padded with 1-bits first); tile scan again
//   k_jpeg_stuff   : header, the stuffed scan, EOI, length and status
// Frames lie side by side in blockIdx.y; nothing depends on F.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include "dsn_level.h"
#include <climits>

#define JPEG_TILE 1024            // entries per tile of the scan: 256 threads x 4
#define JPEG_SCAN_THREADS 256
#define JPEG_CHUNK 16             // bytes of the unstuffed stream per thread of the stuffing kernels

namespace {

// ---- tables of ITU-T T.81 Annex K ------------------------------------------------------------------------------------------------
constexpr uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                                 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                                 60, 61, 54, 47, 55, 62, 63};          // zigzag position -> natural index
constexpr uint8_t kQLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
                                51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121,
                                120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kAcVals[2][162] = {
    {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51,
     98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84,
     85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136,
     137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183,
     184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229,
     230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98,
     114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
     83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133,
     134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
     181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227,
     228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// a symbol's code in the low 16 bits, its length above: codes of each length count upwards, lengths ascending (Annex C)
struct JpegHuff { uint32_t dc[2][12]; uint32_t ac[2][256]; };
constexpr JpegHuff make_huff() {
    JpegHuff h{};
    for (int t = 0; t < 2; ++t) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kDcBits[t][len - 1]; ++i) h.dc[t][kDcVals[k++]] = (uint32_t)len << 16 | code++;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kAcBits[t][len - 1]; ++i) h.ac[t][kAcVals[t][k++]] = (uint32_t)len << 16 | code++;
            code <<= 1;
        }
    }
    return h;
}
__constant__ const JpegHuff c_huff = make_huff();
struct JpegZigzag { uint8_t z[64]; };
constexpr JpegZigzag make_zigzag() {
    JpegZigzag t{};
    for (int i = 0; i < 64; ++i) t.z[i] = kZigzag[i];
    return t;
}
__constant__ const JpegZigzag c_zigzag = make_zigzag();

struct JpegQuant { uint16_t d[2][64]; };            // 8 x the table entry, in ZIGZAG order: the divisor of coefficient slot i
struct JpegHeader { uint8_t b[DSN_JPEG_HEADER_MAX]; int len; };

struct JpegGeom {
    int H, W, mode, mw, mh, bpm, nb;                // MCU columns / rows, blocks per MCU, blocks per frame
    int tiles1;                                     // tiles of the block scan
    int chunks, tiles2;                             // 16-byte chunks of the unstuffed stream's capacity, tiles of their scan
    size_t stream_bytes;                            // capacity of a frame's unstuffed stream
};

bool jpeg_geom(int H, int W, int mode, JpegGeom& g) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || mode < DSN_JPEG_420 || mode > DSN_JPEG_GRAY) return false;
    const int s = mode == DSN_JPEG_420 ? 16 : 8;
    g.H = H; g.W = W; g.mode = mode;
    g.mw = (W + s - 1) / s; g.mh = (H + s - 1) / s;
    g.bpm = mode == DSN_JPEG_420 ? 6 : mode == DSN_JPEG_444 ? 3 : 1;
    const long long nb = (long long)g.mw * g.mh * g.bpm;
    if (nb * (DSN_JPEG_BLOCK_BYTES * 8) > (long long)INT_MAX) return false;
    g.nb = (int)nb;
    g.tiles1 = (g.nb + JPEG_TILE - 1) / JPEG_TILE;
    g.stream_bytes = (size_t)g.nb * DSN_JPEG_BLOCK_BYTES;          // a multiple of 16
    g.chunks = (int)(g.stream_bytes / JPEG_CHUNK);
    g.tiles2 = (g.chunks + JPEG_TILE - 1) / JPEG_TILE;
    return true;
}

void jpeg_quant_host(int quality, uint8_t tab[2][64]) {              // natural order
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = ((t ? kQChroma[i] : kQLuma[i]) * s + 50) / 100;
            tab[t][i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

int jpeg_header_host(const JpegGeom& g, int quality, uint8_t* o) {
    uint8_t tab[2][64];
    jpeg_quant_host(quality, tab);
    const int nc = g.mode == DSN_JPEG_GRAY ? 1 : 3, nt = nc == 1 ? 1 : 2;
    int n = 0;
    auto put = [&](int v) { o[n++] = (uint8_t)v; };
    auto seg = [&](int marker, int payload) { put(0xFF); put(marker); put((payload + 2) >> 8); put((payload + 2) & 255); };
    put(0xFF); put(0xD8);
    seg(0xE0, 14);
    for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);          // "JFIF\0" 1.01, units 0, 1 x 1, no thumbnail
    for (int t = 0; t < nt; ++t) {
        seg(0xDB, 65);
        put(t);
        for (int i = 0; i < 64; ++i) put(tab[t][kZigzag[i]]);
    }
    seg(0xC0, 6 + 3 * nc);
    put(8); put(g.H >> 8); put(g.H & 255); put(g.W >> 8); put(g.W & 255); put(nc);
    for (int c = 0; c < nc; ++c) { put(c + 1); put(c == 0 && g.mode == DSN_JPEG_420 ? 0x22 : 0x11); put(c ? 1 : 0); }
    for (int t = 0; t < nt; ++t) {
        seg(0xC4, 1 + 16 + 12);
        put(t);
        for (int i = 0; i < 16; ++i) put(kDcBits[t][i]);
        for (int i = 0; i < 12; ++i) put(kDcVals[i]);
        seg(0xC4, 1 + 16 + 162);
        put(0x10 | t);
        for (int i = 0; i < 16; ++i) put(kAcBits[t][i]);
        for (int i = 0; i < 162; ++i) put(kAcVals[t][i]);
    }
    seg(0xDA, 4 + 2 * nc);
    put(nc);
    for (int c = 0; c < nc; ++c) { put(c + 1); put(c ? 0x11 : 0x00); }
    put(0); put(63); put(0);
    return n;
}

// ---- coefficients ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int jpeg_level(const void* __restrict__ img, int dtype, size_t idx, float scale, bool& bad) {
    return dsn_image_level(img, dtype, idx, scale, bad);          // (dsn_level.h: shared with the PNG encoder)
}

__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of the IJG slow-integer forward DCT over d[0], d[stride], ..., in place
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct_pass(int* d, int stride) {
    const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride], d6 = d[6 * stride],
              d7 = d[7 * stride];
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? 11 : 15;
    d[0] = FIRST ? (t10 + t11) << 2 : jpeg_descale(t10 + t11, 2);
    d[4 * stride] = FIRST ? (t10 - t11) << 2 : jpeg_descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2 * stride] = jpeg_descale(z1 + t13 * 6270, n);
    d[6 * stride] = jpeg_descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    d[7 * stride] = jpeg_descale(t4 + z1 + z3, n);
    d[5 * stride] = jpeg_descale(t5 + z2 + z4, n);
    d[3 * stride] = jpeg_descale(t6 + z2 + z3, n);
    d[stride] = jpeg_descale(t7 + z1 + z4, n);
}

// component c (0 Y, 1 Cb, 2 Cr; GRAY: the level itself) of pixel (y, x), both inside the image
__device__ __forceinline__ int jpeg_sample(const void* __restrict__ img, int dtype, size_t frame_base, int W, int y, int x, int c, bool gray,
                                           bool rgb, float scale, bool& bad) {
    const size_t p = (size_t)y * W + x;
    if (gray) return jpeg_level(img, dtype, frame_base + p, scale, bad);
    const int c0 = jpeg_level(img, dtype, frame_base + 3 * p, scale, bad), G = jpeg_level(img, dtype, frame_base + 3 * p + 1, scale, bad),
              c2 = jpeg_level(img, dtype, frame_base + 3 * p + 2, scale, bad);
    const int R = rgb ? c0 : c2, B = rgb ? c2 : c0;
    if (c == 0) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    if (c == 1) return (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    return (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}

// grid (MCUs, F), 64 * bpm threads: wave k of the workgroup owns block k of the MCU
__global__ void __launch_bounds__(384) k_jpeg_coef(const void* __restrict__ img, int dtype, JpegGeom g, JpegQuant q, int rgb, float scale,
                                                   int16_t* __restrict__ coef, uint32_t* __restrict__ status) {
    __shared__ int s_blk[6][64];
    __shared__ int s_dc[6];
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6, f = blockIdx.y;
    const int mx = blockIdx.x % g.mw, my = blockIdx.x / g.mw;
    const int r = lane >> 3, c = lane & 7;
    const bool gray = g.mode == DSN_JPEG_GRAY;
    const size_t frame_base = (size_t)f * g.H * g.W * (gray ? 1 : 3);
    const int H = g.H, W = g.W;
    bool bad = false, dummy = false;
    int comp, v;
    if (g.mode == DSN_JPEG_420 && k < 4) {                       // luma of a 16 x 16 MCU
        comp = 0;
        const int by = my * 2 + (k >> 1), bx = mx * 2 + (k & 1);
        dummy = by >= (H + 7) / 8 || bx >= (W + 7) / 8;
        v = jpeg_sample(img, dtype, frame_base, W, min(by * 8 + r, H - 1), min(bx * 8 + c, W - 1), 0, false, rgb, scale, bad);
    } else if (g.mode == DSN_JPEG_420) {                         // chroma: 2 x 2 means with the alternating bias
        comp = k - 3;
        const int cy = min(my * 8 + r, (H + 1) / 2 - 1), cx = mx * 8 + c;
        const int y0 = 2 * cy, y1 = min(2 * cy + 1, H - 1), x0 = min(2 * cx, W - 1), x1 = min(2 * cx + 1, W - 1);
        v = jpeg_sample(img, dtype, frame_base, W, y0, x0, comp, false, rgb, scale, bad)
          + jpeg_sample(img, dtype, frame_base, W, y0, x1, comp, false, rgb, scale, bad)
          + jpeg_sample(img, dtype, frame_base, W, y1, x0, comp, false, rgb, scale, bad)
          + jpeg_sample(img, dtype, frame_base, W, y1, x1, comp, false, rgb, scale, bad);
        v = (v + 1 + (cx & 1)) >> 2;
    } else {
        comp = gray ? 0 : k;
        v = jpeg_sample(img, dtype, frame_base, W, min(my * 8 + r, H - 1), min(mx * 8 + c, W - 1), comp, gray, rgb, scale, bad);
    }
    s_blk[k][lane] = v - 128;
    __syncthreads();
    if (lane < 8) jpeg_fdct_pass<true>(&s_blk[k][lane * 8], 1);
    __syncthreads();
    if (lane < 8) jpeg_fdct_pass<false>(&s_blk[k][lane], 8);
    __syncthreads();
    // lane = zigzag slot
    const int x = s_blk[k][c_zigzag.z[lane]];
    const int d = q.d[comp ? 1 : 0][lane];
    const int a = (x < 0 ? -x : x) + (d >> 1);
    int qv = a >= d ? a / d : 0;
    qv = x < 0 ? -qv : qv;
    if (lane == 0) s_dc[k] = qv;
    __syncthreads();
    if (dummy) {                                                 // k >= 1: walk back to the last real block of the MCU
        int j = k - 1;
        while (j > 0) {
            const int by = my * 2 + (j >> 1), bx = mx * 2 + (j & 1);
            if (by < (H + 7) / 8 && bx < (W + 7) / 8) break;
            --j;
        }
        qv = lane == 0 ? s_dc[j] : 0;
    }
    coef[((size_t)f * g.nb + (size_t)blockIdx.x * g.bpm + k) * 64 + lane] = (int16_t)qv;
    if (__any(bad) && lane == 0) atomicOr(&status[f], DSN_JPEG_NONFINITE);
}

__global__ void k_jpeg_zero_status(uint32_t* __restrict__ status, int F) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < F) status[i] = 0;
}

// ---- entropy coding ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int jpeg_nbits(int a) { return a ? 32 - __clz(a) : 0; }          // bits of a >= 0

// the bits slot `lane` of block b contributes: value in `val` (most significant bit first when written), count returned
__device__ __forceinline__ int jpeg_lane_word(const int16_t* __restrict__ cf, const JpegGeom& g, int b, int lane, uint64_t& val) {
    const int k = b % g.bpm;
    const int comp = g.mode == DSN_JPEG_420 ? (k < 4 ? 0 : k - 3) : g.mode == DSN_JPEG_444 ? k : 0;
    const int t = comp ? 1 : 0;
    int v = cf[(size_t)b * 64 + lane];
    const unsigned long long nzall = __ballot(v != 0);
    val = 0;
    if (lane == 0) {
        // the previous block of the same component: Y of a 420 MCU follows Y inside the MCU, Y00 follows the MCU before's Y11
        const int back = g.mode == DSN_JPEG_420 ? (comp == 0 ? (k == 0 ? 3 : 1) : 6) : g.bpm;
        const int prev = b - back >= 0 ? cf[(size_t)(b - back) * 64] : 0;
        const int diff = v - prev;
        const int s = min(jpeg_nbits(diff < 0 ? -diff : diff), 11);          // (beyond 11 / 10 bits no baseline code exists: coefficients
        const uint32_t h = c_huff.dc[t][s];                                   //  a caller made up stay inside the block's 1658 bits)
        val = ((uint64_t)(h & 0xFFFF) << s) | ((uint32_t)(diff < 0 ? diff + (1 << s) - 1 : diff) & ((1u << s) - 1));
        return (int)(h >> 16) + s;
    }
    if (v != 0) {
        const unsigned long long below = nzall & ((1ull << lane) - 1) & ~1ull;          // non-zero AC slots before this one
        const int p = below ? 63 - __clzll(below) : 0;
        const int run = lane - p - 1;
        const int s = min(jpeg_nbits(v < 0 ? -v : v), 10);
        const uint32_t zrl = c_huff.ac[t][0xF0], h = c_huff.ac[t][((run & 15) << 4) | s];
        const int zl = (int)(zrl >> 16), nz = run >> 4;
        uint64_t w = 0;
        for (int i = 0; i < nz; ++i) w = (w << zl) | (zrl & 0xFFFF);
        w = (w << (h >> 16)) | (h & 0xFFFF);
        val = (w << s) | ((uint32_t)(v < 0 ? v + (1 << s) - 1 : v) & ((1u << s) - 1));
        return nz * zl + (int)(h >> 16) + s;
    }
    if (lane == 63) {                                            // coefficient 63 is zero: end of block
        const uint32_t h = c_huff.ac[t][0];
        val = h & 0xFFFF;
        return (int)(h >> 16);
    }
    return 0;
}

__device__ __forceinline__ int jpeg_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int jpeg_wave_exclusive(int v, int lane) {
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(s, o);
        if (lane >= o) s += u;
    }
    return s - v;
}

// grid (ceil(nb / 4), F), 256 threads: a wave per block
__global__ void __launch_bounds__(256) k_jpeg_bits(const int16_t* __restrict__ coef, JpegGeom g, int* __restrict__ bits) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6), f = blockIdx.y;
    if (b >= g.nb) return;
    uint64_t val;
    const int n = jpeg_wave_sum(jpeg_lane_word(coef + (size_t)f * g.nb * 64, g, b, lane, val));
    if (lane == 0) bits[(size_t)f * g.nb + b] = n;
}

// exclusive scan over the workgroup's threads in thread order; returns the total
__device__ __forceinline__ int jpeg_block_scan(int v, int& total) {
    __shared__ int s_w[JPEG_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ex = jpeg_wave_exclusive(v, lane);
    __syncthreads();                                             // (s_w may still be read from a previous call)
    if (lane == 63) s_w[w] = ex + v;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < JPEG_SCAN_THREADS / 64; ++i) { if (i < w) base += s_w[i]; total += s_w[i]; }
    return base + ex;
}

// grid (tiles, F): x[f][i] becomes its exclusive prefix inside its tile of JPEG_TILE, tot[f][tile] the tile's sum
__global__ void __launch_bounds__(JPEG_SCAN_THREADS) k_jpeg_tile(int* __restrict__ x, int n, int tiles, int* __restrict__ tot) {
    const int f = blockIdx.y, i0 = blockIdx.x * JPEG_TILE + threadIdx.x * 4;
    int* xf = x + (size_t)f * n;
    int v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = i0 + j < n ? xf[i0 + j] : 0; s += v[j]; }
    int total;
    int ex = jpeg_block_scan(s, total);
#pragma unroll
    for (int j = 0; j < 4; ++j) { if (i0 + j < n) xf[i0 + j] = ex; ex += v[j]; }
    if (threadIdx.x == 0) tot[(size_t)f * (tiles + 1) + blockIdx.x] = total;
}

// grid (F), one workgroup: exclusive scan of a frame's tile totals in place, [tiles] = the grand total
__global__ void __launch_bounds__(JPEG_SCAN_THREADS) k_jpeg_tiles(int* __restrict__ tot, int tiles) {
    int* t = tot + (size_t)blockIdx.x * (tiles + 1);
    int carry = 0;
    for (int i0 = 0; i0 < tiles; i0 += JPEG_SCAN_THREADS) {
        const int i = i0 + threadIdx.x;
        const int v = i < tiles ? t[i] : 0;
        int total;
        const int ex = jpeg_block_scan(v, total);
        if (i < tiles) t[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) t[tiles] = carry;
}

// grid (ceil(stream words / 256), F): zero the words the frame's bits will touch
__global__ void __launch_bounds__(256) k_jpeg_clear(uint32_t* __restrict__ stream, JpegGeom g, const int* __restrict__ tot1) {
    const int f = blockIdx.y;
    const int total = tot1[(size_t)f * (g.tiles1 + 1) + g.tiles1];
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w < (total + 31) / 32) stream[(size_t)f * (g.stream_bytes / 4) + w] = 0;
}

// grid (ceil(nb / 4), F), 256 threads: a wave per block ORs its lanes' words into the stream (word w holds stream bytes 4 w ... 4 w + 3)
__global__ void __launch_bounds__(256) k_jpeg_emit(const int16_t* __restrict__ coef, JpegGeom g, const int* __restrict__ bits,
                                                   const int* __restrict__ tot1, uint32_t* __restrict__ stream) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6), f = blockIdx.y;
    if (b >= g.nb) return;
    uint64_t val;
    const int n = jpeg_lane_word(coef + (size_t)f * g.nb * 64, g, b, lane, val);
    const int at = bits[(size_t)f * g.nb + b] + tot1[(size_t)f * (g.tiles1 + 1) + b / JPEG_TILE] + jpeg_wave_exclusive(n, lane);
    if (n == 0) return;
    uint32_t* s = stream + (size_t)f * (g.stream_bytes / 4);
    // the n bits occupy stream bits [at, at + n): at most three words (n <= 59)
    int w = at >> 5, left = n, room = 32 - (at & 31);           // room: free bits of word w below the write position
    while (left > 0) {
        const int take = left < room ? left : room;
        const uint32_t piece = (uint32_t)((val >> (left - take)) & ((1ull << take) - 1)) << (room - take);
        if (piece) atomicOr(&s[w], __builtin_bswap32(piece));
        left -= take;
        ++w;
        room = 32;
    }
}

// the 16 bytes of chunk c of the frame's stream with the final byte padded; returns how many of them belong to the scan
__device__ __forceinline__ int jpeg_chunk(const uint8_t* __restrict__ s, int c, int total_bits, uint8_t b[JPEG_CHUNK]) {
    const int nbytes = (total_bits + 7) >> 3;
    const int have = min(JPEG_CHUNK, nbytes - c * JPEG_CHUNK);
    if (have <= 0) return 0;
    const uint4 q = *(const uint4*)(s + (size_t)c * JPEG_CHUNK);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < JPEG_CHUNK; ++i) b[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    const int last = nbytes - 1 - c * JPEG_CHUNK;
    if (last < JPEG_CHUNK && (total_bits & 7)) {
        const uint8_t pad = (uint8_t)((1 << (8 - (total_bits & 7))) - 1);
#pragma unroll
        for (int i = 0; i < JPEG_CHUNK; ++i) if (i == last) b[i] |= pad;
    }
    return have;
}

// grid (tiles2 * 4, F), 256 threads: 0xFF bytes per chunk
__global__ void __launch_bounds__(256) k_jpeg_ffcount(const uint8_t* __restrict__ stream, JpegGeom g, const int* __restrict__ tot1,
                                                      int* __restrict__ ff) {
    const int f = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= g.chunks) return;
    const int total = tot1[(size_t)f * (g.tiles1 + 1) + g.tiles1];
    uint8_t b[JPEG_CHUNK];
    const int have = jpeg_chunk(stream + (size_t)f * g.stream_bytes, c, total, b);
    int n = 0;
#pragma unroll
    for (int i = 0; i < JPEG_CHUNK; ++i) n += (i < have && b[i] == 0xFF) ? 1 : 0;
    ff[(size_t)f * g.chunks + c] = n;
}

// grid (tiles2 * 4, F), 256 threads: header, stuffed scan, EOI, length, status
__global__ void __launch_bounds__(256) k_jpeg_stuff(const uint8_t* __restrict__ stream, JpegGeom g, JpegHeader hdr, const int* __restrict__ tot1,
                                                    const int* __restrict__ ff, const int* __restrict__ tot2,
                                                    const uint32_t* __restrict__ status_in, uint8_t* __restrict__ out, size_t capacity,
                                                    int* __restrict__ lengths, uint32_t* __restrict__ status) {
    const int f = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    uint8_t* o = out + (size_t)f * capacity;
    const int total = tot1[(size_t)f * (g.tiles1 + 1) + g.tiles1];
    const int nbytes = (total + 7) >> 3;
    const int* t2 = tot2 + (size_t)f * (g.tiles2 + 1);
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < hdr.len; i += 256) if ((size_t)i < capacity) o[i] = hdr.b[i];
        if (threadIdx.x == 0) {
            const size_t end = (size_t)hdr.len + nbytes + t2[g.tiles2];          // EOI goes here
            if (end < capacity) o[end] = 0xFF;
            if (end + 1 < capacity) o[end + 1] = 0xD9;
            lengths[f] = (int)(end + 2);
            status[f] = (status_in ? status_in[f] : 0u) | (end + 2 > capacity ? DSN_JPEG_OVERFLOW : 0u);
        }
    }
    if (c >= g.chunks) return;
    uint8_t b[JPEG_CHUNK];
    const int have = jpeg_chunk(stream + (size_t)f * g.stream_bytes, c, total, b);
    if (have == 0) return;
    size_t at = (size_t)hdr.len + (size_t)c * JPEG_CHUNK + t2[c / JPEG_TILE] + ff[(size_t)f * g.chunks + c];
#pragma unroll
    for (int i = 0; i < JPEG_CHUNK; ++i) {
        if (i < have) {
            if (at < capacity) o[at] = b[i];
            ++at;
            if (b[i] == 0xFF) { if (at < capacity) o[at] = 0; ++at; }
        }
    }
}

struct JpegWorkspace { int16_t* coef; int* bits; int* tot1; uint32_t* stream; int* ff; int* tot2; uint32_t* status; size_t bytes; };

JpegWorkspace jpeg_carve(void* base, int F, const JpegGeom& g, bool with_coef) {
    JpegWorkspace w;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off += (n + 255) & ~(size_t)255; return (char*)base + at; };
    w.coef = (int16_t*)take(with_coef ? (size_t)F * g.nb * 64 * sizeof(int16_t) : 0);
    w.bits = (int*)take((size_t)F * g.nb * sizeof(int));
    w.tot1 = (int*)take((size_t)F * (g.tiles1 + 1) * sizeof(int));
    w.stream = (uint32_t*)take((size_t)F * g.stream_bytes);
    w.ff = (int*)take((size_t)F * g.chunks * sizeof(int));
    w.tot2 = (int*)take((size_t)F * (g.tiles2 + 1) * sizeof(int));
    w.status = (uint32_t*)take((size_t)F * sizeof(uint32_t));
    w.bytes = off;
    return w;
}

}  // namespace

size_t dsn_jpeg_header_bytes(int mode) { return mode == DSN_JPEG_GRAY ? 328 : 623; }

bool dsn_jpeg_blocks(int H, int W, int mode, int* blocks) {
    JpegGeom g;
    if (!jpeg_geom(H, W, mode, g)) return false;
    *blocks = g.nb;
    return true;
}

size_t dsn_jpeg_workspace_size(int F, int H, int W, int mode, bool with_coef) {
    JpegGeom g;
    if (F < 1 || F > DSN_JPEG_MAX_FRAMES || !jpeg_geom(H, W, mode, g)) return 0;
    return jpeg_carve(nullptr, F, g, with_coef).bytes;
}

int dsn_jpeg_write_header_host(int H, int W, int mode, int quality, uint8_t* out) {
    JpegGeom g;
    if (!jpeg_geom(H, W, mode, g)) return 0;
    return jpeg_header_host(g, quality, out);
}

void dsn_launch_jpeg_coefficients(const void* images, int dtype, int F, int H, int W, int mode, int quality, int rgb, float scale,
                                  int16_t* coef, uint32_t* status, hipStream_t st) {
    JpegGeom g;
    jpeg_geom(H, W, mode, g);
    uint8_t tab[2][64];
    jpeg_quant_host(quality, tab);
    JpegQuant q;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) q.d[t][i] = (uint16_t)(8 * tab[t][kZigzag[i]]);
    hipLaunchKernelGGL(k_jpeg_zero_status, dim3((F + 255) / 256), dim3(256), 0, st, status, F);
    hipLaunchKernelGGL(k_jpeg_coef, dim3(g.mw * g.mh, F), dim3(64 * g.bpm), 0, st, images, dtype, g, q, rgb, scale, coef, status);
}

void dsn_launch_jpeg_scan(const int16_t* coef, const uint32_t* status_in, int F, int H, int W, int mode, int quality, uint8_t* out,
                          size_t capacity, int32_t* lengths, uint32_t* status, void* workspace, bool ws_has_coef, hipStream_t st) {
    JpegGeom g;
    jpeg_geom(H, W, mode, g);
    const JpegWorkspace w = jpeg_carve(workspace, F, g, ws_has_coef);
    JpegHeader hdr;
    hdr.len = jpeg_header_host(g, quality, hdr.b);
    const dim3 waves((g.nb + 3) / 4, F), chunks((g.chunks + 255) / 256, F);
    hipLaunchKernelGGL(k_jpeg_bits, waves, dim3(256), 0, st, coef, g, w.bits);
    hipLaunchKernelGGL(k_jpeg_tile, dim3(g.tiles1, F), dim3(JPEG_SCAN_THREADS), 0, st, w.bits, g.nb, g.tiles1, w.tot1);
    hipLaunchKernelGGL(k_jpeg_tiles, dim3(F), dim3(JPEG_SCAN_THREADS), 0, st, w.tot1, g.tiles1);
    hipLaunchKernelGGL(k_jpeg_clear, dim3((unsigned)((g.stream_bytes / 4 + 255) / 256), F), dim3(256), 0, st, w.stream, g, w.tot1);
    hipLaunchKernelGGL(k_jpeg_emit, waves, dim3(256), 0, st, coef, g, w.bits, w.tot1, w.stream);
    hipLaunchKernelGGL(k_jpeg_ffcount, chunks, dim3(256), 0, st, (const uint8_t*)w.stream, g, w.tot1, w.ff);
    hipLaunchKernelGGL(k_jpeg_tile, dim3(g.tiles2, F), dim3(JPEG_SCAN_THREADS), 0, st, w.ff, g.chunks, g.tiles2, w.tot2);
    hipLaunchKernelGGL(k_jpeg_tiles, dim3(F), dim3(JPEG_SCAN_THREADS), 0, st, w.tot2, g.tiles2);
    hipLaunchKernelGGL(k_jpeg_stuff, chunks, dim3(256), 0, st, (const uint8_t*)w.stream, g, hdr, w.tot1, w.ff, w.tot2, status_in, out, capacity,
                       lengths, status);
}

void dsn_launch_jpeg_encode(const void* images, int dtype, int F, int H, int W, int mode, int quality, int rgb, float scale, uint8_t* out,
                            size_t capacity, int32_t* lengths, uint32_t* status, void* workspace, hipStream_t st) {
    JpegGeom g;
    jpeg_geom(H, W, mode, g);
    const JpegWorkspace w = jpeg_carve(workspace, F, g, true);
    dsn_launch_jpeg_coefficients(images, dtype, F, H, W, mode, quality, rgb, scale, w.coef, w.status, st);
    dsn_launch_jpeg_scan(w.coef, w.status, F, H, W, mode, quality, out, capacity, lengths, status, workspace, true, st);
}

// the tile scan on its own (dsn_jpegd.hip): x [F][n] becomes its exclusive prefix inside tiles of JPEG_TILE, tot [F][tiles + 1] the
// tiles' exclusive prefixes and, in [tiles], the row's sum
void dsn_launch_jpeg_tile_scan(int* x, int n, int F, int* tot, hipStream_t st) {
    const int tiles = (n + JPEG_TILE - 1) / JPEG_TILE;
    hipLaunchKernelGGL(k_jpeg_tile, dim3(tiles, F), dim3(JPEG_SCAN_THREADS), 0, st, x, n, tiles, tot);
    hipLaunchKernelGGL(k_jpeg_tiles, dim3(F), dim3(JPEG_SCAN_THREADS), 0, st, tot, tiles);
}
