// dsn_pnge.hip - PNG ENCODING on the device (dsn_png_filter, dsn_png_deflate, dsn_huff_lengths, dsn_png_container, dsn_png_encode; the
// rule is in include/dsnerf.h and restated in tests/png_encode_restate.py).  Integer arithmetic throughout; the only atomics are 32-bit
// integer adds in LDS (histograms), adds of sums mod 65521 (Adler-32), XORs (CRC-32) and ORs into cleared stream words and status words.
//   k_pe_zero     : clears the frames' status, Adler and CRC words
//   k_pe_filter   : a workgroup per row: levels, the five filters' sums of |int8|, the choice, the row of the raw stream
//   k_pe_adler / k_pe_adler_fin : sums mod 65521 per 64 KiB block, added per frame; then the value
//   k_pe_match    : a thread per byte of the raw stream: the longest of the (at most three) candidate matches inside its chunk
//   k_pe_codes    : ONE WAVE PER CHUNK: the serial greedy parse (64 positions per turn, the carry in a scalar), histograms by LDS atomics,
//                   both Huffman codes and the code-length code, the block header, the three costs and the block type; clears the slot
//   k_pe_emit     : a workgroup per chunk: bit lengths per token, prefix sums, the codes OR-ed into the chunk's slot
//   (tile scan of the chunks' byte lengths: dsn_jpeg.hip's)
//   k_pe_compact  : a workgroup per chunk: its bytes to their place in the frame's stream
//   k_pe_cont_copy / k_pe_cont_tail : the stream into the file with CRC-32 slices combined by x^(8 n) mod the polynomial; the rest of the file
// Frames lie side by side in blockIdx.y; nothing depends on F.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include "dsn_level.h"

#define PE_TILE 1024              // the tile scan's tile (dsn_jpeg.hip)
#define PE_TABLE 320              // code words per chunk: 288 literal/length, 32 distance
#define PE_INFO 4                 // int32 words per chunk: block type, header bits, bits up to and including the end-of-block code, bytes
#define PE_ADLER_BLOCK 65536
#define PE_MOD 65521u
#define PE_FILE_HEAD 43           // signature 8, IHDR 25, IDAT length 4, "IDAT" 4, 78 01
#define PE_FILE_EXTRA 63          // ... + Adler-32 4, CRC 4, IEND 12

namespace {

// ---- CRC-32 (reflected 0xEDB88320), with the multiplication mod the polynomial that moves a register past n bytes ------------------------
struct PeCrcTable { uint32_t t[256]; uint32_t x2n[32]; };          // x2n[k] = x^(2^k) mod P
constexpr uint32_t pe_mulmod_c(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & m) p ^= b;
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
constexpr PeCrcTable pe_make_crc() {
    PeCrcTable c{};
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t v = n;
        for (int k = 0; k < 8; ++k) v = (v & 1) ? 0xEDB88320u ^ (v >> 1) : v >> 1;
        c.t[n] = v;
    }
    uint32_t p = 1u << 30;                                       // x^1
    for (int k = 0; k < 32; ++k) { c.x2n[k] = p; p = pe_mulmod_c(p, p); }
    return c;
}
constexpr PeCrcTable kPeCrc = pe_make_crc();
__constant__ const PeCrcTable c_pe_crc = pe_make_crc();

uint32_t pe_crc_host(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = kPeCrc.t[(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

__device__ __forceinline__ uint32_t pe_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll 4
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
// the register r (no pre- or post-conditioning) after n further zero bytes: r x^(8 n) mod P
__device__ __forceinline__ uint32_t pe_crc_shift(uint32_t r, uint32_t n) {
    uint32_t p = 1u << 31;                                       // x^0
    for (int k = 3; n; n >>= 1, ++k)
        if (n & 1u) p = pe_mulmod(c_pe_crc.x2n[k & 31], p);
    return pe_mulmod(p, r);
}

struct PeHead { uint8_t b[33]; };                                // signature and IHDR, the same for every frame of a call

PeHead pe_head_host(int W, int H, int channels) {
    PeHead h;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) h.b[i] = sig[i];
    uint8_t* c = h.b + 8;
    c[0] = 0; c[1] = 0; c[2] = 0; c[3] = 13;
    c[4] = 'I'; c[5] = 'H'; c[6] = 'D'; c[7] = 'R';
    for (int i = 0; i < 4; ++i) { c[8 + i] = (uint8_t)((uint32_t)W >> (24 - 8 * i)); c[12 + i] = (uint8_t)((uint32_t)H >> (24 - 8 * i)); }
    c[16] = 8; c[17] = channels == 3 ? 2 : 0; c[18] = 0; c[19] = 0; c[20] = 0;
    const uint32_t crc = pe_crc_host(c + 4, 17);
    for (int i = 0; i < 4; ++i) c[21 + i] = (uint8_t)(crc >> (24 - 8 * i));
    return h;
}

// ---- geometry ------------------------------------------------------------------------------------------------------------------------------
struct PeDef { size_t n; int C, nch, slot, tiles; size_t zmax, zcap; };          // the deflate stage of n raw bytes per frame

bool pe_chunk_ok(int C) { return C >= DSN_PNGE_CHUNK_MIN && C <= DSN_PNGE_CHUNK_MAX && (C & (C - 1)) == 0; }

bool pe_def(size_t n, int C, PeDef& d) {
    if (n < 1 || n > ((size_t)1 << 30) + ((size_t)1 << 15) || !pe_chunk_ok(C)) return false;
    d.n = n; d.C = C;
    d.nch = (int)((n + C - 1) / C);
    d.slot = C + 32;                                             // a chunk with its empty block is at most C + 10 bytes
    d.tiles = (d.nch + PE_TILE - 1) / PE_TILE;
    d.zmax = n + (size_t)10 * d.nch - 5;                         // every chunk stored: 5 + its bytes, + the 5 of the empty block behind all but the last
    d.zcap = (d.zmax + 15) & ~(size_t)15;
    return true;
}

struct PeDefWs { uint16_t* match; int* info; uint32_t* table; uint8_t* slots; int* nbytes; int* tot; size_t bytes; };

PeDefWs pe_def_carve(void* base, int F, const PeDef& d) {
    PeDefWs w;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off += (n + 255) & ~(size_t)255; return (char*)base + at; };
    w.match = (uint16_t*)take((size_t)F * d.n * sizeof(uint16_t));
    w.info = (int*)take((size_t)F * d.nch * PE_INFO * sizeof(int));
    w.table = (uint32_t*)take((size_t)F * d.nch * PE_TABLE * sizeof(uint32_t));
    w.slots = (uint8_t*)take((size_t)F * d.nch * d.slot);
    w.nbytes = (int*)take((size_t)F * d.nch * sizeof(int));
    w.tot = (int*)take((size_t)F * (d.tiles + 1) * sizeof(int));
    w.bytes = off;
    return w;
}

struct PeGeom { int W, H, mode, ch, in_ch, rb, bpp; size_t n; };

bool pe_geom(int W, int H, int mode, PeGeom& g) {
    if (W < 1 || H < 1 || W > DSN_PNG_MAX_DIM || H > DSN_PNG_MAX_DIM || mode < DSN_PNGE_GRAY || mode > DSN_PNGE_REPLICATE) return false;
    g.W = W; g.H = H; g.mode = mode;
    g.ch = mode == DSN_PNGE_GRAY ? 1 : 3;
    g.in_ch = mode == DSN_PNGE_COLOUR ? 3 : 1;
    g.rb = W * g.ch;
    g.bpp = g.ch;
    g.n = (size_t)H * (1 + g.rb);
    return true;
}

struct PeEncWs { uint8_t* raw; uint32_t* words; uint8_t* zs; int32_t* zlen; uint32_t* zstatus; void* def; size_t bytes; };
// words: uint32 [5][F] = status of the filter stage, Adler sum a, Adler sum b, Adler-32, CRC register
PeEncWs pe_enc_carve(void* base, int F, const PeGeom& g, const PeDef& d) {
    PeEncWs w;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off += (n + 255) & ~(size_t)255; return (char*)base + at; };
    w.raw = (uint8_t*)take((size_t)F * g.n);
    w.words = (uint32_t*)take((size_t)F * 5 * sizeof(uint32_t));
    w.zs = (uint8_t*)take((size_t)F * d.zcap);
    w.zlen = (int32_t*)take((size_t)F * sizeof(int32_t));
    w.zstatus = (uint32_t*)take((size_t)F * sizeof(uint32_t));
    w.def = (void*)take(pe_def_carve(nullptr, F, d).bytes);
    w.bytes = off;
    return w;
}

// ---- small kernels ---------------------------------------------------------------------------------------------------------------------------
__global__ void k_pe_zero(uint32_t* __restrict__ p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

__device__ __forceinline__ int pe_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- filter ----------------------------------------------------------------------------------------------------------------------------------
// byte i of row y of the file's unfiltered pixels (0 outside the image)
__device__ __forceinline__ int pe_byte(const void* __restrict__ img, int dtype, size_t frame_px, const PeGeom& g, int rgb, float scale, int y,
                                       int i, bool& bad) {
    if (y < 0 || i < 0) return 0;
    const int x = g.ch == 3 ? i / 3 : i, k = g.ch == 3 ? i - 3 * x : 0;
    const size_t p = frame_px + (size_t)y * g.W + x;
    return dsn_image_level(img, dtype, g.in_ch == 3 ? 3 * p + (rgb ? k : 2 - k) : p, scale, bad);
}

__device__ __forceinline__ int pe_filtered(int ft, int x, int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    const int paeth = (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
    const int sub = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0;
    return (x - sub) & 255;
}

// grid (H, F), 256 threads
__global__ void __launch_bounds__(256) k_pe_filter(const void* __restrict__ img, int dtype, PeGeom g, int rgb, float scale, int filter,
                                                   uint8_t* __restrict__ raw, uint32_t* __restrict__ status) {
    __shared__ int s_sum[5];
    const int y = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    const size_t frame_px = (size_t)f * g.H * g.W;
    uint8_t* row = raw + (size_t)f * g.n + (size_t)y * (1 + g.rb);
    bool bad = false, other = false;
    int ft = filter;
    if (filter == DSN_PNGE_ADAPTIVE) {
        if (t < 5) s_sum[t] = 0;
        __syncthreads();
        int sum[5] = {0, 0, 0, 0, 0};
        for (int i = t; i < g.rb; i += 256) {
            const int x = pe_byte(img, dtype, frame_px, g, rgb, scale, y, i, bad), a = pe_byte(img, dtype, frame_px, g, rgb, scale, y, i - g.bpp, other),
                      b = pe_byte(img, dtype, frame_px, g, rgb, scale, y - 1, i, other),
                      c = pe_byte(img, dtype, frame_px, g, rgb, scale, y - 1, i - g.bpp, other);
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int v = pe_filtered(k, x, a, b, c);
                sum[k] += v < 128 ? v : 256 - v;
            }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int s = pe_wave_sum(sum[k]);
            if ((t & 63) == 0) atomicAdd(&s_sum[k], s);
        }
        __syncthreads();
        ft = 0;
        for (int k = 1; k < 5; ++k) if (s_sum[k] < s_sum[ft]) ft = k;          // ties: the lower filter number
    }
    if (t == 0) row[0] = (uint8_t)ft;
    for (int i = t; i < g.rb; i += 256) {
        const int x = pe_byte(img, dtype, frame_px, g, rgb, scale, y, i, bad), a = pe_byte(img, dtype, frame_px, g, rgb, scale, y, i - g.bpp, other),
                  b = pe_byte(img, dtype, frame_px, g, rgb, scale, y - 1, i, other),
                  c = pe_byte(img, dtype, frame_px, g, rgb, scale, y - 1, i - g.bpp, other);
        row[1 + i] = (uint8_t)pe_filtered(ft, x, a, b, c);
    }
    if (__any(bad) && (t & 63) == 0) atomicOr(&status[f], DSN_PNGE_NONFINITE);
}

// ---- Adler-32 --------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(n / 65536), F), 256 threads: sums[0][f] += sum d_i, sums[1][f] += sum ((n - i) mod 65521) d_i, both mod 65521
__global__ void __launch_bounds__(256) k_pe_adler(const uint8_t* __restrict__ raw, size_t n, int F, uint32_t* __restrict__ sums) {
    const int f = blockIdx.y;
    const uint8_t* r = raw + (size_t)f * n;
    const size_t base = (size_t)blockIdx.x * PE_ADLER_BLOCK;
    uint64_t sa = 0, sb = 0;
    for (int k = threadIdx.x; k < PE_ADLER_BLOCK; k += 256) {
        const size_t i = base + k;
        if (i < n) {
            const uint32_t d = r[i];
            sa += d;
            sb += (uint64_t)((n - i) % PE_MOD) * d;
        }
    }
    int a = (int)(sa % PE_MOD), b = (int)(sb % PE_MOD);          // (below 2^16 each: a wave's sum stays below 2^22)
    a = pe_wave_sum(a); b = pe_wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&sums[f], (uint32_t)a % PE_MOD);
        atomicAdd(&sums[F + f], (uint32_t)b % PE_MOD);           // (at most 2^14 blocks x 4 waves x 65520 < 2^32)
    }
}

__global__ void k_pe_adler_fin(const uint32_t* __restrict__ sums, size_t n, int F, uint32_t* __restrict__ adler) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const uint32_t a = (1u + sums[f] % PE_MOD) % PE_MOD, b = ((uint32_t)(n % PE_MOD) + sums[F + f] % PE_MOD) % PE_MOD;
    adler[f] = b << 16 | a;
}

// ---- matches ---------------------------------------------------------------------------------------------------------------------------------
struct PeDist { int d[3]; int nd; };                             // candidate distances, ascending, no duplicates, none above 32768

// grid (ceil(n / 256), F), 256 threads: match[p] = length | candidate index << 9, 0 for a literal
__global__ void __launch_bounds__(256) k_pe_match(const uint8_t* __restrict__ raw, PeDef d, PeDist cand, uint16_t* __restrict__ match) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= d.n) return;
    const uint8_t* r = raw + (size_t)blockIdx.y * d.n;
    const size_t cs = p & ~(size_t)(d.C - 1);
    const size_t ce = cs + d.C < d.n ? cs + d.C : d.n;
    const int cap = (int)(ce - p < 258 ? ce - p : 258);
    int best = 0, bk = 0;
    for (int k = 0; k < cand.nd; ++k) {
        const size_t dist = (size_t)cand.d[k];
        if (p < cs + dist) break;                                // (ascending: the rest reach before the chunk start too)
        int len = 0;
        while (len < cap && r[p + len] == r[p + len - dist]) ++len;
        if (len > best) { best = len; bk = k; }                  // ties: the smaller distance
    }
    const bool lit = best < 3 || (best == 3 && cand.d[bk] > 4096);
    match[(size_t)blockIdx.y * d.n + p] = lit ? (uint16_t)0 : (uint16_t)(best | bk << 9);
}

// ---- codes -----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pe_len_code(int len, int& code, int& nb, int& ext) {          // code: 0 ... 28 (symbol 257 + code)
    const int l = len - 3;
    if (len == 258) { code = 28; nb = 0; ext = 0; return; }
    if (l < 4) { code = l; nb = 0; ext = 0; return; }
    nb = (31 - __clz(l)) - 2;
    code = 4 * nb + 4 + ((l >> nb) & 3);
    ext = l & ((1 << nb) - 1);
}
__device__ __forceinline__ void pe_dist_code(int dist, int& code, int& nb, int& ext) {
    const int l = dist - 1;
    if (l < 4) { code = l; nb = 0; ext = 0; return; }
    nb = (31 - __clz(l)) - 1;
    code = 2 * nb + 2 + ((l >> nb) & 1);
    ext = l & ((1 << nb) - 1);
}
__device__ __forceinline__ int pe_len_extra(int code) { return code < 8 || code == 28 ? 0 : (code >> 2) - 1; }
__device__ __forceinline__ int pe_dist_extra(int code) { return code < 4 ? 0 : (code >> 1) - 1; }
__device__ __forceinline__ int pe_fixed_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

struct PeHuff {
    uint32_t cnt[288];
    uint16_t order[288];          // used symbols by (count, symbol)
    uint64_t w[576];              // leaves in that order, then the internal nodes in the order they were made
    uint16_t parent[576], depth[576];
    int m;
};

// code lengths of counts[0 ... n) with no length above `limit`, by all 64 lanes of a one-wave workgroup (n <= 288, 2 <= n <= 2^limit)
__device__ void pe_huff_lengths(PeHuff& S, const uint32_t* counts, int n, int limit, uint8_t* lens, int lane) {
    for (int i = lane; i < n; i += 64) { S.cnt[i] = counts[i]; lens[i] = 0; }
    __syncthreads();
    if (lane == 0) {
        int used = 0;
        for (int i = 0; i < n; ++i) used += S.cnt[i] != 0;
        for (int i = 0; i < n && used < 2; ++i) if (!S.cnt[i]) { S.cnt[i] = 1; ++used; }          // zlib's practice: every code is complete
        S.m = used;
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const uint32_t c = S.cnt[i];
        if (!c) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t cj = S.cnt[j];
            rank += (cj && (cj < c || (cj == c && j < i))) ? 1 : 0;
        }
        S.order[rank] = (uint16_t)i;
        S.w[rank] = c;
    }
    __syncthreads();
    if (lane == 0) {
        const int m = S.m;
        int li = 0, ii = m, next = m;                            // two queues: leaves [li, m), internal nodes [ii, next)
        while (next < 2 * m - 1) {
            int pick[2];
            for (int k = 0; k < 2; ++k) {
                const bool leaf = li < m && (ii >= next || S.w[li] <= S.w[ii]);          // ties: a leaf first, then the older internal node
                pick[k] = leaf ? li++ : ii++;
            }
            S.w[next] = S.w[pick[0]] + S.w[pick[1]];
            S.parent[pick[0]] = S.parent[pick[1]] = (uint16_t)next;
            ++next;
        }
        int bl[16];
        for (int l = 0; l < 16; ++l) bl[l] = 0;
        S.depth[2 * m - 2] = 0;
        for (int k = 2 * m - 3; k >= 0; --k) {
            const int dp = S.depth[S.parent[k]] + 1;
            S.depth[k] = (uint16_t)dp;
            if (k < m) ++bl[dp < limit ? dp : limit];           // the deeper counts fold into the limit
        }
        int total = 0;
        for (int l = 1; l <= limit; ++l) total += bl[l] << (limit - l);
        while (total > (1 << limit) && bl[limit] > 0) {
            --bl[limit];
            int l = limit - 1;
            while (l > 0 && bl[l] == 0) --l;
            if (l == 0) break;                                   // (cannot happen for n <= 2^limit)
            --bl[l];
            bl[l + 1] += 2;
            --total;
        }
        int k = 0;
        for (int l = limit; l >= 1; --l)
            for (int c = 0; c < bl[l] && k < m; ++c) lens[S.order[k++]] = (uint8_t)l;          // sorted order: the rarest get the longest
    }
    __syncthreads();
}

// canonical codes (RFC 1951 3.2.2), bit-reversed so that they go out least significant bit first: code | length << 16; lane 0 calls it
__device__ void pe_canonical(const uint8_t* lens, int n, uint32_t* codes) {
    int cnt[16], next[16];
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int i = 0; i < n; ++i) ++cnt[lens[i] & 15];
    cnt[0] = 0;
    int code = 0;
    next[0] = 0;
    for (int l = 1; l < 16; ++l) { code = (code + cnt[l - 1]) << 1; next[l] = code; }
    for (int i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        codes[i] = l ? (__brev((uint32_t)next[l]++) >> (32 - l)) | (uint32_t)l << 16 : 0u;
    }
}

// the header's run-length symbols of lens[0 ... n): sym | extra value << 8 appended to seq, counted in hist; returns the new length
__device__ int pe_rle(const uint8_t* lens, int n, uint16_t* seq, int ns, uint32_t* hist) {
    int i = 0;
    while (i < n) {
        const int v = lens[i];
        int r = 1;
        while (i + r < n && lens[i + r] == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) { const int t = r < 138 ? r : 138; seq[ns++] = (uint16_t)(18 | (t - 11) << 8); ++hist[18]; r -= t; }
            if (r >= 3) { seq[ns++] = (uint16_t)(17 | (r - 3) << 8); ++hist[17]; r = 0; }
        } else {
            seq[ns++] = (uint16_t)v; ++hist[v]; --r;
            while (r >= 3) { const int t = r < 6 ? r : 6; seq[ns++] = (uint16_t)(16 | (t - 3) << 8); ++hist[16]; r -= t; }
        }
        for (; r > 0; --r) { seq[ns++] = (uint16_t)v; ++hist[v]; }
    }
    return ns;
}

struct PeBits {                                                  // lane 0's serial writer: whole 32-bit words, the last one zero-filled
    uint32_t* w;
    uint64_t acc;
    int n, wi;
    __device__ __forceinline__ void put(uint32_t v, int nb) {
        acc |= (uint64_t)v << n;
        n += nb;
        if (n >= 32) { w[wi++] = (uint32_t)acc; acc >>= 32; n -= 32; }
    }
    __device__ __forceinline__ void finish() { if (n > 0) w[wi++] = (uint32_t)acc; }
};

struct PeCodesLds {
    uint32_t hist[PE_TABLE];      // literal/length counts, distance counts from 288
    uint32_t clhist[19];
    uint8_t lens[PE_TABLE], cllens[19];
    uint16_t seq[PE_TABLE];
    uint32_t codes[PE_TABLE], clcodes[19];
    int ns, btype, hdr_bits, body_bits;
    PeHuff H;
};

__constant__ const uint8_t c_pe_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// grid (chunks, F), 64 threads
__global__ void __launch_bounds__(64) k_pe_codes(const uint8_t* __restrict__ raw, PeDef d, PeDist cand, int stored_only,
                                                 uint16_t* __restrict__ match, int* __restrict__ info, int* __restrict__ nbytes,
                                                 uint32_t* __restrict__ table, uint8_t* __restrict__ slots) {
    __shared__ PeCodesLds S;
    const int c = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    const uint8_t* r = raw + (size_t)f * d.n;
    uint16_t* mt = match + (size_t)f * d.n;
    const size_t cs = (size_t)c * d.C, ce = cs + d.C < d.n ? cs + d.C : d.n;
    const int len = (int)(ce - cs);
    const bool last = c == d.nch - 1;
    const size_t ci = (size_t)f * d.nch + c;
    uint32_t* slot = (uint32_t*)(slots + ci * d.slot);
    const int stored_bits = 40 + 8 * len;
    if (stored_only) {
        if (lane == 0) {
            info[ci * PE_INFO] = 0; info[ci * PE_INFO + 1] = 0; info[ci * PE_INFO + 2] = 0;
            info[ci * PE_INFO + 3] = nbytes[ci] = 5 + len + (last ? 0 : 5);
        }
        return;
    }
    for (int i = lane; i < PE_TABLE; i += 64) S.hist[i] = 0;
    if (lane < 19) S.clhist[lane] = 0;
    __syncthreads();
    // the serial greedy parse: `cur` is the next token's position, the same in every lane
    int cur = 0;
    for (int base = 0; base < len; base += 64) {
        const int q = base + lane;
        const uint16_t mv = q < len ? mt[cs + q] : (uint16_t)0;
        const int ml = mv & 511, step = ml ? ml : 1;
        unsigned long long mask = 0;
        while (cur < base + 64 && cur < len) {
            const int idx = __builtin_amdgcn_readfirstlane(cur - base);
            mask |= 1ull << idx;
            cur = __builtin_amdgcn_readfirstlane(cur + __builtin_amdgcn_readlane(step, idx));
        }
        if ((mask >> lane) & 1ull) {
            mt[cs + q] = (uint16_t)(mv | 0x8000u);
            if (ml) {
                int code, nb, ext;
                pe_len_code(ml, code, nb, ext);
                atomicAdd(&S.hist[257 + code], 1u);
                pe_dist_code(cand.d[(mv >> 9) & 3], code, nb, ext);
                atomicAdd(&S.hist[288 + code], 1u);
            } else {
                atomicAdd(&S.hist[r[cs + q]], 1u);
            }
        }
    }
    if (lane == 0) S.hist[256] = 1;
    __syncthreads();
    pe_huff_lengths(S.H, S.hist, 286, 15, S.lens, lane);
    pe_huff_lengths(S.H, S.hist + 288, 30, 15, S.lens + 288, lane);
    int hlit = 286, hdist = 30;
    if (lane == 0) {
        S.lens[286] = S.lens[287] = S.lens[318] = S.lens[319] = 0;
        while (hlit > 257 && S.lens[hlit - 1] == 0) --hlit;
        while (hdist > 1 && S.lens[288 + hdist - 1] == 0) --hdist;
        int ns = pe_rle(S.lens, hlit, S.seq, 0, S.clhist);      // runs do not cross from one alphabet into the other
        S.ns = pe_rle(S.lens + 288, hdist, S.seq, ns, S.clhist);
    }
    __syncthreads();
    pe_huff_lengths(S.H, S.clhist, 19, 7, S.cllens, lane);
    if (lane == 0) {
        int hclen = 19;
        while (hclen > 4 && S.cllens[c_pe_order[hclen - 1]] == 0) --hclen;
        int hdr = 3 + 14 + 3 * hclen;
        for (int i = 0; i < S.ns; ++i) {
            const int s = S.seq[i] & 255;
            hdr += S.cllens[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
        }
        int dyn = 0, fix = 0;
        for (int i = 0; i < 286; ++i) {
            const int e = i > 256 ? pe_len_extra(i - 257) : 0, n = (int)S.hist[i];
            dyn += n * (S.lens[i] + e);
            fix += n * (pe_fixed_len(i) + e);
        }
        for (int i = 0; i < 30; ++i) {
            const int e = pe_dist_extra(i), n = (int)S.hist[288 + i];
            dyn += n * (S.lens[288 + i] + e);
            fix += n * (5 + e);
        }
        dyn += hdr; fix += 3;
        const int bt = stored_bits <= fix && stored_bits <= dyn ? 0 : fix <= dyn ? 1 : 2;          // ties: stored, fixed, dynamic
        S.btype = bt;
        if (bt == 1) {
            for (int i = 0; i < 288; ++i) S.lens[i] = (uint8_t)pe_fixed_len(i);
            for (int i = 288; i < 320; ++i) S.lens[i] = 5;
            hdr = 3;
        }
        S.hdr_bits = bt ? hdr : 0;
        S.body_bits = bt == 2 ? dyn : bt == 1 ? fix : 0;
        if (bt) {
            pe_canonical(S.lens, 288, S.codes);
            pe_canonical(S.lens + 288, 32, S.codes + 288);
            PeBits bw{slot, 0, 0, 0};
            bw.put((last ? 1u : 0u) | (uint32_t)bt << 1, 3);
            if (bt == 2) {
                pe_canonical(S.cllens, 19, S.clcodes);
                bw.put((uint32_t)(hlit - 257), 5); bw.put((uint32_t)(hdist - 1), 5); bw.put((uint32_t)(hclen - 4), 4);
                for (int i = 0; i < hclen; ++i) bw.put(S.cllens[c_pe_order[i]], 3);
                for (int i = 0; i < S.ns; ++i) {
                    const int s = S.seq[i] & 255, e = S.seq[i] >> 8;
                    bw.put(S.clcodes[s] & 0xFFFFu, (int)(S.clcodes[s] >> 16));
                    if (s >= 16) bw.put((uint32_t)e, s == 16 ? 2 : s == 17 ? 3 : 7);
                }
            }
            bw.finish();
        }
        const int e = S.body_bits;                               // bits up to and including the end-of-block code
        info[ci * PE_INFO] = bt;
        info[ci * PE_INFO + 1] = S.hdr_bits;
        info[ci * PE_INFO + 2] = e;
        info[ci * PE_INFO + 3] = nbytes[ci] = bt == 0 ? 5 + len + (last ? 0 : 5) : last ? (e + 7) >> 3 : ((e + 3 + 7) >> 3) + 4;
    }
    __syncthreads();
    if (S.btype == 0) return;
    for (int i = lane; i < PE_TABLE; i += 64) table[ci * PE_TABLE + i] = S.codes[i];
    for (int w = (S.hdr_bits + 31) / 32 + lane; w < d.slot / 4; w += 64) slot[w] = 0;          // the words the tokens will be OR-ed into
}

// grid (B), 64 threads: dsn_huff_lengths
__global__ void __launch_bounds__(64) k_pe_huff(const uint32_t* __restrict__ counts, int n, int limit, uint8_t* __restrict__ lengths) {
    __shared__ PeHuff H;
    __shared__ uint8_t s_lens[288];
    pe_huff_lengths(H, counts + (size_t)blockIdx.x * n, n, limit, s_lens, threadIdx.x);
    for (int i = threadIdx.x; i < n; i += 64) lengths[(size_t)blockIdx.x * n + i] = s_lens[i];
}

// ---- emission --------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pe_or_bits(uint32_t* s, int words, int at, uint64_t val, int n) {          // n <= 48 bits of val at bit `at`
    const int w = at >> 5, sh = at & 31;
    if (n == 0 || w + 2 >= words) return;                        // (never: a chunk's bits end 22 bytes before its slot does)
    const uint64_t lo = val << sh;
    const uint32_t hi = sh ? (uint32_t)(val >> (64 - sh)) : 0u;
    if ((uint32_t)lo) atomicOr(&s[w], (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) atomicOr(&s[w + 1], (uint32_t)(lo >> 32));
    if (hi) atomicOr(&s[w + 2], hi);
}

// exclusive scan over the workgroup's 256 threads in thread order; returns the total
__device__ __forceinline__ int pe_block_scan(int v, int& total) {
    __shared__ int s_w[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(s, o);
        if (lane >= o) s += u;
    }
    __syncthreads();                                             // (s_w may still be read from the call before)
    if (lane == 63) s_w[w] = s;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { if (i < w) base += s_w[i]; total += s_w[i]; }
    return base + s - v;
}

// grid (chunks, F), 256 threads
__global__ void __launch_bounds__(256) k_pe_emit(const uint8_t* __restrict__ raw, PeDef d, PeDist cand, const uint16_t* __restrict__ match,
                                                 const int* __restrict__ info, const uint32_t* __restrict__ table, uint8_t* __restrict__ slots) {
    __shared__ uint32_t s_code[PE_TABLE];
    const int c = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    const uint8_t* r = raw + (size_t)f * d.n;
    const uint16_t* mt = match + (size_t)f * d.n;
    const size_t cs = (size_t)c * d.C, ce = cs + d.C < d.n ? cs + d.C : d.n;
    const int len = (int)(ce - cs);
    const bool last = c == d.nch - 1;
    const size_t ci = (size_t)f * d.nch + c;
    uint8_t* sb = slots + ci * d.slot;
    const int bt = info[ci * PE_INFO];
    if (bt == 0) {
        if (t < 5) sb[t] = t == 0 ? (uint8_t)(last ? 1 : 0) : t == 1 ? (uint8_t)len : t == 2 ? (uint8_t)(len >> 8) : t == 3 ? (uint8_t)~len : (uint8_t)(~len >> 8);
        for (int i = t; i < len; i += 256) sb[5 + i] = r[cs + i];
        if (!last && t < 5) sb[5 + len + t] = t < 3 ? 0 : 0xFF;
        return;
    }
    for (int i = t; i < PE_TABLE; i += 256) s_code[i] = table[ci * PE_TABLE + i];
    __syncthreads();
    uint32_t* slot = (uint32_t*)sb;
    int at = info[ci * PE_INFO + 1];
    for (int base = 0; base < len; base += 256) {
        const int q = base + t;
        const uint16_t mv = q < len ? mt[cs + q] : (uint16_t)0;
        uint64_t val = 0;
        int nb = 0;
        if (mv & 0x8000u) {
            const int ml = mv & 511;
            if (ml) {
                int code, xb, ext;
                pe_len_code(ml, code, xb, ext);
                uint32_t cw = s_code[257 + code];
                val = cw & 0xFFFFu; nb = (int)(cw >> 16);
                val |= (uint64_t)ext << nb; nb += xb;
                pe_dist_code(cand.d[(mv >> 9) & 3], code, xb, ext);
                cw = s_code[288 + code];
                val |= (uint64_t)(cw & 0xFFFFu) << nb; nb += (int)(cw >> 16);
                val |= (uint64_t)ext << nb; nb += xb;
            } else {
                const uint32_t cw = s_code[r[cs + q]];
                val = cw & 0xFFFFu; nb = (int)(cw >> 16);
            }
        }
        int total;
        const int ex = pe_block_scan(nb, total);
        pe_or_bits(slot, d.slot / 4, at + ex, val, nb);
        at += total;
    }
    if (t == 0) {
        const uint32_t cw = s_code[256];
        pe_or_bits(slot, d.slot / 4, at, cw & 0xFFFFu, (int)(cw >> 16));
        const int e = at + (int)(cw >> 16);
        if (!last) pe_or_bits(slot, d.slot / 4, (((e + 3 + 7) >> 3) + 2) * 8, 0xFFFFu, 16);          // 000, zeros to the byte, 00 00 FF FF
    }
}

// grid (chunks, F), 256 threads: nbytes holds the chunks' exclusive prefixes inside tiles, tot the tiles' prefixes and the total
__global__ void __launch_bounds__(256) k_pe_compact(const uint8_t* __restrict__ slots, PeDef d, const int* __restrict__ info,
                                                    const int* __restrict__ nbytes, const int* __restrict__ tot, uint8_t* __restrict__ out,
                                                    size_t capacity, int32_t* __restrict__ lengths, uint32_t* __restrict__ status) {
    const int c = blockIdx.x, f = blockIdx.y;
    const size_t ci = (size_t)f * d.nch + c;
    const uint8_t* sb = slots + ci * d.slot;
    const int nb = info[ci * PE_INFO + 3];
    const size_t off = (size_t)nbytes[ci] + (size_t)tot[(size_t)f * (d.tiles + 1) + c / PE_TILE];
    uint8_t* o = out + (size_t)f * capacity;
    for (int i = threadIdx.x; i < nb; i += 256) if (off + i < capacity) o[off + i] = sb[i];
    if (c == d.nch - 1 && threadIdx.x == 0) {
        lengths[f] = (int32_t)(off + nb);
        status[f] = off + nb > capacity ? DSN_PNGE_OVERFLOW : 0u;
    }
}

// ---- container -------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(zstride / 4096), F), 256 threads, 16 stream bytes each: the copy behind the file's head, and the slices' CRC registers moved
// to the end of the IDAT data and XOR-ed into crc[f]
__global__ void __launch_bounds__(256) k_pe_cont_copy(const uint8_t* __restrict__ zs, size_t zstride, const int32_t* __restrict__ zlen,
                                                      uint8_t* __restrict__ out, size_t capacity, uint32_t* __restrict__ crc) {
    __shared__ uint32_t s_t[256];
    s_t[threadIdx.x] = c_pe_crc.t[threadIdx.x];
    __syncthreads();
    const int f = blockIdx.y;
    const size_t zl = (size_t)(zlen[f] > 0 ? zlen[f] : 0), L = zl < zstride ? zl : zstride;
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    uint32_t reg = 0;
    if (i0 < L) {
        const uint8_t* z = zs + (size_t)f * zstride;
        uint8_t* o = out + (size_t)f * capacity;
        const int have = (int)(L - i0 < 16 ? L - i0 : 16);
        for (int k = 0; k < have; ++k) {
            const uint8_t b = z[i0 + k];
            if (PE_FILE_HEAD + i0 + k < capacity) o[PE_FILE_HEAD + i0 + k] = b;
            reg = s_t[(reg ^ b) & 255u] ^ (reg >> 8);
        }
        reg = pe_crc_shift(reg, (uint32_t)(L - (i0 + have)) + 4u);          // the bytes behind the slice, the Adler-32's four included
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) reg ^= __shfl_xor(reg, o);
    if ((threadIdx.x & 63) == 0 && reg) atomicXor(&crc[f], reg);
}

__device__ __forceinline__ uint32_t pe_crc_bytes(uint32_t reg, const uint8_t* b, int n) {
    for (int i = 0; i < n; ++i) reg = c_pe_crc.t[(reg ^ b[i]) & 255u] ^ (reg >> 8);
    return reg;
}

// F threads: everything of the file but the stream's bytes; length and status
__global__ void k_pe_cont_tail(PeHead head, const int32_t* __restrict__ zlen, const uint32_t* __restrict__ adler, const uint32_t* __restrict__ crc,
                               const uint32_t* __restrict__ status_a, const uint32_t* __restrict__ status_b, int F, uint8_t* __restrict__ out,
                               size_t capacity, int32_t* __restrict__ lengths, uint32_t* __restrict__ status) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    uint8_t* o = out + (size_t)f * capacity;
    const uint32_t L = (uint32_t)(zlen[f] > 0 ? zlen[f] : 0), ad = adler[f], dl = L + 6u;
    auto put = [&](size_t at, uint8_t v) { if (at < capacity) o[at] = v; };
    for (int i = 0; i < 33; ++i) put(i, head.b[i]);
    const uint8_t pre[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
    const uint8_t adb[4] = {(uint8_t)(ad >> 24), (uint8_t)(ad >> 16), (uint8_t)(ad >> 8), (uint8_t)ad};
    for (int i = 0; i < 4; ++i) put(33 + i, (uint8_t)(dl >> (24 - 8 * i)));
    for (int i = 0; i < 6; ++i) put(37 + i, pre[i]);
    for (int i = 0; i < 4; ++i) put((size_t)PE_FILE_HEAD + L + i, adb[i]);
    // CRC-32 of "IDAT" 78 01, the stream and the Adler-32: registers without conditioning are linear, the conditioning is one more term
    uint32_t reg = pe_crc_shift(pe_crc_bytes(0, pre, 6), L + 4u) ^ crc[f] ^ pe_crc_bytes(0, adb, 4);
    reg ^= pe_crc_shift(0xFFFFFFFFu, L + 10u) ^ 0xFFFFFFFFu;
    for (int i = 0; i < 4; ++i) put((size_t)PE_FILE_HEAD + L + 4 + i, (uint8_t)(reg >> (24 - 8 * i)));
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) put((size_t)PE_FILE_HEAD + L + 8 + i, iend[i]);
    const size_t total = (size_t)PE_FILE_EXTRA + L;
    lengths[f] = (int32_t)total;
    status[f] = (status_a ? status_a[f] : 0u) | (status_b ? status_b[f] : 0u) | (total > capacity ? DSN_PNGE_OVERFLOW : 0u);
}

PeDist pe_dist(int bpp, int row_stride) {
    int v[3] = {1, bpp, row_stride};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) if (v[j] < v[i]) { const int t = v[i]; v[i] = v[j]; v[j] = t; }
    PeDist c;
    c.nd = 0;
    c.d[0] = c.d[1] = c.d[2] = 0;
    for (int i = 0; i < 3; ++i)
        if (v[i] >= 1 && v[i] <= 32768 && (c.nd == 0 || c.d[c.nd - 1] != v[i])) c.d[c.nd++] = v[i];
    return c;
}

void pe_launch_adler(const uint8_t* raw, size_t n, int F, uint32_t* sums, uint32_t* adler, hipStream_t st) {
    hipLaunchKernelGGL(k_pe_adler, dim3((unsigned)((n + PE_ADLER_BLOCK - 1) / PE_ADLER_BLOCK), F), dim3(256), 0, st, raw, n, F, sums);
    hipLaunchKernelGGL(k_pe_adler_fin, dim3((F + 255) / 256), dim3(256), 0, st, (const uint32_t*)sums, n, F, adler);
}

}  // namespace

size_t dsn_pnge_deflate_max(size_t n, int chunk) {
    PeDef d;
    return pe_def(n, chunk, d) ? d.zmax : 0;
}

size_t dsn_pnge_deflate_workspace_size(int F, size_t n, int chunk) {
    PeDef d;
    if (F < 1 || F > DSN_PNG_MAX_FILES || !pe_def(n, chunk, d)) return 0;
    return pe_def_carve(nullptr, F, d).bytes;
}

size_t dsn_pnge_raw_bytes(int W, int H, int mode) {
    PeGeom g;
    return pe_geom(W, H, mode, g) ? g.n : 0;
}

size_t dsn_pnge_workspace_size(int F, int W, int H, int mode, int chunk) {
    PeGeom g;
    PeDef d;
    if (F < 1 || F > DSN_PNG_MAX_FILES || !pe_geom(W, H, mode, g) || !pe_def(g.n, chunk, d)) return 0;
    return pe_enc_carve(nullptr, F, g, d).bytes;
}

void dsn_launch_png_filter(const void* images, int dtype, int F, int H, int W, int mode, int rgb, float scale, int filter, uint8_t* raw,
                           uint32_t* status, hipStream_t st) {
    PeGeom g;
    pe_geom(W, H, mode, g);
    hipLaunchKernelGGL(k_pe_zero, dim3((F + 255) / 256), dim3(256), 0, st, status, F);
    hipLaunchKernelGGL(k_pe_filter, dim3(H, F), dim3(256), 0, st, images, dtype, g, rgb, scale, filter, raw, status);
}

void dsn_launch_png_deflate(const uint8_t* raw, int F, size_t n, int bpp, int row_stride, int chunk, int stored_only, uint8_t* out,
                            size_t capacity, int32_t* lengths, uint32_t* status, void* workspace, hipStream_t st) {
    PeDef d;
    pe_def(n, chunk, d);
    const PeDefWs w = pe_def_carve(workspace, F, d);
    const PeDist cand = pe_dist(bpp, row_stride);
    const dim3 chunks(d.nch, F);
    if (!stored_only)
        hipLaunchKernelGGL(k_pe_match, dim3((unsigned)((n + 255) / 256), F), dim3(256), 0, st, raw, d, cand, w.match);
    hipLaunchKernelGGL(k_pe_codes, chunks, dim3(64), 0, st, raw, d, cand, stored_only, w.match, w.info, w.nbytes, w.table, w.slots);
    hipLaunchKernelGGL(k_pe_emit, chunks, dim3(256), 0, st, raw, d, cand, (const uint16_t*)w.match, (const int*)w.info, (const uint32_t*)w.table,
                       w.slots);
    dsn_launch_jpeg_tile_scan(w.nbytes, d.nch, F, w.tot, st);
    hipLaunchKernelGGL(k_pe_compact, chunks, dim3(256), 0, st, (const uint8_t*)w.slots, d, (const int*)w.info, (const int*)w.nbytes,
                       (const int*)w.tot, out, capacity, lengths, status);
}

void dsn_launch_huff_lengths(const uint32_t* counts, int B, int n, int limit, uint8_t* lengths, hipStream_t st) {
    hipLaunchKernelGGL(k_pe_huff, dim3(B), dim3(64), 0, st, counts, n, limit, lengths);
}

// crc_words: uint32 [F] of scratch
void dsn_launch_png_container(const uint8_t* zs, size_t zstride, const int32_t* zlen, const uint32_t* adler, const uint32_t* status_a,
                              const uint32_t* status_b, int F, int W, int H, int channels, uint8_t* out, size_t capacity, int32_t* lengths,
                              uint32_t* status, uint32_t* crc_words, hipStream_t st) {
    const PeHead head = pe_head_host(W, H, channels);
    hipLaunchKernelGGL(k_pe_zero, dim3((F + 255) / 256), dim3(256), 0, st, crc_words, F);
    hipLaunchKernelGGL(k_pe_cont_copy, dim3((unsigned)((zstride + 4095) / 4096), F), dim3(256), 0, st, zs, zstride, zlen, out, capacity, crc_words);
    hipLaunchKernelGGL(k_pe_cont_tail, dim3((F + 255) / 256), dim3(256), 0, st, head, zlen, adler, (const uint32_t*)crc_words, status_a, status_b, F,
                       out, capacity, lengths, status);
}

void dsn_launch_png_adler(const uint8_t* raw, int F, size_t n, uint32_t* adler, uint32_t* sums2, hipStream_t st) {
    hipLaunchKernelGGL(k_pe_zero, dim3((2 * F + 255) / 256), dim3(256), 0, st, sums2, 2 * F);
    pe_launch_adler(raw, n, F, sums2, adler, st);
}

void dsn_launch_png_encode(const void* images, int dtype, int F, int H, int W, int mode, int rgb, float scale, int filter, int chunk,
                           int stored_only, uint8_t* out, size_t capacity, int32_t* lengths, uint32_t* status, void* workspace, hipStream_t st) {
    PeGeom g;
    PeDef d;
    pe_geom(W, H, mode, g);
    pe_def(g.n, chunk, d);
    const PeEncWs w = pe_enc_carve(workspace, F, g, d);
    uint32_t* st0 = w.words, *sums = w.words + F, *adler = w.words + 3 * (size_t)F, *crc = w.words + 4 * (size_t)F;
    dsn_launch_png_filter(images, dtype, F, H, W, mode, rgb, scale, filter, w.raw, st0, st);
    dsn_launch_png_adler(w.raw, F, g.n, adler, sums, st);
    dsn_launch_png_deflate(w.raw, F, g.n, g.bpp, 1 + g.rb, chunk, stored_only, w.zs, d.zcap, w.zlen, w.zstatus, w.def, st);
    dsn_launch_png_container(w.zs, d.zcap, w.zlen, adler, st0, nullptr, F, W, H, g.ch, out, capacity, lengths, status, crc, st);
}
