// dsn_jpegd.hip - baseline JPEG DECODING on the device (dsn_jpeg_parse_host, dsn_jpegd_sync, dsn_jpegd_coefficients,
// dsn_jpegd_pixels, dsn_jpeg_decode; the rule is in include/dsnerf.h and restated in tests/jpeg_decode_restate.py).  Integer
// arithmetic throughout; the only atomics are 32-bit ORs into the frames' flag and "changed" words.
//   k_jd_begin     : clears the frames' eight meta words
//   k_jd_ffcount   : bytes each 16-byte chunk of the stuffed scan keeps (a 0x00 behind a 0xFF goes); markers raise a flag; tile scan
//   k_jd_unstuff   : the kept bytes, placed by the scan's prefix -> the frame's unstuffed stream, its length and subsequence count
//   k_jd_round     : a thread per subsequence, the frame's six Huffman tables in LDS: round 0 decodes from (s B, 0, 0); a later round
//                    takes the exit of s - 1 from the previous round's buffer and decodes again only if that is not the entry it used
//   k_jd_verdict   : per frame: one more round counted; nothing changed -> converged
//   k_jd_zero_coef / k_jd_emit : the subsequences again from their true entries, placed by the tile scan of their block counts
//                    -> int16 coef [F][block][64 zigzag], DC as differences
//   k_jd_status    : the frame's status word from the flags of its own blocks, whether its last block was completed, and the padding
//   k_jd_dc_gather / tile scan / k_jd_dc_apply : per component the prefix sum of the DC differences
//   k_jd_idct      : 32 blocks per workgroup, a lane per column, then per row, through LDS -> the component planes at the MCU grid's size
//   k_jd_colour    : a thread per pixel: libjpeg's fancy 4:2:0 upsampling, YCbCr -> RGB, cropped to H x W; zeros for error frames
// Frames lie side by side in blockIdx.y (k_jd_colour: z); nothing depends on F.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include <string.h>

#define JD_TILE 1024              // the tile scan's tile (dsn_jpeg.hip)
#define JD_CHUNK 16               // bytes of the stuffed scan per thread of the unstuffing kernels
#define JD_THREADS 256
#define JD_MIN_BITS 128           // the smallest subsequence: the subsequence arrays are sized for it
#define JD_MAX_SCAN ((size_t)1 << 27)      // bytes: bit positions stay below 2^30
// meta words of a frame
#define JD_ULEN 0                 // bytes of the unstuffed stream
#define JD_NSUB 1                 // subsequences in use
#define JD_CHANGED 2              // a subsequence decoded again in the round under way
#define JD_CONVERGED 3
#define JD_ROUNDS 4               // rounds run so far
#define JD_FLAGS 5                // DSN_JPEGD_MARKER / _COUNT found while unstuffing
#define JD_PEND 6                 // 1 + the bit position behind the frame's last block (k_jd_emit); 0: it was never completed
#define JD_META 8

namespace {

struct JdZigzag { uint8_t z[64]; };
constexpr JdZigzag jd_make_zigzag() {
    constexpr uint8_t k[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                               21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                               60, 61, 54, 47, 55, 62, 63};          // zigzag position -> natural index
    JdZigzag t{};
    for (int i = 0; i < 64; ++i) t.z[i] = k[i];
    return t;
}
__constant__ const JdZigzag c_jd_zigzag = jd_make_zigzag();

struct JdGeom {
    int H, W, mode, ncomp, mw, mh, bpm, nb;
    int cap;                      // bytes of a frame's unstuffed stream: the scan capacity rounded up to 16
    int chunks, tiles_c;          // 16-byte chunks of it, tiles of their scan
    int s_cap;                    // subsequences at JD_MIN_BITS: the stride of the state arrays
    int ny, tiles_d;              // DC entries per component row, tiles of their scan
};

bool jd_geom(int H, int W, int mode, size_t max_scan, JdGeom& g) {
    int nb;
    if (!dsn_jpeg_blocks(H, W, mode, &nb) || max_scan > JD_MAX_SCAN) return false;
    const int s = mode == DSN_JPEG_420 ? 16 : 8;
    g.H = H; g.W = W; g.mode = mode; g.ncomp = mode == DSN_JPEG_GRAY ? 1 : 3;
    g.mw = (W + s - 1) / s; g.mh = (H + s - 1) / s;
    g.bpm = mode == DSN_JPEG_420 ? 6 : mode == DSN_JPEG_444 ? 3 : 1;
    g.nb = nb;
    g.cap = (int)((max_scan + 15) & ~(size_t)15) + 16;
    g.chunks = g.cap / JD_CHUNK;
    g.tiles_c = (g.chunks + JD_TILE - 1) / JD_TILE;
    g.s_cap = (int)(((long long)g.cap * 8 + JD_MIN_BITS - 1) / JD_MIN_BITS);
    g.ny = g.mw * g.mh * (mode == DSN_JPEG_420 ? 4 : 1);
    g.tiles_d = (g.ny + JD_TILE - 1) / JD_TILE;
    return true;
}
int jd_subs(const JdGeom& g, int B) { return (int)(((long long)g.cap * 8 + B - 1) / B); }          // the grids' extent at B bits

struct JdWorkspace {
    uint32_t* meta; int* kept; int* tot_c; uint8_t* us; uint2* entry; uint2* exit2; int* cnt; int* pre; int* tot_s; uint32_t* flags; int* dc; int* tot_d;
    int16_t* coef; uint8_t* planes; size_t bytes;
};

JdWorkspace jd_carve(void* base, int F, const JdGeom& g) {
    JdWorkspace w;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off += (n + 255) & ~(size_t)255; return (char*)base + at; };
    const size_t tiles_s = (size_t)(g.s_cap + JD_TILE - 1) / JD_TILE;
    w.meta = (uint32_t*)take((size_t)F * JD_META * 4);
    w.kept = (int*)take((size_t)F * g.chunks * 4);
    w.tot_c = (int*)take((size_t)F * (g.tiles_c + 1) * 4);
    w.us = (uint8_t*)take((size_t)F * g.cap);
    w.entry = (uint2*)take((size_t)F * g.s_cap * 8);
    w.exit2 = (uint2*)take((size_t)2 * F * g.s_cap * 8);
    w.cnt = (int*)take((size_t)F * g.s_cap * 4);
    w.pre = (int*)take((size_t)F * g.s_cap * 4);
    w.tot_s = (int*)take((size_t)F * (tiles_s + 1) * 4);
    w.flags = (uint32_t*)take((size_t)F * g.s_cap * 4);
    w.dc = (int*)take((size_t)F * g.ncomp * g.ny * 4);
    w.tot_d = (int*)take((size_t)F * g.ncomp * (g.tiles_d + 1) * 4);
    w.coef = (int16_t*)take((size_t)F * g.nb * 64 * 2);
    w.planes = (uint8_t*)take((size_t)F * g.nb * 64);
    w.bytes = off;
    return w;
}

// ---- the header (host) ---------------------------------------------------------------------------------------------------------------
bool jd_derive(const uint8_t* bits, const uint8_t* vals, int count, bool is_dc, dsn_jpegd_huff& t) {
    memset(&t, 0, sizeof(t));
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        t.bits[len - 1] = bits[len - 1];
        t.base[len - 1] = k - (int32_t)code;
        code += bits[len - 1];
        k += bits[len - 1];
        if (code > (1u << len)) return false;
        t.lim[len - 1] = code << (16 - len);
        code <<= 1;
    }
    if (k != count || k > 256) return false;
    for (int i = 0; i < k; ++i) {
        if (is_dc && vals[i] > 15) return false;
        t.vals[i] = vals[i];
    }
    return true;
}

}  // namespace

int dsn_jpegd_parse_host(const uint8_t* d, size_t n, dsn_jpegd_desc* out) {
    memset(out, 0, sizeof(*out));
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return DSN_JPEGD_NOT_JPEG;
    if (n >= JD_MAX_SCAN) return DSN_JPEGD_TOO_LARGE;
    bool have_q[4] = {}, have_dc[4] = {}, have_ac[4] = {}, have_sof = false;
    int comp_id[3] = {}, nc = 0;
    size_t i = 2;
    for (;;) {
        if (i + 4 > n) return DSN_JPEGD_TRUNCATED;
        if (d[i] != 0xFF) return DSN_JPEGD_BAD_SEGMENT;
        const int m = d[i + 1];
        if (m == 0xFF) { ++i; continue; }          // a fill byte
        const size_t L = (size_t)d[i + 2] << 8 | d[i + 3];
        if (L < 2 || i + 2 + L > n) return DSN_JPEGD_TRUNCATED;
        const uint8_t* seg = d + i + 4;
        const size_t sl = L - 2;
        i += 2 + L;
        if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) continue;
        if (m == 0xDB) {
            for (size_t j = 0; j < sl; j += 65) {
                if (seg[j] >> 4) return DSN_JPEGD_TABLE16;
                if ((seg[j] & 15) > 3 || j + 65 > sl) return DSN_JPEGD_BAD_SEGMENT;
                memcpy(out->quant[seg[j] & 15], seg + j + 1, 64);
                have_q[seg[j] & 15] = true;
            }
        } else if (m == 0xC4) {
            for (size_t j = 0; j < sl;) {
                if (j + 17 > sl || (seg[j] >> 4) > 1 || (seg[j] & 15) > 3) return DSN_JPEGD_BAD_SEGMENT;
                int cnt = 0;
                for (int b = 0; b < 16; ++b) cnt += seg[j + 1 + b];
                if (cnt > 256) return DSN_JPEGD_BAD_TABLE;
                if (j + 17 + cnt > sl) return DSN_JPEGD_BAD_SEGMENT;
                const bool is_dc = (seg[j] >> 4) == 0;
                const int id = seg[j] & 15;
                if (!jd_derive(seg + j + 1, seg + j + 17, cnt, is_dc, is_dc ? out->dc[id] : out->ac[id])) return DSN_JPEGD_BAD_TABLE;
                (is_dc ? have_dc : have_ac)[id] = true;
                j += 17 + cnt;
            }
        } else if (m == 0xC2) {
            return DSN_JPEGD_PROGRESSIVE;
        } else if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
            return DSN_JPEGD_EXTENDED;
        } else if (m >= 0xC9 && m <= 0xCF) {
            return DSN_JPEGD_ARITHMETIC;
        } else if (m == 0xDD) {
            if (sl != 2) return DSN_JPEGD_BAD_SEGMENT;
            if (seg[0] || seg[1]) return DSN_JPEGD_RESTART;
        } else if (m == 0xC0) {
            if (have_sof || sl < 6) return DSN_JPEGD_BAD_SEGMENT;
            if (seg[0] != 8) return DSN_JPEGD_PRECISION;
            out->H = seg[1] << 8 | seg[2];
            out->W = seg[3] << 8 | seg[4];
            nc = seg[5];
            if (nc != 1 && nc != 3) return DSN_JPEGD_COMPONENTS;
            if (sl != (size_t)(6 + 3 * nc) || out->H == 0 || out->W == 0) return DSN_JPEGD_BAD_SEGMENT;
            bool all11 = true, is420 = nc == 3;
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = seg[6 + 3 * c];
                const int hv = seg[7 + 3 * c];
                all11 = all11 && hv == 0x11;
                is420 = is420 && hv == (c == 0 ? 0x22 : 0x11);
                out->qsel[c] = seg[8 + 3 * c];
            }
            if (!all11 && !is420) return DSN_JPEGD_SAMPLING;
            for (int c = 0; c < nc; ++c) if (out->qsel[c] > 3) return DSN_JPEGD_BAD_SEGMENT;
            out->mode = nc == 1 ? DSN_JPEG_GRAY : all11 ? DSN_JPEG_444 : DSN_JPEG_420;
            out->ncomp = nc;
            have_sof = true;
        } else if (m == 0xDA) {
            if (!have_sof || sl < 1) return DSN_JPEGD_BAD_SEGMENT;
            if (seg[0] != nc) return DSN_JPEGD_MULTISCAN;
            if (sl != (size_t)(4 + 2 * nc)) return DSN_JPEGD_BAD_SEGMENT;
            for (int c = 0; c < nc; ++c) {
                const int sel = seg[2 + 2 * c];
                if (seg[1 + 2 * c] != comp_id[c] || (sel >> 4) > 3 || (sel & 15) > 3) return DSN_JPEGD_BAD_SEGMENT;
                out->dcsel[c] = (uint8_t)(sel >> 4);
                out->acsel[c] = (uint8_t)(sel & 15);
            }
            if (seg[1 + 2 * nc] != 0 || seg[2 + 2 * nc] != 63 || seg[3 + 2 * nc] != 0) return DSN_JPEGD_BAD_SEGMENT;
            for (int c = 0; c < nc; ++c)
                if (!have_q[out->qsel[c]] || !have_dc[out->dcsel[c]] || !have_ac[out->acsel[c]]) return DSN_JPEGD_MISSING_TABLE;
            if (d[n - 2] != 0xFF || d[n - 1] != 0xD9 || n - 2 < i) return DSN_JPEGD_NO_EOI;
            int blocks;
            if (!dsn_jpeg_blocks(out->H, out->W, out->mode, &blocks)) return DSN_JPEGD_TOO_LARGE;
            out->scan_offset = (int32_t)i;
            out->scan_length = (int32_t)(n - 2 - i);
            out->file_length = (int32_t)n;
            return DSN_JPEGD_OK;
        } else {
            return DSN_JPEGD_BAD_SEGMENT;
        }
    }
}

namespace {

// ---- unstuffing ------------------------------------------------------------------------------------------------------------------------
// where frame f's scan lies in `files`, clipped to the file's own bytes and to the capacity: nothing outside is ever addressed
struct JdScan { size_t at; int len; bool clipped; };
__device__ __forceinline__ JdScan jd_scan(size_t files_bytes, const int64_t* __restrict__ offsets, const dsn_jpegd_desc* __restrict__ desc,
                                          int f, int max_scan) {
    JdScan s;
    const int64_t o0 = offsets[f], o1 = offsets[f + 1];
    const int64_t so = desc[f].scan_offset, sl = desc[f].scan_length;
    const bool ok = o0 >= 0 && o0 <= o1 && (uint64_t)o1 <= (uint64_t)files_bytes && so >= 0 && sl >= 0 && so <= o1 - o0;
    int64_t len = ok ? sl : 0;
    if (ok && len > o1 - o0 - so) len = o1 - o0 - so;
    if (len > max_scan) len = max_scan;
    s.at = ok ? (size_t)(o0 + so) : 0;
    s.len = (int)len;
    s.clipped = !ok || len != sl;
    return s;
}

// 16 bytes from byte offset a of `files` by two aligned 16-byte loads, each only where it lies inside [0, total) (total % 16 == 0)
__device__ __forceinline__ void jd_load16(const uint8_t* __restrict__ files, size_t total, size_t a, uint8_t b[JD_CHUNK]) {
    const size_t a0 = a & ~(size_t)15;
    const int sh = (int)(a & 15), ws = sh >> 2, bs = (sh & 3) * 8;
    const uint4 z = make_uint4(0, 0, 0, 0);
    const uint4 lo = a0 + 16 <= total ? *(const uint4*)(files + a0) : z, hi = a0 + 32 <= total ? *(const uint4*)(files + a0 + 16) : z;
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t t[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) t[j] = ws == 0 ? w[j] : ws == 1 ? w[j + 1] : ws == 2 ? w[j + 2] : w[j + 3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t v = bs ? (t[j] >> bs) | (t[j + 1] << (32 - bs)) : t[j];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[4 * j + i] = (uint8_t)(v >> (8 * i));
    }
}

// chunk c of the frame's scan: its bytes, how many belong to the scan, which of them are stuffed zeros (bit i of `drop`), and
// whether a marker shows (a non-zero byte behind a 0xFF, or a 0xFF as the scan's last byte)
__device__ __forceinline__ int jd_chunk(const uint8_t* __restrict__ files, size_t total, const JdScan& sc, int c, uint8_t b[JD_CHUNK],
                                        uint32_t& drop, bool& marker) {
    drop = 0;
    marker = false;
    const int have = min(JD_CHUNK, sc.len - c * JD_CHUNK);
    if (have <= 0) return 0;
    const size_t a = sc.at + (size_t)c * JD_CHUNK;
    jd_load16(files, total, a, b);
    int prev = c > 0 ? files[a - 1] : 0;
#pragma unroll
    for (int i = 0; i < JD_CHUNK; ++i) {
        if (i < have) {
            if (prev == 0xFF) { if (b[i] == 0) drop |= 1u << i; else marker = true; }
            if (b[i] == 0xFF && c * JD_CHUNK + i == sc.len - 1) marker = true;
            prev = b[i];
        }
    }
    return have;
}

__global__ void k_jd_begin(uint32_t* __restrict__ meta, int F) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < F * JD_META) meta[i] = 0;
}

// grid (ceil(chunks / 256), F)
__global__ void __launch_bounds__(JD_THREADS) k_jd_ffcount(const uint8_t* __restrict__ files, size_t files_bytes,
                                                           const int64_t* __restrict__ offsets, const dsn_jpegd_desc* __restrict__ desc,
                                                           JdGeom g, uint32_t* __restrict__ meta, int* __restrict__ kept) {
    const int f = blockIdx.y, c = blockIdx.x * JD_THREADS + threadIdx.x;
    if (c >= g.chunks) return;
    const JdScan sc = jd_scan(files_bytes, offsets, desc, f, g.cap - 16);
    uint8_t b[JD_CHUNK];
    uint32_t drop;
    bool marker;
    const int have = jd_chunk(files, files_bytes, sc, c, b, drop, marker);
    kept[(size_t)f * g.chunks + c] = have - __popc(drop);
    const uint32_t fl = (marker ? DSN_JPEGD_MARKER : 0u) | (c == 0 && sc.clipped ? DSN_JPEGD_COUNT : 0u);
    if (fl) atomicOr(&meta[f * JD_META + JD_FLAGS], fl);
}

// grid (ceil(chunks / 256), F): the kept bytes behind the chunk's prefix; the frame's length and subsequence count
__global__ void __launch_bounds__(JD_THREADS) k_jd_unstuff(const uint8_t* __restrict__ files, size_t files_bytes,
                                                           const int64_t* __restrict__ offsets, const dsn_jpegd_desc* __restrict__ desc,
                                                           JdGeom g, int B, const int* __restrict__ kept, const int* __restrict__ tot_c,
                                                           uint32_t* __restrict__ meta, uint8_t* __restrict__ us) {
    const int f = blockIdx.y, c = blockIdx.x * JD_THREADS + threadIdx.x;
    if (c >= g.chunks) return;
    const int* t = tot_c + (size_t)f * (g.tiles_c + 1);
    if (c == 0) {
        const int ulen = min(max(t[g.tiles_c], 0), g.cap - 16);
        meta[f * JD_META + JD_ULEN] = (uint32_t)ulen;
        meta[f * JD_META + JD_NSUB] = (uint32_t)max(1, (int)(((long long)ulen * 8 + B - 1) / B));
    }
    const JdScan sc = jd_scan(files_bytes, offsets, desc, f, g.cap - 16);
    uint8_t b[JD_CHUNK];
    uint32_t drop;
    bool marker;
    const int have = jd_chunk(files, files_bytes, sc, c, b, drop, marker);
    if (have == 0) return;
    int at = kept[(size_t)f * g.chunks + c] + t[c / JD_TILE];
    uint8_t* o = us + (size_t)f * g.cap;
#pragma unroll
    for (int i = 0; i < JD_CHUNK; ++i)
        if (i < have && !(drop >> i & 1)) { if (at >= 0 && at < g.cap) o[at] = b[i]; ++at; }
}

// ---- the entropy decoder ---------------------------------------------------------------------------------------------------------------
struct JdTab { uint32_t lim[6][16]; int32_t base[6][16]; uint32_t vals[6][64]; };          // [component * 2 + (AC ? 1 : 0)]

__device__ __forceinline__ void jd_load_tables(const dsn_jpegd_desc* __restrict__ d, int ncomp, JdTab& T) {
    for (int i = threadIdx.x; i < 6 * 96; i += JD_THREADS) {
        const int t = i / 96, j = i % 96, c = t >> 1;
        if (c >= ncomp) continue;
        const dsn_jpegd_huff* h = (t & 1) ? &d->ac[d->acsel[c] & 3] : &d->dc[d->dcsel[c] & 3];
        if (j < 16) T.lim[t][j] = h->lim[j];
        else if (j < 32) T.base[t][j - 16] = h->base[j - 16];
        else T.vals[t][j - 32] = ((const uint32_t*)h->vals)[j - 32];
    }
}

// 32 bits of the unstuffed stream from bit p on; bits at and past `total` read as 0, and no word at or past `words` is touched
__device__ __forceinline__ uint32_t jd_word(const uint32_t* __restrict__ us, uint32_t words, uint32_t total, uint32_t i) {
    if (i >= words || i * 32u >= total) return 0;
    uint32_t w = __builtin_bswap32(us[i]);
    const uint32_t left = total - i * 32u;
    if (left < 32) w &= ~0u << (32 - left);
    return w;
}
__device__ __forceinline__ uint32_t jd_peek(const uint32_t* __restrict__ us, uint32_t words, uint32_t total, uint32_t p) {
    const uint32_t i = p >> 5, o = p & 31;
    const uint32_t a = jd_word(us, words, total, i);
    return o ? (a << o) | (jd_word(us, words, total, i + 1) >> (32 - o)) : a;
}

// a reader that walks forward: the word under p and the two behind it sit in registers, and the load that replaces one is issued a
// word (half a dozen symbols) before its bits are needed, off the symbols' dependency chain
struct JdBits {
    const uint32_t* __restrict__ us;
    uint32_t words, total, i, w0, w1, w2;
    __device__ __forceinline__ void start(uint32_t p) {
        i = p >> 5;
        w0 = jd_word(us, words, total, i); w1 = jd_word(us, words, total, i + 1); w2 = jd_word(us, words, total, i + 2);
    }
    __device__ __forceinline__ uint32_t peek(uint32_t p) {          // p never moves back, and by less than 32 bits a time
        const uint32_t j = p >> 5;
        if (j == i + 1) { i = j; w0 = w1; w1 = w2; w2 = jd_word(us, words, total, i + 2); }
        else if (j != i) start(p);
        const uint32_t o = p & 31;
        return o ? (w0 << o) | (w1 >> (32 - o)) : w0;
    }
};

// symbols from state (p, k, z) until p >= end or a symbol needs bits past the scan's end.  EMIT: coefficients go to coef [nb][64];
// `blk` is the index the next block to START gets (the one under way is blk - 1); decoding stops behind block nb - 1, whose end
// goes to *pend, and nothing past it is looked at (flags then speak of the frame's own blocks only).
template <bool EMIT>
__device__ __forceinline__ void jd_run(const JdTab& T, const uint32_t* __restrict__ us, uint32_t words, uint32_t total, int mode, int bpm,
                                       uint32_t& p, int& k, int& z, uint32_t end, int& started, uint32_t& flags,
                                       int16_t* __restrict__ coef, int blk, int nb, uint32_t* __restrict__ pend) {
    JdBits rd;
    rd.us = us; rd.words = words; rd.total = total;
    rd.start(p);
    while (p < end) {
        if (EMIT && (blk > nb || (z == 0 && blk == nb))) break;
        const uint32_t v32 = rd.peek(p), v = v32 >> 16;
        const int comp = mode == DSN_JPEG_420 ? (k < 4 ? 0 : k - 3) : mode == DSN_JPEG_444 ? k : 0;
        const int t = comp * 2 + (z ? 1 : 0);
        int l = 0;
        while (l < 16 && v >= T.lim[t][l]) ++l;
        if (l == 16) {                                          // no code: one bit on, unless the window hangs over the end
            if (total - p < 16) break;
            ++p;
            flags |= DSN_JPEGD_UNMATCHED;
            continue;
        }
        const int len = l + 1;
        const uint32_t idx = (uint32_t)(T.base[t][l] + (int32_t)(v >> (16 - len))) & 255u;
        const int sym = (int)(T.vals[t][idx >> 2] >> (8 * (idx & 3))) & 255;
        const int s = sym & 15;
        if (p + len + s > total) break;
        int val = s ? (int)((v32 >> (32 - len - s)) & ((1u << s) - 1)) : 0;
        if (s && !(val >> (s - 1))) val -= (1 << s) - 1;
        p += len + s;
        if (z == 0) {
            if (EMIT && blk < nb) coef[(size_t)blk * 64] = (int16_t)val;
            ++blk;
            ++started;
            z = 1;
        } else {
            const int r = sym >> 4;
            if (s == 0) {
                z = r == 15 ? z + 16 : 64;
                if (z > 64) flags |= DSN_JPEGD_OVERRUN;
            } else {
                z += r;
                if (z > 63) {
                    flags |= DSN_JPEGD_OVERRUN;
                    z = 64;
                } else {
                    if (EMIT && blk > 0 && blk <= nb) coef[(size_t)(blk - 1) * 64 + z] = (int16_t)val;
                    ++z;
                }
            }
        }
        if (z >= 64) {
            k = k + 1 == bpm ? 0 : k + 1;
            z = 0;
            if (EMIT && blk == nb) { *pend = p + 1; break; }
        }
    }
}

__device__ __forceinline__ uint2 jd_pack(uint32_t p, int k, int z) { return make_uint2(p, (uint32_t)k | (uint32_t)z << 8); }
__device__ __forceinline__ void jd_unpack(uint2 s, int bpm, uint32_t& p, int& k, int& z) {          // (a state from memory is made safe)
    p = s.x;
    k = (int)((s.y & 255u) % (uint32_t)bpm);
    z = (int)(s.y >> 8 & 63u);
}

// grid (ceil(SB / 256), F), SB = the subsequences the capacity holds at B bits
template <bool FIRST>
__global__ void __launch_bounds__(JD_THREADS) k_jd_round(const dsn_jpegd_desc* __restrict__ desc, JdGeom g, int B, int SB,
                                                         const uint8_t* __restrict__ us_all, uint32_t* __restrict__ meta,
                                                         uint2* __restrict__ entry, uint2* __restrict__ exit2, int* __restrict__ cnt,
                                                         uint32_t* __restrict__ flags) {
    __shared__ JdTab T;
    const int f = blockIdx.y, F = gridDim.y;
    uint32_t* m = meta + f * JD_META;
    if (!FIRST && m[JD_CONVERGED]) return;                      // (the same for the whole workgroup)
    jd_load_tables(desc + f, g.ncomp, T);
    __syncthreads();
    const int s = blockIdx.x * JD_THREADS + threadIdx.x;
    if (s >= SB || s >= g.s_cap) return;
    const int nsub = (int)min(m[JD_NSUB], (uint32_t)min(SB, g.s_cap));
    const uint32_t total = min(m[JD_ULEN], (uint32_t)(g.cap - 16)) * 8u, r = FIRST ? 0u : m[JD_ROUNDS];
    const size_t row = (size_t)f * g.s_cap;
    if (s >= nsub) {
        if (FIRST) { cnt[(size_t)f * SB + s] = 0; flags[(size_t)f * SB + s] = 0; }
        return;
    }
    uint2* dst = exit2 + (size_t)(r & 1) * F * g.s_cap + row;
    const uint2* src = exit2 + (size_t)((r + 1) & 1) * F * g.s_cap + row;
    uint2 e;
    if (FIRST) {
        e = jd_pack((uint32_t)s * (uint32_t)B, 0, 0);
        if (s == 0) m[JD_CHANGED] = nsub > 1 ? 1u : 0u;
    } else {
        if (s == 0) { dst[0] = src[0]; return; }
        e = src[s - 1];
        const uint2 mine = entry[row + s];
        if (e.x == mine.x && e.y == mine.y) { dst[s] = src[s]; return; }
        atomicOr(&m[JD_CHANGED], 1u);
    }
    uint32_t p, fl = 0;
    int k, z, started = 0;
    jd_unpack(e, g.bpm, p, k, z);
    const uint32_t end = min((uint32_t)(s + 1) * (uint32_t)B, total);
    jd_run<false>(T, (const uint32_t*)(us_all + (size_t)f * g.cap), (uint32_t)g.cap / 4, total, g.mode, g.bpm, p, k, z, end, started, fl,
                  nullptr, 0, 0, nullptr);
    entry[row + s] = e;
    dst[s] = jd_pack(p, k, z);
    cnt[(size_t)f * SB + s] = started;
    flags[(size_t)f * SB + s] = fl;
}

__global__ void k_jd_verdict(uint32_t* __restrict__ meta, int F, uint32_t* __restrict__ out_converged, int32_t* __restrict__ out_rounds) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    uint32_t* m = meta + f * JD_META;
    if (!m[JD_CONVERGED]) {
        m[JD_ROUNDS] += 1;
        if (m[JD_CHANGED] == 0) m[JD_CONVERGED] = 1;
        m[JD_CHANGED] = 0;
    }
    if (out_converged) out_converged[f] = m[JD_CONVERGED];
    if (out_rounds) out_rounds[f] = (int32_t)m[JD_ROUNDS];
}

// (the scan works in place: cnt itself stays); n >= F: the frames' end-of-last-block words are cleared on the way
__global__ void k_jd_copy(const int* __restrict__ a, int* __restrict__ b, size_t n, uint32_t* __restrict__ meta, int F) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)F) meta[i * JD_META + JD_PEND] = 0;
    if (i < n) b[i] = a[i];
}

__global__ void k_jd_zero_coef(uint4* __restrict__ coef, size_t n16) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n16) coef[i] = make_uint4(0, 0, 0, 0);
}

// grid (ceil(SB / 256), F): cnt (a copy of the rounds' counts) holds the exclusive prefix inside its tile, tot_s the tiles' prefixes
__global__ void __launch_bounds__(JD_THREADS) k_jd_emit(const dsn_jpegd_desc* __restrict__ desc, JdGeom g, int B, int SB, int tiles_s,
                                                        const uint8_t* __restrict__ us_all, uint32_t* __restrict__ meta,
                                                        const uint2* __restrict__ entry, const int* __restrict__ cnt,
                                                        const int* __restrict__ tot_s, uint32_t* __restrict__ flags,
                                                        int16_t* __restrict__ coef) {
    __shared__ JdTab T;
    const int f = blockIdx.y;
    uint32_t* m = meta + f * JD_META;
    jd_load_tables(desc + f, g.ncomp, T);
    __syncthreads();
    const int s = blockIdx.x * JD_THREADS + threadIdx.x;
    const int nsub = (int)min(m[JD_NSUB], (uint32_t)min(SB, g.s_cap));
    if (s >= nsub || !m[JD_CONVERGED]) return;
    const uint32_t total = min(m[JD_ULEN], (uint32_t)(g.cap - 16)) * 8u;
    uint32_t p, fl = 0;
    int k, z, started = 0;
    jd_unpack(entry[(size_t)f * g.s_cap + s], g.bpm, p, k, z);
    const int blk = cnt[(size_t)f * SB + s] + tot_s[(size_t)f * (tiles_s + 1) + s / JD_TILE];
    const uint32_t end = min((uint32_t)(s + 1) * (uint32_t)B, total);
    jd_run<true>(T, (const uint32_t*)(us_all + (size_t)f * g.cap), (uint32_t)g.cap / 4, total, g.mode, g.bpm, p, k, z, end, started, fl,
                 coef + (size_t)f * g.nb * 64, blk, g.nb, &m[JD_PEND]);
    flags[(size_t)f * SB + s] = fl;
}

// grid (F), 256 threads
__global__ void __launch_bounds__(JD_THREADS) k_jd_status(JdGeom g, int SB, const uint8_t* __restrict__ us_all,
                                                          const uint32_t* __restrict__ meta, const uint32_t* __restrict__ flags,
                                                          uint32_t* __restrict__ status) {
    __shared__ uint32_t s_or;
    const int f = blockIdx.x;
    const uint32_t* m = meta + f * JD_META;
    if (threadIdx.x == 0) s_or = 0;
    __syncthreads();
    if (!m[JD_CONVERGED]) {                                     // (the same for the whole workgroup)
        if (threadIdx.x == 0) status[f] = DSN_JPEGD_UNCONVERGED;
        return;
    }
    const int nsub = (int)min(m[JD_NSUB], (uint32_t)min(SB, g.s_cap));
    uint32_t fl = 0;
    for (int s = threadIdx.x; s < nsub; s += JD_THREADS) fl |= flags[(size_t)f * SB + s];
    if (fl) atomicOr(&s_or, fl);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t total = min(m[JD_ULEN], (uint32_t)(g.cap - 16)) * 8u;
    uint32_t st = s_or | m[JD_FLAGS];
    if (m[JD_PEND] == 0) st |= DSN_JPEGD_COUNT;
    if (st & (DSN_JPEGD_UNMATCHED | DSN_JPEGD_OVERRUN | DSN_JPEGD_MARKER | DSN_JPEGD_COUNT)) st |= DSN_JPEGD_CORRUPT;
    const uint32_t p = m[JD_PEND] ? m[JD_PEND] - 1 : total, rest = p <= total ? total - p : 0;
    if (rest > 7) st |= DSN_JPEGD_PADDING;
    else if (rest && (jd_peek((const uint32_t*)(us_all + (size_t)f * g.cap), (uint32_t)g.cap / 4, total, p) >> (32 - rest)) != (1u << rest) - 1)
        st |= DSN_JPEGD_PADDING;
    status[f] = st;
}

// ---- DC prediction -----------------------------------------------------------------------------------------------------------------
// block b of a frame -> its component and its index among that component's blocks
__device__ __forceinline__ void jd_block_comp(const JdGeom& g, int b, int& comp, int& j) {
    const int mcu = b / g.bpm, k = b % g.bpm;
    if (g.mode == DSN_JPEG_420) { comp = k < 4 ? 0 : k - 3; j = k < 4 ? mcu * 4 + k : mcu; }
    else { comp = k; j = mcu; }
}

// grid (ceil(ny / 256), F * ncomp): row (f, comp) of dc = the component's DC differences in scan order, zeros behind them
__global__ void __launch_bounds__(JD_THREADS) k_jd_dc_gather(const int16_t* __restrict__ coef, JdGeom g, int* __restrict__ dc) {
    const int j = blockIdx.x * JD_THREADS + threadIdx.x, f = blockIdx.y / g.ncomp, comp = blockIdx.y % g.ncomp;
    if (j >= g.ny) return;
    int b = -1;
    if (g.mode == DSN_JPEG_420) { if (comp == 0) b = (j >> 2) * 6 + (j & 3); else if (j < g.mw * g.mh) b = j * 6 + 3 + comp; }
    else b = j * g.bpm + comp;
    dc[(size_t)blockIdx.y * g.ny + j] = b >= 0 && b < g.nb ? (int)coef[((size_t)f * g.nb + b) * 64] : 0;
}

// grid (ceil(nb / 256), F)
__global__ void __launch_bounds__(JD_THREADS) k_jd_dc_apply(int16_t* __restrict__ coef, JdGeom g, const int* __restrict__ dc,
                                                            const int* __restrict__ tot_d) {
    const int b = blockIdx.x * JD_THREADS + threadIdx.x, f = blockIdx.y;
    if (b >= g.nb) return;
    int comp, j;
    jd_block_comp(g, b, comp, j);
    const size_t row = (size_t)f * g.ncomp + comp;
    int16_t* c = coef + ((size_t)f * g.nb + b) * 64;
    *c = (int16_t)(dc[row * g.ny + j] + tot_d[row * (g.tiles_d + 1) + j / JD_TILE] + (int)*c);
}

// ---- IDCT ------------------------------------------------------------------------------------------------------------------------------
// one pass of jpeg_idct_islow over d[0] ... d[7]; unsigned arithmetic, so that what does not fit int32 wraps
template <int SHIFT>
__device__ __forceinline__ void jd_idct_pass(const int (&d)[8], int (&o)[8]) {
    typedef uint32_t U;
    const U i0 = (U)d[0], i1 = (U)d[1], i2 = (U)d[2], i3 = (U)d[3], i4 = (U)d[4], i5 = (U)d[5], i6 = (U)d[6], i7 = (U)d[7];
    U z1 = (i2 + i6) * 4433u;
    U t2 = z1 + i6 * (U)-15137, t3 = z1 + i2 * 6270u;
    U t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = i7; t1 = i5; t2 = i3; t3 = i1;
    z1 = t0 + t3;
    U z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const U z5 = (z3 + z4) * 9633u;
    t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
    z1 *= (U)-7373; z2 *= (U)-20995; z3 = z3 * (U)-16069 + z5; z4 = z4 * (U)-3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    constexpr U half = 1u << (SHIFT - 1);
    o[0] = (int)(t10 + t3 + half) >> SHIFT; o[7] = (int)(t10 - t3 + half) >> SHIFT;
    o[1] = (int)(t11 + t2 + half) >> SHIFT; o[6] = (int)(t11 - t2 + half) >> SHIFT;
    o[2] = (int)(t12 + t1 + half) >> SHIFT; o[5] = (int)(t12 - t1 + half) >> SHIFT;
    o[3] = (int)(t13 + t0 + half) >> SHIFT; o[4] = (int)(t13 - t0 + half) >> SHIFT;
}

#define JD_LD 72          // ints per block in LDS: 64 + 8, so that the eight blocks of a wave start on different banks

// grid (ceil(nb / 32), F), 256 threads: a wave serves 8 blocks; lane = block * 8 + column (pass 1), block * 8 + row (pass 2)
__global__ void __launch_bounds__(JD_THREADS) k_jd_idct(const int16_t* __restrict__ coef, const dsn_jpegd_desc* __restrict__ desc, JdGeom g,
                                                        uint8_t* __restrict__ planes) {
    __shared__ int s_q[3][64];
    __shared__ int s_blk[32 * JD_LD];
    const int f = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x < 64 * g.ncomp) s_q[threadIdx.x >> 6][lane] = desc[f].quant[desc[f].qsel[threadIdx.x >> 6] & 3][lane];
    __syncthreads();
    const int wb = w * 8 + (lane >> 3), b = blockIdx.x * 32 + wb, sub = lane & 7;
    const bool live = b < g.nb;
    int comp = 0, k = 0, mcu = 0;
    if (live) {
        mcu = b / g.bpm; k = b % g.bpm;
        comp = g.mode == DSN_JPEG_420 ? (k < 4 ? 0 : k - 3) : k;
        const uint4 q = *(const uint4*)(coef + ((size_t)f * g.nb + b) * 64 + sub * 8);
        const uint32_t c[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int zz = sub * 8 + i;
            const int v = (int)(int16_t)(c[i >> 1] >> (16 * (i & 1)));
            s_blk[wb * JD_LD + c_jd_zigzag.z[zz]] = v * s_q[comp][zz];
        }
    }
    __syncthreads();
    int d[8], o[8];
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = s_blk[wb * JD_LD + r * 8 + sub];
        jd_idct_pass<11>(d, o);
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) s_blk[wb * JD_LD + r * 8 + sub] = o[r];
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int c = 0; c < 8; ++c) d[c] = s_blk[wb * JD_LD + sub * 8 + c];
    jd_idct_pass<18>(d, o);
    uint32_t pk[2] = {0, 0};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int x = o[c] & 1023;
        x = (x >= 512 ? x - 1024 : x) + 128;
        x = x < 0 ? 0 : x > 255 ? 255 : x;
        pk[c >> 2] |= (uint32_t)x << (8 * (c & 3));
    }
    const int mx = mcu % g.mw, my = mcu / g.mw;
    size_t base;
    int bx, by, pw;
    if (g.mode == DSN_JPEG_420) {
        if (k < 4) { bx = mx * 2 + (k & 1); by = my * 2 + (k >> 1); pw = g.mw * 16; base = 0; }
        else { bx = mx; by = my; pw = g.mw * 8; base = (size_t)g.mw * g.mh * (256 + 64 * (k - 4)); }
    } else { bx = mx; by = my; pw = g.mw * 8; base = (size_t)g.mw * g.mh * 64 * comp; }
    *(uint2*)(planes + (size_t)f * g.nb * 64 + base + (size_t)(by * 8 + sub) * pw + bx * 8) = make_uint2(pk[0], pk[1]);
}

// ---- upsampling and colour ---------------------------------------------------------------------------------------------------------------
// libjpeg's h2v2 fancy upsampling of chroma plane P (row stride pw; real part ch x cw) at output pixel (y, x)
__device__ __forceinline__ int jd_fancy(const uint8_t* __restrict__ P, int pw, int ch, int cw, int y, int x) {
    const int cy = y >> 1, cx = x >> 1;
    if (cw <= 2) return P[(size_t)cy * pw + cx];
    const int far = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    const uint8_t* a = P + (size_t)cy * pw;
    const uint8_t* b = P + (size_t)far * pw;
    const int here = 3 * a[cx] + b[cx];
    if (x & 1) {
        const int n = cx + 1 < cw ? 3 * a[cx + 1] + b[cx + 1] : here;
        return (3 * here + n + 7) >> 4;
    }
    const int n = cx > 0 ? 3 * a[cx - 1] + b[cx - 1] : here;
    return (3 * here + n + 8) >> 4;
}

__device__ __forceinline__ uint8_t jd_clamp8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// grid (ceil(W / 64), ceil(H / 4), F), block (64, 4)
__global__ void __launch_bounds__(256) k_jd_colour(const uint8_t* __restrict__ planes, const uint32_t* __restrict__ status, JdGeom g, int rgb,
                                                   int gray_out, uint8_t* __restrict__ out) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z;
    if (x >= g.W || y >= g.H) return;
    const size_t px = ((size_t)f * g.H + y) * g.W + x;
    const bool bad = status && (status[f] & (DSN_JPEGD_CORRUPT | DSN_JPEGD_UNCONVERGED));
    const uint8_t* P = planes + (size_t)f * g.nb * 64;
    const int yw = g.mw * (g.mode == DSN_JPEG_420 ? 16 : 8);
    const int Y = bad ? 0 : P[(size_t)y * yw + x];
    if (gray_out) { out[px] = (uint8_t)Y; return; }
    int R = Y, G = Y, B = Y;
    if (g.mode != DSN_JPEG_GRAY && !bad) {
        int cb, cr;
        if (g.mode == DSN_JPEG_420) {
            const size_t ysz = (size_t)g.mw * g.mh * 256, csz = (size_t)g.mw * g.mh * 64;
            cb = jd_fancy(P + ysz, g.mw * 8, (g.H + 1) / 2, (g.W + 1) / 2, y, x) - 128;
            cr = jd_fancy(P + ysz + csz, g.mw * 8, (g.H + 1) / 2, (g.W + 1) / 2, y, x) - 128;
        } else {
            const size_t sz = (size_t)g.mw * g.mh * 64;
            cb = P[sz + (size_t)y * yw + x] - 128;
            cr = P[2 * sz + (size_t)y * yw + x] - 128;
        }
        R = Y + ((91881 * cr + 32768) >> 16);
        G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        B = Y + ((116130 * cb + 32768) >> 16);
    }
    out[3 * px] = jd_clamp8(rgb ? R : B);
    out[3 * px + 1] = jd_clamp8(G);
    out[3 * px + 2] = jd_clamp8(rgb ? B : R);
}

}  // namespace

size_t dsn_jpegd_workspace_size(int F, int H, int W, int mode, size_t max_scan_bytes) {
    JdGeom g;
    if (F < 1 || F > DSN_JPEGD_MAX_FRAMES || !jd_geom(H, W, mode, max_scan_bytes, g)) return 0;
    return jd_carve(nullptr, F, g).bytes;
}

int16_t* dsn_jpegd_workspace_coef(void* workspace, int F, int H, int W, int mode, size_t max_scan_bytes) {
    JdGeom g;
    jd_geom(H, W, mode, max_scan_bytes, g);
    return jd_carve(workspace, F, g).coef;
}

void dsn_launch_jpegd_sync(const uint8_t* files, size_t files_bytes, const int64_t* offsets, const dsn_jpegd_desc* desc, int F, int H, int W,
                           int mode, size_t max_scan_bytes, int B, bool restart, int rounds, uint32_t* out_converged, int32_t* out_rounds,
                           void* workspace, hipStream_t st) {
    JdGeom g;
    jd_geom(H, W, mode, max_scan_bytes, g);
    const JdWorkspace w = jd_carve(workspace, F, g);
    const int SB = jd_subs(g, B);
    const dim3 chunks((g.chunks + JD_THREADS - 1) / JD_THREADS, F), subs((SB + JD_THREADS - 1) / JD_THREADS, F), one((F + 255) / 256);
    if (restart) {
        hipLaunchKernelGGL(k_jd_begin, dim3((F * JD_META + 255) / 256), dim3(256), 0, st, w.meta, F);
        hipLaunchKernelGGL(k_jd_ffcount, chunks, dim3(JD_THREADS), 0, st, files, files_bytes, offsets, desc, g, w.meta, w.kept);
        dsn_launch_jpeg_tile_scan(w.kept, g.chunks, F, w.tot_c, st);
        hipLaunchKernelGGL(k_jd_unstuff, chunks, dim3(JD_THREADS), 0, st, files, files_bytes, offsets, desc, g, B, w.kept, w.tot_c, w.meta, w.us);
        if (rounds > 0) {
            hipLaunchKernelGGL(k_jd_round<true>, subs, dim3(JD_THREADS), 0, st, desc, g, B, SB, w.us, w.meta, w.entry, w.exit2, w.cnt, w.flags);
            hipLaunchKernelGGL(k_jd_verdict, one, dim3(256), 0, st, w.meta, F, out_converged, out_rounds);
            --rounds;
        }
    }
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_jd_round<false>, subs, dim3(JD_THREADS), 0, st, desc, g, B, SB, w.us, w.meta, w.entry, w.exit2, w.cnt, w.flags);
        hipLaunchKernelGGL(k_jd_verdict, one, dim3(256), 0, st, w.meta, F, out_converged, out_rounds);
    }
}

void dsn_launch_jpegd_coefficients(const dsn_jpegd_desc* desc, int F, int H, int W, int mode, size_t max_scan_bytes, int B, int16_t* coef,
                                   uint32_t* status, void* workspace, hipStream_t st) {
    JdGeom g;
    jd_geom(H, W, mode, max_scan_bytes, g);
    const JdWorkspace w = jd_carve(workspace, F, g);
    const int SB = jd_subs(g, B), tiles_s = (SB + JD_TILE - 1) / JD_TILE;
    const size_t n16 = (size_t)F * g.nb * 8;          // 16-byte groups of coef
    hipLaunchKernelGGL(k_jd_zero_coef, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, (uint4*)coef, n16);
    const size_t nc = (size_t)F * SB;
    hipLaunchKernelGGL(k_jd_copy, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, (const int*)w.cnt, w.pre, nc, w.meta, F);
    dsn_launch_jpeg_tile_scan(w.pre, SB, F, w.tot_s, st);
    hipLaunchKernelGGL(k_jd_emit, dim3((SB + JD_THREADS - 1) / JD_THREADS, F), dim3(JD_THREADS), 0, st, desc, g, B, SB, tiles_s, w.us, w.meta,
                       w.entry, w.pre, w.tot_s, w.flags, coef);
    hipLaunchKernelGGL(k_jd_status, dim3(F), dim3(JD_THREADS), 0, st, g, SB, w.us, w.meta, w.flags, status);
    hipLaunchKernelGGL(k_jd_dc_gather, dim3((g.ny + JD_THREADS - 1) / JD_THREADS, F * g.ncomp), dim3(JD_THREADS), 0, st, coef, g, w.dc);
    dsn_launch_jpeg_tile_scan(w.dc, g.ny, F * g.ncomp, w.tot_d, st);
    hipLaunchKernelGGL(k_jd_dc_apply, dim3((g.nb + JD_THREADS - 1) / JD_THREADS, F), dim3(JD_THREADS), 0, st, coef, g, w.dc, w.tot_d);
}

void dsn_launch_jpegd_pixels(const int16_t* coef, const uint32_t* status, const dsn_jpegd_desc* desc, int F, int H, int W, int mode,
                             size_t max_scan_bytes, int rgb, int gray_out, uint8_t* out, void* workspace, hipStream_t st) {
    JdGeom g;
    jd_geom(H, W, mode, max_scan_bytes, g);
    const JdWorkspace w = jd_carve(workspace, F, g);
    hipLaunchKernelGGL(k_jd_idct, dim3((g.nb + 31) / 32, F), dim3(JD_THREADS), 0, st, coef, desc, g, w.planes);
    hipLaunchKernelGGL(k_jd_colour, dim3((W + 63) / 64, (H + 3) / 4, F), dim3(64, 4), 0, st, (const uint8_t*)w.planes, status, g, rgb, gray_out,
                       out);
}
