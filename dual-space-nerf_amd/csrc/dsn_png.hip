// dsn_png.hip - PNG DECODING on the device (dsn_png_parse_host, dsn_png_workspace_*, dsn_png_decode; the rule is in include/dsnerf.h and
// restated in tests/png_decode_restate.py).  Integer arithmetic throughout; the only atomics are 32-bit integer adds in LDS and ORs
// into the frames' status words.
//   k_pn_gather   : a thread per byte of a file's zlib stream: its IDAT segment by bisection, zeros behind the stream
//   k_pn_inflate  : one wave per file.  The symbol loop is the same in every lane; the window (32 KiB), the canonical tables and the
//                   direct lookups for short codes lie in LDS; tables are built by all lanes, matches are copied by all lanes
//   k_pn_adler    : a workgroup per file: integer sums mod 65521 over the bytes inflate wrote, against the stored value
//   k_pn_unfilter : a wave per file, lane j on row r + j one pixel behind lane j - 1 (the row above arrives by wave shuffles)
//   k_pn_pixels   : a thread per pixel: unpack, scale, palette, channel order, zeros for frames with a status
// Files lie side by side in blockIdx (gather: y, pixels: z); nothing depends on F.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include <string.h>

#define PN_WIN 32768              // the window: a power of two, deflate's largest distance
#define PN_FAST_L 10              // bits of the literal/length lookup
#define PN_FAST_D 8               // bits of the distance lookup
#define PN_META 8                 // uint32 words per frame
#define PN_OUTLEN 0
#define PN_STATUS 1
#define PN_STORED 2
#define PN_ADLER 3
#define PN_ENDBIT 4
#define PN_MAX_STREAM ((size_t)1 << 28)
#define PN_MAX_RAW ((int64_t)1 << 30)

namespace {

struct PnGeom {
    int W, H, bits, ctype, channels, rb, need, bpp, npx;
    int scap;                     // bytes of a file's stream in the workspace: max_stream rounded up to 16, + 16
    int rcap;                     // bytes of a file's inflated data: raw_bytes rounded up to 16, + 16
    int rowcap;                   // bytes of a file's unfiltered rows
};

int pn_channels(int bits, int ctype) {          // 0: not a pair this decoder takes
    const bool low = bits == 1 || bits == 2 || bits == 4;
    switch (ctype) {
    case 0: return (low || bits == 8) ? 1 : 0;
    case 2: return bits == 8 ? 3 : 0;
    case 3: return (low || bits == 8) ? 1 : 0;
    case 4: return bits == 8 ? 2 : 0;
    case 6: return bits == 8 ? 4 : 0;
    }
    return 0;
}

bool pn_geom(int W, int H, int bits, int ctype, size_t max_stream, PnGeom& g) {
    const int ch = pn_channels(bits, ctype);
    if (!ch || W < 1 || H < 1 || W > DSN_PNG_MAX_DIM || H > DSN_PNG_MAX_DIM || max_stream > PN_MAX_STREAM) return false;
    g.W = W; g.H = H; g.bits = bits; g.ctype = ctype; g.channels = ch;
    g.rb = (W * bits * ch + 7) / 8;
    const int64_t need = (int64_t)H * (1 + g.rb);
    if (need > PN_MAX_RAW) return false;
    g.need = (int)need;
    g.bpp = bits * ch >= 8 ? bits * ch / 8 : 1;
    g.npx = g.rb / g.bpp;
    g.scap = (int)((max_stream + 15) & ~(size_t)15) + 16;
    g.rcap = (int)((need + 15) & ~(int64_t)15) + 16;
    g.rowcap = (int)(((int64_t)H * g.rb + 15) & ~(int64_t)15) + 16;
    return true;
}

struct PnWorkspace { uint32_t* meta; uint8_t* streams; uint8_t* raw; uint8_t* rows; size_t off[4]; size_t bytes; };

PnWorkspace pn_carve(void* base, int F, const PnGeom& g) {
    PnWorkspace w;
    size_t off = 0;
    int k = 0;
    auto take = [&](size_t n) { const size_t at = off; w.off[k++] = at; off += (n + 255) & ~(size_t)255; return (char*)base + at; };
    w.meta = (uint32_t*)take((size_t)F * PN_META * 4);
    w.streams = (uint8_t*)take((size_t)F * g.scap);
    w.raw = (uint8_t*)take((size_t)F * g.rcap);
    w.rows = (uint8_t*)take((size_t)F * g.rowcap);
    w.bytes = off;
    return w;
}

// ---- the container (host) --------------------------------------------------------------------------------------------------------------
struct PnCrcTable { uint32_t t[256]; };
constexpr PnCrcTable pn_make_crc() {
    PnCrcTable c{};
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t v = n;
        for (int k = 0; k < 8; ++k) v = (v & 1) ? 0xEDB88320u ^ (v >> 1) : v >> 1;
        c.t[n] = v;
    }
    return c;
}
const PnCrcTable pn_crc_table = pn_make_crc();

uint32_t pn_crc(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = pn_crc_table.t[(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

uint32_t pn_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

}  // namespace

int dsn_png_parse(const uint8_t* d, size_t n, dsn_png_desc* out, uint32_t* segs, size_t seg_capacity) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    memset(out, 0, sizeof(*out));
    if (n < 8 || memcmp(d, sig, 8) != 0) return DSN_PNG_NOT_PNG;
    out->file_length = (int32_t)(n > 0x7FFFFFFFu ? 0x7FFFFFFF : n);
    bool first = true, have_plte = false, have_iend = false;
    uint64_t zlen = 0;
    size_t nseg = 0;
    uint8_t z[2] = {0, 0};
    size_t i = 8;
    while (i < n) {
        if (n - i < 12) return DSN_PNG_TRUNCATED;
        const uint32_t L = pn_be32(d + i);
        if ((size_t)L > n - i - 12) return DSN_PNG_TRUNCATED;
        const uint8_t* type = d + i + 4;
        const uint8_t* data = d + i + 8;
        const bool ihdr = memcmp(type, "IHDR", 4) == 0, plte = memcmp(type, "PLTE", 4) == 0, idat = memcmp(type, "IDAT", 4) == 0,
                   iend = memcmp(type, "IEND", 4) == 0;
        if (first && !ihdr) return DSN_PNG_NO_IHDR;
        if ((ihdr || plte || idat || iend) && pn_crc(type, (size_t)L + 4) != pn_be32(data + L)) return DSN_PNG_CRC;
        if (ihdr) {
            if (!first || L != 13) return DSN_PNG_BAD_IHDR;
            const uint32_t W = pn_be32(data), H = pn_be32(data + 4);
            const int bits = data[8], ctype = data[9];
            if (W == 0 || H == 0) return DSN_PNG_ZERO_DIM;
            if (bits == 16 && (ctype == 0 || ctype == 2 || ctype == 4 || ctype == 6)) return DSN_PNG_DEPTH16;
            const int ch = pn_channels(bits, ctype);
            if (!ch || data[10] != 0 || data[11] != 0 || data[12] > 1) return DSN_PNG_BAD_IHDR;
            if (data[12] == 1) return DSN_PNG_INTERLACE;
            if (W > DSN_PNG_MAX_DIM || H > DSN_PNG_MAX_DIM) return DSN_PNG_TOO_LARGE;
            const int rb = (int)((W * (uint32_t)bits * (uint32_t)ch + 7) / 8);
            if ((int64_t)H * (1 + rb) > PN_MAX_RAW) return DSN_PNG_TOO_LARGE;
            out->W = (int32_t)W; out->H = (int32_t)H; out->bits = bits; out->ctype = ctype; out->channels = ch;
            out->row_bytes = rb;
            out->raw_bytes = (int32_t)((int64_t)H * (1 + rb));
        } else if (plte) {
            if (L == 0 || L > 768 || L % 3) return DSN_PNG_NO_PLTE;
            if (nseg == 0) {
                memset(out->palette, 0, sizeof(out->palette));
                memcpy(out->palette, data, L);
                out->npal = (int32_t)(L / 3);
                have_plte = true;
            }
        } else if (idat) {
            if (out->ctype == 3 && !have_plte) return DSN_PNG_NO_PLTE;
            for (uint32_t k = 0; k < L && zlen + k < 2; ++k) z[zlen + k] = data[k];
            if (nseg < seg_capacity && segs) { segs[2 * nseg] = (uint32_t)(i + 8); segs[2 * nseg + 1] = L; }
            ++nseg;
            zlen += L;
            if (zlen > PN_MAX_STREAM || nseg > 0x7FFFFFFFu) return DSN_PNG_TOO_LARGE;
        } else if (iend) {
            have_iend = true;
            break;
        }
        first = false;
        i += 12 + (size_t)L;
    }
    if (first) return DSN_PNG_NO_IHDR;
    if (!have_iend) return DSN_PNG_TRUNCATED;
    if (nseg == 0 || zlen < 2) return DSN_PNG_NO_IDAT;
    out->nseg = (int32_t)nseg;
    out->zlen = (int32_t)zlen;
    if ((z[0] & 15) != 8 || (z[0] >> 4) > 7) return DSN_PNG_ZLIB_METHOD;
    if (z[1] & 0x20) return DSN_PNG_ZLIB_DICT;
    if (((uint32_t)z[0] * 256 + z[1]) % 31) return DSN_PNG_ZLIB_CHECK;
    return DSN_PNG_OK;
}

namespace {

// ---- gather ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pn_zlen(const dsn_png_desc* __restrict__ desc, int f, const PnGeom& g) {
    return min(max(desc[f].zlen, 0), g.scap - 16);
}

// grid (ceil(scap / 256), F)
__global__ void __launch_bounds__(256) k_pn_gather(const uint8_t* __restrict__ files, size_t files_bytes, const int64_t* __restrict__ segs,
                                                   int S, const int32_t* __restrict__ seg_first, const dsn_png_desc* __restrict__ desc,
                                                   PnGeom g, uint8_t* __restrict__ streams) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.scap) return;
    uint8_t b = 0;
    if (i < pn_zlen(desc, f, g)) {
        const int lo = min(max(seg_first[f], 0), S), hi = min(max(seg_first[f + 1], lo), S);
        int a = lo, c = hi;          // the last segment of [lo, hi) that starts at or before i
        while (c - a > 1) {
            const int m = (a + c) >> 1;
            if (segs[3 * (size_t)m + 1] <= (int64_t)i) a = m; else c = m;
        }
        if (a < hi) {
            const int64_t src = segs[3 * (size_t)a], k = (int64_t)i - segs[3 * (size_t)a + 1], len = segs[3 * (size_t)a + 2];
            if (k >= 0 && k < len && src >= 0 && (uint64_t)src < (uint64_t)files_bytes && (uint64_t)k < (uint64_t)files_bytes - (uint64_t)src)
                b = files[src + k];
        }
    }
    streams[(size_t)f * g.scap + i] = b;
}

// ---- inflate -----------------------------------------------------------------------------------------------------------------------------
struct PnTab { uint16_t v[32]; };
__constant__ const PnTab c_pn_lbase = {{3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258, 0, 0, 0}};
__constant__ const PnTab c_pn_lext = {{0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0, 0, 0, 0}};
__constant__ const PnTab c_pn_dbase = {{1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
                                        12289, 16385, 24577, 0, 0}};
__constant__ const PnTab c_pn_dext = {{0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 0, 0}};
__constant__ const PnTab c_pn_order = {{16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};

struct PnHuff { uint16_t count[16]; uint16_t sym[288]; };          // codes per length; the symbols in code order
struct PnLds {
    uint8_t win[PN_WIN];
    uint16_t fast_l[1 << PN_FAST_L], fast_d[1 << PN_FAST_D];          // (symbol << 4) | length for codes the lookup's bits hold; 0: none
    PnHuff L, D, C;
    uint8_t lens[320], clens[32];
    uint32_t cnt[16];
};

// the bit reader: the same in every lane.  At least 32 bits are on hand behind need(); a word at or past `words` reads 0; the word that
// will be wanted next is loaded a word ahead, off the symbols' dependency chain
struct PnBits {
    const uint32_t* __restrict__ w;
    uint32_t words, wi, nxt, pos;
    uint64_t bb;
    int bc;
    __device__ __forceinline__ uint32_t load(uint32_t i) const { return i < words ? w[i] : 0u; }
    __device__ __forceinline__ void start(uint32_t byte) {
        wi = byte >> 2;
        const int sh = (int)(byte & 3) * 8;
        bb = (uint64_t)(load(wi) >> sh);
        bc = 32 - sh;
        ++wi;
        nxt = load(wi);
        pos = byte * 8u;
    }
    __device__ __forceinline__ void need() {
        if (bc < 32) { bb |= (uint64_t)nxt << bc; bc += 32; ++wi; nxt = load(wi); }
    }
    __device__ __forceinline__ void drop(int n) { bb >>= n; bc -= n; pos += (uint32_t)n; }
    __device__ __forceinline__ uint32_t take(int n) {          // n <= 16
        const uint32_t v = (uint32_t)bb & ((1u << n) - 1u);
        drop(n);
        return v;
    }
};

// counts, symbols in code order and (fast != null) the direct lookup of the code lengths lens[0 ... n), by all 64 lanes.
// Returns whether the set is usable: complete, or (incomplete_ok) empty or one single code of length 1.
__device__ __forceinline__ bool pn_build(PnLds& S, PnHuff& h, uint16_t* fast, int fb, const uint8_t* lens, int n, bool incomplete_ok, int lane) {
    if (lane < 16) S.cnt[lane] = 0;
    if (fast) for (int k = lane; k < (1 << fb); k += 64) fast[k] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) atomicAdd(&S.cnt[lens[i] & 15], 1u);
    __syncthreads();
    int offs[16], run[16], first[16];
    int left = 1, code = 0, o = 0, prev = 0;
    offs[0] = run[0] = first[0] = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) {
        const int c = (int)S.cnt[l];
        left = left < 0 ? -1 : (left << 1) - c;
        code = (code + prev) << 1;
        first[l] = code; offs[l] = o; run[l] = o;
        o += c;
        prev = c;
    }
    const int c1 = (int)S.cnt[1];
    if (lane < 16) h.count[lane] = lane ? (uint16_t)S.cnt[lane] : (uint16_t)0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane, l = i < n ? (lens[i] & 15) : 0;
        int at = -1, mine = 0;
#pragma unroll
        for (int v = 1; v < 16; ++v) {
            const unsigned long long m = __ballot(l == v);
            if (l == v) {
                at = run[v] + __popcll(m & ((1ull << lane) - 1ull));
                mine = first[v] + (at - offs[v]);
            }
            run[v] += __popcll(m);
        }
        if (at >= 0 && at < 288) {
            h.sym[at] = (uint16_t)i;
            if (fast && l <= fb) {
                const uint32_t r = __brev((uint32_t)mine) >> (32 - l);
                for (uint32_t k = r; k < (1u << fb); k += 1u << l) fast[k] = (uint16_t)(i << 4 | l);
            }
        }
    }
    __syncthreads();
    return left == 0 || (incomplete_ok && left > 0 && (o == 0 || (o == 1 && c1 == 1)));
}

// one symbol from the bits on hand (need() came before): the lookup for short codes, else the canonical walk; -1: no code, nothing taken
__device__ __forceinline__ int pn_decode(const uint16_t* fast, int fb, const PnHuff& h, PnBits& br) {
    const uint32_t w = (uint32_t)br.bb;
    if (fast) {
        const uint32_t e = fast[w & ((1u << fb) - 1u)];
        if (e & 15u) { br.drop((int)(e & 15u)); return (int)(e >> 4); }
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)(w >> (l - 1)) & 1;
        const int c = h.count[l];
        if (code - c < first) { br.drop(l); return h.sym[min(index + (code - first), 287)]; }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// grid (F), 64 threads
__global__ void __launch_bounds__(64) k_pn_inflate(const uint8_t* __restrict__ streams, const dsn_png_desc* __restrict__ desc, PnGeom g,
                                                   uint8_t* __restrict__ raws, uint32_t* __restrict__ meta) {
    __shared__ PnLds S;
    const int f = blockIdx.x, lane = threadIdx.x;
    const uint8_t* zs = streams + (size_t)f * g.scap;
    uint8_t* out = raws + (size_t)f * g.rcap;
    const uint32_t zlen = (uint32_t)pn_zlen(desc, f, g), total = zlen * 8u, cap = (uint32_t)g.need;
    PnBits br;
    br.w = (const uint32_t*)zs;
    br.words = (uint32_t)g.scap / 4u;
    br.start(2);
    uint32_t st = 0, op = 0, stored = 0;
    bool fixed_built = false;
    for (;;) {                                                  // a block per turn: its header takes 3 bits
        br.need();
        const uint32_t bfinal = br.take(1), btype = br.take(2);
        if (br.pos > total) { st = DSN_PNG_EARLY_END; break; }
        if (btype == 3) { st = DSN_PNG_BLOCK_TYPE; break; }
        if (btype == 0) {
            br.drop((int)((0u - br.pos) & 7u));
            br.need();
            const uint32_t len = br.take(16), nlen = br.take(16);
            if (br.pos > total) { st = DSN_PNG_EARLY_END; break; }
            if ((len ^ 0xFFFFu) != nlen) { st = DSN_PNG_STORED_LEN; break; }
            const uint32_t at = br.pos >> 3;
            if (at + len > zlen) { st = DSN_PNG_EARLY_END; break; }
            if (op + len > cap) { st = DSN_PNG_TOO_MUCH; break; }
            for (uint32_t i = lane; i < len; i += 64) {
                const uint8_t b = zs[at + i];
                S.win[(op + i) & (PN_WIN - 1)] = b;
                out[op + i] = b;
            }
            __syncthreads();
            op += len;
            br.start(at + len);
        } else {
            if (btype == 1) {
                if (!fixed_built) {
                    for (int i = lane; i < 320; i += 64) S.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
                    __syncthreads();
                    pn_build(S, S.L, S.fast_l, PN_FAST_L, S.lens, 288, false, lane);
                    pn_build(S, S.D, S.fast_d, PN_FAST_D, S.lens + 288, 32, false, lane);
                    fixed_built = true;
                }
            } else {
                fixed_built = false;
                br.need();
                const int hlit = (int)br.take(5) + 257, hdist = (int)br.take(5) + 1, hclen = (int)br.take(4) + 4;
                if (br.pos > total) { st = DSN_PNG_EARLY_END; break; }
                if (hlit > 286 || hdist > 30) { st = DSN_PNG_BAD_CODES; break; }
                if (lane < 32) S.clens[lane] = 0;
                __syncthreads();
                for (int k = 0; k < hclen; ++k) {
                    br.need();
                    const uint32_t v = br.take(3);
                    if (lane == 0) S.clens[c_pn_order.v[k]] = (uint8_t)v;
                }
                if (br.pos > total) { st = DSN_PNG_EARLY_END; break; }
                __syncthreads();
                if (!pn_build(S, S.C, nullptr, 0, S.clens, 19, false, lane)) { st = DSN_PNG_BAD_CODES; break; }
                const int nall = hlit + hdist;
                int idx = 0, prev = 0;
                while (idx < nall) {                            // a code-length symbol per turn: at least one bit
                    br.need();
                    const int sym = pn_decode(nullptr, 0, S.C, br);
                    if (sym < 0) { st = DSN_PNG_NO_CODE; break; }
                    int rep = 1, val = sym;
                    if (sym == 16) { rep = 3 + (int)br.take(2); val = prev; }
                    else if (sym == 17) { rep = 3 + (int)br.take(3); val = 0; }
                    else if (sym >= 18) { rep = 11 + (int)br.take(7); val = 0; }
                    if (br.pos > total) { st = DSN_PNG_EARLY_END; break; }
                    if ((sym == 16 && idx == 0) || idx + rep > nall) { st = DSN_PNG_BAD_CODES; break; }
                    for (int i = lane; i < rep; i += 64) S.lens[idx + i] = (uint8_t)val;
                    idx += rep;
                    prev = val;
                }
                if (st) break;
                __syncthreads();
                if (S.lens[256] == 0) { st = DSN_PNG_BAD_CODES; break; }
                const bool okl = pn_build(S, S.L, S.fast_l, PN_FAST_L, S.lens, hlit, true, lane);
                const bool okd = pn_build(S, S.D, S.fast_d, PN_FAST_D, S.lens + hlit, hdist, true, lane);
                if (!okl || !okd) { st = DSN_PNG_BAD_CODES; break; }
            }
            for (;;) {                                          // a literal/length symbol per turn: at least one bit
                br.need();
                const int sym = pn_decode(S.fast_l, PN_FAST_L, S.L, br);
                if (sym < 0) { st = DSN_PNG_NO_CODE; break; }
                if (sym < 256) {
                    if (br.pos > total) { st = DSN_PNG_EARLY_END; break; }
                    if (op >= cap) { st = DSN_PNG_TOO_MUCH; break; }
                    if (lane == 0) { S.win[op & (PN_WIN - 1)] = (uint8_t)sym; out[op] = (uint8_t)sym; }
                    ++op;
                    continue;
                }
                const int li = min(max(sym - 257, 0), 31);
                const uint32_t len = sym == 256 ? 0u : c_pn_lbase.v[li] + br.take(c_pn_lext.v[li]);
                if (br.pos > total) { st = DSN_PNG_EARLY_END; break; }
                if (sym == 256) break;
                if (sym > 285) { st = DSN_PNG_NO_CODE; break; }
                br.need();
                const int ds = pn_decode(S.fast_d, PN_FAST_D, S.D, br);
                if (ds < 0) { st = DSN_PNG_NO_CODE; break; }
                const int di = min(ds, 31);
                const uint32_t dist = c_pn_dbase.v[di] + br.take(c_pn_dext.v[di]);
                if (br.pos > total) { st = DSN_PNG_EARLY_END; break; }
                if (ds > 29) { st = DSN_PNG_NO_CODE; break; }
                if (dist > op) { st = DSN_PNG_FAR_DISTANCE; break; }
                if (op + len > cap) { st = DSN_PNG_TOO_MUCH; break; }
                // every source byte lies before op: all of them are read, then all lanes write (len <= 258 <= 5 x 64)
                __syncthreads();
                uint8_t b[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const uint32_t i = (uint32_t)(k * 64 + lane);
                    b[k] = 0;
                    if (i < len) b[k] = S.win[(op - dist + (dist >= len ? i : i % dist)) & (PN_WIN - 1)];
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const uint32_t i = (uint32_t)(k * 64 + lane);
                    if (i < len) { S.win[(op + i) & (PN_WIN - 1)] = b[k]; out[op + i] = b[k]; }
                }
                op += len;
            }
            if (st) break;
        }
        if (bfinal) break;
    }
    if (st == 0) {
        const uint32_t at = (br.pos + 7u) >> 3;
        if (at + 4u > zlen) st = DSN_PNG_EARLY_END;
        else {
            stored = (uint32_t)zs[at] << 24 | (uint32_t)zs[at + 1] << 16 | (uint32_t)zs[at + 2] << 8 | zs[at + 3];
            if (op < cap) st = DSN_PNG_TOO_LITTLE;
        }
    }
    if (lane < PN_META) {
        const uint32_t v = lane == PN_OUTLEN ? op : lane == PN_STATUS ? st : lane == PN_STORED ? stored : lane == PN_ENDBIT ? br.pos : 0u;
        meta[f * PN_META + lane] = v;
    }
}

// ---- Adler-32 ------------------------------------------------------------------------------------------------------------------------------
// grid (F), 256 threads
__global__ void __launch_bounds__(256) k_pn_adler(const uint8_t* __restrict__ raws, PnGeom g, uint32_t* __restrict__ meta) {
    __shared__ uint32_t s_a, s_b;
    const int f = blockIdx.x;
    uint32_t* m = meta + f * PN_META;
    if (m[PN_STATUS] & ~DSN_PNG_TOO_LITTLE) return;          // (the same for the whole workgroup)
    if (threadIdx.x == 0) { s_a = 0; s_b = 0; }
    __syncthreads();
    const uint32_t n = min(m[PN_OUTLEN], (uint32_t)g.need);
    const uint8_t* raw = raws + (size_t)f * g.rcap;
    uint64_t sa = 0, sb = 0;
    for (uint32_t base = threadIdx.x * 16u; base < n; base += 256u * 16u) {
        const uint4 q = *(const uint4*)(raw + base);          // (rcap is a multiple of 16 above raw_bytes)
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t i = base + j, d = (w[j >> 2] >> (8 * (j & 3))) & 255u;
            if (i < n) { sa += d; sb += (uint64_t)((n - i) % 65521u) * d; }
        }
    }
    atomicAdd(&s_a, (uint32_t)(sa % 65521u));
    atomicAdd(&s_b, (uint32_t)(sb % 65521u));
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t a = (1u + s_a % 65521u) % 65521u, b = (n % 65521u + s_b % 65521u) % 65521u, v = b << 16 | a;
    m[PN_ADLER] = v;
    if (v != m[PN_STORED]) m[PN_STATUS] |= DSN_PNG_ADLER;
}

// ---- unfilter ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pn_unfilter_px(int ft, int bpp, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < bpp) {
            const int xv = (int)(x >> (8 * k)) & 255, av = (int)(a >> (8 * k)) & 255, bv = (int)(b >> (8 * k)) & 255, cv = (int)(c >> (8 * k)) & 255;
            const int p = av + bv - cv, pa = abs(p - av), pb = abs(p - bv), pc = abs(p - cv);
            const int paeth = (pa <= pb && pa <= pc) ? av : pb <= pc ? bv : cv;
            const int add = ft == 1 ? av : ft == 2 ? bv : ft == 3 ? (av + bv) >> 1 : ft == 4 ? paeth : 0;
            r |= (uint32_t)((xv + add) & 255) << (8 * k);
        }
    }
    return r;
}

// grid (F), 64 threads: bands of 64 rows; at step t lane j is at pixel t - j of row r0 + j
__global__ void __launch_bounds__(64) k_pn_unfilter(const uint8_t* __restrict__ raws, PnGeom g, uint32_t* __restrict__ meta,
                                                    uint8_t* __restrict__ rows_all) {
    const int f = blockIdx.x, lane = threadIdx.x;
    if (meta[f * PN_META + PN_STATUS]) return;                  // (the same for the whole wave)
    const uint8_t* raw = raws + (size_t)f * g.rcap;
    uint8_t* rows = rows_all + (size_t)f * g.rowcap;
    const int bpp = g.bpp, npx = g.npx, rb = g.rb;
    bool bad_filter = false;
    for (int r0 = 0; r0 < g.H; r0 += 64) {
        const int r = r0 + lane;
        const bool live = r < g.H;
        const uint8_t* src = raw + (size_t)(live ? r : 0) * (1 + rb);
        uint8_t* dst = rows + (size_t)(live ? r : 0) * rb;
        const uint8_t* above = rows + (size_t)(r0 > 0 ? r0 - 1 : 0) * rb;          // lane 0's row above, finished by the band before
        int ft = live ? src[0] : 0;
        if (ft > 4) { bad_filter = true; ft = 0; }
        uint32_t p1 = 0, p2 = 0, up0 = 0;                       // this row's last two pixels; lane 0: the last pixel of the row above
        for (int t = 0; t < npx + 63; ++t) {
            uint32_t b = __shfl_up(p1, 1), c = __shfl_up(p2, 1);
            const int x = t - lane;
            const bool on = live && x >= 0 && x < npx;
            uint32_t xin = 0, upv = 0;
            if (on) {
                for (int k = 0; k < bpp; ++k) xin |= (uint32_t)src[1 + x * bpp + k] << (8 * k);
                if (lane == 0 && r0 > 0)
                    for (int k = 0; k < bpp; ++k) upv |= (uint32_t)above[x * bpp + k] << (8 * k);
            }
            if (lane == 0) { b = upv; c = up0; up0 = upv; }
            if (on) {
                const uint32_t v = pn_unfilter_px(ft, bpp, xin, p1, b, c);
                for (int k = 0; k < bpp; ++k) dst[x * bpp + k] = (uint8_t)(v >> (8 * k));
                p2 = p1;
                p1 = v;
            }
        }
        __syncthreads();
    }
    if (bad_filter) atomicOr(&meta[f * PN_META + PN_STATUS], DSN_PNG_FILTER);
}

// ---- pixels --------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 64), ceil(H / 4), F), block (64, 4)
__global__ void __launch_bounds__(256) k_pn_pixels(const uint8_t* __restrict__ rows_all, const uint32_t* __restrict__ meta,
                                                   const dsn_png_desc* __restrict__ desc, PnGeom g, int channels, int first_channel,
                                                   uint8_t* __restrict__ out, uint32_t* __restrict__ out_status) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z;
    const uint32_t st = meta[f * PN_META + PN_STATUS];
    if (x == 0 && y == 0 && out_status) out_status[f] = st;
    if (x >= g.W || y >= g.H) return;
    const uint8_t* row = rows_all + (size_t)f * g.rowcap + (size_t)y * g.rb;
    uint32_t s[4] = {0, 0, 0, 0};
    if (!st) {
        if (g.bits == 8) {
            for (int k = 0; k < g.channels; ++k) s[k] = row[x * g.channels + k];
        } else {
            const int bit = x * g.bits;
            s[0] = ((uint32_t)row[bit >> 3] >> (8 - g.bits - (bit & 7))) & ((1u << g.bits) - 1u);
        }
    }
    uint32_t nat[4] = {s[0], s[1], s[2], s[3]}, R, G, B;
    if (g.ctype == 0 || g.ctype == 4) {
        const uint32_t v = s[0] * (g.bits == 1 ? 255u : g.bits == 2 ? 85u : g.bits == 4 ? 17u : 1u);
        nat[0] = v;
        R = G = B = v;
    } else if (g.ctype == 3) {
        const uint8_t* p = desc[f].palette[s[0] & 255u];
        R = st ? 0u : p[0]; G = st ? 0u : p[1]; B = st ? 0u : p[2];
    } else {
        R = s[0]; G = s[1]; B = s[2];
    }
    const size_t px = ((size_t)f * g.H + y) * g.W + x;
    if (channels == DSN_PNG_NATIVE) {
        if (first_channel) { out[px] = (uint8_t)nat[0]; return; }
        for (int k = 0; k < g.channels; ++k) out[px * g.channels + k] = (uint8_t)nat[k];
        return;
    }
    const uint32_t c0 = channels == DSN_PNG_RGB ? R : B, c2 = channels == DSN_PNG_RGB ? B : R;
    if (first_channel) { out[px] = (uint8_t)c0; return; }
    out[3 * px] = (uint8_t)c0;
    out[3 * px + 1] = (uint8_t)G;
    out[3 * px + 2] = (uint8_t)c2;
}

}  // namespace

size_t dsn_png_workspace_size(int F, int W, int H, int bits, int ctype, size_t max_stream_bytes, size_t* out8) {
    PnGeom g;
    if (F < 1 || F > DSN_PNG_MAX_FILES || !pn_geom(W, H, bits, ctype, max_stream_bytes, g)) return 0;
    const PnWorkspace w = pn_carve(nullptr, F, g);
    if (out8) {
        out8[0] = w.off[0]; out8[1] = w.off[1]; out8[2] = (size_t)g.scap; out8[3] = w.off[2]; out8[4] = (size_t)g.rcap; out8[5] = w.off[3];
        out8[6] = (size_t)g.rowcap; out8[7] = w.bytes;
    }
    return w.bytes;
}

void dsn_launch_png_decode(const uint8_t* files, size_t files_bytes, const int64_t* segs, int S, const int32_t* seg_first,
                           const dsn_png_desc* desc, int F, int W, int H, int bits, int ctype, size_t max_stream_bytes, int channels,
                           int first_channel, int stages, uint8_t* out, uint32_t* out_status, void* workspace, hipStream_t st) {
    PnGeom g;
    pn_geom(W, H, bits, ctype, max_stream_bytes, g);
    const PnWorkspace w = pn_carve(workspace, F, g);
    if (stages & DSN_PNG_STAGE_GATHER)
        hipLaunchKernelGGL(k_pn_gather, dim3((g.scap + 255) / 256, F), dim3(256), 0, st, files, files_bytes, segs, S, seg_first, desc, g, w.streams);
    if (stages & DSN_PNG_STAGE_INFLATE)
        hipLaunchKernelGGL(k_pn_inflate, dim3(F), dim3(64), 0, st, (const uint8_t*)w.streams, desc, g, w.raw, w.meta);
    if (stages & DSN_PNG_STAGE_ADLER) hipLaunchKernelGGL(k_pn_adler, dim3(F), dim3(256), 0, st, (const uint8_t*)w.raw, g, w.meta);
    if (stages & DSN_PNG_STAGE_UNFILTER)
        hipLaunchKernelGGL(k_pn_unfilter, dim3(F), dim3(64), 0, st, (const uint8_t*)w.raw, g, w.meta, w.rows);
    if (stages & DSN_PNG_STAGE_PIXELS)
        hipLaunchKernelGGL(k_pn_pixels, dim3((W + 63) / 64, (H + 3) / 4, F), dim3(64, 4), 0, st, (const uint8_t*)w.rows,
                           (const uint32_t*)w.meta, desc, g, channels, first_channel, out, out_status);
}
