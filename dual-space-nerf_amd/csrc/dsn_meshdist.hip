// dsn_meshdist.hip - the exact nearest point on a triangle mesh for a set of query points, and the measures built on it
// (dsn_mesh_dist_build / _query / _reduce, dsn_mesh_sample_surface; the rules are in include/dsnerf.h).
//
// The answer is the brute-force answer: the minimum over all valid faces of the float32 squared distance that md_closest() computes,
// ties to the lowest face index.  The uniform grid below only decides which faces a query looks at, and it may leave a face out only
// where that face's COMPUTED distance is provably larger than the best one found (the margin of md_shell_stops()).
//
//   build:  k_md_levels   one thread per face: valid?  its level-0 cell box; the number of (face, cell) pairs it would list at each of
//                         the MD_LEVELS grid levels (level l merges 2^l level-0 cells per axis), summed in 64-bit integers
//           k_md_pick     one thread: the finest level whose pair count fits the entry cap -> the header the other kernels read.  The
//                         host never learns the level: every later launch is sized for the caps, which depend on T alone.
//           k_md_cells<0> one thread per face: an int32 atomic add per overlapped cell
//           k_md_rank / k_md_tiles / k_md_offsets   exclusive prefix of the cell counts: in-tile scan, one block over the tile totals,
//                         add - integers, no atomics
//           k_md_cells<1> one thread per face: its slot in each overlapped cell through an atomic cursor (the counts, counted down).
//                         The order inside a cell is arbitrary; the query resolves ties by index explicitly, so no sort.
//   query:  k_md_query    ONE QUERY PER LANE, 256 lanes per workgroup, no LDS.  The alternatives were a wave that walks one query's
//                         candidate list together, and staging a shell's cell lists in LDS.  Chosen against both from the shape of the
//                         work, not from a measurement (nobody has one for this access pattern): the caps keep the cell lists
//                         short, so 64 lanes on one list would idle most of them and pay a wave reduction per cell;
//                         lanes of a wave sit in different cells, so there is no common list to stage.  What hides the latency of the
//                         gathered loads (start pair, face index, three indices, nine coordinates per candidate) is occupancy: the
//                         kernel needs few registers and no LDS, so a SIMD holds its eight waves.  Queries that arrive in mesh order
//                         (the vertices of a marching-cubes mesh, x-major) put neighbouring lanes into the same or neighbouring cells,
//                         and their gathers then hit the same cache lines; randomly ordered surface samples do not have that.
//   reduce: k_md_partial / k_md_finish   float64 sums in a fixed order (see the header), per-block partials and one finishing block.
//   sample: k_ms_tile / k_ms_group / k_ms_top / k_ms_cum   face areas in float64 and their inclusive prefix in a fixed three-level
//           order; k_ms_draw one thread per sample: Philox4x32-10 (the generator of dsn_train_draws) keyed by (seed, sample index).
// All global atomics are integer, relaxed, agent scope.  Everything read back from the workspace is range-checked before it is used
// as an index.  -ffp-contract=off (build.py): one rounding per operation, nothing fused.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include "dsn_philox.h"
#include <cmath>
#include <cstring>

#define MD_THREADS 256
#define MD_LEVELS 13                     // DSN_MESH_DIST_MAX_G = 4096 = 2^12: level 12 is a single cell
#define MD_TILE 1024                     // cells per scan tile (256 threads x 4)
#define MD_MAGIC 0x4d444958
#define MD_RED_PER 4                     // elements per thread of a reduction block: DSN_MESH_DIST_REDUCE_TILE = 256 x 4
#define MS_TILE 32                       // DSN_MESH_SAMPLE_TILE
#define MS_KIND_SURFACE 2u               // the generator's `kind` word (0 and 1: the jitter and the noise of dsn_train_draws)

// the header at the start of the workspace (device memory; written by build, read by query)
struct MdHead {
    int32_t magic, level, g[3], g0[3];
    float origin[3], cell0, inv0, slack;
    uint32_t ncells, entries;
    unsigned long long n_valid;
    unsigned long long pairs[MD_LEVELS];
};

static size_t md_up(size_t n) { return (n + 15) & ~(size_t)15; }
static int64_t md_cells_cap(int64_t T) { const int64_t m = 2 * T + 64; return m < ((int64_t)1 << 26) ? m : ((int64_t)1 << 26); }
static int64_t md_entries_cap(int64_t T) { const int64_t m = 8 * T + 64; return m < 0x7fffffffLL ? m : 0x7fffffffLL; }

// header 256 B | cell counts uint32 [cells_cap] | cell starts uint32 [cells_cap + 1] | tile totals uint32 [tiles + 1] |
// entries int32 [entries_cap]                                                             (every part 16-byte aligned)
struct MdWs { MdHead* head; uint32_t* cnt; uint32_t* start; uint32_t* tw; int32_t* ent; int64_t cells_cap, entries_cap, tiles; size_t bytes; };
static MdWs md_ws(void* w, int64_t T) {
    MdWs r;
    r.cells_cap = md_cells_cap(T);
    r.entries_cap = md_entries_cap(T);
    r.tiles = (r.cells_cap + MD_TILE - 1) / MD_TILE;
    char* p = (char*)w;
    size_t o = 0;
    static_assert(sizeof(MdHead) <= 256, "header");
    r.head = (MdHead*)(p + o); o += 256;
    r.cnt = (uint32_t*)(p + o); o += md_up((size_t)4 * r.cells_cap);
    r.start = (uint32_t*)(p + o); o += md_up((size_t)4 * (r.cells_cap + 1));
    r.tw = (uint32_t*)(p + o); o += md_up((size_t)4 * (r.tiles + 1));
    r.ent = (int32_t*)(p + o); o += md_up((size_t)4 * r.entries_cap);
    r.bytes = o;
    return r;
}
size_t dsn_mesh_dist_workspace_size(int64_t T) { return md_ws(nullptr, T).bytes; }

// the level-0 grid from the face count and the box (the rule of include/dsnerf.h), on the host, in double
void dsn_mesh_dist_grid_rule(int64_t T, const float* box6, int* g0, float* cell0) {
    double ext[3], L = 0.0;
    for (int a = 0; a < 3; ++a) { ext[a] = (double)box6[3 + a] - (double)box6[a]; L = ext[a] > L ? ext[a] : L; }
    g0[0] = g0[1] = g0[2] = 1;
    *cell0 = 1.0f;
    if (!(L > 0.0)) return;
    const int64_t M = md_cells_cap(T);
    auto count = [&](int n, int* g) {
        int64_t c = 1;
        for (int a = 0; a < 3; ++a) {
            const int64_t k = (int64_t)floor(ext[a] * (double)n / L) + 1;
            g[a] = (int)(k < n ? k : n);
            c *= g[a];
        }
        return c;
    };
    int lo = 1, hi = DSN_MESH_DIST_MAX_G, g[3];          // the largest n in [1, 4096] whose cell count fits (n = 1 always does)
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (count(mid, g) <= M) lo = mid; else hi = mid - 1;
    }
    const float c = (float)(L / (double)lo * (1.0 + 0x1p-20));
    const float inv = 1.0f / c;
    if (!(c > 0.0f) || !std::isfinite(inv) || !std::isfinite(c)) return;      // (a box too small to divide: one cell)
    for (int a = 0; a < 3; ++a) {
        const int64_t k = (int64_t)floor(ext[a] / (double)c) + 1;
        g0[a] = (int)(k < lo ? k : lo);
    }
    *cell0 = c;
}

__device__ __forceinline__ bool md_finite3(const float* __restrict__ p) {
    const float inf = __builtin_inff();
    return fabsf(p[0]) < inf && fabsf(p[1]) < inf && fabsf(p[2]) < inf;      // (NaN fails the comparison)
}

// a valid face: three indices in [0, V) and nine finite coordinates
__device__ __forceinline__ bool md_face(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t t, int64_t V, int32_t i[3]) {
    i[0] = faces[3 * t]; i[1] = faces[3 * t + 1]; i[2] = faces[3 * t + 2];
    if ((uint32_t)i[0] >= (uint32_t)V || (uint32_t)i[1] >= (uint32_t)V || (uint32_t)i[2] >= (uint32_t)V) return false;
    return md_finite3(verts + 3 * (int64_t)i[0]) && md_finite3(verts + 3 * (int64_t)i[1]) && md_finite3(verts + 3 * (int64_t)i[2]);
}

// level-0 cell of a finite coordinate along one axis: floor((x - origin) inv0) clamped to [0, g0 - 1].  Monotone in x.
__device__ __forceinline__ int md_cell0(float x, float origin, float inv0, int g0) {
    float t = (x - origin) * inv0;
    t = fminf(fmaxf(t, 0.0f), (float)(g0 - 1));
    return (int)floorf(t);
}

// the level-0 cell box of a valid face
__device__ __forceinline__ void md_face_box(const float* __restrict__ verts, const int32_t i[3], const float origin[3], float inv0,
                                            const int g0[3], int lo[3], int hi[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x0 = verts[3 * (int64_t)i[0] + a], x1 = verts[3 * (int64_t)i[1] + a], x2 = verts[3 * (int64_t)i[2] + a];
        lo[a] = md_cell0(fminf(x0, fminf(x1, x2)), origin[a], inv0, g0[a]);
        hi[a] = md_cell0(fmaxf(x0, fmaxf(x1, x2)), origin[a], inv0, g0[a]);
    }
}

struct MdGrid { float origin[3]; float cell0, inv0, slack; int g0[3]; };

__global__ void __launch_bounds__(MD_THREADS) k_md_zero(MdHead* __restrict__ head, uint32_t* __restrict__ cnt, int64_t cells_cap) {
    const int64_t c = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (c == 0) { head->magic = 0; head->n_valid = 0; }
    if (c < MD_LEVELS) head->pairs[c] = 0;
    if (c < cells_cap) cnt[c] = 0;
}

__global__ void __launch_bounds__(MD_THREADS) k_md_levels(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                          MdGrid G, unsigned long long cap, MdHead* __restrict__ head) {
    __shared__ unsigned long long s[MD_LEVELS + 1];
    if (threadIdx.x <= MD_LEVELS) s[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    int32_t i[3];
    if (t < T && md_face(verts, faces, t, V, i)) {
        int lo[3], hi[3];
        md_face_box(verts, i, G.origin, G.inv0, G.g0, lo, hi);
        for (int l = 0; l < MD_LEVELS; ++l) {
            unsigned long long n = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) n *= (unsigned long long)((hi[a] >> l) - (lo[a] >> l) + 1);      // <= 2^36
            n = n > cap + 1 ? cap + 1 : n;                   // saturated: T such terms stay below 2^63, and a sum above the cap stays above it
            atomicAdd(&s[l], n);
        }
        atomicAdd(&s[MD_LEVELS], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < MD_LEVELS && s[threadIdx.x])
        __hip_atomic_fetch_add(&head->pairs[threadIdx.x], s[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == MD_LEVELS && s[MD_LEVELS])
        __hip_atomic_fetch_add(&head->n_valid, s[MD_LEVELS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_md_pick(MdGrid G, unsigned long long cap, MdHead* __restrict__ head, int64_t* __restrict__ out_counts4) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int l = 0;
    while (l < MD_LEVELS - 1 && head->pairs[l] > cap) ++l;               // (level 12 is one cell: its count is n_valid <= T <= cap)
    head->level = l;
    uint32_t nc = 1;
    for (int a = 0; a < 3; ++a) {
        head->g0[a] = G.g0[a];
        head->g[a] = ((G.g0[a] - 1) >> l) + 1;
        head->origin[a] = G.origin[a];
        nc *= (uint32_t)head->g[a];
    }
    head->cell0 = G.cell0; head->inv0 = G.inv0; head->slack = G.slack;
    head->ncells = nc;
    head->entries = (uint32_t)head->pairs[l];
    head->magic = MD_MAGIC;
    if (out_counts4) {
        out_counts4[0] = (int64_t)head->n_valid; out_counts4[1] = (int64_t)head->pairs[l]; out_counts4[2] = l; out_counts4[3] = nc;
    }
}

// what every kernel after k_md_pick reads from the header, checked against the caps the host derived from T
struct MdView { int level, g[3], g0[3]; float origin[3], cell0, inv0, slack; uint32_t ncells, entries; bool ok; };
__device__ __forceinline__ MdView md_view(const MdHead* __restrict__ head, int64_t cells_cap, int64_t entries_cap) {
    MdView v;
    v.level = head->level;
    v.ok = head->magic == MD_MAGIC && v.level >= 0 && v.level < MD_LEVELS;
    uint64_t nc = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v.g[a] = head->g[a]; v.g0[a] = head->g0[a]; v.origin[a] = head->origin[a];
        v.ok = v.ok && v.g0[a] >= 1 && v.g0[a] <= DSN_MESH_DIST_MAX_G && v.g[a] == ((v.g0[a] - 1) >> (v.level & 15)) + 1;
        nc *= (uint64_t)(v.g[a] > 0 ? v.g[a] : 0);
    }
    v.cell0 = head->cell0; v.inv0 = head->inv0; v.slack = head->slack;
    v.ncells = head->ncells; v.entries = head->entries;
    v.ok = v.ok && nc == v.ncells && (int64_t)nc <= cells_cap && (int64_t)v.entries <= entries_cap;
    return v;
}

// FILL = false: count the faces of every cell; true: place them (cnt counts down to 0 and hands out the slots)
template <bool FILL>
__global__ void __launch_bounds__(MD_THREADS) k_md_cells(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                         const MdHead* __restrict__ head, int64_t cells_cap, int64_t entries_cap,
                                                         uint32_t* __restrict__ cnt, const uint32_t* __restrict__ start, int32_t* __restrict__ ent) {
    const int64_t t = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    const MdView v = md_view(head, cells_cap, entries_cap);
    int32_t i[3];
    if (!v.ok || t >= T || !md_face(verts, faces, t, V, i)) return;
    int lo[3], hi[3];
    md_face_box(verts, i, v.origin, v.inv0, v.g0, lo, hi);
    for (int x = lo[0] >> v.level; x <= hi[0] >> v.level; ++x)
        for (int y = lo[1] >> v.level; y <= hi[1] >> v.level; ++y)
            for (int z = lo[2] >> v.level; z <= hi[2] >> v.level; ++z) {
                const uint32_t c = ((uint32_t)x * (uint32_t)v.g[1] + (uint32_t)y) * (uint32_t)v.g[2] + (uint32_t)z;      // < ncells: the box is clamped to the grid
                if (!FILL) {
                    __hip_atomic_fetch_add(cnt + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    const uint32_t k = __hip_atomic_fetch_add(cnt + c, 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1u;
                    const uint64_t at = (uint64_t)start[c] + k;
                    if (at < (uint64_t)v.entries) ent[at] = (int32_t)t;
                }
            }
}

// in-tile exclusive prefix of the cell counts and the tile's total
__global__ void __launch_bounds__(MD_THREADS) k_md_rank(const uint32_t* __restrict__ cnt, const MdHead* __restrict__ head, int64_t cells_cap,
                                                        int64_t entries_cap, uint32_t* __restrict__ start, uint32_t* __restrict__ tw) {
    __shared__ uint32_t sa[MD_THREADS];
    const MdView v = md_view(head, cells_cap, entries_cap);
    const int64_t n = v.ok ? (int64_t)v.ncells : 0;
    const int t = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * MD_TILE + (int64_t)t * 4;
    uint32_t c[4], a = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { c[q] = c0 + q < n ? cnt[c0 + q] : 0u; a += c[q]; }
    sa[t] = a;
    __syncthreads();
    for (int off = 1; off < MD_THREADS; off <<= 1) {
        const uint32_t x = t >= off ? sa[t - off] : 0u;
        __syncthreads();
        sa[t] += x;
        __syncthreads();
    }
    uint32_t p = sa[t] - a;
#pragma unroll
    for (int q = 0; q < 4; ++q) { if (c0 + q < n) start[c0 + q] = p; p += c[q]; }
    if (t == MD_THREADS - 1) tw[blockIdx.x] = sa[t];
}

// one workgroup: exclusive scan of the tile totals in place
__global__ void __launch_bounds__(MD_THREADS) k_md_tiles(uint32_t* __restrict__ tw, int64_t tiles) {
    __shared__ uint32_t sa[MD_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (tiles + MD_THREADS - 1) / MD_THREADS;
    const int64_t b0 = t * per < tiles ? t * per : tiles, b1 = b0 + per < tiles ? b0 + per : tiles;
    uint32_t a = 0;
    for (int64_t k = b0; k < b1; ++k) a += tw[k];
    sa[t] = a;
    __syncthreads();
    for (int off = 1; off < MD_THREADS; off <<= 1) {
        const uint32_t x = t >= off ? sa[t - off] : 0u;
        __syncthreads();
        sa[t] += x;
        __syncthreads();
    }
    uint32_t r = sa[t] - a;
    for (int64_t k = b0; k < b1; ++k) { const uint32_t x = tw[k]; tw[k] = r; r += x; }
    if (t == MD_THREADS - 1) tw[tiles] = sa[t];
}

__global__ void __launch_bounds__(MD_THREADS) k_md_offsets(const MdHead* __restrict__ head, int64_t cells_cap, int64_t entries_cap,
                                                           uint32_t* __restrict__ start, const uint32_t* __restrict__ tw) {
    const MdView v = md_view(head, cells_cap, entries_cap);
    if (!v.ok) return;
    const int64_t c = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (c < (int64_t)v.ncells) start[c] += tw[c / MD_TILE];
    if (c == (int64_t)v.ncells) start[c] = v.entries;
}

__device__ __forceinline__ float md_dot(float x0, float x1, float x2, float y0, float y1, float y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }

// The closest point of the closed triangle (a, b, c) to p and its squared distance: the seven-region form (three vertex regions, three
// edge regions, the interior), float32, the operation order of include/dsnerf.h.  An edge region needs a denominator > 0: an edge of
// length zero (a == b makes d1 = d3 = 0 and vc = 0 for every p) has no region of its own, its end points and the other edges answer.
__device__ __forceinline__ float md_closest(const float p[3], const float a[3], const float b[3], const float c[3], float q[3]) {
    const float ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
    const float ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
    const float ap0 = p[0] - a[0], ap1 = p[1] - a[1], ap2 = p[2] - a[2];
    const float d1 = md_dot(ab0, ab1, ab2, ap0, ap1, ap2), d2 = md_dot(ac0, ac1, ac2, ap0, ap1, ap2);
    const float bp0 = p[0] - b[0], bp1 = p[1] - b[1], bp2 = p[2] - b[2];
    const float d3 = md_dot(ab0, ab1, ab2, bp0, bp1, bp2), d4 = md_dot(ac0, ac1, ac2, bp0, bp1, bp2);
    const float cp0 = p[0] - c[0], cp1 = p[1] - c[1], cp2 = p[2] - c[2];
    const float d5 = md_dot(ab0, ab1, ab2, cp0, cp1, cp2), d6 = md_dot(ac0, ac1, ac2, cp0, cp1, cp2);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const float den3 = d1 - d3, den5 = d2 - d6, den6 = e43 + e56;
    if (d1 <= 0.0f && d2 <= 0.0f) { q[0] = a[0]; q[1] = a[1]; q[2] = a[2]; }
    else if (d3 >= 0.0f && d4 <= d3) { q[0] = b[0]; q[1] = b[1]; q[2] = b[2]; }
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f && den3 > 0.0f) {
        const float v = d1 / den3;
        q[0] = a[0] + v * ab0; q[1] = a[1] + v * ab1; q[2] = a[2] + v * ab2;
    } else if (d6 >= 0.0f && d5 <= d6) { q[0] = c[0]; q[1] = c[1]; q[2] = c[2]; }
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f && den5 > 0.0f) {
        const float w = d2 / den5;
        q[0] = a[0] + w * ac0; q[1] = a[1] + w * ac1; q[2] = a[2] + w * ac2;
    } else if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f && den6 > 0.0f) {
        const float w = e43 / den6;
        q[0] = b[0] + w * (c[0] - b[0]); q[1] = b[1] + w * (c[1] - b[1]); q[2] = b[2] + w * (c[2] - b[2]);
    } else {
        const float inv = 1.0f / ((va + vb) + vc), v = vb * inv, w = vc * inv;
        q[0] = (a[0] + ab0 * v) + ac0 * w; q[1] = (a[1] + ab1 * v) + ac1 * w; q[2] = (a[2] + ab2 * v) + ac2 * w;
    }
    const float r0 = p[0] - q[0], r1 = p[1] - q[1], r2 = p[2] - q[2];
    return md_dot(r0, r1, r2, r0, r1, r2);
}

// May the search stop after the shells 0 ... r around cell c?  Every face not listed in those cells lies, along some axis, wholly in the
// cells beyond the cube: above the plane of cell index c + r + 1 or below the plane of cell index c - r (planes in level cells; a side
// on which the grid has no more cells holds no face).  `lb` is the smallest of the computed distances from p to those planes.
// The margin.  A face is skipped only if its COMPUTED squared distance exceeds `best`.  With S = the largest absolute coordinate of the
// box and eps = 2^-24:
//   - the computed plane fl(origin + fl(k cell0)) and the cell function fl(fl(x - origin) inv0) disagree about where cell k starts by
//     at most ~6 eps S (three roundings of quantities up to 2 S);
//   - the computed closest point is a + v ab + w ac with weights in [0, 1]: it lies within ~21 eps S of the triangle (sums of terms
//     up to 5 S per axis, three axes), so the computed distance is at least (true distance - 21 eps S) (1 - 4 eps), the last factor
//     for the roundings of p - q and of the dot product, which are relative to the distance itself;
//   - lb itself and lb lb carry three more relative roundings.
// slack = 128 eps S = S 2^-17 (set by the host) covers the absolute part four times over, the factor 1 - 2^-16 the relative part
// (seven roundings of 2^-24) more than a hundred times.  The comparison is strict; a shell is searched whenever it is not provably farther.
__device__ __forceinline__ bool md_shell_stops(const float p[3], const int c[3], int r, const MdView& v, float best) {
    float lb = __builtin_inff();
    bool any = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int up = c[a] + r + 1, dn = c[a] - r;
        if (up < v.g[a]) { any = true; lb = fminf(lb, (v.origin[a] + (float)((int64_t)up << v.level) * v.cell0) - p[a]); }
        if (dn > 0) { any = true; lb = fminf(lb, p[a] - (v.origin[a] + (float)((int64_t)dn << v.level) * v.cell0)); }
    }
    if (!any) return true;                                   // every cell has been searched
    lb = (lb - v.slack) * (1.0f - 0x1p-16f);
    return lb > 0.0f && lb * lb > best;
}

__global__ void __launch_bounds__(MD_THREADS) k_md_query(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                         const MdHead* __restrict__ head, int64_t cells_cap, int64_t entries_cap,
                                                         const uint32_t* __restrict__ start, const int32_t* __restrict__ ent,
                                                         const float* __restrict__ points, int64_t n, float* __restrict__ out_d2,
                                                         int32_t* __restrict__ out_face, float* __restrict__ out_point) {
    const int64_t i = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (i >= n) return;
    const MdView v = md_view(head, cells_cap, entries_cap);
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    const float nan = __builtin_nanf("");
    float best = __builtin_inff(), bq[3] = {nan, nan, nan};
    int32_t bf = -1;
    if (!v.ok || !md_finite3(p)) {
        best = nan;
    } else {
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = md_cell0(p[a], v.origin[a], v.inv0, v.g0[a]) >> v.level;      // (a point outside the box: clamped)
        for (int r = 0;; ++r) {
            const int z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = c[2] + r < v.g[2] - 1 ? c[2] + r : v.g[2] - 1;
            const int y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < v.g[1] - 1 ? c[1] + r : v.g[1] - 1;
            const int x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < v.g[0] - 1 ? c[0] + r : v.g[0] - 1;
            for (int x = x0; x <= x1; ++x) {
                const bool xf = x - c[0] == r || c[0] - x == r;
                for (int y = y0; y <= y1; ++y) {
                    const bool full = xf || y - c[1] == r || c[1] - y == r;       // a face of the shell: the whole z run; else its two ends
                    const int zs = full ? z0 : c[2] - r, ze = full ? z1 : c[2] + r, st = full ? 1 : 2 * r;
                    for (int z = zs; z <= ze; z += st) {
                        if (z < 0 || z >= v.g[2]) continue;
                        const uint32_t cell = ((uint32_t)x * (uint32_t)v.g[1] + (uint32_t)y) * (uint32_t)v.g[2] + (uint32_t)z;
                        uint32_t k0 = start[cell], k1 = start[cell + 1];
                        k1 = k1 < v.entries ? k1 : v.entries;
                        for (uint32_t k = k0; k < k1; ++k) {
                            const int32_t f = ent[k];
                            if ((uint32_t)f >= (uint32_t)T) continue;
                            const int32_t ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
                            if ((uint32_t)ia >= (uint32_t)V || (uint32_t)ib >= (uint32_t)V || (uint32_t)ic >= (uint32_t)V) continue;
                            const float* pa = verts + 3 * (int64_t)ia;
                            const float* pb = verts + 3 * (int64_t)ib;
                            const float* pc = verts + 3 * (int64_t)ic;
                            const float A[3] = {pa[0], pa[1], pa[2]}, B[3] = {pb[0], pb[1], pb[2]}, Cc[3] = {pc[0], pc[1], pc[2]};
                            float q[3];
                            const float d = md_closest(p, A, B, Cc, q);
                            if (d < best || (d == best && f < bf)) { best = d; bf = f; bq[0] = q[0]; bq[1] = q[1]; bq[2] = q[2]; }
                        }
                    }
                }
            }
            if (md_shell_stops(p, c, r, v, best)) break;
        }
    }
    if (out_d2) out_d2[i] = best;
    if (out_face) out_face[i] = bf;
    if (out_point) { out_point[3 * i] = bq[0]; out_point[3 * i + 1] = bq[1]; out_point[3 * i + 2] = bq[2]; }
}

void dsn_launch_mesh_dist_build(const float* verts, const int32_t* faces, int64_t V, int64_t T, const float* box6, void* workspace,
                                int64_t* out_counts4, hipStream_t st) {
    const MdWs w = md_ws(workspace, T);
    MdGrid G;
    dsn_mesh_dist_grid_rule(T, box6, G.g0, &G.cell0);
    G.inv0 = 1.0f / G.cell0;
    float S = 0.0f;
    for (int a = 0; a < 3; ++a) { G.origin[a] = box6[a]; S = fmaxf(S, fmaxf(fabsf(box6[a]), fabsf(box6[3 + a]))); }
    G.slack = S * 0x1p-17f;
    const unsigned blocksT = (unsigned)((T + MD_THREADS - 1) / MD_THREADS);
    const unsigned long long cap = (unsigned long long)w.entries_cap;
    hipLaunchKernelGGL(k_md_zero, dim3((unsigned)((w.cells_cap + MD_THREADS - 1) / MD_THREADS)), dim3(MD_THREADS), 0, st, w.head, w.cnt,
                       w.cells_cap);
    hipLaunchKernelGGL(k_md_levels, dim3(blocksT), dim3(MD_THREADS), 0, st, verts, faces, V, T, G, cap, w.head);
    hipLaunchKernelGGL(k_md_pick, dim3(1), dim3(64), 0, st, G, cap, w.head, out_counts4);
    hipLaunchKernelGGL(k_md_cells<false>, dim3(blocksT), dim3(MD_THREADS), 0, st, verts, faces, V, T, (const MdHead*)w.head, w.cells_cap,
                       w.entries_cap, w.cnt, (const uint32_t*)w.start, w.ent);
    hipLaunchKernelGGL(k_md_rank, dim3((unsigned)w.tiles), dim3(MD_THREADS), 0, st, (const uint32_t*)w.cnt, (const MdHead*)w.head, w.cells_cap,
                       w.entries_cap, w.start, w.tw);
    hipLaunchKernelGGL(k_md_tiles, dim3(1), dim3(MD_THREADS), 0, st, w.tw, w.tiles);
    hipLaunchKernelGGL(k_md_offsets, dim3((unsigned)((w.cells_cap + 1 + MD_THREADS - 1) / MD_THREADS)), dim3(MD_THREADS), 0, st,
                       (const MdHead*)w.head, w.cells_cap, w.entries_cap, w.start, (const uint32_t*)w.tw);
    hipLaunchKernelGGL(k_md_cells<true>, dim3(blocksT), dim3(MD_THREADS), 0, st, verts, faces, V, T, (const MdHead*)w.head, w.cells_cap,
                       w.entries_cap, w.cnt, (const uint32_t*)w.start, w.ent);
}

void dsn_launch_mesh_dist_query(const float* verts, const int32_t* faces, int64_t V, int64_t T, const void* workspace, const float* points,
                                int64_t n, float* out_d2, int32_t* out_face, float* out_point, hipStream_t st) {
    if (n == 0) return;
    const MdWs w = md_ws(const_cast<void*>(workspace), T);
    hipLaunchKernelGGL(k_md_query, dim3((unsigned)((n + MD_THREADS - 1) / MD_THREADS)), dim3(MD_THREADS), 0, st, verts, faces, V, T,
                       (const MdHead*)w.head, w.cells_cap, w.entries_cap, (const uint32_t*)w.start, (const int32_t*)w.ent, points, n, out_d2,
                       out_face, out_point);
}

// ---------------------------------------------------------------------------------------------
// the reduction (dsn_mesh_dist_reduce)
// ---------------------------------------------------------------------------------------------
struct MdPart { double sum_d, sum_d2; unsigned long long count, nans; float max_d2; int32_t pad; int64_t arg; };      // 48 bytes

__device__ __forceinline__ void md_max(float& m, int64_t& at, float m2, int64_t at2) {
    if (at2 >= 0 && (at < 0 || m2 > m || (m2 == m && at2 < at))) { m = m2; at = at2; }
}

// the tree both reduction kernels end with: x[t] += x[t + s] for s = 128, 64, ..., 1
__device__ __forceinline__ MdPart md_tree(MdPart mine, MdPart* __restrict__ sh) {
    const int t = threadIdx.x;
    sh[t] = mine;
    __syncthreads();
    for (int s = MD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            MdPart x = sh[t];
            const MdPart y = sh[t + s];
            x.sum_d = x.sum_d + y.sum_d; x.sum_d2 = x.sum_d2 + y.sum_d2; x.count += y.count; x.nans += y.nans;
            md_max(x.max_d2, x.arg, y.max_d2, y.arg);
            sh[t] = x;
        }
        __syncthreads();
    }
    return sh[0];
}

__global__ void __launch_bounds__(MD_THREADS) k_md_partial(const float* __restrict__ d2, int64_t n, MdPart* __restrict__ parts) {
    __shared__ MdPart sh[MD_THREADS];
    MdPart m = {0.0, 0.0, 0ull, 0ull, 0.0f, 0, -1};
    const int64_t base = (int64_t)blockIdx.x * (MD_THREADS * MD_RED_PER) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < MD_RED_PER; ++j) {
        const int64_t i = base + (int64_t)j * MD_THREADS;
        if (i >= n) continue;
        const float x = d2[i];
        if (x != x) { m.nans += 1; continue; }
        m.count += 1;
        m.sum_d2 = m.sum_d2 + (double)x;
        m.sum_d = m.sum_d + sqrt((double)x);
        md_max(m.max_d2, m.arg, x, i);
    }
    const MdPart r = md_tree(m, sh);
    if (threadIdx.x == 0) parts[blockIdx.x] = r;
}

__global__ void __launch_bounds__(MD_THREADS) k_md_finish(const MdPart* __restrict__ parts, int64_t blocks, double* __restrict__ out6) {
    __shared__ MdPart sh[MD_THREADS];
    MdPart m = {0.0, 0.0, 0ull, 0ull, 0.0f, 0, -1};
    for (int64_t b = threadIdx.x; b < blocks; b += MD_THREADS) {
        const MdPart y = parts[b];
        m.sum_d = m.sum_d + y.sum_d; m.sum_d2 = m.sum_d2 + y.sum_d2; m.count += y.count; m.nans += y.nans;
        md_max(m.max_d2, m.arg, y.max_d2, y.arg);
    }
    const MdPart r = md_tree(m, sh);
    if (threadIdx.x == 0) {
        out6[0] = (double)r.count; out6[1] = (double)r.nans; out6[2] = r.sum_d; out6[3] = r.sum_d2;
        out6[4] = r.arg >= 0 ? sqrt((double)r.max_d2) : 0.0; out6[5] = (double)r.arg;
    }
}

static int64_t md_red_blocks(int64_t n) { return (n + MD_THREADS * MD_RED_PER - 1) / (MD_THREADS * MD_RED_PER); }
size_t dsn_mesh_dist_reduce_workspace_size(int64_t n) { return md_up(sizeof(MdPart) * (size_t)(md_red_blocks(n) > 0 ? md_red_blocks(n) : 1)); }

void dsn_launch_mesh_dist_reduce(const float* d2, int64_t n, void* workspace, double* out6, hipStream_t st) {
    const int64_t blocks = md_red_blocks(n);
    if (blocks > 0) hipLaunchKernelGGL(k_md_partial, dim3((unsigned)blocks), dim3(MD_THREADS), 0, st, d2, n, (MdPart*)workspace);
    hipLaunchKernelGGL(k_md_finish, dim3(1), dim3(MD_THREADS), 0, st, (const MdPart*)workspace, blocks, out6);
}

// ---------------------------------------------------------------------------------------------
// area-weighted surface samples (dsn_mesh_sample_surface)
// ---------------------------------------------------------------------------------------------
// cum float64 [T] | tile totals float64 [tiles] | group totals float64 [groups] | total float64 [2]
struct MsWs { double* cum; double* tile; double* group; double* total; int64_t tiles, groups; size_t bytes; };
static MsWs ms_ws(void* w, int64_t T) {
    MsWs r;
    r.tiles = (T + MS_TILE - 1) / MS_TILE;
    r.groups = (r.tiles + MS_TILE - 1) / MS_TILE;
    char* p = (char*)w;
    size_t o = 0;
    r.cum = (double*)(p + o); o += md_up((size_t)8 * T);
    r.tile = (double*)(p + o); o += md_up((size_t)8 * r.tiles);
    r.group = (double*)(p + o); o += md_up((size_t)8 * r.groups);
    r.total = (double*)(p + o); o += 16;
    r.bytes = o;
    return r;
}
size_t dsn_mesh_sample_workspace_size(int64_t T) { return ms_ws(nullptr, T).bytes; }

// float64 area of a valid face (0 for the others): half the norm of the cross product of b - a and c - a
__device__ __forceinline__ double ms_area(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t t, int64_t V) {
    int32_t i[3];
    if (!md_face(verts, faces, t, V, i)) return 0.0;
    const float* a = verts + 3 * (int64_t)i[0];
    const float* b = verts + 3 * (int64_t)i[1];
    const float* c = verts + 3 * (int64_t)i[2];
    const double e0 = (double)b[0] - (double)a[0], e1 = (double)b[1] - (double)a[1], e2 = (double)b[2] - (double)a[2];
    const double f0 = (double)c[0] - (double)a[0], f1 = (double)c[1] - (double)a[1], f2 = (double)c[2] - (double)a[2];
    const double n0 = e1 * f2 - e2 * f1, n1 = e2 * f0 - e0 * f2, n2 = e0 * f1 - e1 * f0;
    return 0.5 * sqrt((n0 * n0 + n1 * n1) + n2 * n2);
}

// one thread per tile of MS_TILE faces: the running sums inside the tile, in face order, and the tile's total
__global__ void __launch_bounds__(MD_THREADS) k_ms_tile(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                        MsWs w) {
    const int64_t k = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (k >= w.tiles) return;
    double s = 0.0;
    const int64_t t1 = (k + 1) * MS_TILE < T ? (k + 1) * MS_TILE : T;
    for (int64_t t = k * MS_TILE; t < t1; ++t) { s = s + ms_area(verts, faces, t, V); w.cum[t] = s; }
    w.tile[k] = s;
}
// one thread per group of MS_TILE tiles: the running sums of the tile totals inside the group (in place) and the group's total
__global__ void __launch_bounds__(MD_THREADS) k_ms_group(MsWs w) {
    const int64_t g = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (g >= w.groups) return;
    double s = 0.0;
    const int64_t k1 = (g + 1) * MS_TILE < w.tiles ? (g + 1) * MS_TILE : w.tiles;
    for (int64_t k = g * MS_TILE; k < k1; ++k) { s = s + w.tile[k]; w.tile[k] = s; }
    w.group[g] = s;
}
// one thread: the running sums of the group totals (in place) and the total
__global__ void k_ms_top(MsWs w) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int64_t g = 0; g < w.groups; ++g) { s = s + w.group[g]; w.group[g] = s; }
    w.total[0] = s;
}
// cum[t] = groups before + (tiles before, inside the group + faces up to t, inside the tile)
__global__ void __launch_bounds__(MD_THREADS) k_ms_cum(int64_t T, MsWs w) {
    const int64_t t = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (t >= T) return;
    const int64_t k = t / MS_TILE, g = k / MS_TILE;
    const double before_tile = k % MS_TILE ? w.tile[k - 1] : 0.0, before_group = g ? w.group[g - 1] : 0.0;
    w.cum[t] = before_group + (before_tile + w.cum[t]);
}

__global__ void __launch_bounds__(MD_THREADS) k_ms_draw(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                        uint32_t k0, uint32_t k1, MsWs w, int64_t n, float* __restrict__ out_points,
                                                        int32_t* __restrict__ out_face) {
    const int64_t i = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (i >= n) return;
    const double total = w.total[0];
    const DsnPhiloxOut r = dsn_philox4x32_10((uint32_t)i, 0u, 0u, MS_KIND_SURFACE, k0, k1);
    const float nan = __builtin_nanf("");
    float q[3] = {nan, nan, nan};
    int64_t f = -1;
    if (total > 0.0 && total < (double)__builtin_inff()) {
        const double u0 = (double)(((unsigned long long)r.x[0] << 20) | (unsigned long long)(r.x[1] >> 12)) * 0x1p-52;      // 52 bits: u0 total < total
        const double x = u0 * total;
        int64_t lo = 0, hi = T - 1;                              // the first face whose running sum exceeds x (cum[T - 1] = total > x)
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (w.cum[mid] > x) hi = mid; else lo = mid + 1;
        }
        f = lo;
        int32_t j[3];
        if (md_face(verts, faces, f, V, j)) {                    // (a face with a positive area is valid)
            float u = (float)(r.x[2] >> 8) * 0x1p-24f, v = (float)(r.x[3] >> 8) * 0x1p-24f;
            if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
            const float* a = verts + 3 * (int64_t)j[0];
            const float* b = verts + 3 * (int64_t)j[1];
            const float* c = verts + 3 * (int64_t)j[2];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) q[ax] = (a[ax] + u * (b[ax] - a[ax])) + v * (c[ax] - a[ax]);
        } else {
            f = -1;
        }
    }
    if (out_points) { out_points[3 * i] = q[0]; out_points[3 * i + 1] = q[1]; out_points[3 * i + 2] = q[2]; }
    if (out_face) out_face[i] = (int32_t)f;
}

void dsn_launch_mesh_sample_surface(const float* verts, const int32_t* faces, int64_t V, int64_t T, uint64_t seed, int64_t n, void* workspace,
                                    float* out_points, int32_t* out_face, hipStream_t st) {
    const MsWs w = ms_ws(workspace, T);
    auto blocks = [](int64_t k) { return dim3((unsigned)((k + MD_THREADS - 1) / MD_THREADS)); };
    hipLaunchKernelGGL(k_ms_tile, blocks(w.tiles), dim3(MD_THREADS), 0, st, verts, faces, V, T, w);
    hipLaunchKernelGGL(k_ms_group, blocks(w.groups), dim3(MD_THREADS), 0, st, w);
    hipLaunchKernelGGL(k_ms_top, dim3(1), dim3(64), 0, st, w);
    hipLaunchKernelGGL(k_ms_cum, blocks(T), dim3(MD_THREADS), 0, st, T, w);
    if (n > 0)
        hipLaunchKernelGGL(k_ms_draw, blocks(n), dim3(MD_THREADS), 0, st, verts, faces, V, T, (uint32_t)seed, (uint32_t)(seed >> 32), w, n,
                           out_points, out_face);
}
