// dsn_mesh.hip - what utils/visualizer.py Visualizer3D does with a trained model, on the device: the points of its density grid
// (get_grid_pred_batch; the warp and the field behind them are dsn_warp's and k_field16's, orchestrated by dsn_density_grid) and
// a deterministic marching cubes over the grid (get_mesh_from_grid's skimage.measure.marching_cubes, with the rule of
// include/dsnerf.h).
//
// Marching cubes in two passes over tiles of MC_TILE consecutive grid points, one workgroup per tile, no atomics:
//   count: per point its crossing edges (bit d: the edge to the neighbour along axis d changes sign) and, per cell whose base corner
//          it is, the number of triangles of its case.  The points' vertex prefixes inside the tile are one workgroup scan; each
//          point keeps (prefix << 3 | crossing bits) in one int32 word, each tile its two totals.  One workgroup then scans the
//          tiles' totals (int64) into tile offsets and writes [vertices, triangles].
//   emit : vertex of edge (n, d) = tile offset + the point's prefix + crossing bits of n below d, i.e. ascending edge id 3 n + d;
//          a cell's triangles go to the tile offset + the workgroup scan of the triangle counts, in table order; each triangle's
//          corners are the vertex numbers of its three cube edges, looked up in the owning points' words.
#include "dsn_common.h"
#include "dsn_kernels.h"
#include "../../include/dsnerf.h"

// ---------------------------------------------------------------------------------------------
// density grid points: slab point m = (x[i0 + m / (ny nz)], y[(m / nz) % ny], z[m % nz]) - the order of the reference's
// torch.meshgrid(x, y, z) + vstack(...).T (get_grid, utils/visualizer.py:228-229)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_grid_points(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                     int i0, int ny, int nz, int64_t n, float* __restrict__ pts) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= n) return;
    const int64_t plane = (int64_t)ny * nz;
    const int64_t r = m % plane;
    pts[3 * m + 0] = x[i0 + (int)(m / plane)];
    pts[3 * m + 1] = y[(int)(r / nz)];
    pts[3 * m + 2] = z[(int)(r % nz)];
}

void dsn_launch_grid_points(const float* x, const float* y, const float* z, int i0, int ny, int nz, int64_t n, float* pts, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_grid_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, z, i0, ny, nz, n, pts);
}

// ---------------------------------------------------------------------------------------------
// case table, generated at compile time (numbering: include/dsnerf.h)
//   corner c = dx + 2 dy + 4 dz;  edge e = 4 d + q along axis d (0 = x, 1 = y, 2 = z), q = b1 + 2 b2 over the two other axes in
//   increasing order; its corners are c0 (bit d clear) and c0 | 1 << d.  Inside = value > level.
// ---------------------------------------------------------------------------------------------
namespace {
struct McTable {
    int8_t tri[256][DSN_MC_MAX_TRI * 3];
    int8_t ntri[256];
};

constexpr int mc_other(int d, int k) { return d == 0 ? (k == 0 ? 1 : 2) : (d == 1 ? (k == 0 ? 0 : 2) : (k == 0 ? 0 : 1)); }
constexpr int mc_bit(int c, int a) { return (c >> a) & 1; }
constexpr int mc_edge_c0(int e) {
    const int d = e / 4, q = e % 4;
    return ((q & 1) << mc_other(d, 0)) | ((q >> 1) << mc_other(d, 1));
}
constexpr int mc_edge_of(int ca, int cb) {      // the cube edge between two corners that differ in one bit
    const int x = ca ^ cb;
    const int d = x == 1 ? 0 : (x == 2 ? 1 : 2);
    const int c0 = ca < cb ? ca : cb;
    return 4 * d + mc_bit(c0, mc_other(d, 0)) + 2 * mc_bit(c0, mc_other(d, 1));
}

constexpr McTable mc_make_table() {
    McTable t{};
    for (int cs = 0; cs < 256; ++cs) {
        int next[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
        bool cross[12] = {};
        for (int e = 0; e < 12; ++e) {
            const int c0 = mc_edge_c0(e), c1 = c0 | (1 << (e / 4));
            cross[e] = mc_bit(cs, c0) != mc_bit(cs, c1);
        }
        // face segments: face (axis fa, side s), corners in cyclic order over its two other axes (u, v): (0,0) (1,0) (1,1) (0,1)
        for (int fa = 0; fa < 3; ++fa)
            for (int s = 0; s < 2; ++s) {
                const int u = mc_other(fa, 0), v = mc_other(fa, 1);
                int C[4] = {}, E[4] = {};
                const int cu[4] = {0, 1, 1, 0}, cv[4] = {0, 0, 1, 1};
                for (int k = 0; k < 4; ++k) C[k] = (s << fa) | (cu[k] << u) | (cv[k] << v);
                for (int k = 0; k < 4; ++k) E[k] = mc_edge_of(C[k], C[(k + 1) % 4]);
                int seg[2][2] = {}, nseg = 0, ncross = 0;
                for (int k = 0; k < 4; ++k) ncross += cross[E[k]] ? 1 : 0;
                if (ncross == 2) {
                    int a = -1, b = -1;
                    for (int k = 0; k < 4; ++k)
                        if (cross[E[k]]) { if (a < 0) a = E[k]; else b = E[k]; }
                    seg[0][0] = a; seg[0][1] = b; nseg = 1;
                } else if (ncross == 4) {
                    // ambiguous face (diagonal corners inside): each inside corner is cut off on its own
                    for (int k = 0; k < 4; ++k)
                        if (mc_bit(cs, C[k])) { seg[nseg][0] = E[(k + 3) % 4]; seg[nseg][1] = E[k]; ++nseg; }
                }
                for (int g = 0; g < nseg; ++g) {
                    // orient P -> Q so that the surface normal (right-hand rule along the loop) points from inside to outside:
                    // with g = outside corner - inside corner of P's edge, t = Q - P (edge midpoints) and n the face's outward
                    // normal, (g x t) . n < 0
                    const int P = seg[g][0], Q = seg[g][1];
                    const int p0 = mc_edge_c0(P), p1 = p0 | (1 << (P / 4)), q0 = mc_edge_c0(Q), q1 = q0 | (1 << (Q / 4));
                    const int cin = mc_bit(cs, p0) ? p0 : p1, cout = mc_bit(cs, p0) ? p1 : p0;
                    int gv[3] = {}, tv[3] = {}, nv[3] = {};
                    for (int a = 0; a < 3; ++a) {
                        gv[a] = mc_bit(cout, a) - mc_bit(cin, a);
                        tv[a] = (mc_bit(q0, a) + mc_bit(q1, a)) - (mc_bit(p0, a) + mc_bit(p1, a));
                    }
                    nv[fa] = s ? 1 : -1;
                    const int cx = gv[1] * tv[2] - gv[2] * tv[1], cy = gv[2] * tv[0] - gv[0] * tv[2], cz = gv[0] * tv[1] - gv[1] * tv[0];
                    const int dot = cx * nv[0] + cy * nv[1] + cz * nv[2];
                    if (dot < 0) next[P] = Q; else next[Q] = P;
                }
            }
        // loops in order of their lowest edge, each fanned from that edge
        bool seen[12] = {};
        int nt = 0;
        for (int e = 0; e < 12; ++e) {
            if (!cross[e] || seen[e]) continue;
            int loop[12] = {}, L = 0, cur = e;
            do { loop[L++] = cur; seen[cur] = true; cur = next[cur]; } while (cur != e && cur >= 0 && L < 12);
            for (int k = 1; k + 1 < L; ++k) {
                t.tri[cs][3 * nt + 0] = (int8_t)loop[0];
                t.tri[cs][3 * nt + 1] = (int8_t)loop[k];
                t.tri[cs][3 * nt + 2] = (int8_t)loop[k + 1];
                ++nt;
            }
        }
        t.ntri[cs] = (int8_t)nt;
        for (int k = 3 * nt; k < DSN_MC_MAX_TRI * 3; ++k) t.tri[cs][k] = -1;
    }
    return t;
}

constexpr bool mc_table_ok(const McTable& t) {
    for (int cs = 0; cs < 256; ++cs) {
        if (t.ntri[cs] < 0 || t.ntri[cs] > DSN_MC_MAX_TRI) return false;
        for (int k = 0; k < 3 * t.ntri[cs]; ++k)
            if (t.tri[cs][k] < 0 || t.tri[cs][k] > 11) return false;
    }
    return t.ntri[0] == 0 && t.ntri[255] == 0;
}
constexpr McTable k_mc_table = mc_make_table();
static_assert(mc_table_ok(k_mc_table), "marching-cubes case table");
}  // namespace

__constant__ McTable g_mc_table = k_mc_table;

void dsn_mc_table_copy(int32_t* out) {
    for (int cs = 0; cs < 256; ++cs) {
        out[cs * DSN_MC_TABLE_ROW] = k_mc_table.ntri[cs];
        for (int k = 0; k < 3 * DSN_MC_MAX_TRI; ++k) out[cs * DSN_MC_TABLE_ROW + 1 + k] = k_mc_table.tri[cs][k];
    }
}

// ---------------------------------------------------------------------------------------------
// marching cubes passes
// ---------------------------------------------------------------------------------------------
#define MC_THREADS 256
#define MC_PER 16                              // consecutive grid points per thread
#define MC_TILE (MC_THREADS * MC_PER)          // 4096 grid points per workgroup
#define MC_SCAN_THREADS 1024

static int64_t mc_tiles(int64_t N) { return (N + MC_TILE - 1) / MC_TILE; }
// words int32 [N] (8-byte aligned) | tile vertex offsets int64 [tiles + 1] | tile triangle offsets int64 [tiles + 1]
size_t dsn_mc_workspace_size(int64_t N) {
    return ((size_t)4 * N + 7) / 8 * 8 + 2 * 8 * (size_t)(mc_tiles(N) + 1);
}
struct McWs { int32_t* words; int64_t* tv; int64_t* tf; };
static McWs mc_ws(void* w, int64_t N) {
    char* p = (char*)w;
    McWs r;
    r.words = (int32_t*)p;
    r.tv = (int64_t*)(p + ((size_t)4 * N + 7) / 8 * 8);
    r.tf = r.tv + mc_tiles(N) + 1;
    return r;
}

__device__ __forceinline__ bool mc_in(float v, float level) { return v > level; }      // (NaN: outside)

// exclusive scan of (a, b) over the workgroup in thread order; returns the totals
__device__ __forceinline__ void mc_block_scan(int& a, int& b, int& tot_a, int& tot_b) {
    __shared__ int sa[MC_THREADS], sb[MC_THREADS];
    const int t = threadIdx.x;
    sa[t] = a; sb[t] = b;
    __syncthreads();
    for (int off = 1; off < MC_THREADS; off <<= 1) {
        const int xa = t >= off ? sa[t - off] : 0, xb = t >= off ? sb[t - off] : 0;
        __syncthreads();
        sa[t] += xa; sb[t] += xb;
        __syncthreads();
    }
    tot_a = sa[MC_THREADS - 1]; tot_b = sb[MC_THREADS - 1];
    a = sa[t] - a; b = sb[t] - b;
    __syncthreads();
}

struct McPoint { int i, j, k; };
__device__ __forceinline__ McPoint mc_ijk(int64_t n, int ny, int nz) {
    const int64_t plane = (int64_t)ny * nz;
    const int64_t r = n % plane;
    return McPoint{(int)(n / plane), (int)(r / nz), (int)(r % nz)};
}
__device__ __forceinline__ void mc_step(McPoint& p, int ny, int nz) {
    if (++p.k == nz) { p.k = 0; if (++p.j == ny) { p.j = 0; ++p.i; } }
}
// crossing bits of point n (bit d: edge to the neighbour along axis d) and the case of the cell it is the base corner of (-1: none)
__device__ __forceinline__ void mc_point(const float* __restrict__ vol, int64_t n, const McPoint& p, int nx, int ny, int nz, float level,
                                         int& bits, int& cs) {
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const bool in0 = mc_in(vol[n], level);
    bits = 0;
    if (p.i + 1 < nx && mc_in(vol[n + sx], level) != in0) bits |= 1;
    if (p.j + 1 < ny && mc_in(vol[n + sy], level) != in0) bits |= 2;
    if (p.k + 1 < nz && mc_in(vol[n + 1], level) != in0) bits |= 4;
    cs = -1;
    if (p.i + 1 < nx && p.j + 1 < ny && p.k + 1 < nz) {
        cs = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int64_t o = (c & 1) * sx + ((c >> 1) & 1) * sy + ((c >> 2) & 1);
            if (mc_in(vol[n + o], level)) cs |= 1 << c;
        }
    }
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_count(const float* __restrict__ vol, int nx, int ny, int nz, float level,
                                                         int32_t* __restrict__ words, int64_t* __restrict__ tv, int64_t* __restrict__ tf) {
    const int64_t N = (int64_t)nx * ny * nz;
    const int64_t n0 = (int64_t)blockIdx.x * MC_TILE + (int64_t)threadIdx.x * MC_PER;
    int nv = 0, nf = 0;
    uint32_t bits_all[MC_PER / 8] = {};       // 3 bits per point, packed (4 bits a point: 8 points a word)
    if (n0 < N) {
        McPoint p = mc_ijk(n0, ny, nz);
        for (int q = 0; q < MC_PER && n0 + q < N; ++q) {
            int bits, cs;
            mc_point(vol, n0 + q, p, nx, ny, nz, level, bits, cs);
            bits_all[q >> 3] |= (uint32_t)bits << (4 * (q & 7));
            nv += __popc(bits);
            if (cs >= 0) nf += g_mc_table.ntri[cs];
            mc_step(p, ny, nz);
        }
    }
    int pv = nv, pf = nf, tot_v, tot_f;
    mc_block_scan(pv, pf, tot_v, tot_f);
    for (int q = 0; q < MC_PER && n0 + q < N; ++q) {
        const int bits = (bits_all[q >> 3] >> (4 * (q & 7))) & 7;
        words[n0 + q] = (pv << 3) | bits;
        pv += __popc(bits);
    }
    if (threadIdx.x == 0) { tv[blockIdx.x] = tot_v; tf[blockIdx.x] = tot_f; }
}

// one workgroup: exclusive scan of the tiles' totals in place, [tiles] = the grand totals, also copied to out[0..1]
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_mc_scan(int64_t* __restrict__ tv, int64_t* __restrict__ tf, int64_t tiles,
                                                             int64_t* __restrict__ out) {
    __shared__ int64_t sa[MC_SCAN_THREADS], sb[MC_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (tiles + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int64_t b0 = t * per, b1 = b0 + per < tiles ? b0 + per : tiles;
    int64_t a = 0, b = 0;
    for (int64_t k = b0; k < b1; ++k) { a += tv[k]; b += tf[k]; }
    sa[t] = a; sb[t] = b;
    __syncthreads();
    for (int off = 1; off < MC_SCAN_THREADS; off <<= 1) {
        const int64_t xa = t >= off ? sa[t - off] : 0, xb = t >= off ? sb[t - off] : 0;
        __syncthreads();
        sa[t] += xa; sb[t] += xb;
        __syncthreads();
    }
    int64_t ra = sa[t] - a, rb = sb[t] - b;
    for (int64_t k = b0; k < b1; ++k) {
        const int64_t va = tv[k], vb = tf[k];
        tv[k] = ra; tf[k] = rb;
        ra += va; rb += vb;
    }
    if (t == MC_SCAN_THREADS - 1) {
        tv[tiles] = sa[t]; tf[tiles] = sb[t];
        out[0] = sa[t]; out[1] = sb[t];
    }
}

// vertex number of the crossing edge (m, d): its tile's offset + the point's prefix + its crossing bits below d
__device__ __forceinline__ int64_t mc_vertex(const int32_t* __restrict__ words, const int64_t* __restrict__ tv, int64_t m, int d) {
    const int w = words[m];
    return tv[m / MC_TILE] + (w >> 3) + __popc(w & ((1 << d) - 1));
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_emit(const float* __restrict__ vol, int nx, int ny, int nz, const float* __restrict__ ax,
                                                        const float* __restrict__ ay, const float* __restrict__ az, float level, int ascent,
                                                        const int32_t* __restrict__ words, const int64_t* __restrict__ tv,
                                                        const int64_t* __restrict__ tf, float* __restrict__ verts, int64_t vcap,
                                                        int32_t* __restrict__ faces, int64_t fcap) {
    const int64_t N = (int64_t)nx * ny * nz;
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const int64_t n0 = (int64_t)blockIdx.x * MC_TILE + (int64_t)threadIdx.x * MC_PER;
    int nf = 0;
    if (n0 < N) {      // triangle counts again (the workgroup scan below orders them)
        McPoint p = mc_ijk(n0, ny, nz);
        for (int q = 0; q < MC_PER && n0 + q < N; ++q) {
            int bits, cs;
            mc_point(vol, n0 + q, p, nx, ny, nz, level, bits, cs);
            if (cs >= 0) nf += g_mc_table.ntri[cs];
            mc_step(p, ny, nz);
        }
    }
    int pv = 0, pf = nf, tot_v, tot_f;
    mc_block_scan(pv, pf, tot_v, tot_f);
    if (n0 >= N) return;
    int64_t fo = tf[blockIdx.x] + pf;
    McPoint p = mc_ijk(n0, ny, nz);
    for (int q = 0; q < MC_PER && n0 + q < N; ++q) {
        const int64_t n = n0 + q;
        const int w = words[n];
        const int bits = w & 7;
        if (bits) {
            int64_t vo = tv[blockIdx.x] + (w >> 3);
            const float a = vol[n];
            const float base[3] = {ax[p.i], ay[p.j], az[p.k]};
            for (int d = 0; d < 3; ++d) {
                if (!((bits >> d) & 1)) continue;
                const float b = vol[n + (d == 0 ? sx : (d == 1 ? sy : 1))];
                const float t = (level - a) / (b - a);
                const float* A = d == 0 ? ax : (d == 1 ? ay : az);
                const int id = d == 0 ? p.i : (d == 1 ? p.j : p.k);
                float o[3] = {base[0], base[1], base[2]};
                o[d] = A[id] + t * (A[id + 1] - A[id]);
                if (vo < vcap) { verts[3 * vo] = o[0]; verts[3 * vo + 1] = o[1]; verts[3 * vo + 2] = o[2]; }
                ++vo;
            }
        }
        if (p.i + 1 < nx && p.j + 1 < ny && p.k + 1 < nz) {
            int cs = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int64_t o = (c & 1) * sx + ((c >> 1) & 1) * sy + ((c >> 2) & 1);
                if (mc_in(vol[n + o], level)) cs |= 1 << c;
            }
            const int nt = g_mc_table.ntri[cs];
            for (int t = 0; t < nt; ++t) {
                int32_t v[3];
                for (int r = 0; r < 3; ++r) {
                    const int e = g_mc_table.tri[cs][3 * t + r];
                    const int d = e >> 2, qq = e & 3;
                    // the edge's base corner: bit q0 on the first other axis, bit q1 on the second (dsnerf.h numbering)
                    const int c0 = ((qq & 1) << (d == 0 ? 1 : 0)) | ((qq >> 1) << (d == 2 ? 1 : 2));
                    const int64_t m = n + (c0 & 1) * sx + ((c0 >> 1) & 1) * sy + ((c0 >> 2) & 1);
                    v[r] = (int32_t)mc_vertex(words, tv, m, d);
                }
                if (fo < fcap) {
                    faces[3 * fo] = ascent ? v[2] : v[0];
                    faces[3 * fo + 1] = v[1];
                    faces[3 * fo + 2] = ascent ? v[0] : v[2];
                }
                ++fo;
            }
        }
        mc_step(p, ny, nz);
    }
}

// vertex normals (dsn_mc_normals, the rule of include/dsnerf.h): one thread per grid point, from the words of the count pass.  The
// gradient of the volume at a grid point is a difference quotient over the grid's own coordinates (central inside, one-sided on the
// grid's outer faces); a vertex takes the gradients of its edge's two points, mixed with the t of its position.
__device__ __forceinline__ float mc_grad1(const float* __restrict__ vol, int64_t n, int64_t s, const float* __restrict__ A, int i, int nd) {
    const int lo = i > 0 ? i - 1 : 0, hi = i + 1 < nd ? i + 1 : nd - 1;      // (nd >= 2: lo < hi)
    return (vol[n + (int64_t)(hi - i) * s] - vol[n - (int64_t)(i - lo) * s]) / (A[hi] - A[lo]);
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_normals(const float* __restrict__ vol, int nx, int ny, int nz, const float* __restrict__ ax,
                                                           const float* __restrict__ ay, const float* __restrict__ az, float level, float sign,
                                                           const int32_t* __restrict__ words, const int64_t* __restrict__ tv,
                                                           float* __restrict__ normals, int64_t vcap) {
    const int64_t N = (int64_t)nx * ny * nz;
    const int64_t n = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (n >= N) return;
    const int w = words[n];
    const int bits = w & 7;
    if (!bits) return;
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const McPoint p = mc_ijk(n, ny, nz);
    const float a = vol[n];
    const float ga[3] = {mc_grad1(vol, n, sx, ax, p.i, nx), mc_grad1(vol, n, sy, ay, p.j, ny), mc_grad1(vol, n, 1, az, p.k, nz)};
    int64_t vo = tv[n / MC_TILE] + (w >> 3);
    for (int d = 0; d < 3; ++d) {
        if (!((bits >> d) & 1)) continue;          // (a set bit: the neighbour along d exists)
        const int64_t m = n + (d == 0 ? sx : (d == 1 ? sy : 1));
        const float gb[3] = {mc_grad1(vol, m, sx, ax, p.i + (d == 0), nx), mc_grad1(vol, m, sy, ay, p.j + (d == 1), ny),
                             mc_grad1(vol, m, 1, az, p.k + (d == 2), nz)};
        const float t = (level - a) / (vol[m] - a);
        const float g0 = ga[0] + t * (gb[0] - ga[0]), g1 = ga[1] + t * (gb[1] - ga[1]), g2 = ga[2] + t * (gb[2] - ga[2]);
        const float nn = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
        const bool ok = nn > 0.0f && nn < __builtin_inff();      // (NaN fails both; a finite norm: finite components)
        if (vo < vcap) {
            normals[3 * vo] = ok ? (sign * g0) / nn : 0.0f;
            normals[3 * vo + 1] = ok ? (sign * g1) / nn : 0.0f;
            normals[3 * vo + 2] = ok ? (sign * g2) / nn : 0.0f;
        }
        ++vo;
    }
}

void dsn_launch_mc_count(const float* vol, int nx, int ny, int nz, float level, void* workspace, int64_t* out_counts, hipStream_t st) {
    const int64_t N = (int64_t)nx * ny * nz, tiles = mc_tiles(N);
    McWs w = mc_ws(workspace, N);
    hipLaunchKernelGGL(k_mc_count, dim3((unsigned)tiles), dim3(MC_THREADS), 0, st, vol, nx, ny, nz, level, w.words, w.tv, w.tf);
    hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.tv, w.tf, tiles, out_counts);
}

void dsn_launch_mc_emit(const float* vol, int nx, int ny, int nz, const float* x, const float* y, const float* z, float level, int ascent,
                        const void* workspace, float* verts, int64_t vcap, int32_t* faces, int64_t fcap, hipStream_t st) {
    const int64_t N = (int64_t)nx * ny * nz, tiles = mc_tiles(N);
    McWs w = mc_ws((void*)workspace, N);
    hipLaunchKernelGGL(k_mc_emit, dim3((unsigned)tiles), dim3(MC_THREADS), 0, st, vol, nx, ny, nz, x, y, z, level, ascent, w.words, w.tv,
                       w.tf, verts, vcap, faces, fcap);
}

void dsn_launch_mc_normals(const float* vol, int nx, int ny, int nz, const float* x, const float* y, const float* z, float level, int ascent,
                           const void* workspace, float* normals, int64_t vcap, hipStream_t st) {
    const int64_t N = (int64_t)nx * ny * nz;
    McWs w = mc_ws((void*)workspace, N);
    hipLaunchKernelGGL(k_mc_normals, dim3((unsigned)((N + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, st, vol, nx, ny, nz, x, y, z,
                       level, ascent ? 1.0f : -1.0f, w.words, w.tv, normals, vcap);
}

// ---------------------------------------------------------------------------------------------
// density grid, coarse to fine (dsn_grid_hier_mark / _list / _assemble + the points of dsn_density_points; the rule of include/dsnerf.h)
//   mark    : core (one thread per coarse cell: its eight corners) -> active (box maximum of radius r over the core mask) -> count (tiles
//             of MC_TILE consecutive fine points: how many lie in the closed box of an active cell; one workgroup scans the tiles'
//             totals).  The cell counters are integer adds, one per wave.
//   list    : the same tiles again: the points' prefixes inside the tile are one workgroup scan, the tile's offset comes from the mark
//             stage - ascending fine indices without atomics.
//   assemble: fill (every fine point: the coarse value at the lowest corner of its owner cell) -> scatter (the listed values) -> leaks
//             (one thread per listed point: a sign-changing edge has an evaluated end - two filled neighbours never differ in side - so
//             edge (n, d) is looked at from n where n is listed and from its other end where it is not; an integer add per wave).
// A fine point is evaluated when one of the (up to eight) coarse cells whose closed box holds it is active; neither stage stores that
// per point - it is a few reads of the active mask, which stays in cache.
// ---------------------------------------------------------------------------------------------
struct HierGeom { int n[3]; int m[3]; int sh; };      // fine points and coarse points per axis, log2 of the factor

static int hier_coarse_n(int n, int sh) { return ((n - 1 + (1 << sh) - 1) >> sh) + 1; }
static HierGeom hier_geom(int nx, int ny, int nz, int sh) {
    HierGeom g;
    g.n[0] = nx; g.n[1] = ny; g.n[2] = nz; g.sh = sh;
    for (int a = 0; a < 3; ++a) g.m[a] = hier_coarse_n(g.n[a], sh);
    return g;
}
static int64_t hier_cells(const HierGeom& g) { return (int64_t)(g.m[0] - 1) * (g.m[1] - 1) * (g.m[2] - 1); }
static size_t hier_up(size_t b) { return (b + 255) / 256 * 256; }
// core mask uint8 [cells] | active mask uint8 [cells] | tile offsets of the evaluated points int64 [tiles + 1]
struct HierWs { uint8_t* core; uint8_t* active; int64_t* tp; size_t bytes; };
static HierWs hier_ws(void* w, const HierGeom& g) {
    char* p = (char*)w;
    const size_t cells = (size_t)hier_cells(g);
    const int64_t N = (int64_t)g.n[0] * g.n[1] * g.n[2];
    HierWs r;
    r.core = (uint8_t*)p;                 p += hier_up(cells);
    r.active = (uint8_t*)p;               p += hier_up(cells);
    r.tp = (int64_t*)p;                   p += hier_up(8 * (size_t)(mc_tiles(N) + 1));
    r.bytes = (size_t)(p - (char*)w);
    return r;
}
size_t dsn_grid_hier_workspace_size(int nx, int ny, int nz, int sh) { return hier_ws(nullptr, hier_geom(nx, ny, nz, sh)).bytes; }
void dsn_grid_hier_coarse_shape(int nx, int ny, int nz, int sh, int* m3) {
    const HierGeom g = hier_geom(nx, ny, nz, sh);
    m3[0] = g.m[0]; m3[1] = g.m[1]; m3[2] = g.m[2];
}

// the coarse cells along one axis whose closed index box holds fine index i: [lo, hi] (two where i is an inner coarse point)
__device__ __forceinline__ void hier_span(int i, int sh, int cells, int& lo, int& hi) {
    const int q = i >> sh;
    hi = q < cells ? q : cells - 1;
    lo = (q < cells && q > 0 && (i & ((1 << sh) - 1)) == 0) ? q - 1 : hi;
}
__device__ __forceinline__ bool hier_evaluated(const uint8_t* __restrict__ active, const HierGeom& g, int i, int j, int k) {
    int l0, h0, l1, h1, l2, h2;
    const int c1 = g.m[1] - 1, c2 = g.m[2] - 1;
    hier_span(i, g.sh, g.m[0] - 1, l0, h0);
    hier_span(j, g.sh, c1, l1, h1);
    hier_span(k, g.sh, c2, l2, h2);
    for (int a = l0; a <= h0; ++a)
        for (int b = l1; b <= h1; ++b)
            for (int c = l2; c <= h2; ++c)
                if (active[((int64_t)a * c1 + b) * c2 + c]) return true;
    return false;
}
// the fill of a fine point: the coarse value at the lowest corner of its owner cell
__device__ __forceinline__ float hier_fill(const float* __restrict__ coarse, const HierGeom& g, int i, int j, int k) {
    const int a = min(i >> g.sh, g.m[0] - 2), b = min(j >> g.sh, g.m[1] - 2), c = min(k >> g.sh, g.m[2] - 2);
    return coarse[((int64_t)a * g.m[1] + b) * g.m[2] + c];
}

__global__ void __launch_bounds__(MC_THREADS) k_hier_core(const float* __restrict__ coarse, HierGeom g, float level, int64_t cells,
                                                          uint8_t* __restrict__ core, unsigned long long* __restrict__ counts) {
    const int64_t cell = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    bool is = false;
    if (cell < cells) {
        const int c1 = g.m[1] - 1, c2 = g.m[2] - 1;
        const int64_t ab = cell / c2;
        const int a = (int)(ab / c1), b = (int)(ab % c1), c = (int)(cell % c2);
        const int64_t sx = (int64_t)g.m[1] * g.m[2], sy = g.m[2], base = ((int64_t)a * g.m[1] + b) * g.m[2] + c;
        int in = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) in += mc_in(coarse[base + (q & 1) * sx + ((q >> 1) & 1) * sy + ((q >> 2) & 1)], level) ? 1 : 0;
        is = in != 0 && in != 8;
        core[cell] = is ? 1 : 0;
    }
    const unsigned long long m = __ballot(is);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counts, (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(MC_THREADS) k_hier_dilate(const uint8_t* __restrict__ core, HierGeom g, int r, int64_t cells,
                                                            uint8_t* __restrict__ active, unsigned long long* __restrict__ counts) {
    const int64_t cell = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    bool is = false;
    if (cell < cells) {
        const int c0 = g.m[0] - 1, c1 = g.m[1] - 1, c2 = g.m[2] - 1;
        const int64_t ab = cell / c2;
        const int a = (int)(ab / c1), b = (int)(ab % c1), c = (int)(cell % c2);
        const int a0 = max(a - r, 0), a1 = min(a + r, c0 - 1), b0 = max(b - r, 0), b1 = min(b + r, c1 - 1);
        const int z0 = max(c - r, 0), z1 = min(c + r, c2 - 1);
        for (int u = a0; u <= a1 && !is; ++u)
            for (int v = b0; v <= b1 && !is; ++v)
                for (int w = z0; w <= z1; ++w)
                    if (core[((int64_t)u * c1 + v) * c2 + w]) { is = true; break; }
        active[cell] = is ? 1 : 0;
    }
    const unsigned long long m = __ballot(is);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counts + 1, (unsigned long long)__popcll(m));
}

// evaluated flags of the thread's MC_PER consecutive fine points from n0 on (bit q: point n0 + q)
__device__ __forceinline__ uint32_t hier_flags(const uint8_t* __restrict__ active, const HierGeom& g, int64_t n0, int64_t N) {
    uint32_t f = 0;
    if (n0 < N) {
        McPoint p = mc_ijk(n0, g.n[1], g.n[2]);
        for (int q = 0; q < MC_PER && n0 + q < N; ++q) {
            if (hier_evaluated(active, g, p.i, p.j, p.k)) f |= 1u << q;
            mc_step(p, g.n[1], g.n[2]);
        }
    }
    return f;
}

__global__ void __launch_bounds__(MC_THREADS) k_hier_count(const uint8_t* __restrict__ active, HierGeom g, int64_t N,
                                                           int64_t* __restrict__ tp) {
    const int64_t n0 = (int64_t)blockIdx.x * MC_TILE + (int64_t)threadIdx.x * MC_PER;
    int a = __popc(hier_flags(active, g, n0, N)), b = 0, tot_a, tot_b;
    mc_block_scan(a, b, tot_a, tot_b);
    if (threadIdx.x == 0) tp[blockIdx.x] = tot_a;
}

// one workgroup: exclusive scan of the tiles' totals in place, [tiles] = the grand total, also written to *out
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_hier_scan(int64_t* __restrict__ tp, int64_t tiles, unsigned long long* __restrict__ out) {
    __shared__ int64_t sa[MC_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (tiles + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int64_t b0 = t * per, b1 = b0 + per < tiles ? b0 + per : tiles;
    int64_t a = 0;
    for (int64_t k = b0; k < b1; ++k) a += tp[k];
    sa[t] = a;
    __syncthreads();
    for (int off = 1; off < MC_SCAN_THREADS; off <<= 1) {
        const int64_t xa = t >= off ? sa[t - off] : 0;
        __syncthreads();
        sa[t] += xa;
        __syncthreads();
    }
    int64_t ra = sa[t] - a;
    for (int64_t k = b0; k < b1; ++k) {
        const int64_t va = tp[k];
        tp[k] = ra;
        ra += va;
    }
    if (t == MC_SCAN_THREADS - 1) { tp[tiles] = sa[t]; *out = (unsigned long long)sa[t]; }
}

__global__ void __launch_bounds__(MC_THREADS) k_hier_list(const uint8_t* __restrict__ active, HierGeom g, int64_t N,
                                                          const int64_t* __restrict__ tp, int32_t* __restrict__ index, int64_t cap) {
    const int64_t n0 = (int64_t)blockIdx.x * MC_TILE + (int64_t)threadIdx.x * MC_PER;
    const uint32_t f = hier_flags(active, g, n0, N);
    int a = __popc(f), b = 0, tot_a, tot_b;
    mc_block_scan(a, b, tot_a, tot_b);
    int64_t o = tp[blockIdx.x] + a;
    for (int q = 0; q < MC_PER; ++q)
        if ((f >> q) & 1) {
            if (o < cap) index[o] = (int32_t)(n0 + q);
            ++o;
        }
}

__global__ void __launch_bounds__(MC_THREADS) k_hier_fill(const float* __restrict__ coarse, HierGeom g, int64_t N, float* __restrict__ vol) {
    const int64_t n0 = ((int64_t)blockIdx.x * MC_THREADS + threadIdx.x) * 4;      // four consecutive points a thread
    if (n0 >= N) return;
    McPoint p = mc_ijk(n0, g.n[1], g.n[2]);
    for (int q = 0; q < 4 && n0 + q < N; ++q) {
        vol[n0 + q] = hier_fill(coarse, g, p.i, p.j, p.k);
        mc_step(p, g.n[1], g.n[2]);
    }
}

__global__ void __launch_bounds__(MC_THREADS) k_hier_scatter(const int32_t* __restrict__ index, const float* __restrict__ values, int64_t M,
                                                             int64_t N, float* __restrict__ vol) {
    const int64_t m = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (m >= M) return;
    const int64_t n = index[m];
    if (n >= 0 && n < N) vol[n] = values[m];
}

// is one of the points of the normal stencil of (i, j, k) - the point and its in-grid +-1 neighbours along the three axes - filled?
__device__ __forceinline__ bool hier_stencil_filled(const uint8_t* __restrict__ active, const HierGeom& g, int i, int j, int k) {
    if (!hier_evaluated(active, g, i, j, k)) return true;
    if (i > 0 && !hier_evaluated(active, g, i - 1, j, k)) return true;
    if (i + 1 < g.n[0] && !hier_evaluated(active, g, i + 1, j, k)) return true;
    if (j > 0 && !hier_evaluated(active, g, i, j - 1, k)) return true;
    if (j + 1 < g.n[1] && !hier_evaluated(active, g, i, j + 1, k)) return true;
    if (k > 0 && !hier_evaluated(active, g, i, j, k - 1)) return true;
    if (k + 1 < g.n[2] && !hier_evaluated(active, g, i, j, k + 1)) return true;
    return false;
}

__global__ void __launch_bounds__(MC_THREADS) k_hier_leaks(const float* __restrict__ vol, const uint8_t* __restrict__ active, HierGeom g,
                                                           int64_t N, float level, const int32_t* __restrict__ index, int64_t M,
                                                           unsigned long long* __restrict__ leaks) {
    const int64_t m = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    int found = 0;
    const int64_t n = m < M ? (int64_t)index[m] : -1;
    if (n >= 0 && n < N) {
        const McPoint p = mc_ijk(n, g.n[1], g.n[2]);
        const int at[3] = {p.i, p.j, p.k};
        const int64_t stride[3] = {(int64_t)g.n[1] * g.n[2], g.n[2], 1};
        const bool in0 = mc_in(vol[n], level);
        int own = -1;      // (the point's own stencil: looked at only once a crossing edge needs it)
        for (int d = 0; d < 3; ++d)
            for (int s = -1; s <= 1; s += 2) {
                const int o = at[d] + s;
                if (o < 0 || o >= g.n[d]) continue;
                int q[3] = {p.i, p.j, p.k};
                q[d] = o;
                // the edge to the neighbour below belongs to that neighbour where it is listed itself
                if (s < 0 && hier_evaluated(active, g, q[0], q[1], q[2])) continue;
                if (mc_in(vol[n + s * stride[d]], level) == in0) continue;
                if (own < 0) own = hier_stencil_filled(active, g, p.i, p.j, p.k) ? 1 : 0;
                if (own || hier_stencil_filled(active, g, q[0], q[1], q[2])) ++found;
            }
    }
    // (up to six edges a thread: the wave's sum by one ballot per possible count bit)
    unsigned long long total = 0;
    for (int bit = 0; bit < 3; ++bit) total += (unsigned long long)__popcll(__ballot((found >> bit) & 1)) << bit;
    if ((threadIdx.x & 63) == 0 && total) atomicAdd(leaks, total);
}

// grid points of a list: point m = the grid point with the linear index index[m] (an index outside the grid: point 0, and
// k_points_invalid puts NaN where its value would go)
__global__ void __launch_bounds__(256) k_list_points(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                     const int32_t* __restrict__ index, int ny, int nz, int64_t N, int64_t n,
                                                     float* __restrict__ pts) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= n) return;
    int64_t l = index[m];
    if (l < 0 || l >= N) l = 0;
    const int64_t plane = (int64_t)ny * nz;
    const int64_t r = l % plane;
    pts[3 * m + 0] = x[(int)(l / plane)];
    pts[3 * m + 1] = y[(int)(r / nz)];
    pts[3 * m + 2] = z[(int)(r % nz)];
}

__global__ void __launch_bounds__(256) k_points_invalid(const int32_t* __restrict__ index, int64_t N, int64_t n, float* __restrict__ values) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= n) return;
    const int64_t l = index[m];
    if (l < 0 || l >= N) values[m] = __builtin_nanf("");
}

void dsn_launch_list_points(const float* x, const float* y, const float* z, const int32_t* index, int ny, int nz, int64_t N, int64_t n,
                            float* pts, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_list_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, z, index, ny, nz, N, n, pts);
}

void dsn_launch_points_invalid(const int32_t* index, int64_t N, int64_t n, float* values, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_points_invalid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, index, N, n, values);
}

static unsigned hier_blocks(int64_t n) { return (unsigned)((n + MC_THREADS - 1) / MC_THREADS); }

// out_counts (3 int64) must be zero on entry (the API zeroes it on the stream)
void dsn_launch_grid_hier_mark(const float* coarse, int nx, int ny, int nz, int sh, int dilate, float level, void* workspace,
                               int64_t* out_counts, hipStream_t st) {
    const HierGeom g = hier_geom(nx, ny, nz, sh);
    const HierWs w = hier_ws(workspace, g);
    const int64_t cells = hier_cells(g), N = (int64_t)nx * ny * nz, tiles = mc_tiles(N);
    unsigned long long* cnt = (unsigned long long*)out_counts;
    const int longest = g.m[0] > g.m[1] ? (g.m[0] > g.m[2] ? g.m[0] : g.m[2]) : (g.m[1] > g.m[2] ? g.m[1] : g.m[2]);
    const int r = dilate < longest ? dilate : longest;            // (a radius beyond the lattice's longest axis changes nothing)
    hipLaunchKernelGGL(k_hier_core, dim3(hier_blocks(cells)), dim3(MC_THREADS), 0, st, coarse, g, level, cells, w.core, cnt);
    hipLaunchKernelGGL(k_hier_dilate, dim3(hier_blocks(cells)), dim3(MC_THREADS), 0, st, w.core, g, r, cells, w.active, cnt);
    hipLaunchKernelGGL(k_hier_count, dim3((unsigned)tiles), dim3(MC_THREADS), 0, st, w.active, g, N, w.tp);
    hipLaunchKernelGGL(k_hier_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.tp, tiles, cnt + 2);
}

void dsn_launch_grid_hier_list(int nx, int ny, int nz, int sh, const void* workspace, int32_t* index, int64_t cap, hipStream_t st) {
    const HierGeom g = hier_geom(nx, ny, nz, sh);
    const HierWs w = hier_ws((void*)workspace, g);
    const int64_t N = (int64_t)nx * ny * nz;
    hipLaunchKernelGGL(k_hier_list, dim3((unsigned)mc_tiles(N)), dim3(MC_THREADS), 0, st, w.active, g, N, w.tp, index, cap);
}

// out_leaks (int64) must be zero on entry (the API zeroes it on the stream)
void dsn_launch_grid_hier_assemble(const float* coarse, int nx, int ny, int nz, int sh, float level, const void* workspace,
                                   const int32_t* index, const float* values, int64_t M, float* volume, int64_t* out_leaks, hipStream_t st) {
    const HierGeom g = hier_geom(nx, ny, nz, sh);
    const HierWs w = hier_ws((void*)workspace, g);
    const int64_t N = (int64_t)nx * ny * nz;
    hipLaunchKernelGGL(k_hier_fill, dim3(hier_blocks((N + 3) / 4)), dim3(MC_THREADS), 0, st, coarse, g, N, volume);
    if (M > 0) {
        hipLaunchKernelGGL(k_hier_scatter, dim3(hier_blocks(M)), dim3(MC_THREADS), 0, st, index, values, M, N, volume);
        hipLaunchKernelGGL(k_hier_leaks, dim3(hier_blocks(M)), dim3(MC_THREADS), 0, st, volume, w.active, g, N, level, index, M,
                           (unsigned long long*)out_leaks);
    }
}

// ---------------------------------------------------------------------------------------------
// connected components of an indexed mesh and its largest piece (dsn_mesh_cc_label / dsn_mesh_cc_emit, the rule of include/dsnerf.h)
//   label : init -> unite (lock-free union-find over the vertex array, one thread per face) -> flatten (every vertex to its root, unused
//           vertices -1) -> sums (per face 64-bit integer adds to its root's slots, aggregated per wave) -> select (the arg-max over the
//           roots, per tile and then over the tiles: no atomics, the same winner every call) -> count + scan (kept vertices and faces per
//           tile of CC_TILE, k_mc_scan over the tiles' totals);
//   emit  : vertices (the workgroup scan again: new index, source_vertex, the vertex map), then faces renumbered through the map.
// ---------------------------------------------------------------------------------------------
#define CC_PER 4                               // consecutive vertices / faces per thread
#define CC_TILE (MC_THREADS * CC_PER)
static_assert(CC_TILE == DSN_MESH_CC_TILE, "compaction tile");

static int64_t cc_tiles(int64_t n) { return (n + CC_TILE - 1) / CC_TILE; }
static size_t cc_up(size_t b) { return (b + 15) / 16 * 16; }
// header 64 B (int32 word 0: the winner) | label int32 [V] | vmap int32 [V] | sum uint64 [V] | cnt uint64 [V] | used uint8 [V] |
// tile vertex offsets int64 [tiles + 1] | tile face offsets int64 [tiles + 1] | tile best sum uint64 [tilesV] | tile best label
// int32 [tilesV] | tile component count int32 [tilesV]            (tiles = max(tilesV, tilesT); every part 16-byte aligned)
struct CcWs {
    int32_t* head; int32_t* label; int32_t* vmap; unsigned long long* sum; unsigned long long* cnt; uint8_t* used;
    int64_t* tv; int64_t* tf; unsigned long long* bsum; int32_t* blab; int32_t* bcomp; size_t bytes;
};
static CcWs cc_ws(void* w, int64_t V, int64_t T) {
    const int64_t tilesV = cc_tiles(V), tilesT = cc_tiles(T), tiles = tilesV > tilesT ? tilesV : tilesT;
    char* p = (char*)w;
    size_t o = 0;
    CcWs r;
    r.head = (int32_t*)(p + o); o += 64;
    r.label = (int32_t*)(p + o); o += cc_up((size_t)4 * V);
    r.vmap = (int32_t*)(p + o); o += cc_up((size_t)4 * V);
    r.sum = (unsigned long long*)(p + o); o += cc_up((size_t)8 * V);
    r.cnt = (unsigned long long*)(p + o); o += cc_up((size_t)8 * V);
    r.used = (uint8_t*)(p + o); o += cc_up((size_t)V);
    r.tv = (int64_t*)(p + o); o += cc_up((size_t)8 * (tiles + 1));
    r.tf = (int64_t*)(p + o); o += cc_up((size_t)8 * (tiles + 1));
    r.bsum = (unsigned long long*)(p + o); o += cc_up((size_t)8 * tilesV);
    r.blab = (int32_t*)(p + o); o += cc_up((size_t)4 * tilesV);
    r.bcomp = (int32_t*)(p + o); o += cc_up((size_t)4 * tilesV);
    r.bytes = o;
    return r;
}
size_t dsn_mesh_cc_workspace_size(int64_t V, int64_t T) { return cc_ws(nullptr, V, T).bytes; }

__global__ void __launch_bounds__(MC_THREADS) k_cc_init(int32_t* __restrict__ parent, unsigned long long* __restrict__ sum,
                                                        unsigned long long* __restrict__ cnt, uint8_t* __restrict__ used, int V) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= V) return;
    parent[v] = (int32_t)v; sum[v] = 0; cnt[v] = 0; used[v] = 0;
}

// The union-find of k_cc_unite.  Invariant: parent[x] <= x, always - a root is only ever hooked under a smaller root (compare-and-swap)
// and a shortcut only ever lowers an entry to one of its ancestors (atomic minimum).  Every access is a relaxed agent-scope atomic: the
// eight L2s are not coherent for plain loads of lines another compute unit's atomics rewrote.  Whatever value a load returns - a stale
// one included - is an ancestor <= x, so cc_find walks strictly downward and ends; no thread ever waits for another's write.
// The walks compare unsigned and follow an entry only while it is below its index: whatever bytes the array holds (the measurement
// entries can run a phase on a workspace the phases before it never wrote), no index leaves [0, x].
__device__ __forceinline__ int32_t cc_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t cc_find(int32_t* __restrict__ parent, int32_t x) {
    int32_t p = cc_load(parent + x);
    while ((uint32_t)p < (uint32_t)x) {            // (a root: p == x)
        const int32_t g = cc_load(parent + p);     // g <= p
        if ((uint32_t)g < (uint32_t)p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // path halving
        x = p; p = g;
    }
    return x;
}
__device__ __forceinline__ void cc_unite(int32_t* __restrict__ parent, int32_t a, int32_t b) {
    for (;;) {
        a = cc_find(parent, a); b = cc_find(parent, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        int32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        if ((uint32_t)seen >= (uint32_t)hi) return;
        a = seen; b = lo;                          // hi was hooked meanwhile: go on from what the atomic returned (an ancestor of hi)
    }
}
__device__ __forceinline__ bool cc_face(const int32_t* __restrict__ faces, int64_t t, int V, int32_t& i0, int32_t& i1, int32_t& i2) {
    i0 = faces[3 * t]; i1 = faces[3 * t + 1]; i2 = faces[3 * t + 2];
    return (uint32_t)i0 < (uint32_t)V && (uint32_t)i1 < (uint32_t)V && (uint32_t)i2 < (uint32_t)V;
}

__global__ void __launch_bounds__(MC_THREADS) k_cc_unite(const int32_t* __restrict__ faces, int V, int64_t T, int32_t* __restrict__ parent,
                                                         uint8_t* __restrict__ used) {
    const int64_t t = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (t >= T) return;
    int32_t i0, i1, i2;
    if (!cc_face(faces, t, V, i0, i1, i2)) return;
    used[i0] = 1; used[i1] = 1; used[i2] = 1;      // (every writer stores the same byte; read by the next launch)
    cc_unite(parent, i0, i1);
    cc_unite(parent, i0, i2);
}

// every vertex to its root, in place (a walk meets entries of before this launch or roots already written: ancestors either way);
// a vertex no valid face uses: -1 (a singleton, no other walk passes through it)
__global__ void __launch_bounds__(MC_THREADS) k_cc_flatten(int32_t* __restrict__ parent, const uint8_t* __restrict__ used, int V,
                                                           int32_t* __restrict__ labels_out) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= V) return;
    int32_t r = -1;
    if (used[v]) {
        r = (int32_t)v;
        for (int32_t p = parent[r]; (uint32_t)p < (uint32_t)r; p = parent[r]) r = p;
    }
    parent[v] = r;
    if (labels_out) labels_out[v] = r;
}

// doubled area of a face in float32 (dsnerf.h), as the integer floor(d 2^k): scale = 2^k
__device__ __forceinline__ unsigned long long cc_area_q(const float* __restrict__ verts, int32_t i0, int32_t i1, int32_t i2, double scale) {
    const float* a = verts + 3 * (int64_t)i0; const float* b = verts + 3 * (int64_t)i1; const float* c = verts + 3 * (int64_t)i2;
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    float d = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (!(d < __builtin_inff())) d = 0.0f;         // (NaN and infinity)
    const double x = floor((double)d * scale);     // exact: a power of two times a float
    return x < 9223372036854775808.0 ? (unsigned long long)x : 9223372036854775808ull;      // (2^63: only a shift the host rule never gives)
}

__global__ void __launch_bounds__(MC_THREADS) k_cc_sums(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int64_t T,
                                                        const int32_t* __restrict__ label, double scale,
                                                        unsigned long long* __restrict__ sum, unsigned long long* __restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t i0 = 0, i1 = 0, i2 = 0, root = -1;
    unsigned long long q = 0;
    bool todo = t < T && cc_face(faces, t, V, i0, i1, i2);
    if (todo) { root = label[i0]; q = cc_area_q(verts, i0, i1, i2, scale); }
    todo = todo && (uint32_t)root < (uint32_t)V;   // (always, after k_cc_flatten)
    // per wave: the lanes that share the first pending lane's root add up among themselves, one lane issues the two atomics
    for (;;) {
        const unsigned long long pending = __ballot(todo);
        if (!pending) break;
        const int leader = __ffsll((long long)pending) - 1;
        const int32_t r0 = __shfl(root, leader);
        const bool mine = todo && root == r0;
        unsigned long long qs = mine ? q : 0ull;
        int n = mine ? 1 : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { qs += __shfl_xor(qs, off); n += __shfl_xor(n, off); }
        if (lane == leader) { atomicAdd(sum + r0, qs); atomicAdd(cnt + r0, (unsigned long long)n); }
        todo = todo && !mine;
    }
}

// (sum, label) a beats b: the larger sum, on equal sums the smaller label; label -1 = none
__device__ __forceinline__ bool cc_better(unsigned long long sa, int32_t la, unsigned long long sb, int32_t lb) {
    if (la < 0) return false;
    if (lb < 0) return true;
    return sa > sb || (sa == sb && la < lb);
}
template <int THREADS>
__device__ __forceinline__ void cc_block_best(unsigned long long& s, int32_t& l, int& n) {
    __shared__ unsigned long long ss[THREADS];
    __shared__ int32_t sl[THREADS];
    __shared__ int sn[THREADS];
    const int t = threadIdx.x;
    ss[t] = s; sl[t] = l; sn[t] = n;
    __syncthreads();
    for (int off = THREADS / 2; off >= 1; off >>= 1) {
        if (t < off) {
            if (cc_better(ss[t + off], sl[t + off], ss[t], sl[t])) { ss[t] = ss[t + off]; sl[t] = sl[t + off]; }
            sn[t] += sn[t + off];
        }
        __syncthreads();
    }
    s = ss[0]; l = sl[0]; n = sn[0];
}

__global__ void __launch_bounds__(MC_THREADS) k_cc_select_tiles(const int32_t* __restrict__ label, const unsigned long long* __restrict__ sum,
                                                                const unsigned long long* __restrict__ cnt, int V,
                                                                unsigned long long* __restrict__ bsum, int32_t* __restrict__ blab,
                                                                int32_t* __restrict__ bcomp) {
    const int64_t v0 = (int64_t)blockIdx.x * CC_TILE + (int64_t)threadIdx.x * CC_PER;
    unsigned long long s = 0; int32_t l = -1; int n = 0;
    for (int q = 0; q < CC_PER && v0 + q < V; ++q) {
        const int32_t v = (int32_t)(v0 + q);
        if (label[v] != v || cnt[v] == 0) continue;      // (a root with at least one face)
        ++n;
        if (cc_better(sum[v], v, s, l)) { s = sum[v]; l = v; }
    }
    cc_block_best<MC_THREADS>(s, l, n);
    if (threadIdx.x == 0) { bsum[blockIdx.x] = s; blab[blockIdx.x] = l; bcomp[blockIdx.x] = n; }
}

// one workgroup over the tiles: out[0] components, out[1] winner, out[4] its sum, out[5] its faces; head[0] = winner
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_cc_select_final(const unsigned long long* __restrict__ bsum, const int32_t* __restrict__ blab,
                                                                     const int32_t* __restrict__ bcomp, int64_t tilesV,
                                                                     const unsigned long long* __restrict__ cnt, int V,
                                                                     int32_t* __restrict__ head, int64_t* __restrict__ out) {
    unsigned long long s = 0; int32_t l = -1; int n = 0;
    for (int64_t k = threadIdx.x; k < tilesV; k += MC_SCAN_THREADS) {
        n += bcomp[k];
        if (cc_better(bsum[k], blab[k], s, l)) { s = bsum[k]; l = blab[k]; }
    }
    cc_block_best<MC_SCAN_THREADS>(s, l, n);
    if (threadIdx.x == 0) {
        head[0] = l;
        out[0] = n; out[1] = l; out[4] = (int64_t)s; out[5] = (uint32_t)l < (uint32_t)V ? (int64_t)cnt[l] : 0;
    }
}

__device__ __forceinline__ bool cc_keep_face(const int32_t* __restrict__ faces, int64_t t, int V, const int32_t* __restrict__ label,
                                             int32_t winner, int32_t& i0, int32_t& i1, int32_t& i2) {
    return cc_face(faces, t, V, i0, i1, i2) && label[i0] == winner;
}

// kept vertices and faces of tile blockIdx.x (either may lie beyond the mesh: 0)
__global__ void __launch_bounds__(MC_THREADS) k_cc_count(const int32_t* __restrict__ faces, int V, int64_t T, const int32_t* __restrict__ label,
                                                         const int32_t* __restrict__ head, int64_t* __restrict__ tv, int64_t* __restrict__ tf) {
    const int32_t winner = head[0];
    const int64_t n0 = (int64_t)blockIdx.x * CC_TILE + (int64_t)threadIdx.x * CC_PER;
    int nv = 0, nf = 0;
    if (winner >= 0)
        for (int q = 0; q < CC_PER; ++q) {
            int32_t i0, i1, i2;
            if (n0 + q < V && label[n0 + q] == winner) ++nv;
            if (n0 + q < T && cc_keep_face(faces, n0 + q, V, label, winner, i0, i1, i2)) ++nf;
        }
    int tot_v, tot_f;
    mc_block_scan(nv, nf, tot_v, tot_f);
    if (threadIdx.x == 0) { tv[blockIdx.x] = tot_v; tf[blockIdx.x] = tot_f; }
}

__global__ void __launch_bounds__(MC_THREADS) k_cc_emit_verts(const float* __restrict__ verts, int V, const int32_t* __restrict__ label,
                                                              const int32_t* __restrict__ head, const int64_t* __restrict__ tv,
                                                              int32_t* __restrict__ vmap, float* __restrict__ out_verts, int64_t vcap,
                                                              int32_t* __restrict__ source) {
    const int32_t winner = head[0];
    const int64_t n0 = (int64_t)blockIdx.x * CC_TILE + (int64_t)threadIdx.x * CC_PER;
    int keep = 0, nv = 0, none = 0, tot_v, tot_n;
    if (winner >= 0)
        for (int q = 0; q < CC_PER; ++q)
            if (n0 + q < V && label[n0 + q] == winner) { keep |= 1 << q; ++nv; }
    mc_block_scan(nv, none, tot_v, tot_n);
    int64_t o = tv[blockIdx.x] + nv;
    for (int q = 0; q < CC_PER && n0 + q < V; ++q) {
        const int64_t v = n0 + q;
        if (!((keep >> q) & 1)) { vmap[v] = -1; continue; }
        vmap[v] = (int32_t)o;
        if ((uint64_t)o < (uint64_t)vcap) {
            out_verts[3 * o] = verts[3 * v]; out_verts[3 * o + 1] = verts[3 * v + 1]; out_verts[3 * o + 2] = verts[3 * v + 2];
            if (source) source[o] = (int32_t)v;
        }
        ++o;
    }
}

__global__ void __launch_bounds__(MC_THREADS) k_cc_emit_faces(const int32_t* __restrict__ faces, int V, int64_t T, const int32_t* __restrict__ label,
                                                              const int32_t* __restrict__ head, const int64_t* __restrict__ tf,
                                                              const int32_t* __restrict__ vmap, int32_t* __restrict__ out_faces, int64_t fcap) {
    const int32_t winner = head[0];
    const int64_t n0 = (int64_t)blockIdx.x * CC_TILE + (int64_t)threadIdx.x * CC_PER;
    int32_t idx[CC_PER][3];
    int keep = 0, nf = 0, none = 0, tot_f, tot_n;
    if (winner >= 0)
#pragma unroll
        for (int q = 0; q < CC_PER; ++q)
            if (n0 + q < T && cc_keep_face(faces, n0 + q, V, label, winner, idx[q][0], idx[q][1], idx[q][2])) { keep |= 1 << q; ++nf; }
    mc_block_scan(nf, none, tot_f, tot_n);
    int64_t o = tf[blockIdx.x] + nf;
#pragma unroll
    for (int q = 0; q < CC_PER; ++q) {
        if (!((keep >> q) & 1)) continue;
        if ((uint64_t)o < (uint64_t)fcap) { out_faces[3 * o] = vmap[idx[q][0]]; out_faces[3 * o + 1] = vmap[idx[q][1]]; out_faces[3 * o + 2] = vmap[idx[q][2]]; }
        ++o;
    }
}

void dsn_launch_mesh_cc_label(const float* verts, const int32_t* faces, int64_t V, int64_t T, double scale, void* workspace, int32_t* labels_v,
                              int64_t* out_counts, int phases, hipStream_t st) {
    CcWs w = cc_ws(workspace, V, T);
    const int64_t tilesV = cc_tiles(V), tilesT = cc_tiles(T), tiles = tilesV > tilesT ? tilesV : tilesT;
    const unsigned gV = (unsigned)((V + MC_THREADS - 1) / MC_THREADS), gT = (unsigned)((T + MC_THREADS - 1) / MC_THREADS);
    if ((phases & DSN_CC_INIT) && gV) hipLaunchKernelGGL(k_cc_init, dim3(gV), dim3(MC_THREADS), 0, st, w.label, w.sum, w.cnt, w.used, (int)V);
    if ((phases & DSN_CC_UNITE) && gT && gV) hipLaunchKernelGGL(k_cc_unite, dim3(gT), dim3(MC_THREADS), 0, st, faces, (int)V, T, w.label, w.used);
    if ((phases & DSN_CC_FLATTEN) && gV) hipLaunchKernelGGL(k_cc_flatten, dim3(gV), dim3(MC_THREADS), 0, st, w.label, w.used, (int)V, labels_v);
    if ((phases & DSN_CC_SUMS) && gT && gV)
        hipLaunchKernelGGL(k_cc_sums, dim3(gT), dim3(MC_THREADS), 0, st, verts, faces, (int)V, T, w.label, scale, w.sum, w.cnt);
    if (phases & DSN_CC_SELECT) {
        if (tilesV)
            hipLaunchKernelGGL(k_cc_select_tiles, dim3((unsigned)tilesV), dim3(MC_THREADS), 0, st, w.label, w.sum, w.cnt, (int)V, w.bsum, w.blab, w.bcomp);
        hipLaunchKernelGGL(k_cc_select_final, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.bsum, w.blab, w.bcomp, tilesV, w.cnt, (int)V, w.head,
                           out_counts);
    }
    if (phases & DSN_CC_COUNT) {
        if (tiles) hipLaunchKernelGGL(k_cc_count, dim3((unsigned)tiles), dim3(MC_THREADS), 0, st, faces, (int)V, T, w.label, w.head, w.tv, w.tf);
        hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.tv, w.tf, tiles, out_counts + 2);
    }
}

void dsn_launch_mesh_cc_emit(const float* verts, const int32_t* faces, int64_t V, int64_t T, void* workspace, float* out_verts, int64_t vcap,
                             int32_t* out_faces, int64_t fcap, int32_t* source_vertex, int phases, hipStream_t st) {
    CcWs w = cc_ws(workspace, V, T);
    const int64_t tilesV = cc_tiles(V), tilesT = cc_tiles(T);
    if ((phases & DSN_CC_EMIT_VERTS) && tilesV)
        hipLaunchKernelGGL(k_cc_emit_verts, dim3((unsigned)tilesV), dim3(MC_THREADS), 0, st, verts, (int)V, w.label, w.head, w.tv, w.vmap, out_verts,
                           vcap, source_vertex);
    if ((phases & DSN_CC_EMIT_FACES) && tilesT && tilesV && fcap > 0)
        hipLaunchKernelGGL(k_cc_emit_faces, dim3((unsigned)tilesT), dim3(MC_THREADS), 0, st, faces, (int)V, T, w.label, w.head, w.tf, w.vmap,
                           out_faces, fcap);
}

// ---------------------------------------------------------------------------------------------
// a mesh bound to the body: dsn_mesh_bind_normals / dsn_mesh_pose / dsn_mesh_stretch (the rule of include/dsnerf.h)
//   records: per pose and body face the DsnFaceRec of the target body - dsn_make_face, the values k_face_setup writes - into the workspace
//            ([P, Fb] x 64 B: a few hundred KB per pose, read back from L2); a body face with an index outside [0, Vb) gives a NaN record.
//   pose   : one thread per mesh vertex - its binding (face, u, v, h and the covector: 28 B) once, then per pose one record gather,
//            dsn_map2face and the covector's image; consecutive lanes write consecutive 12-byte rows.  No atomics on floats: every
//            output word has one writer.  A binding outside [0, Fb): NaN rows and one integer atomic OR on the status word.
//   stretch: one thread per mesh face, the bind lengths once, then per pose the three posed edges.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MC_THREADS) k_mesh_face_recs(const float* __restrict__ target, int P, int Vb, const int32_t* __restrict__ bfaces,
                                                               int Fb, DsnFaceRec* __restrict__ recs) {
    const int64_t k = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (k >= (int64_t)P * Fb) return;
    const int f = (int)(k % Fb);
    const float* verts = target + (k / Fb) * 3 * (int64_t)Vb;
    const int32_t i0 = bfaces[3 * f], i1 = bfaces[3 * f + 1], i2 = bfaces[3 * f + 2];
    float4* o = (float4*)(recs + k);
    if ((uint32_t)i0 >= (uint32_t)Vb || (uint32_t)i1 >= (uint32_t)Vb || (uint32_t)i2 >= (uint32_t)Vb) {
        const float q = __builtin_nanf("");
        o[0] = o[1] = o[2] = o[3] = make_float4(q, q, q, q);
        return;
    }
    float v0[3], v1[3], v2[3];
    for (int c = 0; c < 3; ++c) { v0[c] = verts[3 * i0 + c]; v1[c] = verts[3 * i1 + c]; v2[c] = verts[3 * i2 + c]; }
    DsnFaceRec r;
    dsn_make_face(v0, v1, v2, r);
    o[0] = make_float4(r.m0[0], r.m0[1], r.m0[2], r.d00);
    o[1] = make_float4(r.v10[0], r.v10[1], r.v10[2], r.d01);
    o[2] = make_float4(r.v20[0], r.v20[1], r.v20[2], r.d11);
    o[3] = make_float4(r.n[0], r.n[1], r.n[2], r.inv);
}

__global__ void __launch_bounds__(MC_THREADS) k_mesh_bind_normals(const float* __restrict__ body, int Vb, const int32_t* __restrict__ bfaces, int Fb,
                                                                  const int32_t* __restrict__ face_idx, const float* __restrict__ normals,
                                                                  int64_t N, float* __restrict__ cov) {
    const int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= N) return;
    const int32_t f = face_idx[i];
    float o[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
    if ((uint32_t)f < (uint32_t)Fb) {
        const int32_t i0 = bfaces[3 * f], i1 = bfaces[3 * f + 1], i2 = bfaces[3 * f + 2];
        if ((uint32_t)i0 < (uint32_t)Vb && (uint32_t)i1 < (uint32_t)Vb && (uint32_t)i2 < (uint32_t)Vb) {
            float v0[3], v1[3], v2[3];
            for (int c = 0; c < 3; ++c) { v0[c] = body[3 * i0 + c]; v1[c] = body[3 * i1 + c]; v2[c] = body[3 * i2 + c]; }
            DsnFaceRec r;
            dsn_make_face(v0, v1, v2, r);
            const float n[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
            o[0] = dsn_dot3(n, r.v20); o[1] = dsn_dot3(n, r.v10); o[2] = dsn_dot3(n, r.n);
        }
    }
    cov[3 * i] = o[0]; cov[3 * i + 1] = o[1]; cov[3 * i + 2] = o[2];
}

__global__ void __launch_bounds__(MC_THREADS) k_mesh_pose(const DsnFaceRec* __restrict__ recs, int P, int Fb, const int32_t* __restrict__ face_idx,
                                                          const float* __restrict__ uv, const float* __restrict__ h, const float* __restrict__ cov,
                                                          int64_t N, float* __restrict__ out_verts, float* __restrict__ out_normals,
                                                          int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= N) return;
    const int32_t f = face_idx[i];
    const bool want_n = out_normals != nullptr;
    if ((uint32_t)f >= (uint32_t)Fb) {
        const float q = __builtin_nanf("");
        for (int p = 0; p < P; ++p) {
            const int64_t o = 3 * ((int64_t)p * N + i);
            out_verts[o] = q; out_verts[o + 1] = q; out_verts[o + 2] = q;
            if (want_n) { out_normals[o] = q; out_normals[o + 1] = q; out_normals[o + 2] = q; }
        }
        if (status) atomicOr(status, DSN_MESH_POSE_BAD_BINDING);
        return;
    }
    const float u = uv[2 * i], v = uv[2 * i + 1], hh = h[i];
    float cv[3] = {0.f, 0.f, 0.f};
    if (want_n) { cv[0] = cov[3 * i]; cv[1] = cov[3 * i + 1]; cv[2] = cov[3 * i + 2]; }
    for (int p = 0; p < P; ++p) {
        const DsnFaceRec r = dsn_load_face(recs + (int64_t)p * Fb, f);
        const int64_t o = 3 * ((int64_t)p * N + i);
        float x[3];
        dsn_map2face(u, v, hh, r, x);
        out_verts[o] = x[0]; out_verts[o + 1] = x[1]; out_verts[o + 2] = x[2];
        if (want_n) {
            float c[3], a[3], b[3], m[3], n[3];
            dsn_cross3(r.v10, r.v20, c);      // (the record's n is c / |c|)
            dsn_cross3(r.n, r.v10, a);
            dsn_cross3(r.v20, r.n, b);
            for (int k = 0; k < 3; ++k) m[k] = (cv[0] * a[k] + cv[1] * b[k]) + cv[2] * c[k];
            dsn_normalize3(m, n);
            out_normals[o] = n[0]; out_normals[o + 1] = n[1]; out_normals[o + 2] = n[2];
        }
    }
}

__global__ void __launch_bounds__(MC_THREADS) k_mesh_stretch(const float* __restrict__ bind, const float* __restrict__ posed, int P, int64_t N,
                                                             const int32_t* __restrict__ faces, int64_t T, float* __restrict__ stretch) {
    const int64_t t = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (t >= T) return;
    const int32_t idx[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
    if (idx[0] < 0 || idx[0] >= N || idx[1] < 0 || idx[1] >= N || idx[2] < 0 || idx[2] >= N) {
        for (int p = 0; p < P; ++p) stretch[(int64_t)p * T + t] = __builtin_inff();
        return;
    }
    float lb[3];      // edge k: vertex k -> vertex k + 1 (mod 3)
    for (int k = 0; k < 3; ++k) {
        const float* a = bind + 3 * (int64_t)idx[k];
        const float* b = bind + 3 * (int64_t)idx[(k + 1) % 3];
        const float e[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        lb[k] = dsn_norm3(e);
    }
    for (int p = 0; p < P; ++p) {
        const float* pv = posed + 3 * (int64_t)p * N;
        float s = 1.0f;
        bool any = false;
        for (int k = 0; k < 3; ++k) {
            if (lb[k] == 0.0f) continue;
            const float* a = pv + 3 * (int64_t)idx[k];
            const float* b = pv + 3 * (int64_t)idx[(k + 1) % 3];
            const float e[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
            const float r = dsn_div(dsn_norm3(e), lb[k]);
            s = (!any || r > s || r != r) ? r : s;      // the maximum; a NaN ratio stays
            any = true;
        }
        stretch[(int64_t)p * T + t] = s;
    }
}

static unsigned mesh_blocks(int64_t n) { return (unsigned)((n + MC_THREADS - 1) / MC_THREADS); }

void dsn_launch_mesh_bind_normals(const float* body, int Vb, const int32_t* bfaces, int Fb, const int32_t* face_idx, const float* normals,
                                  int64_t N, float* cov, hipStream_t st) {
    if (N <= 0) return;
    hipLaunchKernelGGL(k_mesh_bind_normals, dim3(mesh_blocks(N)), dim3(MC_THREADS), 0, st, body, Vb, bfaces, Fb, face_idx, normals, N, cov);
}

void dsn_launch_mesh_pose(const float* target, int P, int Vb, const int32_t* bfaces, int Fb, const int32_t* face_idx, const float* uv,
                          const float* h, const float* cov, int64_t N, float* out_verts, float* out_normals, int32_t* status, void* workspace,
                          hipStream_t st) {
    if (N <= 0) return;
    DsnFaceRec* recs = (DsnFaceRec*)workspace;
    hipLaunchKernelGGL(k_mesh_face_recs, dim3(mesh_blocks((int64_t)P * Fb)), dim3(MC_THREADS), 0, st, target, P, Vb, bfaces, Fb, recs);
    hipLaunchKernelGGL(k_mesh_pose, dim3(mesh_blocks(N)), dim3(MC_THREADS), 0, st, recs, P, Fb, face_idx, uv, h, cov, N, out_verts,
                       cov ? out_normals : nullptr, status);
}

void dsn_launch_mesh_stretch(const float* bind, const float* posed, int P, int64_t N, const int32_t* faces, int64_t T, float* stretch,
                             hipStream_t st) {
    if (T <= 0) return;
    hipLaunchKernelGGL(k_mesh_stretch, dim3(mesh_blocks(T)), dim3(MC_THREADS), 0, st, bind, posed, P, N, faces, T, stretch);
}

// ---------------------------------------------------------------------------------------------
// vertex clustering with a picked representative (dsn_mesh_simplify_*, the rule of include/dsnerf.h)
//   count: zero (the bit grid, the cluster slots, the triple table) -> mark (one thread per vertex: its cell, one bit per occupied cell)
//          -> rank (popcount prefix over the bit-grid words, the tile scan of the marching cubes: a cell's cluster is the number of occupied
//          cells below it) -> sum (64-bit integer adds of the members' fixed-point coordinates, aggregated per run of equal clusters in the
//          wave) -> pick (one 64-bit unsigned atomic minimum of (float32 distance bits, vertex index) per run) -> faces (the clusters of a
//          face; a live face claims the slot of its sorted triple in a lock-free open-addressing table by compare-and-swap and leaves the
//          minimum of its index there) -> keep (a face is kept when it is its slot's minimum; the tile scan over the keep flags);
//   emit : one thread per cluster copies its representative, the workgroup scan over the keep flags orders the faces.
// Every value read back from the workspace is range-checked before it is used as an index: the measurement entries can run a phase on a
// workspace the phases before it never wrote.
// ---------------------------------------------------------------------------------------------
#define SP_CAP ((int64_t)1 << DSN_MESH_SIMPLIFY_MAX_LOG2)
#define SP_EMPTY 0xFFFFFFFFFFFFFFFFull          // (a packed triple has bit 63 clear)
enum { SP_K = 0, SP_KEPT = 1, SP_LIVE = 2, SP_OUTSIDE = 3, SP_BAD = 4, SP_STATUS = 5 };      // the header's 64-bit words

struct SpGrid { float o[3]; float inv; int g[3]; };

static int64_t sp_cells(const int* g) { return (int64_t)g[0] * g[1] * g[2]; }
static int64_t sp_table_slots(int64_t T) {      // a power of two, load <= 1/2
    int64_t c = 64;
    while (c < 2 * T) c <<= 1;
    return c;
}
// header 64 B | cell int32 [V] | cluster int32 [V] | bit grid uint32 [W] | in-tile word prefix int32 [W] | word tile offsets int64
// [tilesW + 1] | cluster sums int64 [Kmax, 4] (s0, s1, s2, n) | cluster keys uint64 [Kmax] | table keys uint64 [slots] | table minima
// int32 [slots] | keep uint8 [T] | face tile offsets int64 [tilesT + 1]            (every part 16-byte aligned)
struct SpWs {
    unsigned long long* head; int32_t* cell; int32_t* vc; uint32_t* bits; int32_t* pre; int64_t* tw; unsigned long long* sum;
    unsigned long long* key; unsigned long long* tab; int32_t* tmin; uint8_t* keep; int64_t* tf;
    int64_t G, W, tilesW, Kmax, slots, tilesT; size_t bytes;
};
static SpWs sp_ws(void* w, int64_t V, int64_t T, const int* g) {
    SpWs r;
    r.G = sp_cells(g);
    r.W = (r.G + 31) / 32;
    r.tilesW = mc_tiles(r.W);
    r.Kmax = V < r.G ? V : r.G;
    if (r.Kmax > SP_CAP) r.Kmax = SP_CAP;
    r.slots = sp_table_slots(T);
    r.tilesT = cc_tiles(T);
    char* p = (char*)w;
    size_t o = 0;
    r.head = (unsigned long long*)(p + o); o += 64;
    r.cell = (int32_t*)(p + o); o += cc_up((size_t)4 * V);
    r.vc = (int32_t*)(p + o); o += cc_up((size_t)4 * V);
    r.bits = (uint32_t*)(p + o); o += cc_up((size_t)4 * r.W);
    r.pre = (int32_t*)(p + o); o += cc_up((size_t)4 * r.W);
    r.tw = (int64_t*)(p + o); o += cc_up((size_t)8 * (r.tilesW + 1));
    r.sum = (unsigned long long*)(p + o); o += cc_up((size_t)32 * r.Kmax);
    r.key = (unsigned long long*)(p + o); o += cc_up((size_t)8 * r.Kmax);
    r.tab = (unsigned long long*)(p + o); o += cc_up((size_t)8 * r.slots);
    r.tmin = (int32_t*)(p + o); o += cc_up((size_t)4 * r.slots);
    r.keep = (uint8_t*)(p + o); o += cc_up((size_t)T);
    r.tf = (int64_t*)(p + o); o += cc_up((size_t)8 * (r.tilesT + 1));
    r.bytes = o;
    return r;
}
size_t dsn_mesh_simplify_workspace_size(int64_t V, int64_t T, const int* g) { return sp_ws(nullptr, V, T, g).bytes; }

static SpGrid sp_grid(const float* origin, float cell, const int* g) {
    SpGrid r;
    for (int a = 0; a < 3; ++a) { r.o[a] = origin[a]; r.g[a] = g[a]; }
    r.inv = 1.0f / cell;
    return r;
}

// zero: the bit grid, the cluster slots (sums 0, keys all ones), the table (keys empty, minima INT_MAX), the header's counters
__global__ void __launch_bounds__(MC_THREADS) k_sp_zero(uint32_t* __restrict__ bits, int64_t W, unsigned long long* __restrict__ sum,
                                                        unsigned long long* __restrict__ key, int64_t Kmax, unsigned long long* __restrict__ tab,
                                                        int32_t* __restrict__ tmin, int64_t slots, unsigned long long* __restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * MC_THREADS;
    const int64_t i0 = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    for (int64_t i = i0; i < W; i += stride) bits[i] = 0u;
    for (int64_t i = i0; i < Kmax; i += stride) { sum[4 * i] = 0; sum[4 * i + 1] = 0; sum[4 * i + 2] = 0; sum[4 * i + 3] = 0; key[i] = SP_EMPTY; }
    for (int64_t i = i0; i < slots; i += stride) { tab[i] = SP_EMPTY; tmin[i] = 0x7FFFFFFF; }
    if (i0 < 8) head[i0] = 0;
}

// t_a = (x_a - origin_a) inv; inside: every t_a finite, >= 0 and < g_a (NaN fails the comparisons, +inf the second)
__device__ __forceinline__ bool sp_locate(const float* __restrict__ verts, int64_t v, const SpGrid& G, float t[3], int64_t& cell) {
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        t[a] = (verts[3 * v + a] - G.o[a]) * G.inv;
        in = in && t[a] >= 0.0f && t[a] < (float)G.g[a];
    }
    cell = -1;
    if (in) cell = ((int64_t)(int)floorf(t[0]) * G.g[1] + (int)floorf(t[1])) * G.g[2] + (int)floorf(t[2]);
    return in;
}
// q_a = floor(double(t_a) 2^20): exact, below 2^32
__device__ __forceinline__ unsigned long long sp_q(float t) { return (unsigned long long)floor((double)t * 1048576.0); }

__global__ void __launch_bounds__(MC_THREADS) k_sp_mark(const float* __restrict__ verts, int64_t V, SpGrid G, int32_t* __restrict__ cellv,
                                                        uint32_t* __restrict__ bits, unsigned long long* __restrict__ head) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool have = v < V;
    float t[3];
    int64_t cell = -1;
    const bool in = have && sp_locate(verts, v, G, t, cell);
    const int32_t c = in ? (int32_t)cell : -1;      // (cells < 2^31)
    if (have) cellv[v] = c;
    // marching-cubes vertices arrive x-major: neighbouring lanes share cells, a run of equal cells issues one atomic
    const int32_t prev = __shfl_up(c, 1);
    if (in && (lane == 0 || prev != c)) __hip_atomic_fetch_or(bits + (c >> 5), 1u << (c & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long out = __ballot(have && !in);
    if (lane == 0 && out) atomicAdd(head + SP_OUTSIDE, (unsigned long long)__popcll(out));
}

// in-tile exclusive popcount prefix of every bit-grid word, and the tile's total
__global__ void __launch_bounds__(MC_THREADS) k_sp_rank(const uint32_t* __restrict__ bits, int64_t W, int32_t* __restrict__ pre,
                                                        int64_t* __restrict__ tw) {
    const int64_t w0 = (int64_t)blockIdx.x * MC_TILE + (int64_t)threadIdx.x * MC_PER;
    int n = 0;
    for (int q = 0; q < MC_PER && w0 + q < W; ++q) n += __popc(bits[w0 + q]);
    int a = n, b = 0, tot_a, tot_b;
    mc_block_scan(a, b, tot_a, tot_b);
    for (int q = 0; q < MC_PER && w0 + q < W; ++q) { pre[w0 + q] = a; a += __popc(bits[w0 + q]); }
    if (threadIdx.x == 0) tw[blockIdx.x] = tot_a;
}

// one workgroup: exclusive scan of the tiles' totals in place, [tiles] = the total, also to *total; cap > 0: a total above it sets
// DSN_MESH_SIMPLIFY_TOO_MANY in *status
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_sp_scan(int64_t* __restrict__ tv, int64_t tiles, unsigned long long* __restrict__ total,
                                                             int64_t cap, unsigned long long* __restrict__ status) {
    __shared__ int64_t sa[MC_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (tiles + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int64_t b0 = t * per < tiles ? t * per : tiles, b1 = b0 + per < tiles ? b0 + per : tiles;
    int64_t a = 0;
    for (int64_t k = b0; k < b1; ++k) a += tv[k];
    sa[t] = a;
    __syncthreads();
    for (int off = 1; off < MC_SCAN_THREADS; off <<= 1) {
        const int64_t xa = t >= off ? sa[t - off] : 0;
        __syncthreads();
        sa[t] += xa;
        __syncthreads();
    }
    int64_t ra = sa[t] - a;
    for (int64_t k = b0; k < b1; ++k) { const int64_t va = tv[k]; tv[k] = ra; ra += va; }
    if (t == MC_SCAN_THREADS - 1) {
        tv[tiles] = sa[t];
        *total = (unsigned long long)sa[t];
        if (cap > 0 && sa[t] > cap) atomicOr(status, (unsigned long long)DSN_MESH_SIMPLIFY_TOO_MANY);
    }
}

// the run of equal keys a lane belongs to (keys of neighbouring lanes; a key that comes back later in the wave starts a new run)
__device__ __forceinline__ int sp_run(int32_t key, int lane, bool& first) {
    const int32_t prev = __shfl_up(key, 1);
    first = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(first);
    return __popcll(heads & ((2ull << lane) - 1ull));
}

// every vertex's cluster = the occupied cells below its cell; the clusters' integer sums
__global__ void __launch_bounds__(MC_THREADS) k_sp_sum(const float* __restrict__ verts, int64_t V, SpGrid G, int64_t ncell,
                                                       const int32_t* __restrict__ cellv, const uint32_t* __restrict__ bits,
                                                       const int32_t* __restrict__ pre, const int64_t* __restrict__ tw, int64_t Kmax,
                                                       const unsigned long long* __restrict__ head, int32_t* __restrict__ vc,
                                                       int32_t* __restrict__ vc_out, unsigned long long* __restrict__ sum) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool capped = (head[SP_STATUS] & DSN_MESH_SIMPLIFY_TOO_MANY) != 0;
    int32_t cl = -1;
    if (v < V) {
        const int32_t c = cellv[v];
        if ((uint64_t)(uint32_t)c < (uint64_t)ncell && c >= 0) {
            const int64_t w = c >> 5;
            cl = (int32_t)(tw[w / MC_TILE] + pre[w] + __popc(bits[w] & ((1u << (c & 31)) - 1u)));
        }
        vc[v] = cl;
        if (vc_out) vc_out[v] = cl;
    }
    const bool doit = !capped && (uint64_t)(uint32_t)cl < (uint64_t)Kmax && cl >= 0;
    unsigned long long q0 = 0, q1 = 0, q2 = 0;
    int n = 0;
    if (doit) {
        float t[3];
        int64_t cell;
        sp_locate(verts, v, G, t, cell);
        q0 = sp_q(t[0]); q1 = sp_q(t[1]); q2 = sp_q(t[2]); n = 1;
    }
    bool first;
    const int32_t key = doit ? cl : -1;
    const int run = sp_run(key, lane, first);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long x0 = __shfl_down(q0, off), x1 = __shfl_down(q1, off), x2 = __shfl_down(q2, off);
        const int xn = __shfl_down(n, off), xr = __shfl_down(run, off);
        if (lane + off < 64 && xr == run) { q0 += x0; q1 += x1; q2 += x2; n += xn; }
    }
    if (first && doit) {
        unsigned long long* s = sum + 4 * (int64_t)cl;
        atomicAdd(s, q0); atomicAdd(s + 1, q1); atomicAdd(s + 2, q2); atomicAdd(s + 3, (unsigned long long)n);
    }
}

// the representative: the member that minimises (bits of float32(d)) << 32 | vertex index
__global__ void __launch_bounds__(MC_THREADS) k_sp_pick(const float* __restrict__ verts, int64_t V, SpGrid G, const int32_t* __restrict__ vc,
                                                        int64_t Kmax, const unsigned long long* __restrict__ head,
                                                        const unsigned long long* __restrict__ sum, unsigned long long* __restrict__ key) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool capped = (head[SP_STATUS] & DSN_MESH_SIMPLIFY_TOO_MANY) != 0;
    const int32_t cl = v < V ? vc[v] : -1;
    const bool doit = !capped && (uint64_t)(uint32_t)cl < (uint64_t)Kmax && cl >= 0;
    unsigned long long k = SP_EMPTY;
    if (doit) {
        float t[3];
        int64_t cell;
        sp_locate(verts, v, G, t, cell);
        const unsigned long long* s = sum + 4 * (int64_t)cl;
        const double n = (double)(long long)s[3];
        const double e0 = (double)(long long)sp_q(t[0]) - (double)(long long)s[0] / n;
        const double e1 = (double)(long long)sp_q(t[1]) - (double)(long long)s[1] / n;
        const double e2 = (double)(long long)sp_q(t[2]) - (double)(long long)s[2] / n;
        const double d = (e0 * e0 + e1 * e1) + e2 * e2;
        k = ((unsigned long long)__float_as_uint((float)d) << 32) | (unsigned long long)(uint32_t)v;
    }
    bool first;
    const int run = sp_run(doit ? cl : -1, lane, first);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long xk = __shfl_down(k, off);
        const int xr = __shfl_down(run, off);
        if (lane + off < 64 && xr == run && xk < k) k = xk;
    }
    if (first && doit) __hip_atomic_fetch_min(key + cl, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the clusters of face t: 0 a bad index, 1 not live (a vertex outside or two clusters equal), 2 live with the packed sorted triple
__device__ __forceinline__ int sp_face(const int32_t* __restrict__ faces, int64_t t, int64_t V, const int32_t* __restrict__ vc, int32_t c[3],
                                       unsigned long long& packed) {
    int32_t i0, i1, i2;
    if (!cc_face(faces, t, (int)V, i0, i1, i2)) return 0;
    c[0] = vc[i0]; c[1] = vc[i1]; c[2] = vc[i2];
    if ((uint32_t)c[0] >= (uint32_t)SP_CAP || (uint32_t)c[1] >= (uint32_t)SP_CAP || (uint32_t)c[2] >= (uint32_t)SP_CAP) return 1;
    if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return 1;
    const int32_t lo = min(c[0], min(c[1], c[2])), hi = max(c[0], max(c[1], c[2])), mid = c[0] ^ c[1] ^ c[2] ^ lo ^ hi;
    packed = ((unsigned long long)lo << 42) | ((unsigned long long)mid << 21) | (unsigned long long)hi;
    return 2;
}
__device__ __forceinline__ uint64_t sp_hash(unsigned long long k) {      // (splitmix64's finaliser)
    k ^= k >> 30; k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 27; k *= 0x94D049BB133111EBull;
    return k ^ (k >> 31);
}

// a live face claims the slot of its triple and leaves the minimum of its index there.  The probe is bounded by the table's capacity and
// no thread waits for another: a slot's key goes from empty to one triple once and never changes again.
__global__ void __launch_bounds__(MC_THREADS) k_sp_faces(const int32_t* __restrict__ faces, int64_t V, int64_t T, const int32_t* __restrict__ vc,
                                                         unsigned long long* __restrict__ tab, int32_t* __restrict__ tmin, int64_t slots,
                                                         unsigned long long* __restrict__ head) {
    const int64_t t = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool capped = (head[SP_STATUS] & DSN_MESH_SIMPLIFY_TOO_MANY) != 0;
    int32_t c[3];
    unsigned long long packed = 0;
    const int kind = (t < T && !capped) ? sp_face(faces, t, V, vc, c, packed) : -1;
    if (kind == 2) {
        uint64_t s = sp_hash(packed) & (uint64_t)(slots - 1);
        bool placed = false;
        for (int64_t step = 0; step < slots; ++step) {
            unsigned long long seen = __hip_atomic_load(tab + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen == SP_EMPTY)
                seen = __hip_atomic_compare_exchange_strong(tab + s, &seen, packed, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                           ? packed : seen;      // (a failed exchange leaves the slot's triple in `seen`)
            if (seen == packed) {
                __hip_atomic_fetch_min(tmin + s, (int32_t)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                placed = true;
                break;
            }
            s = (s + 1) & (uint64_t)(slots - 1);
        }
        if (!placed) atomicOr(head + SP_STATUS, (unsigned long long)DSN_MESH_SIMPLIFY_TABLE_FULL);
    }
    const unsigned long long live = __ballot(kind == 2), bad = __ballot(kind == 0);
    if (lane == 0 && live) atomicAdd(head + SP_LIVE, (unsigned long long)__popcll(live));
    if (lane == 0 && bad) atomicAdd(head + SP_BAD, (unsigned long long)__popcll(bad));
}

// keep[t] = the face is live and the smallest index of its triple's slot; the kept faces of tile blockIdx.x
__global__ void __launch_bounds__(MC_THREADS) k_sp_keep(const int32_t* __restrict__ faces, int64_t V, int64_t T, const int32_t* __restrict__ vc,
                                                        const unsigned long long* __restrict__ tab, const int32_t* __restrict__ tmin,
                                                        int64_t slots, const unsigned long long* __restrict__ head, uint8_t* __restrict__ keep,
                                                        int64_t* __restrict__ tf) {
    const bool capped = (head[SP_STATUS] & DSN_MESH_SIMPLIFY_TOO_MANY) != 0;
    const int64_t n0 = (int64_t)blockIdx.x * CC_TILE + (int64_t)threadIdx.x * CC_PER;
    int nf = 0, none = 0, tot_f, tot_n;
    for (int q = 0; q < CC_PER && n0 + q < T; ++q) {
        const int64_t t = n0 + q;
        int32_t c[3];
        unsigned long long packed = 0;
        uint8_t k = 0;
        if (!capped && sp_face(faces, t, V, vc, c, packed) == 2) {
            uint64_t s = sp_hash(packed) & (uint64_t)(slots - 1);
            for (int64_t step = 0; step < slots; ++step) {
                const unsigned long long seen = tab[s];
                if (seen == packed) { k = tmin[s] == (int32_t)t; break; }
                if (seen == SP_EMPTY) break;
                s = (s + 1) & (uint64_t)(slots - 1);
            }
        }
        keep[t] = k;
        nf += k;
    }
    mc_block_scan(nf, none, tot_f, tot_n);
    if (threadIdx.x == 0) tf[blockIdx.x] = tot_f;
}

// out_counts: {K, kept faces, live faces, duplicates dropped, vertices outside, faces with a bad index, status}
__global__ void k_sp_counts(const unsigned long long* __restrict__ head, int64_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool capped = (head[SP_STATUS] & DSN_MESH_SIMPLIFY_TOO_MANY) != 0;
    out[0] = (int64_t)head[SP_K];
    out[1] = capped ? 0 : (int64_t)head[SP_KEPT];
    out[2] = (int64_t)head[SP_LIVE];
    out[3] = capped ? 0 : (int64_t)(head[SP_LIVE] - head[SP_KEPT]);
    out[4] = (int64_t)head[SP_OUTSIDE];
    out[5] = (int64_t)head[SP_BAD];
    out[6] = (int64_t)head[SP_STATUS];
}
__global__ void k_sp_count_cells(const unsigned long long* __restrict__ head, int64_t* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = (int64_t)head[SP_K];
}

__global__ void __launch_bounds__(MC_THREADS) k_sp_emit_verts(const float* __restrict__ verts, int64_t V, const unsigned long long* __restrict__ head,
                                                              const unsigned long long* __restrict__ key, int64_t Kmax,
                                                              float* __restrict__ out_verts, int64_t vcap, int32_t* __restrict__ source) {
    const int64_t k = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (head[SP_STATUS] != 0 || k >= vcap || k >= Kmax || (unsigned long long)k >= head[SP_K]) return;
    const uint32_t src = (uint32_t)key[k];
    if ((uint64_t)src >= (uint64_t)V) return;
    const uint32_t* in = (const uint32_t*)verts + 3 * (int64_t)src;      // the representative's three words, copied
    uint32_t* o = (uint32_t*)out_verts + 3 * k;
    o[0] = in[0]; o[1] = in[1]; o[2] = in[2];
    if (source) source[k] = (int32_t)src;
}

__global__ void __launch_bounds__(MC_THREADS) k_sp_emit_faces(const int32_t* __restrict__ faces, int64_t V, int64_t T, const int32_t* __restrict__ vc,
                                                              const unsigned long long* __restrict__ head, const uint8_t* __restrict__ keep,
                                                              const int64_t* __restrict__ tf, int32_t* __restrict__ out_faces, int64_t fcap) {
    const bool off = head[SP_STATUS] != 0;
    const int64_t n0 = (int64_t)blockIdx.x * CC_TILE + (int64_t)threadIdx.x * CC_PER;
    int mask = 0, nf = 0, none = 0, tot_f, tot_n;
    if (!off)
        for (int q = 0; q < CC_PER && n0 + q < T; ++q)
            if (keep[n0 + q] == 1) { mask |= 1 << q; ++nf; }
    mc_block_scan(nf, none, tot_f, tot_n);
    int64_t o = tf[blockIdx.x] + nf;
    for (int q = 0; q < CC_PER; ++q) {
        if (!((mask >> q) & 1)) continue;
        int32_t i0, i1, i2;
        if ((uint64_t)o < (uint64_t)fcap && (unsigned long long)o < head[SP_KEPT] && cc_face(faces, n0 + q, (int)V, i0, i1, i2)) {
            out_faces[3 * o] = vc[i0]; out_faces[3 * o + 1] = vc[i1]; out_faces[3 * o + 2] = vc[i2];
        }
        ++o;
    }
}

static unsigned sp_fill_blocks(int64_t n) {
    const int64_t b = (n + MC_THREADS - 1) / MC_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

void dsn_launch_mesh_simplify_count(const float* verts, const int32_t* faces, int64_t V, int64_t T, const float* origin, float cell, const int* g,
                                    void* workspace, int32_t* vertex_cluster, int64_t* out_counts, int phases, hipStream_t st) {
    SpWs w = sp_ws(workspace, V, T, g);
    const SpGrid G = sp_grid(origin, cell, g);
    const unsigned gV = mesh_blocks(V), gT = mesh_blocks(T);
    if (phases & DSN_SP_ZERO) {
        const int64_t most = w.W > w.slots ? w.W : w.slots;
        hipLaunchKernelGGL(k_sp_zero, dim3(sp_fill_blocks(most)), dim3(MC_THREADS), 0, st, w.bits, w.W, w.sum, w.key, w.Kmax, w.tab, w.tmin, w.slots,
                           w.head);
    }
    if ((phases & DSN_SP_MARK) && gV) hipLaunchKernelGGL(k_sp_mark, dim3(gV), dim3(MC_THREADS), 0, st, verts, V, G, w.cell, w.bits, w.head);
    if (phases & DSN_SP_RANK) {
        hipLaunchKernelGGL(k_sp_rank, dim3((unsigned)w.tilesW), dim3(MC_THREADS), 0, st, w.bits, w.W, w.pre, w.tw);
        hipLaunchKernelGGL(k_sp_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.tw, w.tilesW, w.head + SP_K, SP_CAP, w.head + SP_STATUS);
    }
    if ((phases & DSN_SP_SUM) && gV)
        hipLaunchKernelGGL(k_sp_sum, dim3(gV), dim3(MC_THREADS), 0, st, verts, V, G, w.G, w.cell, w.bits, w.pre, w.tw, w.Kmax, w.head, w.vc,
                           vertex_cluster, w.sum);
    if ((phases & DSN_SP_PICK) && gV)
        hipLaunchKernelGGL(k_sp_pick, dim3(gV), dim3(MC_THREADS), 0, st, verts, V, G, w.vc, w.Kmax, w.head, w.sum, w.key);
    if ((phases & DSN_SP_FACES) && gT)
        hipLaunchKernelGGL(k_sp_faces, dim3(gT), dim3(MC_THREADS), 0, st, faces, V, T, w.vc, w.tab, w.tmin, w.slots, w.head);
    if (phases & DSN_SP_KEEP) {
        if (w.tilesT)
            hipLaunchKernelGGL(k_sp_keep, dim3((unsigned)w.tilesT), dim3(MC_THREADS), 0, st, faces, V, T, w.vc, w.tab, w.tmin, w.slots, w.head, w.keep,
                               w.tf);
        hipLaunchKernelGGL(k_sp_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.tf, w.tilesT, w.head + SP_KEPT, (int64_t)0, w.head + SP_STATUS);
        hipLaunchKernelGGL(k_sp_counts, dim3(1), dim3(64), 0, st, w.head, out_counts);
    }
}

void dsn_launch_mesh_simplify_cells(const float* verts, int64_t V, const float* origin, float cell, const int* g, void* workspace, int64_t* out_K,
                                    hipStream_t st) {
    SpWs w = sp_ws(workspace, V, 0, g);
    const SpGrid G = sp_grid(origin, cell, g);
    hipLaunchKernelGGL(k_sp_zero, dim3(sp_fill_blocks(w.W)), dim3(MC_THREADS), 0, st, w.bits, w.W, w.sum, w.key, (int64_t)0, w.tab, w.tmin, (int64_t)0,
                       w.head);
    if (V) hipLaunchKernelGGL(k_sp_mark, dim3(mesh_blocks(V)), dim3(MC_THREADS), 0, st, verts, V, G, w.cell, w.bits, w.head);
    hipLaunchKernelGGL(k_sp_rank, dim3((unsigned)w.tilesW), dim3(MC_THREADS), 0, st, w.bits, w.W, w.pre, w.tw);
    hipLaunchKernelGGL(k_sp_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.tw, w.tilesW, w.head + SP_K, (int64_t)0, w.head + SP_STATUS);
    hipLaunchKernelGGL(k_sp_count_cells, dim3(1), dim3(64), 0, st, w.head, out_K);
}

void dsn_launch_mesh_simplify_emit(const float* verts, const int32_t* faces, int64_t V, int64_t T, const int* g, void* workspace, float* out_verts,
                                   int64_t vcap, int32_t* out_faces, int64_t fcap, int32_t* cluster_source, int phases, hipStream_t st) {
    SpWs w = sp_ws(workspace, V, T, g);
    if ((phases & DSN_SP_EMIT_VERTS) && vcap > 0)
        hipLaunchKernelGGL(k_sp_emit_verts, dim3(mesh_blocks(vcap)), dim3(MC_THREADS), 0, st, verts, V, w.head, w.key, w.Kmax, out_verts, vcap,
                           cluster_source);
    if ((phases & DSN_SP_EMIT_FACES) && w.tilesT && fcap > 0)
        hipLaunchKernelGGL(k_sp_emit_faces, dim3((unsigned)w.tilesT), dim3(MC_THREADS), 0, st, faces, V, T, w.vc, w.head, w.keep, w.tf, out_faces, fcap);
}

// ---------------------------------------------------------------------------------------------
// umbrella smoothing and vertex normals from the faces (dsn_mesh_smooth / dsn_mesh_vertex_normals, the rule of include/dsnerf.h)
//   lists : zero -> count (one thread per face: a contributing face adds 1 to each corner's row length, one int32 atomic per run of
//           equal vertices in the wave) -> rank (the rows' 64-bit in-tile prefix over tiles of CC_TILE vertices, the vertices in use and
//           the longest row) + k_sp_scan over the tiles -> fill (the face's entry into each corner's row through an atomic cursor).
//           Entry of corner c of face (i0, i1, i2): the two corners after it in winding order, c in the two sign bits.
//   step  : one thread per vertex gathers its row from the positions of the step before (the integer sums in registers) and writes x';
//           a row longer than DSN_MESH_SMOOTH_HEAVY is summed by its whole wave.  No atomics.
//   normals: the same gather over the same lists, the face normals in float32, the sums in integers.
// Global atomics execute at the memory side: a scatter of 3 T 64-bit adds per step would run at the atomic rate, the gather runs at the
// rate of the loads.  Every value read back from the workspace is range-checked before it is used as an index.
// ---------------------------------------------------------------------------------------------
enum { SM_FACES = 0, SM_USED = 2, SM_LONGEST = 3 };      // the header's 64-bit words

// header 64 B | row lengths int32 [V] | cursors int32 [V] | in-tile row prefix int64 [V] | tile offsets int64 [tiles + 1] |
// entries int32 [3 T, 2] | positions A float [3 V] | positions B float [3 V]            (every part 16-byte aligned)
struct SmWs {
    unsigned long long* head; int32_t* cnt; int32_t* cur; int64_t* pre; int64_t* tw; int2* ent; float* pa; float* pb;
    int64_t tiles; size_t bytes;
};
static SmWs sm_ws(void* w, int64_t V, int64_t T) {
    SmWs r;
    r.tiles = cc_tiles(V);
    char* p = (char*)w;
    size_t o = 0;
    r.head = (unsigned long long*)(p + o); o += 64;
    r.cnt = (int32_t*)(p + o); o += cc_up((size_t)4 * V);
    r.cur = (int32_t*)(p + o); o += cc_up((size_t)4 * V);
    r.pre = (int64_t*)(p + o); o += cc_up((size_t)8 * V);
    r.tw = (int64_t*)(p + o); o += cc_up((size_t)8 * (r.tiles + 1));
    r.ent = (int2*)(p + o); o += cc_up((size_t)24 * T);
    r.pa = (float*)(p + o); o += cc_up((size_t)12 * V);
    r.pb = (float*)(p + o); o += cc_up((size_t)12 * V);
    r.bytes = o;
    return r;
}
size_t dsn_mesh_smooth_workspace_size(int64_t V, int64_t T) { return sm_ws(nullptr, V, T).bytes; }

__global__ void __launch_bounds__(MC_THREADS) k_sm_zero(int32_t* __restrict__ cnt, int32_t* __restrict__ cur, int64_t V,
                                                        unsigned long long* __restrict__ head) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v < 8) head[v] = 0;
    if (v < V) { cnt[v] = 0; cur[v] = 0; }
}

__device__ __forceinline__ bool sm_finite3(const float* __restrict__ p) {
    const float inf = __builtin_inff();
    return fabsf(p[0]) < inf && fabsf(p[1]) < inf && fabsf(p[2]) < inf;      // (NaN fails the comparison)
}
// a contributing face: indices in [0, V), pairwise different, nine finite coordinates
__device__ __forceinline__ bool sm_face(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t t, int64_t V, int32_t i[3]) {
    if (!cc_face(faces, t, (int)V, i[0], i[1], i[2])) return false;
    if (i[0] == i[1] || i[1] == i[2] || i[0] == i[2]) return false;
    return sm_finite3(verts + 3 * (int64_t)i[0]) && sm_finite3(verts + 3 * (int64_t)i[1]) && sm_finite3(verts + 3 * (int64_t)i[2]);
}

// Neighbouring lanes with the same key form a run (the corners of a fan, the shared vertices of a marching-cubes strip): the run's first
// lane adds the run's length to the key's counter with one atomic and every lane takes its own slot of the range that add returned.
__device__ __forceinline__ int32_t sm_claim(int32_t* __restrict__ ctr, int32_t key, bool on, int lane) {
    key = on ? key : -1;
    const int32_t prev = __shfl_up(key, 1);
    const bool first = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(first);                                        // (lane 0 is always a head)
    const int head_lane = 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));
    const unsigned long long above = heads & ~((2ull << head_lane) - 1ull);
    const int next = above ? __ffsll((long long)above) - 1 : 64;
    int32_t base = 0;
    if (first && on) base = __hip_atomic_fetch_add(ctr + key, next - head_lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, head_lane);
    return base + (lane - head_lane);
}

__global__ void __launch_bounds__(MC_THREADS) k_sm_count(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                         int32_t* __restrict__ cnt, unsigned long long* __restrict__ head) {
    const int64_t t = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t i[3] = {0, 0, 0};
    const bool on = t < T && sm_face(verts, faces, t, V, i);
#pragma unroll
    for (int c = 0; c < 3; ++c) sm_claim(cnt, i[c], on, lane);
    const unsigned long long m = __ballot(on);
    if (lane == 0 && m) __hip_atomic_fetch_add(head + SM_FACES, (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the rows' exclusive 64-bit prefix inside tile blockIdx.x and the tile's total; the vertices in use and the longest row
__global__ void __launch_bounds__(MC_THREADS) k_sm_rank(const int32_t* __restrict__ cnt, int64_t V, int64_t* __restrict__ pre,
                                                        int64_t* __restrict__ tw, unsigned long long* __restrict__ head) {
    __shared__ int64_t sa[MC_THREADS];
    const int t = threadIdx.x, lane = threadIdx.x & 63;
    const int64_t v0 = (int64_t)blockIdx.x * CC_TILE + (int64_t)t * CC_PER;
    int32_t c[CC_PER];
    int64_t a = 0;
    int used = 0, longest = 0;
#pragma unroll
    for (int q = 0; q < CC_PER; ++q) {
        c[q] = v0 + q < V ? cnt[v0 + q] : 0;
        if (c[q] < 0) c[q] = 0;
        a += c[q];
        used += c[q] > 0 ? 1 : 0;
        longest = c[q] > longest ? c[q] : longest;
    }
    sa[t] = a;
    __syncthreads();
    for (int off = 1; off < MC_THREADS; off <<= 1) {
        const int64_t x = t >= off ? sa[t - off] : 0;
        __syncthreads();
        sa[t] += x;
        __syncthreads();
    }
    int64_t p = sa[t] - a;
#pragma unroll
    for (int q = 0; q < CC_PER; ++q) {
        if (v0 + q < V) pre[v0 + q] = p;
        p += c[q];
    }
    if (t == MC_THREADS - 1) tw[blockIdx.x] = sa[t];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        used += __shfl_xor(used, off);
        const int o = __shfl_xor(longest, off);
        longest = o > longest ? o : longest;
    }
    if (lane == 0 && used) {
        __hip_atomic_fetch_add(head + SM_USED, (unsigned long long)used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(head + SM_LONGEST, (unsigned long long)longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void k_sm_counts(const unsigned long long* __restrict__ head, int64_t T, int64_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = (int64_t)head[SM_FACES];
    out[1] = T - (int64_t)head[SM_FACES];
    out[2] = (int64_t)head[SM_USED];
    out[3] = (int64_t)head[SM_LONGEST];
}

// row of vertex v: start (into the entries) and length, clamped into [0, 3 T] whatever the workspace holds
__device__ __forceinline__ void sm_row(const int32_t* __restrict__ cnt, const int64_t* __restrict__ pre, const int64_t* __restrict__ tw,
                                       int64_t v, int64_t T, int64_t& start, int32_t& len) {
    start = tw[v / CC_TILE] + pre[v];
    len = cnt[v];
    const int64_t cap = 3 * T;
    if (start < 0 || start > cap || len < 0) { start = 0; len = 0; }
    if (len > cap - start) len = (int32_t)(cap - start);
}

__global__ void __launch_bounds__(MC_THREADS) k_sm_fill(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                        const int32_t* __restrict__ cnt, const int64_t* __restrict__ pre,
                                                        const int64_t* __restrict__ tw, int32_t* __restrict__ cur, int2* __restrict__ ent) {
    const int64_t t = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t i[3] = {0, 0, 0};
    const bool on = t < T && sm_face(verts, faces, t, V, i);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int32_t slot = sm_claim(cur, i[c], on, lane);
        if (!on) continue;
        int64_t start; int32_t len;
        sm_row(cnt, pre, tw, i[c], T, start, len);
        if ((uint32_t)slot >= (uint32_t)len) continue;      // (never, after count and rank)
        const int32_t j = i[(c + 1) % 3], l = i[(c + 2) % 3];
        ent[start + slot] = make_int2(j | (int32_t)((uint32_t)(c & 1) << 31), l | (int32_t)((uint32_t)(c >> 1) << 31));
    }
}

// q = floor((double(x) - double(origin)) 2^k) clamped to [-2^30, 2^30 - 1]; 0 where the difference is not finite
__device__ __forceinline__ int64_t sm_q(float x, double o, double scale) {
    const double r = (double)x - o;
    if (!(fabs(r) < (double)__builtin_inff())) return 0;
    double q = floor(r * scale);
    q = q < -1073741824.0 ? -1073741824.0 : (q > 1073741823.0 ? 1073741823.0 : q);
    return (int64_t)q;
}

struct SmGrid { double o[3]; double scale; double inv; };

// the step's row sum: per entry q_j + q_l over the three axes (the caller takes 2 len q_i off)
struct SmStepAcc {
    int64_t s[3];
    const float* pos; double o[3]; double scale; int64_t V;
    __device__ __forceinline__ void i_set(int64_t) {}
    __device__ __forceinline__ void add(int2 e) {
        const int64_t j = e.x & 0x7FFFFFFF, l = e.y & 0x7FFFFFFF;
        if (j >= V || l >= V) return;                      // (never, after fill)
        const float* a = pos + 3 * j; const float* b = pos + 3 * l;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += sm_q(a[c], o[c], scale) + sm_q(b[c], o[c], scale);
    }
};

// the normals' row sum: the face of every entry in its own winding, its float32 normal, floor(n_c 2^shift).  Branch-free: the loads of
// an entry do not wait for one another's tests (what an entry must not add is selected to 0 at the end).
struct SmNormalAcc {
    int64_t s[3];
    const float* pos; double scale; int64_t V; float p[3];      // p: the row's own vertex
    __device__ __forceinline__ void i_set(int64_t v) { p[0] = pos[3 * v]; p[1] = pos[3 * v + 1]; p[2] = pos[3 * v + 2]; }
    __device__ __forceinline__ void add(int2 e) {
        const int64_t j = e.x & 0x7FFFFFFF, l = e.y & 0x7FFFFFFF;
        const int c = (int)((uint32_t)e.x >> 31) | ((int)((uint32_t)e.y >> 31) << 1);
        bool ok = j < V && l < V && c <= 2;                // (always, after fill)
        const float* pj = pos + 3 * (ok ? j : 0); const float* pl = pos + 3 * (ok ? l : 0);
        const float xj[3] = {pj[0], pj[1], pj[2]}, xl[3] = {pl[0], pl[1], pl[2]};
        float a[3], b[3], cc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {                      // corner c of (a, b, cc) is the row's vertex, j and l follow it in the winding
            a[k] = c == 0 ? p[k] : (c == 1 ? xl[k] : xj[k]);
            b[k] = c == 0 ? xj[k] : (c == 1 ? p[k] : xl[k]);
            cc[k] = c == 0 ? xl[k] : (c == 1 ? xj[k] : p[k]);
        }
        ok = ok && sm_finite3(p) && sm_finite3(xj) && sm_finite3(xl);
        const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
        const float e2x = cc[0] - a[0], e2y = cc[1] - a[1], e2z = cc[2] - a[2];
        const float n[3] = {e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double q = floor((double)n[k] * scale);
            q = q < -4611686018427387904.0 ? -4611686018427387904.0 : (q > 4611686018427387904.0 ? 4611686018427387904.0 : q);
            s[k] += (int64_t)(ok && fabsf(n[k]) < __builtin_inff() ? q : 0.0);
        }
    }
};

// the row of every lane's vertex into acc.s: a light row by its own lane, a heavy one by the whole wave (every lane of the wave calls this)
template <class Acc>
__device__ __forceinline__ void sm_gather(const int2* __restrict__ ent, int64_t start, int32_t len, int64_t v, Acc& acc, int lane) {
    acc.s[0] = acc.s[1] = acc.s[2] = 0;
    if (len <= DSN_MESH_SMOOTH_HEAVY)
        for (int32_t e = 0; e < len; ++e) acc.add(ent[start + e]);
    unsigned long long heavy = __ballot(len > DSN_MESH_SMOOTH_HEAVY);
    while (heavy) {
        const int leader = __ffsll((long long)heavy) - 1;
        heavy &= heavy - 1;
        const int64_t hs = __shfl(start, leader), hv = __shfl(v, leader);
        const int32_t hl = __shfl(len, leader);
        Acc part = acc;
        part.s[0] = part.s[1] = part.s[2] = 0;
        part.i_set(hv);
#pragma unroll 4
        for (int32_t e = lane; e < hl; e += 64) part.add(ent[hs + e]);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) part.s[c] += __shfl_xor(part.s[c], off);
        if (lane == leader) { acc.s[0] = part.s[0]; acc.s[1] = part.s[1]; acc.s[2] = part.s[2]; }
    }
}

__global__ void __launch_bounds__(MC_THREADS) k_sm_step(const float* __restrict__ src, float* __restrict__ dst, int64_t V, int64_t T,
                                                        const int32_t* __restrict__ cnt, const int64_t* __restrict__ pre,
                                                        const int64_t* __restrict__ tw, const int2* __restrict__ ent, SmGrid G, double f) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int64_t start = 0; int32_t len = 0;
    if (v < V) sm_row(cnt, pre, tw, v, T, start, len);
    SmStepAcc acc;
    acc.pos = src; acc.o[0] = G.o[0]; acc.o[1] = G.o[1]; acc.o[2] = G.o[2]; acc.scale = G.scale; acc.V = V;
    sm_gather(ent, start, len, v, acc, lane);
    if (v >= V) return;
    if (len == 0) {                                        // n_i = 0: the three words, copied
        const uint32_t* in = (const uint32_t*)src + 3 * v;
        uint32_t* o = (uint32_t*)dst + 3 * v;
        o[0] = in[0]; o[1] = in[1]; o[2] = in[2];
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = src[3 * v + c];
        const int64_t S = acc.s[c] - 2 * (int64_t)len * sm_q(x, G.o[c], G.scale);
        const double delta = (double)S / (double)(2 * (int64_t)len);
        const double t = f * delta;
        const double u = t * G.inv;
        dst[3 * v + c] = (float)((double)x + u);
    }
}

__global__ void __launch_bounds__(MC_THREADS) k_sm_normals(const float* __restrict__ verts, float* __restrict__ out, int64_t V, int64_t T,
                                                           const int32_t* __restrict__ cnt, const int64_t* __restrict__ pre,
                                                           const int64_t* __restrict__ tw, const int2* __restrict__ ent, double scale) {
    const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int64_t start = 0; int32_t len = 0;
    if (v < V) sm_row(cnt, pre, tw, v, T, start, len);
    SmNormalAcc acc;
    acc.pos = verts; acc.scale = scale; acc.V = V;
    acc.p[0] = acc.p[1] = acc.p[2] = 0.0f;
    if (v < V) acc.i_set(v);
    sm_gather(ent, start, len, v, acc, lane);
    if (v >= V) return;
    const double N0 = (double)acc.s[0], N1 = (double)acc.s[1], N2 = (double)acc.s[2];
    const double L = sqrt((N0 * N0 + N1 * N1) + N2 * N2);
    const bool ok = L > 0.0;
    out[3 * v] = ok ? (float)(N0 / L) : 0.0f;
    out[3 * v + 1] = ok ? (float)(N1 / L) : 0.0f;
    out[3 * v + 2] = ok ? (float)(N2 / L) : 0.0f;
}

__global__ void __launch_bounds__(MC_THREADS) k_sm_copy(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (k < n) dst[k] = src[k];
}

static void sm_lists(const float* verts, const int32_t* faces, int64_t V, int64_t T, const SmWs& w, int64_t* out_counts, int phases,
                     hipStream_t st) {
    const unsigned gV = mesh_blocks(V), gT = mesh_blocks(T);
    if (phases & DSN_SM_COUNT) {
        hipLaunchKernelGGL(k_sm_zero, dim3(gV ? gV : 1), dim3(MC_THREADS), 0, st, w.cnt, w.cur, V, w.head);
        if (gT && gV) hipLaunchKernelGGL(k_sm_count, dim3(gT), dim3(MC_THREADS), 0, st, verts, faces, V, T, w.cnt, w.head);
    }
    if (phases & DSN_SM_SCAN) {
        if (w.tiles) hipLaunchKernelGGL(k_sm_rank, dim3((unsigned)w.tiles), dim3(MC_THREADS), 0, st, w.cnt, V, w.pre, w.tw, w.head);
        hipLaunchKernelGGL(k_sp_scan, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.tw, w.tiles, w.head + 4, (int64_t)0, w.head + 5);
        if (out_counts) hipLaunchKernelGGL(k_sm_counts, dim3(1), dim3(64), 0, st, w.head, T, out_counts);
    }
    if ((phases & DSN_SM_FILL) && gT && gV)
        hipLaunchKernelGGL(k_sm_fill, dim3(gT), dim3(MC_THREADS), 0, st, verts, faces, V, T, w.cnt, w.pre, w.tw, w.cur, w.ent);
}

void dsn_launch_mesh_smooth(const float* verts, const int32_t* faces, int64_t V, int64_t T, const float* origin, int k, const float* factors,
                            int n_steps, void* workspace, float* out_verts, int64_t* out_counts, int phases, hipStream_t st) {
    SmWs w = sm_ws(workspace, V, T);
    sm_lists(verts, faces, V, T, w, out_counts, phases, st);
    if (!(phases & DSN_SM_STEP) || V == 0) return;
    const unsigned gV = mesh_blocks(V);
    if (n_steps == 0) {
        hipLaunchKernelGGL(k_sm_copy, dim3(mesh_blocks(3 * V)), dim3(MC_THREADS), 0, st, (const uint32_t*)verts, (uint32_t*)out_verts, 3 * V);
        return;
    }
    SmGrid G;
    for (int a = 0; a < 3; ++a) G.o[a] = (double)origin[a];
    G.scale = ldexp(1.0, k); G.inv = ldexp(1.0, -k);
    const float* src = verts;
    for (int s = 0; s < n_steps; ++s) {
        float* dst = s == n_steps - 1 ? out_verts : ((s & 1) ? w.pb : w.pa);
        hipLaunchKernelGGL(k_sm_step, dim3(gV), dim3(MC_THREADS), 0, st, src, dst, V, T, w.cnt, w.pre, w.tw, w.ent, G, (double)factors[s]);
        src = dst;
    }
}

void dsn_launch_mesh_vertex_normals(const float* verts, const int32_t* faces, int64_t V, int64_t T, double scale, void* workspace,
                                    float* out_normals, int phases, hipStream_t st) {
    SmWs w = sm_ws(workspace, V, T);
    sm_lists(verts, faces, V, T, w, nullptr, phases, st);
    if ((phases & DSN_SM_NORMALS) && V)
        hipLaunchKernelGGL(k_sm_normals, dim3(mesh_blocks(V)), dim3(MC_THREADS), 0, st, verts, out_normals, V, T, w.cnt, w.pre, w.tw, w.ent, scale);
}
