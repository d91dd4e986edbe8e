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
