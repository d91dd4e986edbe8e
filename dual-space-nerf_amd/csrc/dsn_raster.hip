// dsn_raster.hip - utils/visualizer.py:144-168 Visualizer3D.render_mesh on the device: a deterministic triangle rasteriser with the
// reference's camera and spotlight (dsn_raster_mesh, the rule of include/dsnerf.h).  No pyrender, no GL.
//
// The workload is micro-triangles (a marching-cubes mesh at resolution 512 has 10 M triangles of about one pixel in a 1024 x 1024
// image), so nothing is binned into tiles: a visibility buffer of one 64-bit word per pixel,
//     key = depth bits << 32 | face index        (depth > 0: its float bits order as unsigned integers)
// takes one atomic unsigned minimum per covered pixel centre.  The smallest key wins whatever the order of arrival, and on equal
// depth the lowest face index: every call returns the same bits.
//   k_rm_clear     vis = all ones (empty), the big-triangle counter = 0; nothing relies on the scratch's previous contents
//   k_rm_project   one thread per vertex: sub-pixel screen coordinates (1/256 px), 1/w, validity
//   k_rm_raster    one thread per triangle: int64 edge functions over its pixel bounding box.  A triangle whose box holds more than
//                  big_pixels pixels goes to a list instead (workgroup-aggregated append, as the active lists are built) ...
//   k_rm_raster_big  ... and one wave rasterises each listed triangle, lanes striding over the box: a low-resolution mesh or a close
//                  camera never puts a long pixel loop on one lane
//   k_rm_shade     one thread per pixel: unpacks the winner, writes face / depth / colour
//   k_rm_shade_attr  dsn_raster_mesh_attr's shade step in k_rm_shade's place (the passes before it are the same kernels): the winner's
//                  perspective-correct weights from its edge functions again, vertex normals and colours interpolated with them
// No float atomics, no MFMA, no allocation, no synchronisation; everything on the caller's stream.
#include "dsn_common.h"
#include "dsn_kernels.h"
#include "../../include/dsnerf.h"

#define RM_THREADS 256
#define RM_WAVES (RM_THREADS / 64)
#define RM_GUARD 16777216.0f                   // |X|, |Y| <= 2^24 sub-pixel units: edge-function products stay below 2^52
#define RM_EMPTY 0xFFFFFFFFFFFFFFFFull
#define RM_BIG_BLOCKS 1024                     // k_rm_raster_big: at most this many workgroups; waves stride over the list

namespace {
struct RmCam {
    float R[9];                // camera-to-world rotation, row-major: R[3 i + k] = R_ik
    float t[3];
    float fx, fy, znear, half_w, half_h, fw, fh;
    float k, cos_inner, cos_outer;
    int H, W;
};

// ws: projected vertices int4 [V] | vis uint64 [H W] | big-triangle count int32 [2] | big-triangle list int32 [T]
struct RmWs { int4* pv; unsigned long long* vis; int32_t* count; int32_t* list; };
RmWs rm_ws(void* w, int64_t V, int64_t T, int H, int W) {
    char* p = (char*)w;
    RmWs r;
    r.pv = (int4*)p;
    r.vis = (unsigned long long*)(p + 16 * (size_t)V);
    r.count = (int32_t*)(p + 16 * (size_t)V + 8 * (size_t)H * W);
    r.list = r.count + 2;
    return r;
}

// c_k = (d0 R0k + d1 R1k) + d2 R2k with d = v - t
__device__ __forceinline__ void rm_camera(const RmCam& cam, const float* __restrict__ v, float c[3]) {
    const float d0 = v[0] - cam.t[0], d1 = v[1] - cam.t[1], d2 = v[2] - cam.t[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (d0 * cam.R[k] + d1 * cam.R[3 + k]) + d2 * cam.R[6 + k];
}

struct RmTri {
    int64_t A[3], B[3], C[3];      // E_k(P) = A_k Px + B_k Py + C_k
    int64_t bias[3];               // 0 on top-left edges, 1 elsewhere: covered when E_k - bias_k >= 0
    float iw[3];
    float area;
    int x0, y0, bw, bh;            // pixel bounding box inside the image (bw <= 0 or bh <= 0: nothing)
};

// false: the triangle is dropped (index out of range, invalid vertex, zero area) or covers no pixel centre's box
__device__ __forceinline__ bool rm_setup(const int4* __restrict__ pv, const int32_t* __restrict__ faces, int64_t f, int64_t V, int H, int W,
                                         RmTri& t) {
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
    int4 a = pv[i0], b = pv[i1], c = pv[i2];
    if (!(a.w & b.w & c.w)) return false;
    int64_t area = (int64_t)(b.x - a.x) * (c.y - a.y) - (int64_t)(b.y - a.y) * (c.x - a.x);
    if (area == 0) return false;
    if (area < 0) { const int4 s = b; b = c; c = s; area = -area; }      // two-sided: (v0, v2, v1)
    const int4 P[3] = {a, b, c};
#pragma unroll
    for (int k = 0; k < 3; ++k) {          // E_k: the edge opposite vertex k, from P[k + 1] to P[k + 2]
        const int4 s = P[(k + 1) % 3], e = P[(k + 2) % 3];
        const int64_t dx = e.x - s.x, dy = e.y - s.y;
        t.A[k] = -dy;
        t.B[k] = dx;
        t.C[k] = dy * s.x - dx * s.y;
        t.bias[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
        t.iw[k] = __int_as_float(P[k].z);
    }
    t.area = (float)area;
    const int minx = min(a.x, min(b.x, c.x)), maxx = max(a.x, max(b.x, c.x));
    const int miny = min(a.y, min(b.y, c.y)), maxy = max(a.y, max(b.y, c.y));
    // pixel centres 256 x + 128 inside [min, max] (arithmetic shifts: floor)
    const int x0 = max((minx + 127) >> 8, 0), x1 = min((maxx - 128) >> 8, W - 1);
    const int y0 = max((miny + 127) >> 8, 0), y1 = min((maxy - 128) >> 8, H - 1);
    t.x0 = x0; t.y0 = y0; t.bw = x1 - x0 + 1; t.bh = y1 - y0 + 1;
    return t.bw > 0 && t.bh > 0;
}

__device__ __forceinline__ void rm_pixel(const RmTri& t, int x, int y, int W, uint32_t f, unsigned long long* __restrict__ vis) {
    const int64_t px = 256 * (int64_t)x + 128, py = 256 * (int64_t)y + 128;
    const int64_t e0 = t.A[0] * px + t.B[0] * py + t.C[0];
    const int64_t e1 = t.A[1] * px + t.B[1] * py + t.C[1];
    const int64_t e2 = t.A[2] * px + t.B[2] * py + t.C[2];
    if (((e0 - t.bias[0]) | (e1 - t.bias[1]) | (e2 - t.bias[2])) < 0) return;
    const float l0 = (float)e0 / t.area, l1 = (float)e1 / t.area, l2 = (float)e2 / t.area;
    const float q = (l0 * t.iw[0] + l1 * t.iw[1]) + l2 * t.iw[2];
    const float z = 1.0f / q;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | f;
    unsigned long long* p = vis + (size_t)y * W + x;
    if (key < __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMin(p, key);
}
}  // namespace

__global__ void __launch_bounds__(RM_THREADS) k_rm_clear(unsigned long long* __restrict__ vis, int64_t n, int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x;
    if (i < n) vis[i] = RM_EMPTY;
    if (i == 0) { count[0] = 0; count[1] = 0; }
}

__global__ void __launch_bounds__(RM_THREADS) k_rm_project(const float* __restrict__ verts, int64_t V, RmCam cam, int4* __restrict__ pv) {
    const int64_t i = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x;
    if (i >= V) return;
    float c[3];
    rm_camera(cam, verts + 3 * i, c);
    const float w = -c[2];
    const float xn = (cam.fx * c[0]) / w, yn = (cam.fy * c[1]) / w;
    const float px = (xn + 1.0f) * cam.half_w, py = (1.0f - yn) * cam.half_h;
    const float rx = rintf(px * 256.0f), ry = rintf(py * 256.0f);          // round-half-even
    // (NaN fails every comparison; a finite px whose px * 256 overflows fails the guard band)
    const bool ok = w > cam.znear && fabsf(px) < __builtin_inff() && fabsf(py) < __builtin_inff() && fabsf(rx) <= RM_GUARD && fabsf(ry) <= RM_GUARD;
    int4 o;
    o.x = ok ? (int)rx : 0;
    o.y = ok ? (int)ry : 0;
    o.z = __float_as_int(1.0f / w);
    o.w = ok ? 1 : 0;
    pv[i] = o;
}

__global__ void __launch_bounds__(RM_THREADS) k_rm_raster(const int4* __restrict__ pv, int64_t V, const int32_t* __restrict__ faces, int64_t T,
                                                          int H, int W, int big_pixels, unsigned long long* __restrict__ vis,
                                                          int32_t* __restrict__ big_count, int32_t* __restrict__ big_list) {
    __shared__ int s_cnt[RM_WAVES];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = (int64_t)blockIdx.x * RM_THREADS + tid;
    RmTri t;
    const bool live = f < T && rm_setup(pv, faces, f, V, H, W, t);
    const bool big = live && (int64_t)t.bw * t.bh > big_pixels;
    // workgroup-aggregated append of the big triangles
    const unsigned long long bm = __ballot(big);
    if (lane == 0) s_cnt[wave] = __popcll(bm);
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
#pragma unroll
        for (int k = 0; k < RM_WAVES; ++k) tot += s_cnt[k];
        s_base = tot ? atomicAdd(big_count, tot) : 0;
    }
    __syncthreads();
    if (big) {
        int off = s_base + __popcll(bm & ((1ull << lane) - 1ull));
        for (int k = 0; k < wave; ++k) off += s_cnt[k];
        big_list[off] = (int32_t)f;          // (at most T entries: each triangle is appended once)
    }
    if (!live || big) return;
    for (int y = 0; y < t.bh; ++y)
        for (int x = 0; x < t.bw; ++x) rm_pixel(t, t.x0 + x, t.y0 + y, W, (uint32_t)f, vis);
}

__global__ void __launch_bounds__(RM_THREADS) k_rm_raster_big(const int4* __restrict__ pv, int64_t V, const int32_t* __restrict__ faces,
                                                              int64_t T, int H, int W, unsigned long long* __restrict__ vis,
                                                              const int32_t* __restrict__ big_count, const int32_t* __restrict__ big_list) {
    const int lane = threadIdx.x & 63;
    const int64_t n = big_count[0] < T ? big_count[0] : T;
    const int64_t waves = (int64_t)gridDim.x * RM_WAVES;
    for (int64_t i = (int64_t)blockIdx.x * RM_WAVES + (threadIdx.x >> 6); i < n; i += waves) {
        const int64_t f = big_list[i];
        RmTri t;
        if (f < 0 || f >= T || !rm_setup(pv, faces, f, V, H, W, t)) continue;      // (wave-uniform)
        const int cnt = t.bw * t.bh;                                              // <= 16384^2 = 2^28
        for (int j = lane; j < cnt; j += 64) rm_pixel(t, t.x0 + j % t.bw, t.y0 + j / t.bw, W, (uint32_t)f, vis);
    }
}

__global__ void __launch_bounds__(RM_THREADS) k_rm_shade(const unsigned long long* __restrict__ vis, const float* __restrict__ verts,
                                                         int64_t V, const int32_t* __restrict__ faces, int64_t T, RmCam cam,
                                                         int32_t* __restrict__ out_face,
                                                         float* __restrict__ out_depth, uint8_t* __restrict__ out_color) {
    const int64_t i = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x;
    if (i >= (int64_t)cam.H * cam.W) return;
    const unsigned long long key = vis[i];
    bool hit = key != RM_EMPTY;
    int64_t v0 = 0, v1 = 0, v2 = 0;
    if (hit) {      // (the winner passed k_rm_raster's checks; a visibility buffer of another mesh - phases run apart - reads as empty)
        const int64_t g = (int64_t)(key & 0xFFFFFFFFull);
        hit = g < T;
        if (hit) {
            v0 = faces[3 * g]; v1 = faces[3 * g + 1]; v2 = faces[3 * g + 2];
            hit = v0 >= 0 && v1 >= 0 && v2 >= 0 && v0 < V && v1 < V && v2 < V;
        }
    }
    const int32_t f = hit ? (int32_t)(key & 0xFFFFFFFFull) : -1;
    const float z = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
    if (out_face) out_face[i] = f;
    if (out_depth) out_depth[i] = z;
    if (!out_color) return;
    float level = 255.0f;          // empty: the white background, no ambient light
    if (hit) {
        const int y = (int)(i / cam.W), x = (int)(i % cam.W);
        const float xn = (float)(2 * x + 1) / cam.fw - 1.0f, yn = 1.0f - (float)(2 * y + 1) / cam.fh;
        const float px = (xn * z) / cam.fx, py = (yn * z) / cam.fy;
        const float r2 = (px * px + py * py) + z * z;
        const float r = sqrtf(r2);
        float s = (z / r - cam.cos_outer) / (cam.cos_inner - cam.cos_outer);
        s = s > 0.0f ? s : 0.0f;
        s = s < 1.0f ? s : 1.0f;
        s = s * s;
        float c0[3], c1[3], c2[3];
        rm_camera(cam, verts + 3 * v0, c0);
        rm_camera(cam, verts + 3 * v1, c1);
        rm_camera(cam, verts + 3 * v2, c2);
        const float a0 = c1[0] - c0[0], a1 = c1[1] - c0[1], a2 = c1[2] - c0[2];
        const float b0 = c2[0] - c0[0], b1 = c2[1] - c0[1], b2 = c2[2] - c0[2];
        const float n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
        const float nn = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
        const float ndl = nn == 0.0f ? 0.0f : fabsf((n0 * px + n1 * py) - n2 * z) / (nn * r);
        const float col = ((cam.k * s) * ndl) / r2;
        level = floorf((col < 1.0f ? col : 1.0f) * 255.0f + 0.5f);
    }
    const uint8_t u = (uint8_t)level;
    out_color[3 * i] = u; out_color[3 * i + 1] = u; out_color[3 * i + 2] = u;
}

// dsn_raster_mesh_attr's shade step (the rule of include/dsnerf.h).  face and depth as k_rm_shade writes them; the winner's triangle is
// set up again from the projected vertices (the same integers: the same E_k, area and 1/w as the raster pass saw).
__global__ void __launch_bounds__(RM_THREADS) k_rm_shade_attr(const unsigned long long* __restrict__ vis, const int4* __restrict__ pv,
                                                              const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                              int64_t T, RmCam cam, float intensity, float base,
                                                              const float* __restrict__ vnorm, const float* __restrict__ vcol, int mode,
                                                              int32_t* __restrict__ out_face, float* __restrict__ out_depth,
                                                              uint8_t* __restrict__ out_color, float* __restrict__ out_normal,
                                                              float* __restrict__ out_attr) {
    const int64_t i = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x;
    if (i >= (int64_t)cam.H * cam.W) return;
    const unsigned long long key = vis[i];
    bool hit = key != RM_EMPTY;
    int64_t vi[3] = {0, 0, 0};
    if (hit) {
        const int64_t g = (int64_t)(key & 0xFFFFFFFFull);
        hit = g < T;
        if (hit) {
            vi[0] = faces[3 * g]; vi[1] = faces[3 * g + 1]; vi[2] = faces[3 * g + 2];
            hit = vi[0] >= 0 && vi[1] >= 0 && vi[2] >= 0 && vi[0] < V && vi[1] < V && vi[2] < V;      // (nothing is gathered through a bad index)
        }
    }
    const int32_t f = hit ? (int32_t)(key & 0xFFFFFFFFull) : -1;
    const float z = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
    if (out_face) out_face[i] = f;
    if (out_depth) out_depth[i] = z;
    if (!out_color && !out_normal && !out_attr) return;
    float level[3] = {255.0f, 255.0f, 255.0f};
    float nw[3] = {0.0f, 0.0f, 0.0f}, at[3] = {0.0f, 0.0f, 0.0f};
    RmTri t;
    if (hit && rm_setup(pv, faces, f, V, cam.H, cam.W, t)) {
        const int y = (int)(i / cam.W), x = (int)(i % cam.W);
        // weights b_k = (l_k iw_k) z of P[k]; P = (v0, v2, v1) where the integer area was negative
        const int4 a = pv[vi[0]], b = pv[vi[1]], c = pv[vi[2]];
        if ((int64_t)(b.x - a.x) * (c.y - a.y) - (int64_t)(b.y - a.y) * (c.x - a.x) < 0) { const int64_t s = vi[1]; vi[1] = vi[2]; vi[2] = s; }
        const int64_t cx = 256 * (int64_t)x + 128, cy = 256 * (int64_t)y + 128;
        float bk[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float l = (float)(t.A[k] * cx + t.B[k] * cy + t.C[k]) / t.area;
            bk[k] = (l * t.iw[k]) * z;
        }
        const float xn = (float)(2 * x + 1) / cam.fw - 1.0f, yn = 1.0f - (float)(2 * y + 1) / cam.fh;
        const float px = (xn * z) / cam.fx, py = (yn * z) / cam.fy;
        const float r2 = (px * px + py * py) + z * z;
        const float r = sqrtf(r2);
        float s = (z / r - cam.cos_outer) / (cam.cos_inner - cam.cos_outer);
        s = s > 0.0f ? s : 0.0f;
        s = s < 1.0f ? s : 1.0f;
        s = s * s;
        // the normal in camera space (n, of length nn) and in world space (nw, unit)
        float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, nn = 0.0f;
        bool smooth = (mode & DSN_RM_SMOOTH) != 0;
        if (smooth) {
            float m[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                m[k][0] = vnorm[3 * vi[k]]; m[k][1] = vnorm[3 * vi[k] + 1]; m[k][2] = vnorm[3 * vi[k] + 2];
                const float q = (fabsf(m[k][0]) + fabsf(m[k][1])) + fabsf(m[k][2]);
                smooth = smooth && q > 0.0f && q < __builtin_inff();      // (NaN fails; all three zero fails)
            }
            if (smooth) {
                float u[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) u[e] = (bk[0] * m[0][e] + bk[1] * m[1][e]) + bk[2] * m[2][e];
                const float len = sqrtf((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
                smooth = len > 0.0f && len < __builtin_inff();
                if (smooth) {
                    nw[0] = u[0] / len; nw[1] = u[1] / len; nw[2] = u[2] / len;
                    n0 = (nw[0] * cam.R[0] + nw[1] * cam.R[3]) + nw[2] * cam.R[6];
                    n1 = (nw[0] * cam.R[1] + nw[1] * cam.R[4]) + nw[2] * cam.R[7];
                    n2 = (nw[0] * cam.R[2] + nw[1] * cam.R[5]) + nw[2] * cam.R[8];
                    nn = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
                }
            }
        }
        if (!smooth) {      // the flat rule, from the face's vertices in the order given
            const int64_t g = f;
            float c0[3], c1[3], c2[3];
            rm_camera(cam, verts + 3 * (int64_t)faces[3 * g], c0);
            rm_camera(cam, verts + 3 * (int64_t)faces[3 * g + 1], c1);
            rm_camera(cam, verts + 3 * (int64_t)faces[3 * g + 2], c2);
            const float a0 = c1[0] - c0[0], a1 = c1[1] - c0[1], a2 = c1[2] - c0[2];
            const float b0 = c2[0] - c0[0], b1 = c2[1] - c0[1], b2 = c2[2] - c0[2];
            n0 = a1 * b2 - a2 * b1; n1 = a2 * b0 - a0 * b2; n2 = a0 * b1 - a1 * b0;
            nn = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
            if (nn > 0.0f && nn < __builtin_inff()) {
#pragma unroll
                for (int e = 0; e < 3; ++e) nw[e] = ((cam.R[3 * e] * n0 + cam.R[3 * e + 1] * n1) + cam.R[3 * e + 2] * n2) / nn;
            }
        }
        const float ndl = nn == 0.0f ? 0.0f : fabsf((n0 * px + n1 * py) - n2 * z) / (nn * r);
        float col[3] = {base, base, base};
        if (vcol) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                at[e] = (bk[0] * vcol[3 * vi[0] + e] + bk[1] * vcol[3 * vi[1] + e]) + bk[2] * vcol[3 * vi[2] + e];
                float q = at[e] > 0.0f ? at[e] : 0.0f;          // (NaN: 0)
                col[e] = q < 1.0f ? q : 1.0f;
            }
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            float v = col[e];
            if (!(mode & DSN_RM_UNLIT)) {
                v = ((((col[e] * intensity) / 3.14159265358979323846f) * s) * ndl) / r2;
                v = v < 1.0f ? v : 1.0f;
            }
            level[e] = floorf(v * 255.0f + 0.5f);
        }
    }
    if (out_color) { out_color[3 * i] = (uint8_t)level[0]; out_color[3 * i + 1] = (uint8_t)level[1]; out_color[3 * i + 2] = (uint8_t)level[2]; }
    if (out_normal) { out_normal[3 * i] = nw[0]; out_normal[3 * i + 1] = nw[1]; out_normal[3 * i + 2] = nw[2]; }
    if (out_attr) { out_attr[3 * i] = at[0]; out_attr[3 * i + 1] = at[1]; out_attr[3 * i + 2] = at[2]; }
}

size_t dsn_raster_workspace_size(int64_t V, int64_t T, int H, int W) {
    return 16 * (size_t)V + 8 * (size_t)H * W + 8 + 4 * (size_t)T;
}

void dsn_launch_raster_mesh_attr(const float* verts, int64_t V, const int32_t* faces, int64_t T, const float* pose12, float fx, float fy,
                                 float znear, const float* light4, int H, int W, int32_t* out_face, float* out_depth, uint8_t* out_color,
                                 void* workspace, int phases, int big_pixels, const float* vertex_normals, const float* vertex_colors,
                                 int mode, float* out_normal, float* out_attr, hipStream_t st) {
    RmCam cam;
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) cam.R[3 * i + k] = pose12[4 * i + k];
        cam.t[i] = pose12[4 * i + 3];
    }
    cam.fx = fx; cam.fy = fy; cam.znear = znear;
    cam.fw = (float)W; cam.fh = (float)H;
    cam.half_w = cam.fw * 0.5f; cam.half_h = cam.fh * 0.5f;
    cam.k = (light4[3] * light4[0]) / 3.14159265358979323846f;
    cam.cos_inner = light4[1]; cam.cos_outer = light4[2];
    cam.H = H; cam.W = W;
    const RmWs w = rm_ws(workspace, V, T, H, W);
    const int64_t P = (int64_t)H * W;
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + RM_THREADS - 1) / RM_THREADS)); };
    if (phases & DSN_RM_CLEAR) hipLaunchKernelGGL(k_rm_clear, blocks(P), dim3(RM_THREADS), 0, st, w.vis, P, w.count);
    if ((phases & DSN_RM_PROJECT) && V > 0) hipLaunchKernelGGL(k_rm_project, blocks(V), dim3(RM_THREADS), 0, st, verts, V, cam, w.pv);
    if ((phases & DSN_RM_RASTER) && T > 0)
        hipLaunchKernelGGL(k_rm_raster, blocks(T), dim3(RM_THREADS), 0, st, w.pv, V, faces, T, H, W, big_pixels, w.vis, w.count, w.list);
    if ((phases & DSN_RM_RASTER_BIG) && T > 0) {
        const int64_t nb = (T + RM_WAVES - 1) / RM_WAVES;
        hipLaunchKernelGGL(k_rm_raster_big, dim3((unsigned)(nb < RM_BIG_BLOCKS ? nb : RM_BIG_BLOCKS)), dim3(RM_THREADS), 0, st, w.pv, V,
                           faces, T, H, W, w.vis, w.count, w.list);
    }
    if (!(phases & DSN_RM_SHADE)) return;
    if (!vertex_normals && !vertex_colors && !mode && !out_normal && !out_attr)
        hipLaunchKernelGGL(k_rm_shade, blocks(P), dim3(RM_THREADS), 0, st, w.vis, verts, V, faces, T, cam, out_face, out_depth, out_color);
    else
        hipLaunchKernelGGL(k_rm_shade_attr, blocks(P), dim3(RM_THREADS), 0, st, w.vis, w.pv, verts, V, faces, T, cam, light4[0], light4[3],
                           vertex_normals, vertex_colors, mode, out_face, out_depth, out_color, out_normal, out_attr);
}

void dsn_launch_raster_mesh(const float* verts, int64_t V, const int32_t* faces, int64_t T, const float* pose12, float fx, float fy,
                            float znear, const float* light4, int H, int W, int32_t* out_face, float* out_depth, uint8_t* out_color,
                            void* workspace, int phases, int big_pixels, hipStream_t st) {
    dsn_launch_raster_mesh_attr(verts, V, faces, T, pose12, fx, fy, znear, light4, H, W, out_face, out_depth, out_color, workspace, phases,
                                big_pixels, nullptr, nullptr, 0, nullptr, nullptr, st);
}
