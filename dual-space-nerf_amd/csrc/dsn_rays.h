// dsn_rays.h - the per-pixel bodies of the camera-ray kernels, shared by the whole-image kernels of dsn_geom.hip
// (dsn_camera_rays) and the training-batch sampler of dsn_sample.hip (dsn_train_rays): one text, so a drawn pixel carries the bits
// the whole-image call writes for it.
#pragma once
#include "dsn_common.h"

struct DsnPixelRay {
    float o[3], d[3];
    float near, far;      // 0 where the ray misses the box
    bool hit;             // mask_at_box
};

// utils/rays_utils.py:16-30 get_rays, :63-97 get_near_far as used by my_sample_ray(nrays<=0), :176-184.
// The reference does this in float64 numpy on the CPU and casts to float32: rays are produced in double,
// ROUNDED to float32 (:177-178), and the slab intersections are evaluated in double FROM THE ROUNDED rays (:179);
// the same order is kept here so that results are the reference's to the last float32 bit (up to BLAS summation order
// in the 1e-16 range).  K^-1 by the adjugate.  p = row * W + column.
__device__ __forceinline__ DsnPixelRay dsn_pixel_ray_zju(const double* __restrict__ K, const double* __restrict__ Rm,
                                                         const double* __restrict__ T, const double* __restrict__ bounds, int W, int p) {
    DsnPixelRay out;
    const double k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5], k20 = K[6], k21 = K[7], k22 = K[8];
    const double det = k00 * (k11 * k22 - k12 * k21) - k01 * (k10 * k22 - k12 * k20) + k02 * (k10 * k21 - k11 * k20);
    const double id = 1.0 / det;
    const double Ki[9] = {(k11 * k22 - k12 * k21) * id, (k02 * k21 - k01 * k22) * id, (k01 * k12 - k02 * k11) * id,
                          (k12 * k20 - k10 * k22) * id, (k00 * k22 - k02 * k20) * id, (k02 * k10 - k00 * k12) * id,
                          (k10 * k21 - k11 * k20) * id, (k01 * k20 - k00 * k21) * id, (k00 * k11 - k01 * k10) * id};
    // rays_o = -R^T T
    double o[3];
    for (int c = 0; c < 3; ++c) o[c] = -(Rm[0 * 3 + c] * T[0] + Rm[1 * 3 + c] * T[1] + Rm[2 * 3 + c] * T[2]);
    const double i = (double)(float)(p % W), j = (double)(float)(p / W);
    double pc[3], pw[3];
    for (int c = 0; c < 3; ++c) pc[c] = i * Ki[c * 3 + 0] + j * Ki[c * 3 + 1] + Ki[c * 3 + 2];   // xy1 . Kinv^T
    for (int c = 0; c < 3; ++c)
        pw[c] = (pc[0] - T[0]) * Rm[0 * 3 + c] + (pc[1] - T[1]) * Rm[1 * 3 + c] + (pc[2] - T[2]) * Rm[2 * 3 + c];   // (pc - T) . R
    float of[3], df[3];
    for (int c = 0; c < 3; ++c) { of[c] = (float)o[c]; df[c] = (float)(pw[c] - o[c]); }
    for (int c = 0; c < 3; ++c) { out.o[c] = of[c]; out.d[c] = df[c]; }
    // get_near_far on the float32-rounded rays, in double
    const double ro[3] = {(double)of[0], (double)of[1], (double)of[2]}, rd[3] = {(double)df[0], (double)df[1], (double)df[2]};
    double b[2][3];
    for (int c = 0; c < 3; ++c) { b[0][c] = bounds[c] + (-0.01); b[1][c] = bounds[3 + c] + 0.01; }
    const double eps = 1e-6;
    int hits = 0;
    double dsel[2] = {0.0, 0.0};
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 3; ++c) {   // plane order of the reference's reshape(-1, 6): min xyz, then max xyz
            const double dint = (b[s][c] - ro[c]) / rd[c];
            const double px = dint * rd[0] + ro[0], py = dint * rd[1] + ro[1], pz = dint * rd[2] + ro[2];
            const bool in = (px >= b[0][0] - eps) && (px <= b[1][0] + eps) && (py >= b[0][1] - eps) && (py <= b[1][1] + eps) &&
                            (pz >= b[0][2] - eps) && (pz <= b[1][2] + eps);
            if (in) {
                if (hits < 2) {
                    const double ex = px - ro[0], ey = py - ro[1], ez = pz - ro[2];
                    dsel[hits] = sqrt(ex * ex + ey * ey + ez * ez);
                }
                ++hits;
            }
        }
    const bool m = hits == 2;   // "intersect exactly twice" (:86)
    // np.linalg.norm on the float32 rays stays in float32 (:92): sqrt((x*x + y*y) + z*z), unfused
    const double nr = (double)sqrtf((df[0] * df[0] + df[1] * df[1]) + df[2] * df[2]);
    const double d0 = dsel[0] / nr, d1 = dsel[1] / nr;
    out.hit = m;
    out.near = m ? (float)fmin(d0, d1) : 0.0f;
    out.far = m ? (float)fmax(d0, d1) : 0.0f;
    return out;
}

// Human3.6M convention (utils/h36m_utils.py:14-28 get_rays, :61-76 get_near_far, composed by get_rays_within_bounds
// :162-176 / the test split of sample_ray_h36m :147-157): the direction is NORMALISED in float64 before the cast to
// float32 (:26), and the box test is the float32 slab test on the unit direction with the reference's +-1e-5 clamp of
// near-zero components (:64-66), against the FIRST ray's origin (ray_o[:1], :67-68) and the UNPADDED float32 bounds;
// near / far are divided by the float32 norm of the (already unit) direction (:74-75).  All of get_near_far is float32
// numpy: one rounding per operation, kept here (-ffp-contract=off).
__device__ __forceinline__ DsnPixelRay dsn_pixel_ray_h36m(const double* __restrict__ K, const double* __restrict__ Rm,
                                                          const double* __restrict__ T, const double* __restrict__ bounds, int W, int p) {
    DsnPixelRay out;
    const double k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5], k20 = K[6], k21 = K[7], k22 = K[8];
    const double det = k00 * (k11 * k22 - k12 * k21) - k01 * (k10 * k22 - k12 * k20) + k02 * (k10 * k21 - k11 * k20);
    const double id = 1.0 / det;
    const double Ki[9] = {(k11 * k22 - k12 * k21) * id, (k02 * k21 - k01 * k22) * id, (k01 * k12 - k02 * k11) * id,
                          (k12 * k20 - k10 * k22) * id, (k00 * k22 - k02 * k20) * id, (k02 * k10 - k00 * k12) * id,
                          (k10 * k21 - k11 * k20) * id, (k01 * k20 - k00 * k21) * id, (k00 * k11 - k01 * k10) * id};
    double o[3];
    for (int c = 0; c < 3; ++c) o[c] = -(Rm[0 * 3 + c] * T[0] + Rm[1 * 3 + c] * T[1] + Rm[2 * 3 + c] * T[2]);
    const double i = (double)(float)(p % W), j = (double)(float)(p / W);
    double pc[3], pw[3], dd[3];
    for (int c = 0; c < 3; ++c) pc[c] = i * Ki[c * 3 + 0] + j * Ki[c * 3 + 1] + Ki[c * 3 + 2];
    for (int c = 0; c < 3; ++c)
        pw[c] = (pc[0] - T[0]) * Rm[0 * 3 + c] + (pc[1] - T[1]) * Rm[1 * 3 + c] + (pc[2] - T[2]) * Rm[2 * 3 + c];
    for (int c = 0; c < 3; ++c) dd[c] = pw[c] - o[c];
    const double nd = sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]);       // np.linalg.norm(axis=2) in float64 (:26)
    float of[3], df[3];
    for (int c = 0; c < 3; ++c) { of[c] = (float)o[c]; df[c] = (float)(dd[c] / nd); }
    for (int c = 0; c < 3; ++c) { out.o[c] = of[c]; out.d[c] = df[c]; }
    // get_near_far (:61-76), float32 throughout
    const float nrm = sqrtf((df[0] * df[0] + df[1] * df[1]) + df[2] * df[2]);
    float tn = -INFINITY, tf = INFINITY;
    bool nan = false;     // np.minimum / np.max keep a NaN where fminf / fmaxf drop it: the reference's near < far is then False
    for (int c = 0; c < 3; ++c) {
        float v = dsn_div(df[c], nrm);
        if (v < 1e-5f && v > -1e-10f) v = 1e-5f;          // the two clamps in the reference's order (:65-66)
        if (v > -1e-5f && v < 1e-10f) v = -1e-5f;
        const float bmin = (float)bounds[c], bmax = (float)bounds[3 + c];
        const float a = dsn_div(bmin - of[c], v), b = dsn_div(bmax - of[c], v);   // ray_o[:1]: every ray shares the camera origin
        nan = nan || a != a || b != b;
        tn = fmaxf(tn, fminf(a, b));
        tf = fminf(tf, fmaxf(a, b));
    }
    const bool m = !nan && tn < tf;
    out.hit = m;
    out.near = m ? dsn_div(tn, nrm) : 0.0f;
    out.far = m ? dsn_div(tf, nrm) : 0.0f;
    return out;
}
