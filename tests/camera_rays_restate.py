"""numpy restatement of csrc/dsn_rays.h, pixel by pixel and operation for operation: dsn_pixel_ray_zju and dsn_pixel_ray_h36m.

Every pixel is computed on its own (the arrays below only carry many pixels through the same elementwise operations): K^-1 by the
adjugate, every sum in the association the header writes, float64 and float32 exactly where the header has them, one rounding per
operation.  No linalg.inv, no matmul, no BLAS: nothing here can reorder a sum.  The library is built with -ffp-contract=off and IEEE
division and square root, so these are expected to be the device's words (tests/test_gpu_camera_rays.py).

rays(...)      K, R, T, bounds, H, W -> (ray_o [n,3] f32, ray_d [n,3] f32, near [n] f32, far [n] f32, mask [n] bool), near = far = 0
               where the ray misses the box, as the device writes them
near_far(...)  the box part alone, from given float32 rays

variant= names a mutant (tests/test_camera_rays_host.py shows each one moves a named check on a named camera):
  "at_least_two"   zju: a ray counts when it meets two or more planes, not exactly two
  "signed_t"       zju: near / far from the signed plane parameter instead of the distance |p - o| / |d|
  "no_pad"         zju: the box is not padded by 0.01
  "no_clamp"       h36m: the two +-1e-5 clamps left out
  "clamp_swapped"  h36m: the two clamps in the other order
  "fmin_fmax"      h36m: min / max that drop a NaN operand (C's fminf / fmaxf) in the place of numpy's, which keep it
"""
import numpy as np

ZJU, H36M = "zju", "h36m"
_IGNORE = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def _f64(a, n):
    a = np.asarray(a, np.float64).reshape(-1)
    assert a.size == n
    return a


def _adjugate_inverse(K):
    k00, k01, k02, k10, k11, k12, k20, k21, k22 = (np.float64(v) for v in K)
    det = k00 * (k11 * k22 - k12 * k21) - k01 * (k10 * k22 - k12 * k20) + k02 * (k10 * k21 - k11 * k20)
    inv_det = np.float64(1.0) / det
    return [(k11 * k22 - k12 * k21) * inv_det, (k02 * k21 - k01 * k22) * inv_det, (k01 * k12 - k02 * k11) * inv_det,
            (k12 * k20 - k10 * k22) * inv_det, (k00 * k22 - k02 * k20) * inv_det, (k02 * k10 - k00 * k12) * inv_det,
            (k10 * k21 - k11 * k20) * inv_det, (k01 * k20 - k00 * k21) * inv_det, (k00 * k11 - k01 * k10) * inv_det]


def _origin_and_direction(K, R, T, W, p):
    """float64: o [3] (scalars) and pixel_world - o per pixel ([3] arrays over p)"""
    Ki = _adjugate_inverse(K)
    o = [-(R[0 * 3 + c] * T[0] + R[1 * 3 + c] * T[1] + R[2 * 3 + c] * T[2]) for c in range(3)]
    i = (p % W).astype(np.float32).astype(np.float64)
    j = (p // W).astype(np.float32).astype(np.float64)
    pc = [i * Ki[c * 3 + 0] + j * Ki[c * 3 + 1] + Ki[c * 3 + 2] for c in range(3)]
    pw = [(pc[0] - T[0]) * R[0 * 3 + c] + (pc[1] - T[1]) * R[1 * 3 + c] + (pc[2] - T[2]) * R[2 * 3 + c] for c in range(3)]
    return o, [pw[c] - o[c] for c in range(3)]


def _near_far_zju(of, df, bounds, variant):
    """of, df: [3] lists of float32 arrays over the pixels; bounds float64 [6]"""
    ro = [v.astype(np.float64) for v in of]
    rd = [v.astype(np.float64) for v in df]
    pad = 0.0 if variant == "no_pad" else 0.01
    b = [[bounds[c] + (-pad) for c in range(3)], [bounds[3 + c] + pad for c in range(3)]]
    eps = 1e-6
    n = ro[0].shape
    hits = np.zeros(n, np.int64)
    dsel = [np.zeros(n, np.float64), np.zeros(n, np.float64)]
    for s in range(2):
        for c in range(3):
            dint = (b[s][c] - ro[c]) / rd[c]
            px, py, pz = dint * rd[0] + ro[0], dint * rd[1] + ro[1], dint * rd[2] + ro[2]
            inside = ((px >= b[0][0] - eps) & (px <= b[1][0] + eps) & (py >= b[0][1] - eps) & (py <= b[1][1] + eps) &
                      (pz >= b[0][2] - eps) & (pz <= b[1][2] + eps))
            if variant == "signed_t":
                dist = dint
            else:
                ex, ey, ez = px - ro[0], py - ro[1], pz - ro[2]
                dist = np.sqrt(ex * ex + ey * ey + ez * ez)
            for k in range(2):
                take = inside & (hits == k)
                dsel[k] = np.where(take, dist, dsel[k])
            hits = hits + inside
    m = hits >= 2 if variant == "at_least_two" else hits == 2
    if variant == "signed_t":
        d0, d1 = dsel
    else:
        nr = np.sqrt((df[0] * df[0] + df[1] * df[1]) + df[2] * df[2]).astype(np.float64)      # float32 norm, then widened
        d0, d1 = dsel[0] / nr, dsel[1] / nr
    near = np.where(m, np.fmin(d0, d1).astype(np.float32), np.float32(0.0))
    far = np.where(m, np.fmax(d0, d1).astype(np.float32), np.float32(0.0))
    return near.astype(np.float32), far.astype(np.float32), m


def _near_far_h36m(of, df, bounds, variant):
    """float32 throughout.  of: the first ray's origin ([3] float32 scalars or arrays); df: [3] float32 arrays"""
    f32 = np.float32
    nrm = np.sqrt((df[0] * df[0] + df[1] * df[1]) + df[2] * df[2])
    lo_f, hi_f = (np.fmin, np.fmax) if variant == "fmin_fmax" else (np.minimum, np.maximum)
    tn = np.full(df[0].shape, -np.inf, f32)
    tf = np.full(df[0].shape, np.inf, f32)
    for c in range(3):
        v = df[c] / nrm
        first = lambda v: np.where((v < f32(1e-5)) & (v > f32(-1e-10)), f32(1e-5), v)
        second = lambda v: np.where((v > f32(-1e-5)) & (v < f32(1e-10)), f32(-1e-5), v)
        if variant == "clamp_swapped":
            v = first(second(v))
        elif variant != "no_clamp":
            v = second(first(v))
        bmin, bmax = f32(bounds[c]), f32(bounds[3 + c])
        a, b = (bmin - of[c]) / v, (bmax - of[c]) / v
        tn = hi_f(tn, lo_f(a, b))
        tf = lo_f(tf, hi_f(a, b))
    m = tn < tf
    near = np.where(m, tn / nrm, f32(0.0)).astype(f32)
    far = np.where(m, tf / nrm, f32(0.0)).astype(f32)
    return near, far, m


def rays(K, R, T, bounds, H, W, convention=ZJU, variant=None, pixels=None):
    """the five whole-image arrays of dsn_camera_rays (or those of `pixels`, flat indices row * W + column)"""
    assert convention in (ZJU, H36M)
    K, R, T, bounds = _f64(K, 9), _f64(R, 9), _f64(T, 3), _f64(bounds, 6)
    p = np.arange(H * W, dtype=np.int64) if pixels is None else np.asarray(pixels, np.int64).reshape(-1)
    with np.errstate(**_IGNORE):
        o, dd = _origin_and_direction(K, R, T, W, p)
        if convention == H36M:
            nd = np.sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2])
            dd = [dd[c] / nd for c in range(3)]
        of = [np.full(p.shape, np.float32(o[c]), np.float32) for c in range(3)]
        df = [dd[c].astype(np.float32) for c in range(3)]
        near, far, m = (_near_far_h36m if convention == H36M else _near_far_zju)(of, df, bounds, variant)
    return np.stack(of, 1), np.stack(df, 1), near, far, m


def near_far(ray_o, ray_d, bounds, convention=ZJU, variant=None):
    """near, far (0 where the ray misses) and mask from given float32 rays [n,3]; h36m: against the first ray's origin"""
    ray_o, ray_d = np.asarray(ray_o), np.asarray(ray_d)
    assert ray_o.dtype == np.float32 and ray_d.dtype == np.float32 and convention in (ZJU, H36M)
    bounds = _f64(bounds, 6)
    df = [np.ascontiguousarray(ray_d[:, c]) for c in range(3)]
    with np.errstate(**_IGNORE):
        if convention == H36M:
            return _near_far_h36m([ray_o[0, c] for c in range(3)], df, bounds, variant)
        return _near_far_zju([np.ascontiguousarray(ray_o[:, c]) for c in range(3)], df, bounds, variant)
