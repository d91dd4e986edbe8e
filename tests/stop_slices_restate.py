"""Front-to-back ray termination (DSN_EARLY_STOP, csrc/dsn_geom.hip) restated on the host: the transmittance T of every ray at the
start of every slice as an INTERVAL [T_lo, T_hi] that contains the device's value, and from it the decision "this ray gets no more
density" as certainly dead / certainly alive / undetermined.  Plain numpy; the only thing taken from the library is the threshold
(dsn_early_stop_eps_scaled, through the C ABI).  Pinned by tests/test_stop_slices_host.py before test_gpu_stop_slices.py judges the
kernels by it.

Why not float64.  The kernels compute, per sample, alpha = 1 - expf(-sigma dist) and fac = (1 - alpha) + 1e-10f in float32.  For a
strongly absorbing sample (expf below about 2^-18) 1 - alpha comes out in steps of 2^-24, and once expf < 2^-25 alpha rounds to 1 and
fac is exactly 1e-10f - the exact product is smaller by orders of magnitude.  So the float32 arithmetic is restated operation by
operation (numpy float32 arithmetic rounds every operation to nearest, as the kernels do: they are built with -ffp-contract=off):

    sg    = 0 where the sample is transparent, or sigma is NaN or <= 0          (dsn_slice_factor, k_advance_T, k_stop_stats)
    dist  = (z[i + 1] - z[i]) * |d|,  1e10f * |d| for the last sample
    arg   = sg * dist,  e = expf(-arg)
    alpha = 1 - e,  fac = (1 - alpha) + 1e-10f
    slice order:   P = ((1 f0) f1) ... over the samples of ONE slice, then T = T * P      (dsn_slice_factor, k_advance_T)
    running order: t = t * fac, sample by sample                                          (k_stop_stats)

Two things may differ between device and host:

  * |d|.  Device: sqrtf(fmaf(z, z, fmaf(y, y, x * x))) - three roundings of positive terms, at most 3 u relative on the sum of squares
    (u = 2^-24, the unit roundoff), halved by the square root to 1.5 u, plus the square root's own rounding, granted 1 ulp = 2 u:
    3.5 u.  Host: the float64 norm rounded once to float32, 1 u.  |d|_device = |d|_host (1 + a), |a| <= 4.5 u, taken as 5 u.
    dist and arg are each one more rounded product on either side (2 u each for the pair): arg_device = arg_host (1 + b),
    |b| <= 5 u + 2 u + 2 u = 9 u, taken as 10 u.  exp(-arg (1 + b)) = exp(-arg) exp(-arg b): a RELATIVE change of e by 10 u |arg|.
  * expf.  The device's expf is documented at 1 ulp = 2 u relative; granted 2 ulp = 4 u.  The host evaluates exp in float64 (error
    2^-53, nothing beside these).

Together e_device lies in e_host (1 -+ m) with m = (4 + 10 |arg|) u = (2 + 5 |arg|) 2^-23 (M_ULP, M_ARG).  The interval's ends are
rounded to float32 OUTWARDS (nextafter), so the cast costs nothing of m.  Where arg == 0 (transparent, sigma <= 0 or NaN) the device has
e = expf(-0) = 1 exactly whatever |d| is: both ends are 1, and everywhere e_hi <= 1 (arg >= 0: a rounded exp of a non-positive number does
not exceed 1).  Very small e needs no care: below 2^-25 the factor is 1e-10f whether the device flushes a denormal or not.

float32 rounding is monotone, so fac is non-decreasing in e, and a product of non-negative factors taken in a fixed order is
non-decreasing in each of them: evaluating the SAME sequence of float32 operations at e_lo and at e_hi gives T_lo <= T_device <= T_hi.

Decisions ("dead" = T below eps at the start of a slice, the kernels' `T < eps`):
    certainly dead:   T_hi < eps            certainly alive:   not (T_lo < eps)            anything else: undetermined
"""
import numpy as np

F = np.float32
M_ULP, M_ARG = 2.0, 5.0          # m = (M_ULP + M_ARG |arg|) 2^-23: see the derivation above
STEP = 2.0 ** -23
MAX_SLICES = 32                  # = DSN_STOP_MAX_SLICES

# The slicings test_gpu_stop_slices.py runs (and test_stop_slices_host.py runs the restatement alone on): (S, "uniform", value of
# DSN_STOP_SLICE) or (S, "schedule", slice lengths).  Uniform 1 needs S <= 32 (at most 32 slices); 100 = 12 x 8 + 4 = 6 x 16 + 4 = 64 + 36
# and 64 = 21 x 3 + 1 = 12 x 5 + 4 end in a ragged slice; 128 / 8 gives K = 16.
SCHEDULES = [[1, 2, 3, 5, 8, 13, 16, 16], [33, 31], [17, 15, 32], [63, 1], [64]]
SLICINGS = ([(64, "uniform", L) for L in (3, 4, 5, 8, 16, 64)] + [(64, "schedule", s) for s in SCHEDULES]
            + [(24, "uniform", 1), (24, "uniform", 5), (100, "uniform", 8), (100, "uniform", 16), (100, "uniform", 64),
               (128, "uniform", 8), (128, "uniform", 5), (128, "uniform", 64)])
LIST_MODE_SLICINGS = [(64, "uniform", 3), (64, "uniform", 4), (64, "uniform", 8), (100, "uniform", 8)]      # DSN_STOP_ADVANCE=list


def slicing_id(sl):
    S, kind, v = sl
    return f"S{S}-L{v}" if kind == "uniform" else f"S{S}-" + "_".join(str(x) for x in v)


def eps_scaled(S, colour_scale):
    """the threshold the kernels use: dsn_early_stop_eps_scaled(S, colour scale), from the library (no GPU needed)"""
    import ctypes as C
    import dsnerf_amd
    lib = dsnerf_amd._lib.lib()
    lib.dsn_early_stop_eps_scaled.restype = C.c_float
    return F(lib.dsn_early_stop_eps_scaled(int(S), C.c_float(float(colour_scale))))


def uniform_len(L, S):
    """dsn_slice_len for DSN_STOP_SLICE = L: clipped to 1 .. 64, and longer where S / L would exceed 32 slices"""
    L = 8 if L < 1 else min(int(L), 64)
    return L if -(-S // L) <= MAX_SLICES else -(-S // MAX_SLICES)


def stats_len(L, S):
    """dsn_stats_slice_len: the histogram's slices are half the uniform ones where that keeps K <= 32"""
    half = L // 2 if L >= 2 else L
    return half if -(-S // half) <= MAX_SLICES else L


def bounds_of(S, kind, v):
    """slice borders b[0 .. K]: slice k = samples [b[k], b[k + 1])"""
    if kind == "uniform":
        L = uniform_len(v, S)
        return [min(k * L, S) for k in range(-(-S // L) + 1)]
    b = [0]
    for n in v:
        assert 1 <= n <= 64
        b.append(b[-1] + int(n))
    assert b[-1] == S and len(v) <= MAX_SLICES
    return b


def advance_variant(n):
    """the G of k_advance_T<G> that dsn_launch_advance_T picks for a slice of n samples"""
    return next(G for G in (1, 2, 4, 8, 16, 32, 64) if n <= G or G == 64)


def variants_of(bounds):
    """the variants a frame with these borders launches: slice k - 1 is advanced in front of slice k, the last slice never"""
    return {advance_variant(bounds[k + 1] - bounds[k]) for k in range(len(bounds) - 2)}


def factors(sigma, transparent, z_vals, ray_d, widen=1.0):
    """per-sample factors (1 - alpha) + 1e-10f as float32 [R, S]: (lo, nominal, hi), and arg.  widen scales m."""
    z = np.asarray(z_vals, F)
    R, S = z.shape
    sg = np.asarray(sigma, F).reshape(R, S)
    tr = np.asarray(transparent).reshape(R, S).astype(bool)
    sg = np.where(tr | ~(sg > 0), F(0), sg)                      # (NaN > 0 is false: a flagged density counts as 0)
    dn = np.sqrt((np.asarray(ray_d, np.float64) ** 2).sum(-1)).astype(F)
    dist = np.empty((R, S), F)
    dist[:, :-1] = (z[:, 1:] - z[:, :-1]) * dn[:, None]
    dist[:, -1] = F(1e10) * dn
    arg = sg * dist
    assert arg.dtype == F and dist.dtype == F
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a64 = arg.astype(np.float64)
        e64 = np.exp(-a64)
        m = float(widen) * (M_ULP + M_ARG * a64) * STEP
        e_nom = e64.astype(F)
        e_lo = np.nextafter((e64 * np.maximum(1.0 - m, 0.0)).astype(F), F(-np.inf))
        e_hi = np.nextafter((e64 * (1.0 + m)).astype(F), F(np.inf))
    e_lo = np.maximum(e_lo, F(0))
    e_hi = np.minimum(e_hi, F(1))
    zero = arg == 0
    e_lo[zero] = e_hi[zero] = e_nom[zero] = F(1)

    def fac(e):
        alpha = F(1) - e
        return (F(1) - alpha) + F(1e-10)

    out = fac(e_lo), fac(e_nom), fac(e_hi)
    assert all(o.dtype == F for o in out)
    return out + (arg,)


def slice_order(fac, bounds):
    """T at the start of every slice (and behind the last: column K), [R, K + 1] float32, P per slice from 1.0f, then T * P"""
    R = fac.shape[0]
    T = np.ones(R, F)
    cols = [T]
    for k in range(len(bounds) - 1):
        P = np.ones(R, F)
        for i in range(bounds[k], bounds[k + 1]):
            P = P * fac[:, i]
        T = T * P
        cols.append(T)
    out = np.stack(cols, 1)
    assert out.dtype == F
    return out


def running_order(fac, bounds):
    """the same in k_stop_stats' order: t = t * fac sample by sample"""
    R, S = fac.shape
    t = np.ones(R, F)
    at = {b: None for b in bounds}
    for i in range(S):
        if i in at:
            at[i] = t
        t = t * fac[:, i]
    at[S] = t
    out = np.stack([at[b] for b in bounds], 1)
    assert out.dtype == F
    return out


def decide(T_lo, T_hi, eps):
    eps = F(eps)
    dead = T_hi < eps
    alive = ~(T_lo < eps)
    return dead, alive, ~dead & ~alive


def restate(sigma, transparent, z_vals, ray_d, bounds, eps, widen=1.0, order="slice"):
    """everything about one frame and one slicing: T_lo / T_nom / T_hi [R, K + 1], dead / alive / undetermined [R, K] at the start of each
    slice, nt [R, K] = non-transparent samples per ray and slice, m_max = the largest m that mattered (arg below 40)"""
    lo, nom, hi, arg = factors(sigma, transparent, z_vals, ray_d, widen)
    run = slice_order if order == "slice" else running_order
    T_lo, T_nom, T_hi = run(lo, bounds), run(nom, bounds), run(hi, bounds)
    K = len(bounds) - 1
    dead, alive, undet = decide(T_lo[:, :K], T_hi[:, :K], eps)
    R, S = arg.shape
    live = ~np.asarray(transparent).reshape(R, S).astype(bool)
    nt = np.stack([live[:, bounds[k]:bounds[k + 1]].sum(1) for k in range(K)], 1).astype(np.int64)
    small = arg[arg < 40]
    m_max = float(widen) * (M_ULP + M_ARG * float(small.max() if small.size else 0.0)) * STEP
    return {"T_lo": T_lo, "T_nom": T_nom, "T_hi": T_hi, "dead": dead, "alive": alive, "undet": undet, "nt": nt, "bounds": list(bounds),
            "eps": F(eps), "m_max": m_max}


def counts(res):
    """figures of a restated frame: rays that certainly terminate, certainly-dead / undetermined decisions (ray, slice), and the
    non-transparent samples they hold (what the `skipped` counter counts)"""
    dead, undet, nt = res["dead"], res["undet"], res["nt"]
    return {"terminated_rays": int(dead.any(1).sum()), "dead_decisions": int(dead.sum()), "undetermined": int(undet.sum()),
            "skipped_certain": int(nt[dead].sum()), "skipped_undetermined": int(nt[undet].sum())}


def stop_stats(sigma, transparent, z_vals, ray_d, S, L_uniform, L_hist, eps, widen=1.0):
    """what a DSN_STOP_STATS frame records (k_stop_stats, running order): would_skip as (certain, undetermined) by uniform slices of
    L_uniform, and the histogram at its own slice length: hist[g][k] = non-transparent samples of slice k on rays whose first dead slice
    is g (g = K: never) as (hist of the rays whose g is certain, list of (g_first, g_last, per-slice samples) for the others)"""
    bu = bounds_of(S, "uniform", L_uniform)
    ru = restate(sigma, transparent, z_vals, ray_d, bu, eps, widen, order="running")
    would = (int(ru["nt"][ru["dead"]].sum()), int(ru["nt"][ru["undet"]].sum()))
    bh = [min(k * L_hist, S) for k in range(-(-S // L_hist) + 1)]
    rh = restate(sigma, transparent, z_vals, ray_d, bh, eps, widen, order="running")
    K = len(bh) - 1
    first = lambda below: np.where(below.any(1), below.argmax(1), K)       # noqa: E731
    g_late, g_early = first(rh["dead"]), first(~rh["alive"])               # T_hi < eps at the latest, T_lo < eps at the earliest
    hist = np.zeros((K + 1, K), np.int64)
    sure = g_late == g_early
    np.add.at(hist, g_late[sure], rh["nt"][sure])
    open_rays = [(int(g_early[r]), int(g_late[r]), rh["nt"][r]) for r in np.nonzero(~sure)[0]]
    return would, hist, open_rays


def unshaded(sigma, weights, eps):
    """the samples k_cull_lit leaves unshaded (colour 0): density positive and compositing weight below eps; a NaN of either keeps the sample"""
    sg = np.asarray(sigma, F).reshape(-1)
    w = np.asarray(weights, F).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (sg > 0) & (w < F(eps))


def gap_rays(transparent, bounds, R, S):
    """rays with non-transparent samples in some slice, none in at least one whole slice behind it, and some again later: in list mode
    (DSN_STOP_ADVANCE=list) their transmittance catches up over the slices they had no entry in"""
    live = ~np.asarray(transparent).reshape(R, S).astype(bool)
    has = np.stack([live[:, bounds[k]:bounds[k + 1]].any(1) for k in range(len(bounds) - 1)], 1)
    seen = np.maximum.accumulate(has, 1)
    later = np.maximum.accumulate(has[:, ::-1], 1)[:, ::-1]
    return int((seen & ~has & later).any(1).sum())


def resample(sigma, transparent, z_vals, S):
    """golden rays (64 samples) brought to S samples for the host-only test: z interpolated in float32, sigma / transparent taken from
    the nearest earlier sample - rays of the same character, not the reference's rays"""
    z = np.asarray(z_vals, F)
    R, S0 = z.shape
    if S == S0:
        return np.asarray(sigma, F).reshape(R, S0), np.asarray(transparent).reshape(R, S0).astype(bool), z
    t = np.arange(S, dtype=np.float64) * (S0 - 1) / (S - 1)
    i0 = np.minimum(t.astype(np.int64), S0 - 2)
    w = (t - i0).astype(F)
    zs = (z[:, i0] * (F(1) - w) + z[:, i0 + 1] * w).astype(F)
    zs = np.maximum.accumulate(zs, 1)
    near = np.minimum(np.floor(t + 0.5).astype(np.int64), S0 - 1)
    return np.asarray(sigma, F).reshape(R, S0)[:, near], np.asarray(transparent).reshape(R, S0).astype(bool)[:, near], zs
