"""The float margins of the nearest-face list build, restated on the host, and cases that need them (test infrastructure,
imported by tests/test_nn_margins_host.py and tests/test_gpu_nn_margins.py).

The list of a cell B (csrc/dsn_nn.hip) holds face f when  dmin(B, c_f)^2 <= U(B)^2 (1 + 1e-5) + 1e-12  (dsn_in_list), where B is the
cell's box grown by DSN_GRID_GUARD = 1e-4 m on every side (dsn_cell_box) and U(B)^2 = min_g dmax(B, c_g)^2.  The search is exact only
because of these margins: (int)((p - lo) * inv_cell) puts float32 points into a cell that lie outside the cell's own box
lo + ix * cell .. lo + (ix + 1) * cell by an ulp or two of the coordinate.

Restatement (plain numpy float32, no GPU).  grid_header() restates k_grid_params (the level's geometry from the centroids; the cell
size itself is taken from recorded device headers, see device_headers);
restate_cell() restates dsn_cell_box, dsn_box_dmin2, dsn_box_dmax2 and dsn_in_list with `guard`, `rel`, `abs` as parameters.  The
library is built with -ffp-contract=off (build.py: "part of the numerical contract"), and the cell index (nn_cases.cell_of) and the
box edges lo + ix * cell are restated on that footing: one rounding per operation.  The sums dx*dx + dy*dy + dz*dz of dmin^2 and
dmax^2 and the threshold u2 * (1 + rel) + abs do not lean on it: each is evaluated with and without every fma a contracting compiler
could form (two in a sum, one in the threshold), and the lowest and highest results bracket dmin^2, U^2 and the threshold.
A face is then CERTAINLY IN (highest dmin^2 <= lowest threshold), CERTAINLY OUT (lowest dmin^2 > highest threshold) or
undetermined - the three-way decision of tests/stop_slices_restate.py.  d2() restates dsn_d2 exactly (dx*dx, fmaf, fmaf: the fmas are
written in the source), with a correctly rounded float32 fma.

Cases (margin_case): the body of synth.make_body() (uniform, and nonuniform=True) with PROBE PAIRS appended: two triangles (c_g, c*)
per probe cell on vertices of their own, in the posed mesh for the world levels and in the canonical mesh for the canonical ones; in
the other space a probe face copies the vertices of a body face (its centroid there ties with that face's and loses: a higher index).
All probe centroids lie strictly inside the body's centroid box, so the four grids are those of the placeholder mesh (asserted).
Per probe cell B, picked where no body centroid is near and at least 4 cells from every other probe cell:

  * p: per axis the first float32 of the cell (nn_cases.boundary on the lower plane) or the last one (one ulp below the upper plane's
    boundary), whichever lies further OUTSIDE the unguarded box; the axis with the largest excursion is the crossed axis.
  * c_g: the face that attains U(B), placed so that p's corner is its farthest corner: just beyond the opposite corner ("diag",
    U = the cell's diagonal) or just off the cell's centre ("centre", U = half the diagonal).
  * c*: outside the cell, on the crossed axis, at U0 (1 + rel) from p's corner (U0 from the unguarded box and the centroid c_g actually
    has).  The true distance of p is shorter by the excursion, p's distance to c_g longer: c* is p's nearest face, yet
    dmin(B, c*) > U(B) without the margins.  c* is stepped outwards one float32 at a time (rel -2e-6 .. 3e-5) while it stays p's
    nearest face; the builder keeps, per cell, the position whose ACTUAL float32 centroids lose c* under the most telling parameter
    set.  Everything is judged from the centroids the mesh has (((v0 + v1) + v2) / 3 in float32), never from the ones aimed at.
  * the probe triangles are as large as the distance to p (edge vector along c -> p), so p projects inside u, v in [-4, 5], |h| <= 0.1
    where the cell is small enough: the two faces give different canonical points, and a wrong index shows in x_c too.

Beside each p: its neighbours +-1 and +-2 ulp on the crossed axis and p pulled 2 * GRID_GUARD inside on every axis (six points per
cell, in that order), then +-1 / +-2 ulp on the other axes and around the pulled-in point and the cell's seven other corners: about
3 400 probe points per body.

Verdicts (host only).  For every probe cell and each of PARAM_SETS the case records whether the restated list of the cell CERTAINLY
lacks the face that both the float64 brute force and the dsn_d2 restatement name nearest to p.

What the builder reaches (asserted as exact counts by tests/test_nn_margins_host.py, whose docstring holds the table):
  * fine levels: 64 probe cells each; guard 0 with margin 1 loses c* in 60 to 64 of them, guard 0 with the shipped margin in 56 / 63
    canonical and 19 / 0 posed ones, the shipped guard with margin 1 in none.
  * coarse levels: 4 or 5 probe cells, not 8 - the centroid box is about 10 x 10 x 3 coarse cells with the body through its middle, and
    the cells must be 4 apart.  A probe cell must lie INSIDE the centroid box (its two centroids do), hence inside the fine grid: a
    coarse cell that queries actually reach (outside the fine grid) has every centroid on one side of it, its bound U(B) is attained at
    a corner away from the mesh while dmin is measured to the side facing it, and no point's rounding can matter there.  The coarse
    probe cells are therefore reached by a search only on a scene whose fine level does not fit (DSN_NN_FINE_CAP), which is how the
    GPU test queries them; their lists are compared with the restatement in any case.

The clear-cell margin (DSN_CLEAR_MARGIN, dsn_face_clears_box).  make_face / project / face_clears_box restate dsn_make_face, dsn_project
and the flag decision in float32, operation by operation, with the margin as a parameter (pinned against the oracle's uv, h and against
float64 by tests/test_nn_margins_host.py, against the device's flags by tests/test_gpu_nn_margins.py).  clear_scene() is a mesh whose
centroid box is spanned by two far corner faces and which has ONE more face, so that the middle cell's list holds that face alone;
clear_configs() places it float by float: a 0.5 m face 0.1 m above the guarded box (|h|), a 0.02 m face beside it (u / v = 5 and -4),
at the positions where the box's nearest corner is within 8 ulp of the limit, where the restated flag flips with margin 0 and where it
flips with the shipped margin.
"""
import functools

import numpy as np

import nn_cases as N

F32 = np.float32
GUARD = N.GRID_GUARD                 # = DSN_GRID_GUARD
REL = F32(1e-5)                      # dsn_in_list: u2 * (1.0f + 1e-5f) + 1e-12f
ABS = F32(1e-12)
PARAM_SETS = {"none": (F32(0), F32(0), F32(0)), "margin_only": (F32(0), REL, ABS), "guard_only": (GUARD, F32(0), F32(0)),
              "shipped": (GUARD, REL, ABS)}
FINE_MAXCELL, COARSE_MAXCELL = 65536, 16384          # = DSN_NN_FINE_MAXCELL, DSN_NN_COARSE_MAXCELL
PAD_FINE, PAD_COARSE = F32(0.12), F32(0.7)           # dsn_launch_build_nn's pads (csrc/dsn_api.hip)
N_FINE, N_COARSE = 64, 16                            # probe cells per fine / coarse level
REL_FROM, REL_TO, MAX_STEPS = -2e-6, 3e-5, 96        # c* is stepped from U0 (1 + REL_FROM) outwards, at most to U0 (1 + REL_TO)


# ---------------------------------------------------------------------------------------------------------------------------
# float32 arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c), correctly rounded: the product of two float32 is exact in float64, the float64 sum s = p + c is off by e
    (TwoSum), and rounding s to float32 equals rounding p + c unless s is exactly half way between two float32 - then e decides"""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(F32)
    d = s - r.astype(np.float64)
    with np.errstate(invalid="ignore"):
        r2 = np.nextafter(r, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32))
        tie = (d != 0) & (np.abs(r2.astype(np.float64) - s) == np.abs(d)) & (e != 0)
        towards_r2 = np.sign(e) == np.sign(d)
    return np.where(tie & towards_r2, r2, r).astype(F32)


def centroids(verts, faces):
    """((v0 + v1) + v2) / 3 in float32, as k_face_setup and the oracle compute it"""
    v = np.asarray(verts, F32)
    f = np.asarray(faces, np.int64)
    return (((v[f[:, 0]] + v[f[:, 1]]).astype(F32) + v[f[:, 2]]).astype(F32) / F32(3)).astype(F32)


def d2(p, cent):
    """dsn_d2 bit for bit: dx * dx, fmaf(dy, dy, .), fmaf(dz, dz, .) - p [3] or [n, 3], cent [F, 3] -> [F] or [n, F]"""
    p, c = np.asarray(p, F32), np.asarray(cent, F32)
    d = (p[..., None, :] - c).astype(F32)
    r = (d[..., 0] * d[..., 0]).astype(F32)
    r = fma32(d[..., 1], d[..., 1], r)
    return fma32(d[..., 2], d[..., 2], r)


def nearest_d2(p, cent):
    """the serial ascending sweep with strict '<' over dsn_d2: first index of the minimum"""
    p, cent = np.asarray(p, F32), np.asarray(cent, F32)
    if p.ndim == 1 or cent.shape[0] <= 16:
        return np.argmin(d2(p, cent), -1)
    # float64 first: only the 8 nearest centroids can win (asserted: the 8th is further than any float32 rounding reaches)
    d = ((p.astype(np.float64)[:, None, :] - cent.astype(np.float64)) ** 2).sum(-1)
    near = np.sort(np.argpartition(d, 8, 1)[:, :8], 1)                    # ascending face order: the first index wins a tie
    dn = np.take_along_axis(d, near, 1)
    rows = np.nonzero(dn.max(1) <= dn.min(1) * (1 + 1e-4))[0]             # (nine or more within 1e-4: the whole sweep)
    win = near[np.arange(p.shape[0]), np.argmin(d2(p, cent[near]), 1)]  # (d2 broadcasts p [n, 1, 3] against [n, 8, 3])
    for i in rows:
        win[i] = np.argmin(d2(p[i], cent))
    return win


def nearest_f64(p, cent):
    """float64 brute force: (index of the minimum, number of centroids at that minimum)"""
    d = ((np.asarray(p, np.float64)[..., None, :] - np.asarray(cent, np.float64)) ** 2).sum(-1)
    return np.argmin(d, -1), (d == d.min(-1, keepdims=True)).sum(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# the level's geometry and one cell's list
# ---------------------------------------------------------------------------------------------------------------------------
def level_params(level, F):
    """(pad, target cell count, maxcell) of a level for a mesh of F faces: dsn_launch_build_nn"""
    clamp = lambda x, lo, hi: max(lo, min(hi, x))
    if level.endswith("coarse"):
        return PAD_COARSE, clamp(F // 3, 64, 5000), COARSE_MAXCELL
    return PAD_FINE, (clamp(5 * F, 512, 62000) if level.startswith("canon") else clamp(3 * F, 512, 44000)), FINE_MAXCELL


def grid_header(cent, level):
    """k_grid_params in float32: the fields of nn_cases.parse_header that describe the geometry (lo, cell, inv_cell, n, ncell) and the
    extents e the cell size is computed from.  lo and e are exact; `cell` goes through cbrtf, which the device's library and the
    host's round differently in the last place for about half of the inputs - so the cases take the cell size from recorded device
    headers (device_headers) and this restatement says what they depend on: lo, e and the face count"""
    cent = np.asarray(cent, F32)
    pad, target, maxcell = level_params(level, cent.shape[0])
    lo = (cent.min(0) - pad).astype(F32)
    e = ((cent.max(0) + pad).astype(F32) - lo).astype(F32)
    cell = np.cbrt(F32(F32(F32(e[0] * e[1]) * e[2]) / F32(target)), dtype=F32)
    for _ in range(64):
        n = (np.ceil((e / cell).astype(F32)).astype(np.int64) + 1)
        if int(n[0]) * int(n[1]) * int(n[2]) <= maxcell:
            break
        cell = F32(cell * F32(1.08))
    return dict(lo=lo, e=e, cell=F32(cell), inv_cell=F32(F32(1) / cell), n=n.astype(np.int32), ncell=int(n[0] * n[1] * n[2]))


def device_headers(nonuniform):
    """the four level headers the device builds for the case's mesh (tests/golden/nn_margin_headers.json, recorded on an MI355X;
    test_gpu_nn_margins.py asserts that the device still builds exactly these): {level: header}, and the face count they were
    recorded for"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn_margin_headers.json")) as f:
        rec = json.load(f)["nonuniform" if nonuniform else "uniform"]
    bits = lambda x: np.asarray(x, np.uint32).view(F32)
    out = {}
    for lv, r in rec.items():
        n = np.asarray(r["n"], np.int32)
        out[lv] = dict(lo=bits(r["lo"]).copy(), cell=F32(bits([r["cell"]])[0]), inv_cell=F32(bits([r["inv_cell"]])[0]), n=n,
                       ncell=int(n[0]) * int(n[1]) * int(n[2]))
    return out, int(rec["world_fine"]["F"])


def same_header(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("lo", "cell", "inv_cell", "n", "ncell"))


def cell_ijk(hdr, cell):
    n = hdr["n"].astype(np.int64)
    cell = np.asarray(cell, np.int64)
    return np.stack([cell // (n[2] * n[1]), (cell // n[2]) % n[1], cell % n[2]], -1)


def cell_index(hdr, ijk):
    n = hdr["n"].astype(np.int64)
    ijk = np.asarray(ijk, np.int64)
    return (ijk[..., 0] * n[1] + ijk[..., 1]) * n[2] + ijk[..., 2]


def cell_box(hdr, ijk, guard=GUARD):
    """dsn_cell_box: (lo + i * cell) - guard, (lo + (i + 1) * cell) + guard"""
    i = np.asarray(ijk, np.int64)
    out = []
    for k, sgn in ((i, -1), (i + 1, 1)):
        kf = k.astype(F32)
        edge = (hdr["lo"] + (kf * hdr["cell"]).astype(F32)).astype(F32)
        out.append((edge + F32(sgn) * F32(guard)).astype(F32))
    return out[0], out[1]


def _sum_sq_variants(dx, dy, dz):
    """dx*dx + dy*dy + dz*dz with and without the two fmas a contracting compiler may form: [4, ...]"""
    xx, yy, zz = (dx * dx).astype(F32), (dy * dy).astype(F32), (dz * dz).astype(F32)
    out = []
    for s1 in ((xx + yy).astype(F32), fma32(dy, dy, xx)):
        out += [(s1 + zz).astype(F32), fma32(dz, dz, s1)]
    return np.stack(out)


def box_dmin2(cent, blo, bhi):
    c = np.asarray(cent, F32)
    d = np.maximum(np.maximum((blo - c).astype(F32), (c - bhi).astype(F32)), F32(0))
    return _sum_sq_variants(d[..., 0], d[..., 1], d[..., 2])


def box_dmax2(cent, blo, bhi):
    c = np.asarray(cent, F32)
    d = np.maximum(np.abs((c - blo).astype(F32)), np.abs((c - bhi).astype(F32)))
    return _sum_sq_variants(d[..., 0], d[..., 1], d[..., 2])


def threshold(u2, rel=REL, abs_=ABS):
    """u2 * (1.0f + rel) + abs, with and without the fma: [2, ...]"""
    k = F32(F32(1) + F32(rel))
    u2 = np.asarray(u2, F32)
    return np.stack([((u2 * k).astype(F32) + F32(abs_)).astype(F32), fma32(u2, k, F32(abs_))])


def restate_cell(hdr, cent, cell, guard=GUARD, rel=REL, abs_=ABS):
    """the list of one cell: dict(u2_lo, u2_hi, u2_plain, sure_in [F], sure_out [F]) - sure_in / sure_out hold whatever way the
    expressions are fused, u2_plain is the unfused value (what a -ffp-contract=off build computes)"""
    ijk = cell_ijk(hdr, cell)
    cent = np.asarray(cent, F32)
    # float64 first: a face whose dmax^2 is not within 1e-3 of the smallest cannot attain U^2, and one whose dmin^2 is further than 1e-3
    # from the threshold is in or out whatever the rounding (every float32 step is good to 1e-6 of these magnitudes); the float32
    # variants are evaluated for the faces in between only
    blo, bhi = (x.astype(np.float64) for x in cell_box(hdr, ijk, guard))
    c64 = cent.astype(np.float64)
    dmax64 = (np.maximum(np.abs(c64 - blo), np.abs(c64 - bhi)) ** 2).sum(1)
    dmin64 = (np.maximum(np.maximum(blo - c64, c64 - bhi), 0.0) ** 2).sum(1)
    u64 = dmax64.min()
    t64 = u64 * (1.0 + float(rel)) + float(abs_)
    for_u = np.nonzero(dmax64 <= u64 * 1.001)[0]
    edge = np.nonzero(np.abs(dmin64 - t64) <= 1e-3 * t64)[0]
    dmax = box_dmax2(cent[for_u], *cell_box(hdr, ijk, guard))                                                         # [4, n]
    u2_lo, u2_hi = dmax.min(0).min(), dmax.max(0).min()
    thr_lo, thr_hi = threshold(u2_lo, rel, abs_).min(), threshold(u2_hi, rel, abs_).max()
    sure_in, sure_out = dmin64 < t64, dmin64 > t64
    if edge.size:
        dmin = box_dmin2(cent[edge], *cell_box(hdr, ijk, guard))
        sure_in[edge], sure_out[edge] = dmin.max(0) <= thr_lo, dmin.min(0) > thr_hi
    return dict(u2_lo=F32(u2_lo), u2_hi=F32(u2_hi), u2_plain=F32(dmax[0].min()), sure_in=sure_in, sure_out=sure_out)


# ---------------------------------------------------------------------------------------------------------------------------
# the cells' edges against the cell index
# ---------------------------------------------------------------------------------------------------------------------------
def _plane_points(hdr):
    """per axis a and cell k: the first and the last float32 coordinate that dsn_grid_cell_geom puts into cell k, and how far each
    lies outside the cell's own unguarded box (float64 metres, <= 0: inside).  -> first[a][k], last[a][k], exc_lo[a][k], exc_hi[a][k]"""
    first, last, exc_lo, exc_hi = [], [], [], []
    for a in range(3):
        n = int(hdr["n"][a])
        b = np.array([N.boundary(hdr, a, k) for k in range(n + 1)], F32)
        fi, la = b[:-1], np.nextafter(b[1:], F32(-np.inf))
        k = np.arange(n + 1).astype(F32)
        edge = (hdr["lo"][a] + (k * hdr["cell"]).astype(F32)).astype(F32).astype(np.float64)
        first.append(fi)
        last.append(la)
        exc_lo.append(edge[:-1] - fi.astype(np.float64))
        exc_hi.append(la.astype(np.float64) - edge[1:])
    return first, last, exc_lo, exc_hi


def _triangle(c, along, size):
    """three float32 vertices around c: edge vectors size * along and size * (a unit vector across it), offsets summing to zero"""
    a = np.asarray(along, np.float64)
    a = a / np.linalg.norm(a)
    h = np.zeros(3)
    h[int(np.argmin(np.abs(a)))] = 1.0
    b = np.cross(a, h)
    b /= np.linalg.norm(b)
    c = np.asarray(c, np.float64)
    return np.stack([c + size * a, c + size * b, c - size * (a + b)]).astype(F32)


def _aim(tri, want):
    """move the last vertex by a few ulps per axis so that the float32 centroid ((v0 + v1) + v2) / 3 is `want` where that is possible"""
    tri = tri.copy()
    want = np.asarray(want, F32)
    for a in range(3):
        best = None
        v = tri[2, a]
        cand = [v]
        up = dn = v
        for _ in range(6):
            up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
            cand += [up, dn]
        for x in cand:
            got = F32(F32(F32(tri[0, a] + tri[1, a]) + x) / F32(3))
            err = abs(float(got) - float(want[a]))
            if best is None or err < best[0]:
                best = (err, x)
        tri[2, a] = best[1]
    return tri


def _tri_centroid(tri):
    return ((tri[0] + tri[1]).astype(F32) + tri[2]).astype(F32) / F32(3)


def probe_points(p, axis, centre):
    """p, its neighbours +1, -1, +2, -2 ulp on the crossed axis, and p pulled 2 * GRID_GUARD towards the cell's centre on every axis"""
    pts = [p]
    q = {+1: p, -1: p}
    for _ in range(2):
        for s in (+1, -1):
            q[s] = q[s].copy()
            q[s][axis] = np.nextafter(q[s][axis], F32(s * np.inf))
            pts.append(q[s])
    pts.append((p + np.sign(np.asarray(centre, np.float64) - p) * 2 * float(GUARD)).astype(F32))
    return np.asarray(pts, F32)


def _pair_lost(blo, bhi, cg, cs, params):
    """restate_cell for a mesh of the two faces (c_g, c*) alone, on the cell's unguarded box: is c* certainly out?  (The builder's
    search only; the verdicts come from restate_cell over all centroids.)"""
    dmax = box_dmax2(np.stack([cg, cs]), blo, bhi)
    thr_hi = threshold(dmax.max(0).min(), params[1], params[2]).max()
    return bool(box_dmin2(cs[None], blo, bhi).min() > thr_hi)


def _probe_for_cell(hdr, pp, ijk, form, box_lo, box_hi, tree=None, dry=False):
    """the probe of one cell, or None when its centroids would leave the centroid box [box_lo, box_hi].  Returns dict(p, axis, side,
    tri_g, tri_s, rel, form) - the position of c* kept is the one whose actual centroids lose it under margin_only, else under none"""
    first, last, exc_lo, exc_hi = pp
    cellw = float(hdr["cell"])
    side, p, exc = np.zeros(3, np.int64), np.zeros(3, F32), np.zeros(3)
    for a in range(3):
        k = int(ijk[a])
        side[a] = int(exc_hi[a][k] > exc_lo[a][k])
        p[a] = last[a][k] if side[a] else first[a][k]
        exc[a] = max(exc_lo[a][k], exc_hi[a][k])
    axis = int(np.argmax(exc))
    if exc[axis] <= 0:
        return None
    blo, bhi = cell_box(hdr, ijk, F32(0))
    corner = np.where(side == 1, bhi, blo).astype(np.float64)            # p's corner of the unguarded box
    opp = np.where(side == 1, blo, bhi).astype(np.float64)
    out_dir = np.where(side == 1, 1.0, -1.0)                             # from the cell outwards at p's corner
    diag = (opp - corner) / np.linalg.norm(opp - corner)
    if form == "diag":
        cg_want = opp + 0.15 * cellw * diag
    else:
        cg_want = 0.5 * (corner + opp) + 2e-3 * cellw * diag
    dist_g = float(np.linalg.norm(cg_want - corner))
    tri_g = _triangle(cg_want, corner - cg_want, max(dist_g / 2.5, 4e-3))
    cg = _tri_centroid(tri_g)
    u0 = float(np.sqrt(((np.maximum(np.abs(cg - blo.astype(np.float64)), np.abs(cg - bhi.astype(np.float64)))) ** 2).sum()))
    pair = lambda cs: np.stack([cg, cs]).astype(F32)
    cell = int(cell_index(hdr, ijk))
    if tree is not None:                                                  # no body centroid bounds U(B) or is nearer to p than the pair
        near_d, near_i = tree.query(0.5 * (corner + opp), k=16)
        bc = tree.data[near_i]
        dmax2 = (np.maximum(np.abs(bc - blo.astype(np.float64)), np.abs(bc - bhi.astype(np.float64))) ** 2).sum(1)
        if dmax2.min() <= 2.2 * u0 * u0 or tree.query(p.astype(np.float64))[0] <= 1.1 * u0:
            return None
    if dry:                                                               # (is the cell worth a search: both centroids inside the box)
        cs = p.astype(np.float64)
        cs[axis] = corner[axis] + out_dir[axis] * u0 * (1.0 + REL_TO)
        return bool(np.all(cs > box_lo) and np.all(cs < box_hi) and np.all(cg > box_lo) and np.all(cg < box_hi))
    # c* from U0 (1 - 2e-6) outwards, one float32 at a time on the crossed axis, while it stays p's nearest face: the last position
    # that loses it under the most parameter sets is kept
    around = probe_points(p, axis, 0.5 * (corner + opp))
    x = F32(corner[axis] + out_dir[axis] * u0 * (1.0 + REL_FROM))
    along = np.zeros(3)
    along[axis] = -out_dir[axis]
    best = None
    for _ in range(MAX_STEPS):
        want = p.copy()
        want[axis] = x
        tri_s = _aim(_triangle(want.astype(np.float64), along, max(u0 / 2.5, 4e-3)), want)
        cs = _tri_centroid(tri_s)
        if not (np.all(cs > box_lo) and np.all(cs < box_hi) and np.all(cg > box_lo) and np.all(cg < box_hi)):
            return None
        c2 = pair(cs)
        rel = abs(float(cs[axis]) - corner[axis]) / u0 - 1.0
        if rel > REL_TO:
            break
        w32, w64 = nearest_d2(around, c2), nearest_f64(around, c2)[0]
        if not (w32[0] == 1 and w64[0] == 1):
            if best is not None:
                break
        elif np.array_equal(w32, w64):                                    # (float32 and float64 name the same face for p's neighbours too)
            score = 0                                                     # (lost with the shipped margin implies lost with margin 1)
            if _pair_lost(blo, bhi, cg, cs, PARAM_SETS["none"]):
                score = 2 if _pair_lost(blo, bhi, cg, cs, PARAM_SETS["margin_only"]) else 1
            if best is None or score >= best[0]:
                best = (score, rel, tri_s)
        x = np.nextafter(x, F32(out_dir[axis] * np.inf))
    if best is None:
        return None
    return dict(p=p, axis=axis, side=int(side[axis]), tri_g=tri_g, tri_s=best[2], rel=best[1], form=form, ijk=np.asarray(ijk, np.int64),
                cell=cell, score=best[0])


def _pick_cells(hdr, body_cent, want, taken_pts, min_gap_m, forms, pack=False):
    """up to `want` probes of one level: cells by decreasing excursion (relative to the cell) with no body centroid near (checked per
    cell in _probe_for_cell), >= 4 cells from each other and min_gap_m from the probe centroids of other levels"""
    from scipy.spatial import cKDTree
    pp = _plane_points(hdr)
    n = hdr["n"].astype(np.int64)
    cellw = float(hdr["cell"])
    diag = cellw * 3 ** 0.5
    box_lo = body_cent.min(0).astype(np.float64) + 1e-3
    box_hi = body_cent.max(0).astype(np.float64) - 1e-3
    ijk = np.stack(np.meshgrid(*[np.arange(int(x)) for x in n], indexing="ij"), -1).reshape(-1, 3)
    ctr = hdr["lo"].astype(np.float64) + (ijk + 0.5) * cellw
    inside = np.all((ctr > box_lo) & (ctr < box_hi), 1)
    ijk, ctr = ijk[inside], ctr[inside]
    tree = cKDTree(body_cent.astype(np.float64))
    dist = tree.query(ctr)[0]
    # what the rounding is worth against the cell's size: c* gains the excursion on the crossed axis, c_g loses the diagonal's share
    # of all three (an excursion below 0 - the point inside its box - counts as it is)
    e3 = np.stack([np.maximum(pp[2][a][ijk[:, a]], pp[3][a][ijk[:, a]]) for a in range(3)], 1)
    exc = e3.max(1) + np.maximum(e3, 0).sum(1) / 3 ** 0.5
    ok = (dist > 0.75 * diag) & (e3.max(1) > 0)
    order = np.argsort(-exc[ok] / diag, kind="stable")
    ijk, dist = ijk[ok][order], dist[ok][order]
    if pack:
        # few cells qualify (a coarse level): take first those of the stride-4 lattice that holds the most cells worth a search
        fit = np.array([bool(_probe_for_cell(hdr, pp, q, "centre", box_lo, box_hi, tree, dry=True)) for q in ijk])
        ijk, dist = ijk[fit], dist[fit]
        key = (ijk % 4) @ np.array([16, 4, 1])
        on = key == np.argmax(np.bincount(key, minlength=64))
        ijk, dist = np.concatenate([ijk[on], ijk[~on]]), np.concatenate([dist[on], dist[~on]])
    probes, used = [], []
    for q, dq in zip(ijk, dist):
        if len(probes) >= want:
            break
        if used and np.min(np.max(np.abs(np.array(used) - q), 1)) < 4:
            continue
        c = hdr["lo"].astype(np.float64) + (q + 0.5) * cellw
        if taken_pts.shape[0] and np.min(np.linalg.norm(taken_pts - c, axis=1)) < min_gap_m:
            continue
        form = forms[len(probes) % len(forms)]
        if form == "diag" and dq <= 1.8 * diag:
            form = "centre"
        pr = _probe_for_cell(hdr, pp, q, form, box_lo, box_hi, tree)
        if pr is None and form == "diag":
            pr = _probe_for_cell(hdr, pp, q, "centre", box_lo, box_hi, tree)
        if pr is None:
            continue
        probes.append(pr)
        used.append(q)
    return probes


# ---------------------------------------------------------------------------------------------------------------------------
# the case
# ---------------------------------------------------------------------------------------------------------------------------
def placeholder_mesh(nonuniform):
    """the body + 4 (N_FINE + N_COARSE) appended faces that copy body faces in both spaces: the mesh with the final face count and the
    final centroid box, which is all the grids depend on (tests/golden/make_golden_nn_margin_headers.py records the device's headers
    for it).  Returns (body canon, body faces, body xyz, canon, xyz, faces)"""
    from dsnerf_amd import synth
    canon0, faces0 = synth.make_body(nonuniform=bool(nonuniform))
    xyz0 = synth.pose_body(canon0)
    faces0 = np.asarray(faces0, np.int64)
    V0, F0 = canon0.shape[0], faces0.shape[0]
    K = 2 * (N_FINE + N_COARSE)                                           # probe pairs
    donors = (np.arange(2 * K) * 37 + 11) % F0
    ph = np.concatenate([faces0[d] for d in donors])
    canon = np.concatenate([canon0, canon0[ph]]).astype(F32)
    xyz = np.concatenate([xyz0, xyz0[ph]]).astype(F32)
    faces = np.concatenate([faces0, V0 + np.arange(6 * K).reshape(2 * K, 3)])
    return canon0, faces0, xyz0, canon, xyz, faces


@functools.lru_cache(maxsize=None)
def margin_case(nonuniform):
    """dict(canon, faces, xyz, headers {level: header}, probes {level: [probe]}, points {level: [n, 3]}, owner {level: [n] probe
    number of every point}, verdict {level: {parameter set: [probes] bool}}, base_F).  A probe carries p, axis, side, form, rel, cell,
    ijk, face_g, face_s (positions of its two faces)."""
    canon0, faces0, xyz0, canon, xyz, faces = placeholder_mesh(nonuniform)
    V0, F0 = canon0.shape[0], faces0.shape[0]
    verts = {"world": xyz, "canon": canon}
    # the grids: the recorded device headers, which depend on the centroids' box and the face count only - both are restated here for
    # the placeholder mesh and again for the final one
    restated = {lv: grid_header(centroids(verts[lv.split("_")[0]], faces), lv) for lv in N.LEVELS}
    headers, F_rec = device_headers(nonuniform)
    assert F_rec == faces.shape[0]
    for lv in N.LEVELS:
        h, r = headers[lv], restated[lv]
        assert np.array_equal(h["lo"], r["lo"]) and np.array_equal(h["n"], r["n"]) and h["inv_cell"] == F32(F32(1) / h["cell"]), lv
        assert abs(int(h["cell"].view(np.int32)) - int(r["cell"].view(np.int32))) <= 1, lv          # (cbrtf's last place)
    probes, slot = {}, 0
    for space in ("world", "canon"):
        body_cent = centroids(verts[space][:V0], faces0)
        taken = np.zeros((0, 3))
        for lv, want, forms in ((space + "_coarse", N_COARSE, ("centre", "diag")), (space + "_fine", N_FINE, ("diag", "centre"))):
            gap = 1.3 * float(headers[space + "_coarse"]["cell"]) * 3 ** 0.5
            got = _pick_cells(headers[lv], body_cent, want, taken, gap, forms, pack=lv.endswith("coarse"))
            for pr in got:
                pr["face_g"], pr["face_s"] = F0 + slot, F0 + slot + 1
                for j, tri in enumerate((pr["tri_g"], pr["tri_s"])):
                    verts[space][V0 + 3 * (slot + j):V0 + 3 * (slot + j) + 3] = tri
                slot += 2
            probes[lv] = got
            pts = [headers[lv]["lo"].astype(np.float64) + (pr["ijk"] + 0.5) * float(headers[lv]["cell"]) for pr in got]
            taken = np.concatenate([taken, np.array(pts).reshape(-1, 3)])           # (the coarse probe cells: fine probes keep off them)
    cents = {s: centroids(verts[s], faces) for s in ("world", "canon")}
    for lv in N.LEVELS:
        after = grid_header(cents[lv.split("_")[0]], lv)                                       # the probes did not move the grids
        assert np.array_equal(after["lo"], restated[lv]["lo"]) and np.array_equal(after["e"], restated[lv]["e"]), lv
    points, owner, verdict = {}, {}, {}
    for lv in N.LEVELS:
        hdr, cent = headers[lv], cents[lv.split("_")[0]]
        pts, own = [], []
        for k, pr in enumerate(probes[lv]):
            assert int(N.cell_of(hdr, pr["p"][None])[0]) == pr["cell"]
            blo, bhi = cell_box(hdr, pr["ijk"], F32(0))
            pts.append(probe_points(pr["p"], pr["axis"], 0.5 * (blo.astype(np.float64) + bhi)))
            own += [k] * 6
        # further points of every probe cell, behind the six of each: +-1 / +-2 ulp on the two other axes of p and on the crossed axis
        # of the pulled-in point, and the cell's seven other corners (first / last float32 per axis) - kept where float32 and float64
        # name the same face
        first, last = _plane_points(hdr)[:2]
        more, more_own = [], []
        for k, pr in enumerate(probes[lv]):
            p, a = pr["p"], pr["axis"]
            cand = []
            for b in range(3):
                src = pts[k][5] if b == a else p
                for s_ in (+1, -1):
                    q = src.copy()
                    for _ in range(2):
                        q = q.copy()
                        q[b] = np.nextafter(q[b], F32(s_ * np.inf))
                        cand.append(q)
            for bits in range(8):
                q = np.array([(last if (bits >> b) & 1 else first)[b][pr["ijk"][b]] for b in range(3)], F32)
                if not np.array_equal(q, p):
                    cand.append(q)
            more += cand
            more_own += [k] * len(cand)
        more = np.asarray(more, F32).reshape(-1, 3)
        if more.shape[0]:
            w64, ties = nearest_f64(more, cent)
            keep = (nearest_d2(more, cent) == w64) & (ties == 1) & (N.cell_of(hdr, more) >= 0)
            more, more_own = more[keep], np.asarray(more_own, np.int64)[keep]
        points[lv] = np.concatenate([np.asarray(pts, F32).reshape(-1, 3), more])
        owner[lv] = np.concatenate([np.asarray(own, np.int64), np.asarray(more_own, np.int64)])
        verdict[lv] = {}
        ps = np.array([pr["p"] for pr in probes[lv]], F32).reshape(-1, 3)
        n64, n32 = nearest_f64(ps, cent)[0], nearest_d2(ps, cent)
        for name, params in PARAM_SETS.items():
            v = []
            for k, pr in enumerate(probes[lv]):
                r = restate_cell(hdr, cent, pr["cell"], *params)
                v.append(bool(n64[k] == n32[k] and r["sure_out"][n64[k]]))
            verdict[lv][name] = np.array(v, bool)
    return dict(canon=verts["canon"], faces=faces, xyz=verts["world"], headers=headers, probes=probes, points=points, owner=owner,
                verdict=verdict, base_F=F0, base_V=V0, cent=cents)


@functools.lru_cache(maxsize=None)
def shipped_lists(nonuniform, level):
    """({cell: restated list with the shipped constants} for every cell a probe point of the level lies in, the cell of every point)"""
    c = margin_case(nonuniform)
    hdr, cent = c["headers"][level], c["cent"][level.split("_")[0]]
    cells = N.cell_of(hdr, c["points"][level])
    assert (cells >= 0).all()
    return {int(k): restate_cell(hdr, cent, int(k)) for k in np.unique(cells)}, cells


# ---------------------------------------------------------------------------------------------------------------------------
# the clear-cell margin: dsn_make_face, dsn_project and dsn_face_clears_box in float32 (csrc/dsn_common.h, csrc/dsn_nn.hip)
# ---------------------------------------------------------------------------------------------------------------------------
CLEAR_MARGIN = F32(2.0 ** -17)       # = DSN_CLEAR_MARGIN
CLEAR_INV_MAX = F32(1e12)            # = DSN_CLEAR_INV_MAX
CLEAR_MIN_U2 = F32(0.01)             # = DSN_CLEAR_MIN_U2


def _dot3(a, b):
    return (((a[..., 0] * b[..., 0]).astype(F32) + (a[..., 1] * b[..., 1]).astype(F32)).astype(F32) + (a[..., 2] * b[..., 2]).astype(F32)).astype(F32)


def make_face(v0, v1, v2):
    """dsn_make_face: dict(m0, v10, v20, n [.., 3], d00, d01, d11, inv [..]) - one rounding per operation, fmas where the source has them"""
    v0, v1, v2 = (np.asarray(x, F32) for x in (v0, v1, v2))
    v10, v20 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
    cr = lambda i, j: fma32(v10[..., i], v20[..., j], -(v10[..., j] * v20[..., i]).astype(F32))
    n = np.stack([cr(1, 2), cr(2, 0), cr(0, 1)], -1)
    nn = np.sqrt(fma32(n[..., 2], n[..., 2], fma32(n[..., 1], n[..., 1], (n[..., 0] * n[..., 0]).astype(F32)))).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = (n / nn[..., None]).astype(F32)
        d00, d01, d11 = _dot3(v20, v20), _dot3(v20, v10), _dot3(v10, v10)
        inv = (F32(1) / ((d00 * d11).astype(F32) - (d01 * d01).astype(F32)).astype(F32)).astype(F32)
    return dict(m0=v0, v10=v10, v20=v20, n=n, d00=d00, d01=d01, d11=d11, inv=inv)


def project(p, f):
    """dsn_project: (u, v, h) of point(s) p in the frame of face record(s) f"""
    p = np.asarray(p, F32)
    tmp = (p - f["m0"]).astype(F32)
    sd = _dot3(tmp, f["n"])
    q = (p - (f["n"] * sd[..., None]).astype(F32)).astype(F32)
    w = (q - f["m0"]).astype(F32)
    d02, d12 = _dot3(f["v20"], w), _dot3(f["v10"], w)
    u = (((f["d11"] * d02).astype(F32) - (f["d01"] * d12).astype(F32)).astype(F32) * f["inv"]).astype(F32)
    v = (((f["d00"] * d12).astype(F32) - (f["d01"] * d02).astype(F32)).astype(F32) * f["inv"]).astype(F32)
    return u, v, sd


def transparent(u, v, h):
    """the kernels' test: |h| > 0.1 or u, v outside [-4, 5] (NaN compares false)"""
    return (np.abs(h) > F32(0.1)) | (u > F32(5)) | (u < F32(-4)) | (v > F32(5)) | (v < F32(-4))


def clear_box(blo, bhi):
    """centre and half extents of a guarded box as k_grid_count's clear-cell pass computes them"""
    blo, bhi = np.asarray(blo, F32), np.asarray(bhi, F32)
    cc = (F32(0.5) * (blo + bhi).astype(F32)).astype(F32)
    half = ((F32(0.5) * (bhi - blo).astype(F32)).astype(F32) + (F32(2.4e-7) * (np.abs(blo) + np.abs(bhi)).astype(F32)).astype(F32)).astype(F32)
    return cc, half


def face_clears_box(f, c, half, margin=CLEAR_MARGIN):
    """dsn_face_clears_box for face record(s) f and one box (centre c, half extents): bool [..]"""
    c, half, M_ = np.asarray(c, F32), np.asarray(half, F32), F32(margin)
    ab = lambda x: np.abs(x).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        u, v, h = project(c, f)
        an, bn = _dot3(f["v20"], f["n"]), _dot3(f["v10"], f["n"])
        P = (((np.abs(c) + half).astype(F32)) + ab(f["m0"])).astype(F32)
        H = np.zeros(P.shape[:-1], F32)
        rh = np.zeros(P.shape[:-1], F32)
        for i in range(3):
            H = (H + (ab(f["n"][..., i]) * P[..., i]).astype(F32)).astype(F32)
            rh = (rh + (ab(f["n"][..., i]) * half[i]).astype(F32)).astype(F32)
        a = (f["v20"] - (an[..., None] * f["n"]).astype(F32)).astype(F32)
        b = (f["v10"] - (bn[..., None] * f["n"]).astype(F32)).astype(F32)
        by_h = (((ab(h) - rh).astype(F32) - (M_ * H).astype(F32)).astype(F32)) > F32(0.1)
        usable = ab(f["inv"]) <= CLEAR_INV_MAX
        E20, E10, ru, rv = (np.zeros(P.shape[:-1], F32) for _ in range(4))
        for i in range(3):
            W = (P[..., i] + (ab(f["n"][..., i]) * H).astype(F32)).astype(F32)
            E20 = (E20 + (ab(f["v20"][..., i]) * W).astype(F32)).astype(F32)
            E10 = (E10 + (ab(f["v10"][..., i]) * W).astype(F32)).astype(F32)
            ru = (ru + (ab(((f["d11"] * a[..., i]).astype(F32) - (f["d01"] * b[..., i]).astype(F32)).astype(F32)) * half[i]).astype(F32)).astype(F32)
            rv = (rv + (ab(((f["d00"] * b[..., i]).astype(F32) - (f["d01"] * a[..., i]).astype(F32)).astype(F32)) * half[i]).astype(F32)).astype(F32)
        ai = ab(f["inv"])
        mu = ((((M_ * ai).astype(F32) * ((ab(f["d11"]) * E20).astype(F32) + (ab(f["d01"]) * E10).astype(F32)).astype(F32)).astype(F32))
              + (ai * ru).astype(F32)).astype(F32)
        mv = ((((M_ * ai).astype(F32) * ((ab(f["d00"]) * E10).astype(F32) + (ab(f["d01"]) * E20).astype(F32)).astype(F32)).astype(F32))
              + (ai * rv).astype(F32)).astype(F32)
        by_uv = ((u - mu).astype(F32) > F32(5)) | ((u + mu).astype(F32) < F32(-4)) | ((v - mv).astype(F32) > F32(5)) | ((v + mv).astype(F32) < F32(-4))
    return by_h | (usable & by_uv)


def ulp_steps(x, k):
    """the float32 k steps above x (below for k < 0), through its bit pattern; x and the result on one side of zero"""
    x = np.asarray(x, F32)
    bits = x.view(np.int32).astype(np.int64)
    out = (bits + np.where(x < 0, -1, 1) * np.asarray(k, np.int64)).astype(np.int32).view(F32)
    assert np.all(np.sign(out) == np.sign(x))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# cells at the limits of dsn_face_clears_box: one large face beside a cell of an otherwise empty grid
# ---------------------------------------------------------------------------------------------------------------------------
CLEAR_KINDS = ("h", "u5", "um4", "v5", "vm4")
CLEAR_ANCHORS = 1000                 # copies of each of the two corner faces that span the centroid box


def clear_scene():
    """a mesh whose centroid box is spanned by two small faces at (-0.6, -0.6, -0.6) and (0.6, 0.6, 0.6) (CLEAR_ANCHORS copies of each:
    the face count sets the cell size) plus ONE probe face, the last, placed by clear_probe().  Returns (verts, faces); the probe's
    three vertices are the last three, the canonical mesh is the same one."""
    t = np.array([[0.01, 0, 0], [0, 0.01, 0], [-0.01, -0.01, 0]])
    v = np.concatenate([t - 0.6, t + 0.6, t]).astype(F32)
    faces = np.concatenate([np.tile([[0, 1, 2]], (CLEAR_ANCHORS, 1)), np.tile([[3, 4, 5]], (CLEAR_ANCHORS, 1)), [[6, 7, 8]]]).astype(np.int64)
    return v, faces


def clear_probe_family(hdr, ijk, kind, span=1500):
    """the probe face beside cell ijk for every position k = -span .. span (float32 steps of the coordinate that decides `kind`)
    -> vertices [2 span + 1, 3, 3].  "h": a face of 0.5 m in the plane z = (top of the guarded box) + 0.1, centroid above the cell;
    "u5" / "um4" / "v5" / "vm4": a face of 0.02 m in the plane through the cell's middle, placed so that the guarded box's nearest
    corner has u (v) = 5 or -4.  Step 0 is the float32 nearest to that aim."""
    blo, bhi = cell_box(hdr, ijk)
    cc, _ = clear_box(blo, bhi)
    k = np.arange(-span, span + 1)
    if kind == "h":
        L = 0.5
        m0 = np.array([cc[0] - L / 3, cc[1] - L / 3, float(bhi[2]) + 0.1])
        axis = 2
    else:
        L = 0.02
        m0 = cc.astype(np.float64).copy()
        axis = 1 if kind[0] == "u" else 0                      # u runs along v20 = +y, v along v10 = +x
        m0[1 - axis] -= L / 3
        m0[axis] = float(blo[axis]) - 5 * L if kind.endswith("5") else float(bhi[axis]) + 4 * L
    m0 = np.tile(m0.astype(F32), (k.size, 1))
    m0[:, axis] = ulp_steps(m0[:, axis], k)
    v1, v2 = m0.copy(), m0.copy()
    v1[:, 0] = (m0[:, 0] + F32(L)).astype(F32)
    v2[:, 1] = (m0[:, 1] + F32(L)).astype(F32)
    return np.stack([m0, v1, v2], 1)


def clear_configs(hdr, ijk):
    """the positions worth a frame, per kind: those around the step at which the restated flag with the shipped margin flips, around
    the step at which it flips with margin 0, and those whose nearest box corner lies within 8 ulp of the limit itself (|h| = 0.1,
    u / v = 5 or -4).  -> list of dict(kind, k, tri [3, 3], flag, flag0, corner [3], at_limit)"""
    blo, bhi = cell_box(hdr, ijk)
    cc, half = clear_box(blo, bhi)
    out = []
    for kind in CLEAR_KINDS:
        tris = clear_probe_family(hdr, ijk, kind)
        f = make_face(tris[:, 0], tris[:, 1], tris[:, 2])
        flag, flag0 = face_clears_box(f, cc, half), face_clears_box(f, cc, half, F32(0))
        if kind == "h":
            corner = np.tile(np.array([cc[0], cc[1], bhi[2]], F32), (tris.shape[0], 1))
            lim, ulp = F32(0.1), np.spacing(F32(0.1))
            val = np.abs(project(corner, f)[2])
        else:
            a = 1 if kind[0] == "u" else 0
            corner = np.tile(cc, (tris.shape[0], 1))
            corner[:, a] = blo[a] if kind.endswith("5") else bhi[a]
            lim = F32(5) if kind.endswith("5") else F32(-4)
            ulp = np.spacing(F32(abs(lim)))
            val = project(corner, f)[0 if kind[0] == "u" else 1]
        at_limit = np.abs(val.astype(np.float64) - float(lim)) <= 8 * float(ulp)
        pick = set(np.nonzero(at_limit)[0][:6].tolist())
        for fl in (flag, flag0):
            ch = np.nonzero(fl[1:] != fl[:-1])[0]
            assert ch.size >= 1, (kind, "the flag does not flip in the family")
            for j in ch[:2]:
                pick.update(range(max(j - 1, 0), min(j + 3, fl.size)))
        for j in sorted(pick):
            out.append(dict(kind=kind, k=int(j - (tris.shape[0] - 1) // 2), tri=tris[j], flag=bool(flag[j]), flag0=bool(flag0[j]),
                            corner=corner[j], at_limit=bool(at_limit[j])))
    return out


def cell_sample_points(hdr, ijk):
    """27 sample points of a cell: per axis the first float32 of the cell, its middle and its last float32"""
    ax = []
    for a in range(3):
        lo, hi = N.boundary(hdr, a, int(ijk[a])), np.nextafter(N.boundary(hdr, a, int(ijk[a]) + 1), F32(-np.inf))
        ax.append(np.array([lo, F32(0.5) * (lo + hi), hi], F32))
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(F32)
