"""numpy restatement of the mesh-distance rules of include/dsnerf.h (dsn_mesh_dist_query / _reduce, dsn_mesh_sample_surface), written
from the rules, not from the kernels.

  closest_on_triangles   the seven-region closest point in float32, one rounding per operation (numpy float32 arrays round after every
                         operation; nothing here is fused)
  brute_force            the rule itself: the minimum over all valid faces, ties to the lowest index.  No grid.
  grid_rule / GridModel  the level-0 grid rule in double, and a model of the search the header describes (cells, levels, shells, the
                         stopping comparison with or without its margin).  The model is NOT the reference of any bit comparison - brute
                         force is; it exists to construct the case that needs the margin (test 2e) and to show on the CPU that the
                         search with the margin returns the brute-force answer.
  reduce_stats           the reduction in float64 in the documented tree order
  surface_cum / sample_surface   the sampler: float64 areas, the three-level prefix, Philox words from tests/draws_restate.py
"""
import numpy as np

from draws_restate import philox4x32

F32 = np.float32
MAX_G = 4096
REDUCE_TILE = 1024
SAMPLE_TILE = 32
KIND_SURFACE = 2


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def valid_faces(verts, faces):
    """bool [T]: three indices in [0, V) and nine finite coordinates"""
    verts, faces = f32(verts).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    V = verts.shape[0]
    ok = ((faces >= 0) & (faces < V)).all(axis=1)
    fin = np.isfinite(verts).all(axis=1)
    safe = np.where(ok[:, None], faces, 0)
    return ok & (fin[safe].all(axis=1) if V else False)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest_on_triangles(p, a, b, c):
    """p [N,3], a, b, c [F,3] float32 -> (d2 [N,F], q [N,F,3], region [N,F] in 1 ... 7): the rule's closest point of every triangle to
    every point"""
    p = f32(p)[:, None, :]
    a, b, c = f32(a)[None], f32(b)[None], f32(c)[None]
    zero, one = F32(0.0), F32(1.0)
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        shape = np.broadcast(d1, d6).shape

        den3, den5, den6 = d1 - d3, d2 - d6, e43 + e56

        def full(x):
            return np.broadcast_to(x, shape + (3,))
        v3, w5, w6 = (d1 / den3)[..., None], (d2 / den5)[..., None], (e43 / den6)[..., None]
        inv = one / ((va + vb) + vc)
        v7, w7 = (vb * inv)[..., None], (vc * inv)[..., None]
        cand = [full(a), full(b), a + v3 * ab, full(c), a + w5 * ac, b + w6 * (c - b), (a + ab * v7) + ac * w7]
        cond = [(d1 <= zero) & (d2 <= zero), (d3 >= zero) & (d4 <= d3), (vc <= zero) & (d1 >= zero) & (d3 <= zero) & (den3 > zero),
                (d6 >= zero) & (d5 <= d6), (vb <= zero) & (d2 >= zero) & (d6 <= zero) & (den5 > zero),
                (va <= zero) & (e43 >= zero) & (e56 >= zero) & (den6 > zero)]
        region = np.full(shape, 7, np.int32)
        q = np.array(cand[6], dtype=F32)
        for k in range(5, -1, -1):                       # the first region that applies wins: assign in reverse
            region = np.where(cond[k], k + 1, region)
            q = np.where(cond[k][..., None], cand[k], q).astype(F32)
        r = p - q
        dd = _dot(r, r)
    return dd.astype(F32), q, region


def brute_force(verts, faces, points, chunk=1 << 21):
    """the rule: (dist2 [n] float32, face [n] int32, point [n,3] float32) over all valid faces, ties to the lowest index; a point that is
    not finite: NaN, -1, NaN; no valid face: +inf, -1, NaN"""
    verts, faces, points = f32(verts).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3), f32(points).reshape(-1, 3)
    n = points.shape[0]
    keep = np.nonzero(valid_faces(verts, faces))[0]
    best = np.full(n, np.inf, F32)
    bf = np.full(n, -1, np.int64)
    bq = np.full((n, 3), np.nan, F32)
    fin = np.isfinite(points).all(axis=1)
    pts = np.where(fin[:, None], points, F32(0.0))
    step = max(1, chunk // max(n, 1))
    rows = np.arange(n)
    for k0 in range(0, keep.shape[0], step):
        idx = keep[k0:k0 + step]                         # ascending face indices
        tri = verts[faces[idx]]
        dd, q, _ = closest_on_triangles(pts, tri[:, 0], tri[:, 1], tri[:, 2])
        dd_cmp = np.where(np.isnan(dd), np.inf, dd)      # a NaN distance never wins
        j = np.argmin(dd_cmp, axis=1)                    # first occurrence: the lowest index of the chunk
        dj = dd_cmp[rows, j]
        win = dj < best                                  # strict: an earlier chunk (lower indices) keeps a tie
        best = np.where(win, dj, best).astype(F32)
        bf = np.where(win, idx[j], bf)
        bq = np.where(win[:, None], q[rows, j], bq).astype(F32)
    best = np.where(fin, best, F32(np.nan)).astype(F32)
    bf = np.where(fin, bf, -1)
    bq = np.where(fin[:, None], bq, F32(np.nan)).astype(F32)
    return best, bf.astype(np.int32), bq


def finite_box(verts):
    v = f32(verts).reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)]
    return (v.min(axis=0), v.max(axis=0)) if v.shape[0] else None


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
def cells_cap(T):
    return min(2 * T + 64, 1 << 26)


def entries_cap(T):
    return min(8 * T + 64, (1 << 31) - 1)


def grid_rule(T, box):
    """(g [3] int, cell float32): the level-0 grid of the header, in double"""
    lo, hi = np.asarray(box[0], np.float32).astype(np.float64), np.asarray(box[1], np.float32).astype(np.float64)
    ext = hi - lo
    L = float(ext.max())
    one_cell = (np.ones(3, np.int64), F32(1.0))
    if not L > 0.0:
        return one_cell
    M = cells_cap(T)

    def count(n):
        g = np.minimum(np.floor(ext * float(n) / L).astype(np.int64) + 1, n)
        return int(g[0]) * int(g[1]) * int(g[2])
    a, b = 1, MAX_G
    while a < b:
        mid = (a + b + 1) // 2
        if count(mid) <= M:
            a = mid
        else:
            b = mid - 1
    cell = F32(L / float(a) * (1.0 + 2.0 ** -20))
    with np.errstate(all="ignore"):
        inv = F32(1.0) / cell
    if not (cell > 0 and np.isfinite(inv) and np.isfinite(cell)):
        return one_cell
    g = np.minimum(np.floor(ext / float(cell)).astype(np.int64) + 1, a)
    return g, cell


class GridModel:
    """the search of the header, in Python: cells, levels, lists, shells.  margin=False drops the slack and the factor from the stopping
    comparison - the search a reader might write first, which test 2e shows to be wrong."""

    def __init__(self, verts, faces, box=None):
        self.verts, self.faces = f32(verts).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
        T = self.faces.shape[0]
        box = finite_box(self.verts) if box is None else box
        self.origin = f32(box[0]).reshape(3)
        self.g0, self.cell = grid_rule(T, box)
        self.inv = F32(1.0) / self.cell
        S = F32(max(np.abs(f32(box[0])).max(), np.abs(f32(box[1])).max()))
        self.slack = F32(S * F32(2.0 ** -17))
        self.valid = np.nonzero(valid_faces(self.verts, self.faces))[0]
        tri = self.verts[self.faces[self.valid]]                                    # [Tv, 3 corners, 3 axes]
        self.lo0 = np.stack([self.cell0(tri[:, :, a].min(axis=1), a) for a in range(3)], axis=1)
        self.hi0 = np.stack([self.cell0(tri[:, :, a].max(axis=1), a) for a in range(3)], axis=1)
        cap = entries_cap(T)
        self.pairs = []
        for l in range(13):
            self.pairs.append(int(np.prod((self.hi0 >> l) - (self.lo0 >> l) + 1, axis=1).sum()))
        self.level = next(l for l in range(13) if self.pairs[l] <= cap or l == 12)
        self.g = ((self.g0 - 1) >> self.level) + 1
        self.lists = {}
        lo, hi = self.lo0 >> self.level, self.hi0 >> self.level
        for k, f in enumerate(self.valid):
            for x in range(lo[k, 0], hi[k, 0] + 1):
                for y in range(lo[k, 1], hi[k, 1] + 1):
                    for z in range(lo[k, 2], hi[k, 2] + 1):
                        self.lists.setdefault((x, y, z), []).append(int(f))

    def cell0(self, x, axis):
        t = (np.asarray(x, F32) - self.origin[axis]) * self.inv
        t = np.minimum(np.maximum(t, F32(0.0)), F32(self.g0[axis] - 1))
        return np.floor(t).astype(np.int64)

    def plane(self, k, axis):
        """the computed lower plane of level cell k"""
        return F32(self.origin[axis] + F32(F32(int(k) << self.level) * self.cell))

    def lower_bound(self, p, c, r):
        """the smallest computed distance from p to the planes around the cube of radius r, None where no side goes on"""
        lb = None
        for a in range(3):
            up, dn = int(c[a]) + r + 1, int(c[a]) - r
            if up < self.g[a]:
                d = F32(self.plane(up, a) - p[a])
                lb = d if lb is None else min(lb, d)
            if dn > 0:
                d = F32(p[a] - self.plane(dn, a))
                lb = d if lb is None else min(lb, d)
        return lb

    def stops(self, lb, best, margin):
        if lb is None:
            return True
        if margin:
            lb = F32(F32(lb - self.slack) * F32(1.0 - 2.0 ** -16))
        return bool(lb > 0 and F32(lb * lb) > best)

    def query(self, p, margin=True):
        """(dist2, face, point, shells searched) for one finite point"""
        p = f32(p).reshape(3)
        c = [int(self.cell0(p[a], a)) >> self.level for a in range(3)]
        best, bf, bq = F32(np.inf), -1, np.full(3, np.nan, F32)
        r = 0
        while True:
            for x in range(max(c[0] - r, 0), min(c[0] + r, self.g[0] - 1) + 1):
                for y in range(max(c[1] - r, 0), min(c[1] + r, self.g[1] - 1) + 1):
                    for z in range(max(c[2] - r, 0), min(c[2] + r, self.g[2] - 1) + 1):
                        if max(abs(x - c[0]), abs(y - c[1]), abs(z - c[2])) != r:
                            continue
                        for f in self.lists.get((x, y, z), ()):
                            tri = self.verts[self.faces[f]]
                            dd, q, _ = closest_on_triangles(p[None], tri[None, 0], tri[None, 1], tri[None, 2])
                            d = dd[0, 0]
                            if d < best or (d == best and f < bf):
                                best, bf, bq = d, f, q[0, 0]
            if self.stops(self.lower_bound(p, c, r), best, margin):
                return best, bf, bq, r + 1
            r += 1


# ---- the reduction ---------------------------------------------------------------------------------------------------------------------
def _fold(x):
    """x [..., 256] float64: s[t] += s[t + h] for h = 128 ... 1 -> [...]"""
    x = np.array(x, dtype=np.float64)
    h = 128
    while h >= 1:
        x = x[..., :h] + x[..., h:2 * h]
        h //= 2
    return x[..., 0]


def _block_sums(values, skip):
    """values [n] float64 (`skip` entries count as 0.0): per 1024-block, thread t adds t + 256 j for j = 0 ... 3 in order, then the fold"""
    n = values.shape[0]
    blocks = (n + REDUCE_TILE - 1) // REDUCE_TILE
    x = np.zeros(blocks * REDUCE_TILE, np.float64)
    x[:n] = np.where(skip, 0.0, values)                  # adding +0.0 to a sum that started at +0.0 changes no bit
    x = x.reshape(blocks, 4, 256)
    s = np.zeros((blocks, 256), np.float64)
    for j in range(4):
        s = s + x[:, j, :]
    return _fold(s)


def _finish(parts):
    blocks = parts.shape[0]
    rows = (blocks + 255) // 256
    x = np.zeros(rows * 256, np.float64)
    x[:blocks] = parts
    x = x.reshape(rows, 256)
    s = np.zeros(256, np.float64)
    for k in range(rows):
        s = s + x[k]
    return _fold(s)


def reduce_stats(dist2):
    """the six float64 of dsn_mesh_dist_reduce: count, NaN count, sum d, sum d^2, max d, index of the max"""
    x = f32(dist2).reshape(-1)
    nan = np.isnan(x)
    with np.errstate(all="ignore"):
        xd = x.astype(np.float64)
        d = np.sqrt(xd)
        count = int((~nan).sum())
        if x.shape[0] == 0:
            return np.array([0.0, 0.0, 0.0, 0.0, 0.0, -1.0])
        sum_d = _finish(_block_sums(d, nan))
        sum_d2 = _finish(_block_sums(xd, nan))
    if count:
        m = np.where(nan, F32(-1.0), x).max()
        arg = int(np.nonzero(~nan & (x == m))[0][0])
        mx = float(np.sqrt(np.float64(m)))
    else:
        arg, mx = -1, 0.0
    return np.array([float(count), float(nan.sum()), sum_d, sum_d2, mx, float(arg)])


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
def face_areas(verts, faces):
    verts, faces = f32(verts).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(verts, faces)
    tri = verts[np.where(ok[:, None], faces, 0)].astype(np.float64)
    e, f = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    with np.errstate(all="ignore"):
        n0 = e[:, 1] * f[:, 2] - e[:, 2] * f[:, 1]
        n1 = e[:, 2] * f[:, 0] - e[:, 0] * f[:, 2]
        n2 = e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0]
        area = 0.5 * np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    return np.where(ok, area, 0.0)


def _running(x, size):
    """running sums inside consecutive runs of `size` entries (np.cumsum adds in order, one rounding per addition) and each run's total"""
    n = x.shape[0]
    runs = (n + size - 1) // size
    pad = np.zeros(runs * size, np.float64)
    pad[:n] = x
    run = np.cumsum(pad.reshape(runs, size), axis=1)
    last = np.minimum(np.arange(1, runs + 1) * size, n) - np.arange(runs) * size - 1
    return run.reshape(-1)[:n], run[np.arange(runs), last]


def surface_cum(verts, faces):
    """cum [T] float64 in the documented three-level order"""
    area = face_areas(verts, faces)
    T = area.shape[0]
    in_tile, tile_total = _running(area, SAMPLE_TILE)
    in_group, group_total = _running(tile_total, SAMPLE_TILE)
    top = np.cumsum(group_total)
    t = np.arange(T)
    k = t // SAMPLE_TILE
    g = k // SAMPLE_TILE
    before_tile = np.where(k % SAMPLE_TILE != 0, in_group[np.maximum(k - 1, 0)], 0.0)
    before_group = np.where(g != 0, top[np.maximum(g - 1, 0)], 0.0)
    return before_group + (before_tile + in_tile)


def sample_surface(verts, faces, n, seed=0):
    """(points [n,3] float32, face [n] int32)"""
    verts, faces = f32(verts).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    cum = surface_cum(verts, faces)
    total = cum[-1]
    if not (total > 0.0 and np.isfinite(total)) or n == 0:
        return np.full((n, 3), np.nan, F32), np.full(n, -1, np.int32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32((np.arange(n, dtype=np.uint64), 0, 0, KIND_SURFACE), (seed & 0xFFFFFFFF, seed >> 32)).reshape(n, 4).astype(np.uint64)
    u0 = ((w[:, 0] << np.uint64(20)) | (w[:, 1] >> np.uint64(12))).astype(np.float64) * 2.0 ** -52
    x = u0 * total
    face = np.searchsorted(cum, x, side="right")         # the first t with cum[t] > x
    u = (w[:, 2] >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)
    v = (w[:, 3] >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)
    flip = (u + v) > F32(1.0)
    u = np.where(flip, F32(1.0) - u, u).astype(F32)
    v = np.where(flip, F32(1.0) - v, v).astype(F32)
    tri = verts[faces[face]]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    pts = (a + u[:, None] * (b - a)) + v[:, None] * (c - a)
    return pts.astype(F32), face.astype(np.int32)


# ---- small meshes the tests share ------------------------------------------------------------------------------------------------------
def cube_mesh():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7],
                  [1, 7, 3]], np.int32)
    return v, f


def icosphere(subdivisions=2):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        cache, nf = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for (a, b, c) in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int32)


def tiny_triangle(corner, away, e):
    """a small triangle whose nearest point to anything on the other side is `corner`: the other two vertices lie `e` further along
    `away` and `e` to the side"""
    corner, away = np.asarray(corner, np.float64), np.asarray(away, np.float64)
    side = np.roll(away, 1)
    return np.stack([corner, corner + e * away + e * side, corner + e * away + e * np.roll(away, 2)]).astype(F32)


def margin_case(fillers=190, seed=5):
    """The case that needs the stopping margin (test 2e).  A query p sits in cell c; face B lies just inside the next cell along x, face A
    in p's own cell on the other side, a few float32 steps FARTHER than B.  B's corner x_B is a float below the COMPUTED plane of its own
    cell (the cell function and the plane round differently), so the computed bound after shell 0, plane - p_x, exceeds B's distance and
    even A's: a search that compares the bare bound stops with A.  Brute force picks B.
    Returns {"verts", "faces", "point", "near_face" (A, index 0), "far_face" (B, index 1), "model"}."""
    rng = np.random.default_rng(seed)
    for origin in (0.1, 0.3, 0.7, 1.1, 0.05, 2.3):
        lo, hi = F32(origin), F32(origin + 1.2)
        tris = [None, None]
        for cx in (lo, hi):                              # the box: tiny triangles in the eight corners, pointing inwards
            for cy in (lo, hi):
                for cz in (lo, hi):
                    c = np.array([cx, cy, cz], np.float64)
                    s = np.where(c == lo, 1e-3, -1e-3)
                    tris.append(np.stack([c, c + [s[0], 0.0, 0.0], c + [0.0, s[1], 0.0]]).astype(F32))
        while len(tris) < fillers + 2:                   # the rest: tiny triangles in the low-x fifth of the box, far from the query
            c = lo + rng.random(3) * np.array([0.2, 1.0, 1.0]) * 1.19
            tris.append(tiny_triangle(c, np.array([1.0, 0.0, 0.0]), 1e-4))
        T = len(tris)
        g, cell = grid_rule(T, (np.full(3, lo), np.full(3, hi)))
        probe = GridModel(np.zeros((0, 3), F32), np.zeros((0, 3), np.int64), box=(np.full(3, lo), np.full(3, hi)))
        probe.g0, probe.cell, probe.inv = g, cell, F32(1.0) / cell
        for k in range(int(g[0]) - 2, 2, -1):
            plane = F32(lo + F32(F32(k) * cell))
            x, found = plane, None
            for _ in range(8):
                x = np.nextafter(x, F32(-np.inf))
                if int(probe.cell0(x, 0)) >= k:
                    found = x                            # a float below the computed plane that the cell function still puts into cell k
                else:
                    break
            if found is None:
                continue
            ky = int(g[1]) // 2
            py = F32(lo + (ky + 0.5) * float(cell))
            px = F32(float(found) - 0.1 * float(cell))
            dB = F32(found - px)
            ax = F32(px - dB)
            if F32(px - ax) != dB or int(probe.cell0(ax - F32(0.01), 0)) != k - 1 or int(probe.cell0(px, 0)) != k - 1:
                continue
            eta = F32(2.0 ** -16)
            tris[0] = tiny_triangle([ax, F32(py + eta), py], [-1.0, 0.0, 0.0], 1e-3)           # A: off the axis by eta, so a few steps farther
            tris[1] = tiny_triangle([found, py, py], [1.0, 0.0, 0.0], 1e-4)                    # B
            verts = np.concatenate(tris).astype(F32)
            faces = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
            model = GridModel(verts, faces)
            if model.level != 0:
                continue
            return {"verts": verts, "faces": faces, "point": np.array([px, py, py], F32), "near_face": 0, "far_face": 1, "model": model}
    raise AssertionError("margin_case: no float below a computed plane found - the construction needs another origin")
