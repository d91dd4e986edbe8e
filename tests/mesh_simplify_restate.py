"""numpy restatement of the mesh simplification of include/dsnerf.h (dsn_mesh_simplify_count / dsn_mesh_simplify_emit), the whole rule,
with nothing borrowed from the library: the cell of a vertex, the clusters in ascending cell number, the representative nearest to the
members' fixed-point mean (ties: the smaller index), live faces, duplicates (the smallest input index of a cluster triple stays), the
cap and the seven counts; the grid defaults of _lib.mesh_simplify, the probe sequence of simplify_mesh(target_vertices=N) and the gather
of a mesh dict.  Also the inputs the tests share."""
import numpy as np

F32 = np.float32
MAX_G = 4096                 # DSN_MESH_SIMPLIFY_MAX_G
MAX_CELLS = 1 << 31
CAP = 1 << 21                # 2^DSN_MESH_SIMPLIFY_MAX_LOG2
TOO_MANY = 1                 # DSN_MESH_SIMPLIFY_TOO_MANY
TILE = 1024                  # faces per tile of the output scan (DSN_MESH_CC_TILE)
WORD_TILE = 4096 * 32        # cells per tile of the popcount scan
PER_VERTEX_KEYS = ("normals", "albedo", "normal", "colour", "sigma", "valid")
BINDING_KEYS = ("face_idx", "uv", "h", "cov", "x_c")


def grid_ok(g):
    g = [int(x) for x in g]
    return all(1 <= x <= MAX_G for x in g) and g[0] * g[1] * g[2] <= MAX_CELLS


def locate(verts, origin, cell, g):
    """(inside [V] bool, cell number [V] int64 (-1 outside), t [V,3] float32)"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    inv = F32(1.0) / F32(cell)
    with np.errstate(all="ignore"):
        t = (v - np.asarray(origin, F32).reshape(1, 3)) * inv
    assert t.dtype == F32
    gf = np.asarray(g, F32).reshape(1, 3)
    with np.errstate(invalid="ignore"):
        inside = (np.isfinite(t) & (t >= 0) & (t < gf)).all(axis=1)
    i = np.floor(np.where(inside[:, None], t, F32(0))).astype(np.int64)
    num = (i[:, 0] * int(g[1]) + i[:, 1]) * int(g[2]) + i[:, 2]
    return inside, np.where(inside, num, -1), t


def simplify(verts, faces, cell, origin, g):
    """dict: verts [K,3] float32, faces [T',3] int32, cluster_source [K] int32, vertex_cluster [V] int32, counts [7] int64 {K, kept,
    live, duplicates dropped, outside, bad index, status}, keep [T] bool (which input faces stay)"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, T = v.shape[0], f.shape[0]
    assert grid_ok(g) and np.isfinite(F32(cell)) and F32(cell) > 0
    inside, num, t = locate(v, origin, cell, g)
    cells = np.unique(num[inside])                      # ascending cell number
    K = cells.size
    vc = np.full(V, -1, np.int64)
    vc[inside] = np.searchsorted(cells, num[inside])
    outside = int(V - inside.sum())
    if K > CAP:
        return {"verts": np.zeros((0, 3), F32), "faces": np.zeros((0, 3), np.int32), "cluster_source": np.zeros(0, np.int32),
                "vertex_cluster": vc.astype(np.int32), "counts": np.array([K, 0, 0, 0, outside, 0, TOO_MANY], np.int64),
                "keep": np.zeros(T, bool)}
    # representative
    q = np.floor(t[inside].astype(np.float64) * 2.0 ** 20).astype(np.int64)
    assert (q >= 0).all() and (q < 2 ** 32).all()
    cl = vc[inside]
    s = np.zeros((K, 3), np.int64)
    n = np.zeros(K, np.int64)
    np.add.at(s, cl, q)
    np.add.at(n, cl, 1)
    m = s.astype(np.float64) / n.astype(np.float64)[:, None]
    e = q.astype(np.float64) - m[cl]
    d = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    idx = np.flatnonzero(inside)
    key = (d.astype(F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    best = np.full(K, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(best, cl, key)
    src = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    # faces
    ok = ((f >= 0) & (f < V)).all(axis=1)
    bad = int(T - ok.sum())
    c = np.full((T, 3), -1, np.int64)
    c[ok] = vc[f[ok]]
    live = ok & (c >= 0).all(axis=1) & (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    keep = np.zeros(T, bool)
    li = np.flatnonzero(live)
    if li.size:
        tri = np.sort(c[li], axis=1)
        packed = (tri[:, 0] << 42) | (tri[:, 1] << 21) | tri[:, 2]
        _, first = np.unique(packed, return_index=True)      # (the first occurrence: li ascends, so the smallest input index)
        keep[li[first]] = True
    kept = int(keep.sum())
    counts = np.array([K, kept, li.size, li.size - kept, outside, bad, 0], np.int64)
    return {"verts": np.ascontiguousarray(v[src]), "faces": np.ascontiguousarray(c[keep].astype(np.int32)).reshape(-1, 3),
            "cluster_source": src.astype(np.int32), "vertex_cluster": vc.astype(np.int32), "counts": counts, "keep": keep}


def finite_box(verts):
    """(lo [3], hi [3]) float32 over the vertices whose coordinates are all finite, or None"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    fin = np.isfinite(v).all(axis=1)
    if not fin.any():
        return None
    return v[fin].min(axis=0), v[fin].max(axis=0)


def default_grid(verts, cell, origin=None, g=None):
    """origin: the minimum over the finite vertices (zeros without one); g_a = floor((max_a - origin_a) inv) + 1 in the rule's float32
    operations (1 without a finite vertex, or where that is below 1)"""
    box = finite_box(verts)
    if origin is None:
        origin = np.zeros(3, F32) if box is None else box[0]
    origin = np.asarray(origin, F32).reshape(3)
    if g is None:
        if box is None:
            g = [1, 1, 1]
        else:
            inv = F32(1.0) / F32(cell)
            with np.errstate(all="ignore"):
                tt = (box[1] - origin) * inv
            g = [max(int(np.floor(x)) + 1, 1) if np.isfinite(x) else MAX_G + 1 for x in tt]
    return origin, [int(x) for x in g]


def target_cell(verts, n):
    """the cell of n cells along the longest finite extent: float32(extent / n) (1 + 2^-20), every operation float32; 1 where the
    extent is 0 or there is no finite vertex"""
    box = finite_box(verts)
    if box is None:
        return F32(1.0)
    ext = F32((box[1] - box[0]).max())
    if not (ext > 0 and np.isfinite(ext)):
        return F32(1.0)
    c = F32(F32(ext / F32(n)) * F32(1.0 + 2.0 ** -20))
    return c if (c > 0 and np.isfinite(c) and np.isfinite(F32(1.0) / c)) else F32(1.0)


def cell_count(verts, cell, origin, g):
    inside, num, _ = locate(verts, origin, cell, g)
    return int(np.unique(num[inside]).size)


def target_search(verts, N):
    """(n, cell, origin, g, probes): the largest n in [1, 4096] with K(n) <= N by bisection (K treated as monotone; a grid outside the
    library's limits counts as too many); probes = the n of every probe, in order"""
    N = int(N)
    assert N >= 1
    lo, hi, probes = 1, MAX_G, []
    while lo < hi:
        mid = (lo + hi + 1) // 2
        probes.append(mid)
        c = target_cell(verts, mid)
        o, g = default_grid(verts, c)
        if grid_ok(g) and cell_count(verts, c, o, g) <= N:
            lo = mid
        else:
            hi = mid - 1
    c = target_cell(verts, lo)
    o, g = default_grid(verts, c)
    return lo, c, o, g, probes


def gather_dict(mesh, out):
    """the dict simplify_mesh returns for the dict `mesh` (numpy), from simplify()'s `out`: every per-vertex array through
    cluster_source ([K,V,3] forms along axis 1), the binding's entries and source_vertex too"""
    src = out["cluster_source"].astype(np.int64)
    V = np.asarray(mesh["verts"]).reshape(-1, 3).shape[0]
    res = dict(mesh)
    for k in PER_VERTEX_KEYS + BINDING_KEYS + ("source_vertex",):
        a = res.get(k)
        if a is None:
            continue
        a = np.asarray(a)
        res[k] = a[:, src] if (a.ndim == 3 and a.shape[1] == V) else a[src]
    res.update(verts=out["verts"], faces=out["faces"], cluster_source=out["cluster_source"], vertex_cluster=out["vertex_cluster"])
    return res


# ---- mesh properties -----------------------------------------------------------------------------------------------------------
def edge_counts(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)


def euler(n_verts, faces):
    e, _ = edge_counts(faces)
    return int(n_verts) - e.shape[0] + np.asarray(faces).reshape(-1, 3).shape[0]


def closed(faces):
    return bool((edge_counts(faces)[1] == 2).all())


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def icosphere(level):
    """geodesic icosphere: 10 4^level + 2 vertices on the unit sphere, 20 4^level faces (float64 construction, float32 result)"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1),
         (-p, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v).astype(F32), np.array(f, np.int32)


def cube_grid(n):
    """(origin, cell, g) of n cells per axis over [-1.001, 1.001]^3, the grid the icosphere figures were taken with"""
    return np.full(3, -1.001, F32), F32(2.002 / n), [n, n, n]


def planar_grid(m):
    """an m x m planar grid mesh at integer positions + 0.25 (z = 0.25): m^2 vertices, 2 (m - 1)^2 faces"""
    j, i = np.meshgrid(np.arange(m), np.arange(m))
    v = np.stack([i.ravel() + 0.25, j.ravel() + 0.25, np.full(m * m, 0.25)], 1).astype(F32)
    a = (np.arange(m - 1)[:, None] * m + np.arange(m - 1)[None, :]).ravel()
    f = np.concatenate([np.stack([a, a + m, a + 1], 1), np.stack([a + 1, a + m, a + m + 1], 1)])
    return v, f.astype(np.int32)


def distinct_cells(n, g1=128, g2=128):
    """n vertices, each in a cell of its own of a unit-cell grid (g0, g1, g2) at the origin, vertex k in cell perm[k]; returns
    (verts, origin, cell, g, perm)"""
    g0 = (n + g1 * g2 - 1) // (g1 * g2)
    perm = np.random.default_rng(41).permutation(n).astype(np.int64)
    i0, r = perm // (g1 * g2), perm % (g1 * g2)
    v = np.stack([i0, r // g2, r % g2], 1).astype(F32) + F32(0.5)
    return v, np.zeros(3, F32), F32(1.0), [int(g0), g1, g2], perm
