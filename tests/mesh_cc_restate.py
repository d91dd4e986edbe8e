"""numpy restatement of the mesh components of include/dsnerf.h (dsn_mesh_cc_label / dsn_mesh_cc_emit), the whole rule:

valid faces (three indices in [0, V)); components under the shared-vertex-INDEX rule, labelled by their smallest vertex index (-1 for a
vertex in no valid face); the doubled float32 area of a face as the integer floor(d 2^k) summed in uint64 per component; the winner
(largest sum, then the smaller label); the winner as a compacted mesh with source_vertex.  Also the inputs the tests share."""
import math

import numpy as np

F32 = np.float32
TILE = 1024          # DSN_MESH_CC_TILE


def valid_faces(V, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def labels(V, faces):
    """[V] int32: the smallest vertex index of each vertex's component, -1 where no valid face uses the vertex.  Hooking under the
    smaller label and pointer jumping until nothing moves; lab[v] <= v throughout."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(V, f)]
    lab = np.arange(V, dtype=np.int64)
    flat = f.reshape(-1)
    while True:
        m = np.repeat(lab[f].min(axis=1), 3) if f.size else np.zeros(0, np.int64)
        new = lab.copy()
        np.minimum.at(new, flat, m)
        np.minimum.at(new, lab[flat], m)
        while True:
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        if np.array_equal(new, lab):
            break
        lab = new
    used = np.zeros(V, bool)
    used[flat] = True
    return np.where(used, lab, -1).astype(np.int32)


def doubled_area(verts, faces):
    """float32 d of every face (indices must be valid), the order of operations of the rule; not finite -> 0"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        e1, e2 = b - a, c - a
        n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        d = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    assert d.dtype == F32
    return np.where(np.isfinite(d), d, F32(0))


def area_shift(verts, T):
    """k = 61 - bit_length(T) - e clamped to +-60; e the frexp exponent of float32 D2 over the bounding box of the finite vertices"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    fin = np.isfinite(v).all(axis=1)
    e = 0
    if fin.any():
        with np.errstate(all="ignore"):
            d = v[fin].max(axis=0) - v[fin].min(axis=0)
            d2 = F32(F32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        e = int(np.frexp(d2)[1]) if np.isfinite(d2) else 128
    return max(-60, min(60, 61 - int(T).bit_length() - e))


def face_q(verts, faces, k):
    """uint64 q = floor(d 2^k) of every face (valid indices), formed exactly in double"""
    x = np.floor(np.ldexp(doubled_area(verts, faces).astype(np.float64), k))
    big = x >= 2.0 ** 63
    return np.where(big, np.uint64(1 << 63), np.where(big, 0.0, x).astype(np.uint64))


def components(verts, faces, k=None):
    """dict: labels [V] int32, counts [6] int64 {components, winner, V', T', winner's sum, winner's faces}, sums {label: (sum, faces)},
    area_shift, area (the winner's, float)"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, T = v.shape[0], f.shape[0]
    k = area_shift(v, T) if k is None else int(k)
    lab = labels(V, f)
    ok = valid_faces(V, f)
    fv = f[ok]
    root = lab[fv[:, 0]].astype(np.int64)
    q = face_q(v, fv, k)
    sums = np.zeros(V, np.uint64)
    cnt = np.zeros(V, np.int64)
    np.add.at(sums, root, q)
    np.add.at(cnt, root, 1)
    roots = np.flatnonzero(cnt > 0)
    winner = -1
    if roots.size:
        best = sums[roots].max()
        winner = int(roots[sums[roots] == best].min())
    keep_v = (lab == winner) if winner >= 0 else np.zeros(V, bool)
    keep_f = ok.copy()
    keep_f[ok] = root == winner
    if winner < 0:
        keep_f[:] = False
    counts = np.array([roots.size, winner, keep_v.sum(), keep_f.sum(), int(sums[winner]) if winner >= 0 else 0,
                       int(cnt[winner]) if winner >= 0 else 0], np.int64)
    return {"labels": lab, "counts": counts, "sums": {int(r): (int(sums[r]), int(cnt[r])) for r in roots}, "area_shift": k,
            "area": math.ldexp(float(counts[4]), -k - 1), "keep_v": keep_v, "keep_f": keep_f}


def largest_component(verts, faces, k=None):
    """(verts' [V',3] float32, faces' [T',3] int32, source_vertex [V'] int32, the dict of components())"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c = components(v, f, k)
    src = np.flatnonzero(c["keep_v"]).astype(np.int32)
    vmap = np.full(v.shape[0], -1, np.int64)
    vmap[src] = np.arange(src.size)
    fk = f[c["keep_f"]]
    nf = vmap[fk].astype(np.int32).reshape(-1, 3)
    return np.ascontiguousarray(v[src]), np.ascontiguousarray(nf), src, c


def partition_by_edges(V, faces):
    """trimesh's rule, for comparison: component number per face when faces join through a shared EDGE (scipy)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    T = f.shape[0]
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    key = e[:, 0] * V + e[:, 1]
    owner = np.tile(np.arange(T), 3)
    order = np.argsort(key, kind="stable")
    key, owner = key[order], owner[order]
    same = key[1:] == key[:-1]
    g = coo_matrix((np.ones(same.sum()), (owner[:-1][same], owner[1:][same])), shape=(T, T))
    return connected_components(g, directed=False)[1]


def partition_by_vertices(V, faces):
    """the vertex rule by scipy: component number per vertex over the graph of the valid faces' edges, and which vertices are used"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(V, f)]
    r = np.concatenate([f[:, 0], f[:, 0]])
    c = np.concatenate([f[:, 1], f[:, 2]])
    g = coo_matrix((np.ones(r.size), (r, c)), shape=(V, V))
    used = np.zeros(V, bool)
    used[f.reshape(-1)] = True
    return connected_components(g, directed=False)[1], used


def same_partition(a, b):
    """two labelings of the same items induce the same classes"""
    a, b = np.asarray(a), np.asarray(b)
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def axes_of(n):
    a = np.arange(n, dtype=np.float64)
    return a, a.copy(), a.copy()


def noise_volume(n=24, seed=5):
    return np.random.default_rng(seed).random((n, n, n)).astype(F32)


def smooth_volume(n=24, seed=7, passes=3):
    v = np.random.default_rng(seed).random((n, n, n))
    for _ in range(passes):
        for ax in range(3):
            v = (np.roll(v, 1, ax) + v + np.roll(v, -1, ax)) / 3
    return v.astype(F32)


SPHERES = (((11.2, 11.7, 12.1), 7.3), ((24.3, 23.8, 24.6), 4.1), ((4.4, 26.3, 5.2), 1.2))


def spheres_volume(n=32, spheres=SPHERES):
    """max over the spheres of r - |p - c|: positive inside; level 0"""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), -1)
    v = np.full((n, n, n), -np.inf)
    for c, r in spheres:
        v = np.maximum(v, r - np.linalg.norm(g - np.array(c), axis=-1))
    return v.astype(F32)


def strip(n_faces, reverse=False):
    """a triangle strip: face t = (t, t + 1, t + 2) (odd faces with the first two swapped: one winding); reverse: vertex numbers
    mirrored, so the smallest index is at the far end of every chain"""
    t = np.arange(n_faces, dtype=np.int64)
    f = np.stack([t, t + 1, t + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    V = n_faces + 2
    if reverse:
        f = V - 1 - f
    k = np.arange(V)
    pos = k if not reverse else V - 1 - k
    v = np.stack([(pos // 2) * 0.01, (pos % 2) * 0.01, np.zeros(V)], 1).astype(F32)
    return v, f.astype(np.int32)


def fan(n_faces, centre_last=False):
    """n_faces triangles around one vertex: the first (index 0) or the last"""
    V = n_faces + 2
    ang = np.linspace(0, 1.9 * np.pi, n_faces + 1)
    rim = np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], 1)
    t = np.arange(n_faces, dtype=np.int64)
    if centre_last:
        v = np.concatenate([rim, np.zeros((1, 3))])
        f = np.stack([np.full(n_faces, V - 1), t, t + 1], 1)
    else:
        v = np.concatenate([np.zeros((1, 3)), rim])
        f = np.stack([np.zeros(n_faces, np.int64), t + 1, t + 2], 1)
    return v.astype(F32), f.astype(np.int32)


def interleaved_strips(n_strips=1000, faces_each=200):
    """n_strips disjoint strips, their faces interleaved in face order (face j of strip s is face j n_strips + s); strip s is
    (1 + s / n_strips) times as wide as strip 0, so no two areas tie"""
    v0, f0 = strip(faces_each)
    Vs = v0.shape[0]
    vs, fs = [], []
    for s in range(n_strips):
        vs.append(v0 * F32(1 + s / n_strips) + np.array([0, 0, s], F32))
        fs.append(f0.astype(np.int64) + s * Vs)
    f = np.stack(fs, 1).reshape(-1, 3)
    return np.concatenate(vs).astype(F32), f.astype(np.int32)


def mesh_with_counts(n_keep_v, n_keep_f, extra=True):
    """a mesh whose winner has exactly n_keep_v vertices and n_keep_f faces (n_keep_f >= max(n_keep_v - 2, 1), n_keep_v >= 3 or both 0):
    a strip of n_keep_v vertices, its last face repeated to make up the count, between two small decoys and unused vertices"""
    if n_keep_v == 0:
        return np.zeros((5, 3), F32), np.array([[0, 1, 7], [-1, 2, 3]], np.int32)          # (no valid face at all)
    if n_keep_v == 1:          # faces of one repeated index: every sum is 0, the smaller label wins; vertices 0 and 2 are unused
        v = np.array([[0, 0, 0], [1, 2, 3], [4, 5, 6], [7, 8, 9]], F32)
        return v, np.array([[1, 1, 1]] * n_keep_f + [[3, 3, 3]], np.int32)
    v, f = strip(n_keep_v - 2)
    f = np.concatenate([f, np.repeat(f[-1:], n_keep_f - f.shape[0], 0)])
    if not extra:
        return v, f
    dv = np.array([[0, 0, 1], [0.001, 0, 1], [0, 0.001, 1]], F32)
    verts = np.concatenate([dv, np.zeros((2, 3), F32), v * F32(3), dv + F32(1)])
    faces = np.concatenate([[[0, 1, 2]], f.astype(np.int64) + 5, [[5 + v.shape[0] + k for k in range(3)]]])
    return verts, faces.astype(np.int32)
