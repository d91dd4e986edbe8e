"""numpy restatement of the mesh smoothing and face-normal rules of include/dsnerf.h (dsn_mesh_smooth / dsn_mesh_vertex_normals): np.add.at
on int64 for the sums, float64 for the rest, one IEEE rounding per operation.  Reproduces every output bit of the device calls."""
import numpy as np

F32 = np.float32
HEAVY = 64            # DSN_MESH_SMOOTH_HEAVY
MAX_STEPS = 4096      # DSN_MESH_SMOOTH_MAX_STEPS
QLO, QHI = -2.0 ** 30, 2.0 ** 30 - 1.0
NCLAMP = 2.0 ** 62


def finite_box(verts):
    v = np.asarray(verts, F32).reshape(-1, 3)
    fin = np.isfinite(v).all(axis=1)
    return (v[fin].min(axis=0), v[fin].max(axis=0)) if fin.any() else None


def scale_of(verts):
    """(origin float32 [3], k): the caller's scale of the rule"""
    box = finite_box(verts)
    if box is None:
        return np.zeros(3, F32), 27
    D = float(np.max(box[1].astype(np.float64) - box[0].astype(np.float64)))
    return box[0].copy(), 27 - (int(np.frexp(D)[1]) if D > 0 else 0)


def in_range(V, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def contributing(verts, faces):
    """[T] bool: indices in [0, V), pairwise different, nine finite coordinates"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = in_range(v.shape[0], f)
    ok &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    fin = np.isfinite(v).all(axis=1)
    g = np.where(ok[:, None], f, 0)
    return ok & (fin[g].all(axis=1) if v.shape[0] else False)


def quantise(x, origin, k):
    """int64 q of float32 positions x [V,3]"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = x.astype(np.float64) - np.asarray(origin, F32).astype(np.float64)[None, :]
        q = np.clip(np.floor(r * np.ldexp(1.0, k)), QLO, QHI)
    return np.where(np.isfinite(r), q, 0.0).astype(np.int64)


def smooth(verts, faces, factors, origin=None, k=None):
    """dict: verts [V,3] float32, counts [4] int64 {contributing, skipped, vertices with n > 0, most faces at a vertex}, origin, k, n [V]"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, T = v.shape[0], f.shape[0]
    o, kk = scale_of(v)
    origin = o if origin is None else np.asarray(origin, F32).reshape(3)
    k = kk if k is None else int(k)
    fc = f[contributing(v, f)]
    m = np.zeros(V, np.int64)                      # contributing faces per vertex
    np.add.at(m, fc.reshape(-1), 1)
    counts = np.array([fc.shape[0], T - fc.shape[0], int((m > 0).sum()), int(m.max()) if V else 0], np.int64)
    x = v.copy()
    moved = m > 0
    for fac in np.asarray(factors, F32).reshape(-1):
        q = quantise(x, origin, k)
        S = np.zeros((V, 3), np.int64)
        for c in range(3):
            i, j, l = fc[:, c], fc[:, (c + 1) % 3], fc[:, (c + 2) % 3]
            np.add.at(S, i, (q[j] - q[i]) + (q[l] - q[i]))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            delta = S.astype(np.float64) / (2 * m).astype(np.float64)[:, None]
            t = np.float64(fac) * delta
            u = t * np.ldexp(1.0, -k)
            new = (x.astype(np.float64) + u).astype(F32)
        x = np.where(moved[:, None], new, x)
        x.view(np.uint32)[~moved] = v.view(np.uint32)[~moved]      # (bit for bit, NaN payloads included)
    return {"verts": x, "counts": counts, "origin": origin, "k": k, "n": 2 * m}


def face_normals(verts, faces):
    """float32 [T,3] of faces with valid indices: e1 = b - a, e2 = c - a, each component two rounded products and one subtraction"""
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = (b - a).astype(F32), (c - a).astype(F32)
        n = np.stack([(e1[:, 1] * e2[:, 2]).astype(F32) - (e1[:, 2] * e2[:, 1]).astype(F32),
                      (e1[:, 2] * e2[:, 0]).astype(F32) - (e1[:, 0] * e2[:, 2]).astype(F32),
                      (e1[:, 0] * e2[:, 1]).astype(F32) - (e1[:, 1] * e2[:, 0]).astype(F32)], 1).astype(F32)
    return n


def normal_sums(verts, faces, shift):
    v = np.asarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = v.shape[0]
    ok = in_range(V, f)
    fin = np.isfinite(v).all(axis=1)
    g = np.where(ok[:, None], f, 0)
    ok &= fin[g].all(axis=1) if V else False
    fc = f[ok]                                     # (repeated indices count: their normal is exactly 0 or not finite)
    n = face_normals(v, fc)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.floor(np.ldexp(n.astype(np.float64), shift)), -NCLAMP, NCLAMP)
    q = np.where(np.isfinite(n), q, 0.0).astype(np.int64)
    N = np.zeros((V, 3), np.int64)
    for c in range(3):
        np.add.at(N, fc[:, c], q)
    return N


def area_shift(verts, T):
    """mesh_area_shift's: 61 - bit_length(T) - e clamped to +-60, e the frexp exponent of float32 D2 over the finite bounding box"""
    box = finite_box(verts)
    e = 0
    if box is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            d = box[1] - box[0]
            d2 = F32(F32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        e = int(np.frexp(d2)[1]) if np.isfinite(d2) else 128
    return max(-60, min(60, 61 - int(T).bit_length() - e))


def vertex_normals(verts, faces, shift=None):
    """float32 [V,3]"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    shift = area_shift(v, f.shape[0]) if shift is None else int(shift)
    N = normal_sums(v, f, shift).astype(np.float64)
    L = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (N / L[:, None]).astype(F32)
    return np.where((L > 0)[:, None], out, F32(0.0)).astype(F32)


def taubin(iterations, lamb=0.5, mu=-0.53):
    return [lamb] * iterations if mu is None else [lamb, mu] * iterations


# ---- test meshes ---------------------------------------------------------------------------------------------------------------------
def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0), noise=0.0, seed=0):
    """(verts float32 [V,3], faces int32 [T,3]) outward winding; level 3: 642 vertices, 1280 faces; noise: the standard deviation of a relative radial error"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1),
         (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v)
    if noise:
        v = v * (1.0 + noise * np.random.default_rng(seed).standard_normal(v.shape[0]))[:, None]
    return (v * radius + np.asarray(centre, np.float64)).astype(F32), np.array(f, np.int32)


def grid_plane(n=9, z=0.37):
    """an n x n planar grid at height z, every square cut by the same diagonal: interior vertices have the hexagonal umbrella"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i.ravel() * 0.25, j.ravel() * 0.25, np.full(n * n, z)], 1).astype(F32)
    f = []
    for a in range(n - 1):
        for b in range(n - 1):
            p = a * n + b
            f += [(p, p + n, p + n + 1), (p, p + n + 1, p + 1)]
    return v, np.array(f, np.int32)


def volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def umbrella_float64(verts, faces, factor):
    """one step in float64 by scipy.sparse, the rule's multiplicities (every contributing face gives each corner its two others)"""
    from scipy.sparse import coo_matrix
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)[contributing(verts, faces)]
    V = v.shape[0]
    i = np.concatenate([f[:, 0], f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2]])
    j = np.concatenate([f[:, 1], f[:, 2], f[:, 2], f[:, 0], f[:, 0], f[:, 1]])
    W = coo_matrix((np.ones(i.shape[0]), (i, j)), shape=(V, V)).tocsr()
    n = np.asarray(W.sum(axis=1)).reshape(-1)
    out = v.copy()
    m = n > 0
    out[m] = v[m] + factor * ((W @ v)[m] / n[m, None] - v[m])
    return out


BINDING_KEYS = ("face_idx", "uv", "h", "cov", "x_c")


def smooth_dict(mesh, iterations=10, lamb=0.5, mu=-0.53, normals=None):
    """visualizer.smooth_mesh's dict handling on host arrays: verts moved, normals recomputed from the faces when carried or asked for
    (dropped with normals=False), the entries of a binding dropped, everything else carried over, "smooth_info" added"""
    out = smooth(mesh["verts"], mesh["faces"], taubin(iterations, lamb, mu))
    want = mesh.get("normals") is not None if normals is None else bool(normals)
    res = {k: a for k, a in mesh.items() if k not in BINDING_KEYS and k != "normals"}
    res["verts"] = out["verts"]
    if want:
        res["normals"] = vertex_normals(out["verts"], mesh["faces"])
    res["smooth_info"] = {"contributing_faces": int(out["counts"][0]), "skipped_faces": int(out["counts"][1]),
                          "vertices_moved": int(out["counts"][2]), "max_faces_at_vertex": int(out["counts"][3]), "origin": out["origin"],
                          "scale_exp": out["k"], "factors": np.asarray(taubin(iterations, lamb, mu), F32)}
    return res
