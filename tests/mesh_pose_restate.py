"""numpy restatement of the bound-mesh rule of include/dsnerf.h (dsn_mesh_bind_normals, dsn_mesh_pose, dsn_mesh_stretch): float32 with
one rounding per operation in the rule's operation order - the kernels' bits - and, with dtype=np.float64, the twin the closed forms
are checked against.  Fused multiply-adds occur where csrc/dsn_common.h has them (dsn_cross3, dsn_norm3); the float32 one is formed
exactly: the product of two float32 is exact in float64, the sum is rounded to odd there (two-sum residual) and then to float32,
which equals one rounding of the exact value."""
import numpy as np


def fma(a, b, c, dtype=np.float32):
    if dtype == np.float64:
        return np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                # exact: 24 + 24 significant bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)          # two-sum: p + c = s + err exactly
        s = np.atleast_1d(s).copy()
        err = np.broadcast_to(err, s.shape)
        even = (s.view(np.int64) & 1) == 0
        fix = (err != 0) & even & np.isfinite(s)
        toward = np.where(err > 0, np.inf, -np.inf)
        s[fix] = np.nextafter(s[fix], toward[fix])
        return s.astype(np.float32).reshape(np.shape(p))


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def norm3(a):
    dt = a.dtype.type
    return np.sqrt(fma(a[..., 2], a[..., 2], fma(a[..., 1], a[..., 1], a[..., 0] * a[..., 0], dt), dt))


def cross3(a, b):
    dt = a.dtype.type
    return np.stack([fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1]), dt),
                     fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2]), dt),
                     fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]), dt)], axis=-1)


def normalize3(a):
    n = norm3(a)
    n = np.where(n < a.dtype.type(1e-12), a.dtype.type(1e-12), n)
    return a / n[..., None]


def make_face(v0, v1, v2):
    """dsn_make_face's m0, v10, v20, n (unit) and c = v10 x v20 of faces given by their three vertices [..., 3]"""
    v10, v20 = v1 - v0, v2 - v0
    c = cross3(v10, v20)
    return {"m0": v0, "v10": v10, "v20": v20, "c": c, "n": c / norm3(c)[..., None]}


def body_faces(xyz, faces, face_idx, dtype=np.float32):
    """the records of body faces face_idx [N] of body xyz [Vb,3]; (records, ok [N]): not ok where face_idx is outside [0, Fb) or the
    face holds a vertex index outside [0, Vb) (row 0 stands in there: the callers overwrite the result with NaN)"""
    xyz = np.asarray(xyz, dtype)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    face_idx = np.asarray(face_idx).astype(np.int64)
    ok = (face_idx >= 0) & (face_idx < faces.shape[0])
    tri = faces[np.where(ok, face_idx, 0)]
    ok_v = ((tri >= 0) & (tri < xyz.shape[0])).all(axis=-1)
    tri = np.where(ok_v[:, None], tri, 0)
    return make_face(xyz[tri[:, 0]], xyz[tri[:, 1]], xyz[tri[:, 2]]), ok, ok & ok_v


def project(p, rec):
    """dsn_project: (uv [N,2], h [N]) of points p [N,3] in the frames of their faces"""
    sd = dot3(p - rec["m0"], rec["n"])
    w = (p - rec["n"] * sd[..., None]) - rec["m0"]
    d00, d01, d11 = dot3(rec["v20"], rec["v20"]), dot3(rec["v20"], rec["v10"]), dot3(rec["v10"], rec["v10"])
    inv = p.dtype.type(1) / (d00 * d11 - d01 * d01)
    d02, d12 = dot3(rec["v20"], w), dot3(rec["v10"], w)
    return np.stack([(d11 * d02 - d01 * d12) * inv, (d00 * d12 - d01 * d02) * inv], axis=-1), sd


def map2face(uv, h, rec):
    """dsn_map2face: ((m0 + u v20) + v v10) + h n"""
    return ((rec["m0"] + uv[..., 0:1] * rec["v20"]) + uv[..., 1:2] * rec["v10"]) + h[..., None] * rec["n"]


def bind_normals(body_xyz, faces, face_idx, normals, dtype=np.float32):
    """dsn_mesh_bind_normals: cov [N,3] = (n . v20, n . v10, n . n_f); NaN where the binding or its face is bad"""
    with np.errstate(all="ignore"):
        rec, ok_f, ok = body_faces(body_xyz, faces, face_idx, dtype)
        n = np.asarray(normals, dtype).reshape(-1, 3)
        cov = np.stack([dot3(n, rec["v20"]), dot3(n, rec["v10"]), dot3(n, rec["n"])], axis=-1)
        cov[~ok] = np.nan
    return cov


def transport(cov, rec):
    a, b = cross3(rec["n"], rec["v10"]), cross3(rec["v20"], rec["n"])
    m = (cov[..., 0:1] * a + cov[..., 1:2] * b) + cov[..., 2:3] * rec["c"]
    return normalize3(m)


def pose(target_xyz, faces, face_idx, uv, h, cov=None, dtype=np.float32):
    """dsn_mesh_pose: (verts [P,N,3], normals [P,N,3] or None, status) for targets [P,Vb,3]"""
    target_xyz = np.asarray(target_xyz, dtype)
    P = target_xyz.shape[0]
    uv, h = np.asarray(uv, dtype).reshape(-1, 2), np.asarray(h, dtype).reshape(-1)
    N = h.shape[0]
    verts = np.empty((P, N, 3), dtype)
    normals = None if cov is None else np.empty((P, N, 3), dtype)
    status = 0
    with np.errstate(all="ignore"):
        for p in range(P):
            rec, ok_f, ok = body_faces(target_xyz[p], faces, face_idx, dtype)
            verts[p] = map2face(uv, h, rec)
            verts[p][~ok] = np.nan
            if cov is not None:
                normals[p] = transport(np.asarray(cov, dtype).reshape(-1, 3), rec)
                normals[p][~ok] = np.nan
            status |= int((~ok_f).any())
    return verts, normals, status


def stretch(bind_verts, posed_verts, faces, dtype=np.float32):
    """dsn_mesh_stretch: [P,T]"""
    bind = np.asarray(bind_verts, dtype).reshape(-1, 3)
    N = bind.shape[0]
    posed = np.asarray(posed_verts, dtype)
    posed = posed.reshape(posed.shape[0] if posed.ndim == 3 else 1, N, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    P, T = posed.shape[0], faces.shape[0]
    ok = ((faces >= 0) & (faces < N)).all(axis=-1)
    out = np.full((P, T), np.inf, dtype)
    if N == 0 or T == 0:
        return out
    tri = np.where(ok[:, None], faces, 0)
    with np.errstate(all="ignore"):
        lb = [norm3(bind[tri[:, (k + 1) % 3]] - bind[tri[:, k]]) for k in range(3)]
        for p in range(P):
            s, seen = np.ones(T, dtype), np.zeros(T, bool)
            for k in range(3):
                r = norm3(posed[p][tri[:, (k + 1) % 3]] - posed[p][tri[:, k]]) / lb[k]
                use = lb[k] != 0
                take = use & (~seen | (r > s) | (r != r))
                s = np.where(take, r, s)
                seen |= use
            out[p] = np.where(ok, s, np.inf)
    return out
