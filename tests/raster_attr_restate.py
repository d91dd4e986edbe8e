"""numpy restatement of the attribute shade step of include/dsnerf.h (dsn_raster_mesh_attr) on top of tests/raster_restate.py, which
gives the visibility (face, depth): the winner's perspective-correct weights b_k = (l_k iw_k) z from its integer edge functions,
vertex normals and colours interpolated with them, the smooth or flat normal, the lit or unlit colour.  dtype=np.float32 follows the
header's order of operations (numpy does not fuse); dtype=np.float64 evaluates the same rule in double precision from the same
winners, which gives the float32 rule's own error on an input (tests/golden/raster_attr_spread.json).

raster_attr(...) returns raster_restate.raster's dict plus "normal" [H, W, 3] and "attr" [H, W, 3] (0 where empty; attr only with
colours) and "weights" [n, 3] / "hit" [n] (the b_k and the pixel index of every covered pixel) for the tests."""
import numpy as np

import raster_restate as R

F32 = np.float32
SMOOTH, UNLIT = 1, 2


def winners(verts, faces, pose, fx, fy, znear, H, W, face, depth, dtype=F32):
    """per covered pixel: (pixel index, vertex ids in the order P [n, 3], b_k [n, 3]) of the winning triangle"""
    T = dtype
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    hit = np.flatnonzero(face.reshape(-1) >= 0)
    f = faces[face.reshape(-1)[hit]]
    X, Y, iw32, _ = R.project(verts, pose, fx, fy, znear, H, W)
    if T is F32:
        iw = iw32
    else:
        with np.errstate(all="ignore"):
            iw = T(1) / (-R.camera_coords(verts, pose, T)[:, 2])
    px, py = X[f], Y[f]
    area = (px[:, 1] - px[:, 0]) * (py[:, 2] - py[:, 0]) - (py[:, 1] - py[:, 0]) * (px[:, 2] - px[:, 0])
    order = np.where((area < 0)[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    rows = np.arange(f.shape[0])[:, None]
    f, px, py, area = f[rows, order], px[rows, order], py[rows, order], np.abs(area)
    y, x = hit // W, hit % W
    cx, cy = 256 * x + 128, 256 * y + 128
    z = depth.reshape(-1)[hit].astype(T)
    b = np.zeros((hit.size, 3), dtype=T)
    with np.errstate(all="ignore"):
        for k in range(3):
            p, q = (k + 1) % 3, (k + 2) % 3
            dx, dy = px[:, q] - px[:, p], py[:, q] - py[:, p]
            e = dx * (cy - py[:, p]) - dy * (cx - px[:, p])
            l = e.astype(T) / area.astype(T)
            b[:, k] = (l * iw[f[:, k]].astype(T)) * z
    return hit, f, b


def interpolate(b, a):
    """a [n, 3 (vertex), c] -> (b_0 a_0 + b_1 a_1) + b_2 a_2 per component"""
    with np.errstate(all="ignore"):
        return (b[:, 0, None] * a[:, 0] + b[:, 1, None] * a[:, 1]) + b[:, 2, None] * a[:, 2]


def raster_attr(verts, faces, pose=None, fx=None, fy=None, znear=0.05, light=None, H=64, W=None, normals=None, colors=None,
                mode=0, dtype=F32, base=None):
    """base: raster_restate.raster's result for the same mesh and camera (computed here when not given)"""
    T = dtype
    W = H if W is None else W
    pose = R.DEFAULT_POSE if pose is None else pose
    if fx is None or fy is None:
        fx, fy = R.default_scales(height=H, width=W)
    light = R.light_values() if light is None else np.asarray(light, F32)
    out = dict(R.raster(verts, faces, pose, fx, fy, znear, light, H, W) if base is None else base)
    face, depth = out["face"], out["depth"]
    hit, f, b = winners(verts, faces, pose, fx, fy, znear, H, W, face, depth, T)
    n = hit.size
    y, x = hit // W, hit % W
    z = depth.reshape(-1)[hit].astype(T)
    P = np.asarray(pose, F32).reshape(-1, 4)[:3].astype(T)
    Rm = P[:, :3]
    lt = light.astype(T)
    pi = T(F32(np.pi)) if T is F32 else T(np.pi)
    with np.errstate(all="ignore"):
        xn = (2 * x + 1).astype(T) / T(W) - T(1)
        yn = T(1) - (2 * y + 1).astype(T) / T(H)
        px, py = (xn * z) / T(F32(fx)), (yn * z) / T(F32(fy))
        r2 = (px * px + py * py) + z * z
        r = np.sqrt(r2)
        s = (z / r - lt[2]) / (lt[1] - lt[2])
        s = np.where(s > 0, s, T(0))
        s = np.where(s < 1, s, T(1))
        s = s * s
        # flat: camera-space n from the face's vertices in the order given
        c = R.camera_coords(verts, pose, T)
        g = np.asarray(faces).reshape(-1, 3).astype(np.int64)[face.reshape(-1)[hit]]
        a_, b_ = c[g[:, 1]] - c[g[:, 0]], c[g[:, 2]] - c[g[:, 0]]
        nc = np.stack([a_[:, 1] * b_[:, 2] - a_[:, 2] * b_[:, 1], a_[:, 2] * b_[:, 0] - a_[:, 0] * b_[:, 2],
                       a_[:, 0] * b_[:, 1] - a_[:, 1] * b_[:, 0]], axis=1)
        nn = np.sqrt((nc[:, 0] * nc[:, 0] + nc[:, 1] * nc[:, 1]) + nc[:, 2] * nc[:, 2])
        nw = np.stack([((Rm[e, 0] * nc[:, 0] + Rm[e, 1] * nc[:, 1]) + Rm[e, 2] * nc[:, 2]) / nn for e in range(3)], axis=1)
        nw = np.where(((nn > 0) & (nn < np.inf))[:, None], nw, T(0))
        if mode & SMOOTH:
            vn = np.asarray(normals, F32).reshape(-1, 3).astype(T)[f]                  # [n, 3 (vertex), 3]
            q = (np.abs(vn[:, :, 0]) + np.abs(vn[:, :, 1])) + np.abs(vn[:, :, 2])
            ok = ((q > 0) & (q < np.inf)).all(axis=1)
            u = interpolate(b, vn)
            ln = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
            ok &= (ln > 0) & (ln < np.inf)
            m = u / ln[:, None]
            mc = np.stack([(m[:, 0] * Rm[0, k] + m[:, 1] * Rm[1, k]) + m[:, 2] * Rm[2, k] for k in range(3)], axis=1)
            mn = np.sqrt((mc[:, 0] * mc[:, 0] + mc[:, 1] * mc[:, 1]) + mc[:, 2] * mc[:, 2])
            nc = np.where(ok[:, None], mc, nc)
            nn = np.where(ok, mn, nn)
            nw = np.where(ok[:, None], m, nw)
        ndl = np.where(nn == 0, T(0), np.abs((nc[:, 0] * px + nc[:, 1] * py) - nc[:, 2] * z) / (nn * r))
        if colors is not None:
            at = interpolate(b, np.asarray(colors, F32).reshape(-1, 3).astype(T)[f])
            col = np.where(at > 0, at, T(0))
            col = np.where(col < 1, col, T(1))
        else:
            at = None
            col = np.broadcast_to(lt[3], (n, 3))
        if mode & UNLIT:
            v = col
        else:
            v = ((((col * lt[0]) / pi) * s[:, None]) * ndl[:, None]) / r2[:, None]
            v = np.where(v < 1, v, T(1))
        level = np.floor(v * T(255) + T(0.5))
    assert level.dtype == T and nw.dtype == T and b.dtype == T
    color = np.full((H * W, 3), 255, np.uint8)
    color[hit] = level.astype(np.uint8)
    normal = np.zeros((H * W, 3), T)
    normal[hit] = nw
    out.update(color=color.reshape(H, W, 3), normal=normal.reshape(H, W, 3), weights=b, hit=hit, level=level)
    if at is not None:
        attr = np.zeros((H * W, 3), T)
        attr[hit] = at
        out["attr"] = attr.reshape(H, W, 3)
    return out


# ---- inputs the tests share -----------------------------------------------------------------------------------------------------------
QUAD_F = 4.0      # fx = fy of the tilted quad's camera: the quad lies inside the spotlight's cone


def tilted_quad():
    """a quad tilted steeply away from the identity camera at the origin (fx = fy = QUAD_F, an 8 x 8 image): depth 1.5 on its left
    edge, 6 on its right one - screen-space weights are far from the perspective-correct ones.  Its corners project to whole pixels (1 and 7): nothing moves when
    they are rounded to 1/256 pixel.  Returns (verts, faces, pose)."""
    verts = np.array([[-0.28125, 0.28125, -1.5], [1.125, 1.125, -6.0], [1.125, -1.125, -6.0], [-0.28125, -0.28125, -1.5]], F32)
    return verts, np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.eye(4)


AFFINE = (np.array([[0.2, 0.08, -0.08], [-0.12, 0.24, 0.04], [0.08, -0.2, 0.06]]), np.array([0.3, 0.5, 0.4]))


def affine_colour(points):
    """a colour that is an affine function of the world position (float64)"""
    return np.asarray(points, np.float64) @ AFFINE[0].T + AFFINE[1]


def position_colour(verts):
    """a smooth colour in about [0, 1] derived from the position (the two-spheres meshes live in [-1, 1]^3)"""
    v = np.asarray(verts, np.float64)
    return (0.5 + 0.45 * np.sin(3.0 * v + np.array([0.0, 1.0, 2.0]))).astype(F32)


def sphere_inputs(n, table):
    """(verts, faces, normals, colours) of raster_restate.two_spheres(n): the mesh with its restated vertex normals"""
    import mc_normals_restate as N
    ax = tuple(np.linspace(-1.0, 1.0, n + k).astype(F32) for k in range(3))
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in ax], indexing="ij")
    sd = np.maximum(0.55 - np.sqrt((X + 0.25) ** 2 + (Y - 0.1) ** 2 + (Z - 0.3) ** 2),
                    0.5 - np.sqrt((X - 0.3) ** 2 + (Y + 0.15) ** 2 + (Z + 0.2) ** 2)).astype(F32)
    v, f = R.two_spheres(n, table)
    nrm = N.normals(sd, ax, 0.0, "ascent")
    assert nrm.shape == v.shape
    return v, f, nrm, position_colour(v)


def spread(a32, a64):
    """what tests/golden/raster_attr_spread.json records of a float32 and a float64 restatement of one input"""
    hit = a32["face"] >= 0
    d = {"covered": int(hit.sum()), "normal": float(np.abs(a32["normal"].astype(np.float64) - a64["normal"]).max())}
    if "attr" in a32:          # (a NaN colour is NaN in both)
        d["attr"] = float(np.nanmax(np.abs(a32["attr"].astype(np.float64) - a64["attr"]), initial=0.0))
    dl = np.abs(a32["level"].astype(np.float64) - a64["level"]).max(axis=1) if a32["level"].size else np.zeros(0)
    d["level_max"] = float(dl.max()) if dl.size else 0.0
    d["level_share"] = float((dl > 0).mean()) if dl.size else 0.0
    return d


MODES = {"smooth_lit": SMOOTH, "smooth_unlit": SMOOTH | UNLIT, "flat_lit": 0}


def quad_inputs():
    """the tilted quad at 8 x 8 with affine colours and normals that vary over it"""
    v, f, pose = tilted_quad()
    nrm = np.array([[0.6, 0.0, 0.8], [0.5, 0.3, 0.7], [0.7, -0.2, 0.6], [0.4, 0.1, 0.9]], F32)
    return dict(verts=v, faces=f, pose=pose, fx=QUAD_F, fy=QUAD_F, H=8, W=8, normals=nrm, colors=affine_colour(v).astype(F32))


def gpu_inputs(table):
    """name -> keyword arguments of raster_attr for every input of tests/test_gpu_raster_attr.py"""
    out = {"quad": quad_inputs()}
    for n, H, W in R.SPHERE_CASES:
        v, f, nrm, col = sphere_inputs(n, table)
        fx, fy = R.default_scales(height=H, width=W)
        out["spheres%d_%dx%d" % (n, H, W)] = dict(verts=v, faces=f, pose=R.DEFAULT_POSE, fx=fx, fy=fy, H=H, W=W, normals=nrm, colors=col)
    return out
