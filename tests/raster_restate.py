"""numpy restatement of the mesh rasteriser of include/dsnerf.h (dsn_raster_mesh): float32 with int64 edge functions, in the order of
operations the header spells out (numpy does not fuse), vectorised over (triangle, pixel of its bounding box) pairs.

raster(...) returns face [H, W] int32 (-1 empty), depth [H, W] float32 (0 empty), color [H, W, 3] uint8 (255 empty), and for the tests
depth2 [H, W] float32 (the second-nearest fragment's depth, inf where there is none) and count [H, W] (fragments per pixel).
shade_levels(..., dtype=np.float64) evaluates the shading of the same winners in float64."""
import numpy as np

GUARD = 2.0 ** 24
DEFAULT_POSE = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.5], [0.0, 0.0, 0.0, 1.0]])
F32 = np.float32


def default_scales(yfov=np.pi / 3, height=1, width=1):
    """(fx, fy) as the binding computes them (float64, then rounded to float32)"""
    fy = 1.0 / np.tan(0.5 * float(yfov))
    return float(F32(fy * float(height) / float(width))), float(F32(fy))


def light_values(intensity=30.0, inner=np.pi / 16, outer=np.pi / 6, base=0.3):
    """light_host of dsn_raster_mesh: {intensity, cos_inner, cos_outer, base} float32"""
    return np.array([intensity, np.cos(inner), np.cos(outer), base], dtype=F32)


def camera_coords(verts, pose, dtype=F32):
    """c_k = (d0 R0k + d1 R1k) + d2 R2k with d = v - t"""
    v = np.asarray(verts, F32).reshape(-1, 3).astype(dtype)
    P = np.asarray(pose, F32).reshape(-1, 4)[:3].astype(dtype)
    R, t = P[:, :3], P[:, 3]
    with np.errstate(all="ignore"):
        d = v - t
        return np.stack([(d[:, 0] * R[0, k] + d[:, 1] * R[1, k]) + d[:, 2] * R[2, k] for k in range(3)], axis=1)


def project(verts, pose, fx, fy, znear, H, W):
    """(X, Y int64, iw float32, valid) per vertex"""
    c = camera_coords(verts, pose)
    with np.errstate(all="ignore"):
        w = -c[:, 2]
        xn = (F32(fx) * c[:, 0]) / w
        yn = (F32(fy) * c[:, 1]) / w
        px = (xn + F32(1)) * (F32(W) * F32(0.5))
        py = (F32(1) - yn) * (F32(H) * F32(0.5))
        rx, ry = np.rint(px * F32(256)), np.rint(py * F32(256))
        valid = (w > F32(znear)) & np.isfinite(px) & np.isfinite(py) & (np.abs(rx) <= GUARD) & (np.abs(ry) <= GUARD)
        iw = F32(1) / w
    X = np.where(valid, rx, 0).astype(np.int64)
    Y = np.where(valid, ry, 0).astype(np.int64)
    return X, Y, iw.astype(F32), valid


def setup(verts, faces, pose, fx, fy, znear, H, W):
    """the triangles that are kept and whose pixel bounding box is not empty: (face ids, X [n, 3], Y [n, 3], area, iw [n, 3], x0, y0, bw, bh),
    vertices in the order P of the rule (1 and 2 swapped where the area was negative)"""
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V = np.asarray(verts).reshape(-1, 3).shape[0]
    X, Y, iw, valid = project(verts, pose, fx, fy, znear, H, W)
    inr = ((faces >= 0) & (faces < V)).all(axis=1)
    fid = np.flatnonzero(inr)
    f = faces[fid]
    ok = valid[f].all(axis=1)
    fid, f = fid[ok], f[ok]
    px, py = X[f], Y[f]                                     # [n, 3]
    area = (px[:, 1] - px[:, 0]) * (py[:, 2] - py[:, 0]) - (py[:, 1] - py[:, 0]) * (px[:, 2] - px[:, 0])
    nz = area != 0
    fid, f, px, py, area = fid[nz], f[nz], px[nz], py[nz], area[nz]
    neg = area < 0                                         # two-sided: (v0, v2, v1)
    order = np.where(neg[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    rows = np.arange(f.shape[0])[:, None]
    f, px, py, area = f[rows, order], px[rows, order], py[rows, order], np.abs(area)
    tiw = iw[f]
    x0 = np.maximum((px.min(axis=1) + 127) >> 8, 0)
    x1 = np.minimum((px.max(axis=1) - 128) >> 8, W - 1)
    y0 = np.maximum((py.min(axis=1) + 127) >> 8, 0)
    y1 = np.minimum((py.max(axis=1) - 128) >> 8, H - 1)
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    keep = (bw > 0) & (bh > 0)
    return tuple(a[keep] for a in (fid, px, py, area, tiw, x0, y0, bw, bh))


def box_pixels(verts, faces, pose, fx, fy, znear, H, W):
    """pixels in every face's bounding box (0: dropped or off the image) - what selects the wave form of the kernel"""
    fid, _, _, _, _, _, _, bw, bh = setup(verts, faces, pose, fx, fy, znear, H, W)
    out = np.zeros(np.asarray(faces).reshape(-1, 3).shape[0], np.int64)
    out[fid] = bw * bh
    return out


def fragments(verts, faces, pose, fx, fy, znear, H, W, chunk=1 << 21):
    """every covered (pixel, triangle): (pixel index, key = depth bits << 32 | face) arrays"""
    fid, px, py, area, tiw, x0, y0, bw, bh = setup(verts, faces, pose, fx, fy, znear, H, W)
    cnt = bw * bh
    pix_out, key_out = [], []
    start = 0
    n = fid.shape[0]
    csum = np.cumsum(cnt)
    while start < n:
        # triangles [start, stop): at most `chunk` candidate pixels (always at least one triangle)
        base = csum[start - 1] if start else 0
        stop = max(start + 1, int(np.searchsorted(csum, base + chunk, side="right")))
        sl = slice(start, stop)
        c = cnt[sl]
        tri = np.repeat(np.arange(start, stop), c)
        local = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        x = x0[tri] + local % bw[tri]
        y = y0[tri] + local // bw[tri]
        cx, cy = 256 * x + 128, 256 * y + 128
        E = []
        cov = np.ones(tri.shape[0], dtype=bool)
        for k in range(3):          # the edge opposite P[k]: from P[k + 1] to P[k + 2]
            a, b = (k + 1) % 3, (k + 2) % 3
            dx, dy = px[tri, b] - px[tri, a], py[tri, b] - py[tri, a]
            e = dx * (cy - py[tri, a]) - dy * (cx - px[tri, a])
            top_left = (dy < 0) | ((dy == 0) & (dx > 0))
            cov &= (e > 0) | ((e == 0) & top_left)
            E.append(e)
        tri, x, y = tri[cov], x[cov], y[cov]
        fa = area[tri].astype(F32)
        with np.errstate(all="ignore"):
            lam = [E[k][cov].astype(F32) / fa for k in range(3)]
            q = (lam[0] * tiw[tri, 0] + lam[1] * tiw[tri, 1]) + lam[2] * tiw[tri, 2]
            z = (F32(1) / q).astype(F32)
        key_out.append((z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | fid[tri].astype(np.uint64))
        pix_out.append(y * W + x)
        start = stop
    if not pix_out:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    return np.concatenate(pix_out), np.concatenate(key_out)


def shade_levels(verts, faces, pose, fx, fy, light, H, W, face, depth, dtype=F32):
    """the level (float, already floored) of every covered pixel, in pixel order, evaluated in `dtype`"""
    T = dtype
    hit = np.flatnonzero(face.reshape(-1) >= 0)
    f = np.asarray(faces).reshape(-1, 3)[face.reshape(-1)[hit]]
    z = depth.reshape(-1)[hit].astype(T)
    y, x = hit // W, hit % W
    fx, fy = T(F32(fx)), T(F32(fy))
    light = np.asarray(light, F32).astype(T)
    k = (light[3] * light[0]) / T(F32(np.pi) if T is F32 else np.pi)
    ci, co = light[1], light[2]
    c = camera_coords(verts, pose, T)
    with np.errstate(all="ignore"):
        xn = (2 * x + 1).astype(T) / T(W) - T(1)
        yn = T(1) - (2 * y + 1).astype(T) / T(H)
        px, py = (xn * z) / fx, (yn * z) / fy
        r2 = (px * px + py * py) + z * z
        r = np.sqrt(r2)
        s = (z / r - co) / (ci - co)
        s = np.where(s > 0, s, T(0))
        s = np.where(s < 1, s, T(1))
        s = s * s
        a, b = c[f[:, 1]] - c[f[:, 0]], c[f[:, 2]] - c[f[:, 0]]
        n0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        n1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        n2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        nn = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        ndl = np.where(nn == 0, T(0), np.abs((n0 * px + n1 * py) - n2 * z) / (nn * r))
        col = ((k * s) * ndl) / r2
        level = np.floor(np.where(col < 1, col, T(1)) * T(255) + T(0.5))
    assert level.dtype == T
    return hit, level


def raster(verts, faces, pose=None, fx=None, fy=None, znear=0.05, light=None, H=64, W=None):
    W = H if W is None else W
    pose = DEFAULT_POSE if pose is None else pose
    if fx is None or fy is None:
        fx, fy = default_scales(height=H, width=W)
    light = light_values() if light is None else light
    pix, key = fragments(verts, faces, pose, fx, fy, znear, H, W)
    face = np.full(H * W, -1, np.int32)
    depth = np.zeros(H * W, F32)
    depth2 = np.full(H * W, np.inf, F32)
    count = np.bincount(pix, minlength=H * W).astype(np.int64)
    if pix.size:
        o = np.lexsort((key, pix))
        pix, key = pix[o], key[o]
        first = np.flatnonzero(np.r_[True, pix[1:] != pix[:-1]])
        win = key[first]
        face[pix[first]] = (win & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)
        depth[pix[first]] = (win >> np.uint64(32)).astype(np.uint32).view(F32)
        second = first + 1
        second = second[(second < pix.size)]
        second = second[pix[second] == pix[second - 1]]
        depth2[pix[second]] = (key[second] >> np.uint64(32)).astype(np.uint32).view(F32)
    face, depth, depth2, count = (a.reshape(H, W) for a in (face, depth, depth2, count))
    color = np.full((H * W, 3), 255, np.uint8)
    hit, level = shade_levels(verts, faces, pose, fx, fy, light, H, W, face, depth)
    color[hit] = level.astype(np.uint8)[:, None]
    return {"face": face, "depth": depth, "depth2": depth2, "count": count, "color": color.reshape(H, W, 3)}


def ulp_gap(depth, depth2):
    """distance in float32 steps between the two nearest fragments of every pixel (a large number where there is one or none)"""
    a = depth.view(np.uint32).astype(np.int64)
    b = np.where(np.isfinite(depth2), depth2, F32(0)).view(np.uint32).astype(np.int64)
    return np.where(np.isfinite(depth2) & (depth > 0), b - a, np.int64(1) << 40)


# ---- meshes the tests share ---------------------------------------------------------------------------------------------------------
def exact_quad(w=4.0):
    """two triangles in the plane z = -w whose corners and shared diagonal land on pixel centres of an 8 x 8 image with fx = fy = 1
    and the identity pose at the origin: corners at pixel centres (1.5, 1.5) ... (5.5, 5.5)"""
    ndc = lambda p: p / 4.0 - 1.0                # px = (xn + 1) 4
    l, r = ndc(1.5) * w, ndc(5.5) * w
    t, b = -ndc(1.5) * w, -ndc(5.5) * w          # py = (1 - yn) 4: row 0 is the top
    verts = np.array([[l, t, -w], [r, t, -w], [r, b, -w], [l, b, -w]], F32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    pose = np.eye(4)
    return verts, faces, pose


def screen_mesh(tris_px, w, H, W):
    """triangles given by their corners in pixel coordinates ([n, 3, 2]: x to the right, y down), in the plane at distance w[n] in front
    of the identity camera at the origin with fx = fy = 1 (exact where H, W and w are powers of two and the corners dyadic)"""
    t = np.asarray(tris_px, np.float64).reshape(-1, 3, 2)
    w = np.broadcast_to(np.asarray(w, np.float64), (t.shape[0],))[:, None]
    x = (t[:, :, 0] / (W / 2.0) - 1.0) * w
    y = (1.0 - t[:, :, 1] / (H / 2.0)) * w
    verts = np.stack([x, y, -np.broadcast_to(w, x.shape)], axis=-1).reshape(-1, 3).astype(F32)
    return verts, np.arange(verts.shape[0], dtype=np.int32).reshape(-1, 3), np.eye(4)


def box_tri(x0, y0, bw, bh):
    """a right triangle whose bounding box holds exactly the bw x bh pixel centres from (x0, y0)"""
    return [[x0 + 0.25, y0 + 0.25], [x0 + bw - 0.25, y0 + 0.25], [x0 + 0.25, y0 + bh - 0.25]]


def big_triangle_mesh():
    """(verts, faces, pose) for a 256 x 256 image with fx = fy = 1: bounding boxes of 15, 16 (DSN_RM_BIG_PIXELS), 17 and 10 000 pixels
    and one triangle over the whole image, each behind the one before where they overlap"""
    tris = [box_tri(3, 5, 3, 5), box_tri(20, 5, 4, 4), box_tri(40, 5, 1, 17), box_tri(60, 40, 100, 100), [[-300, -300], [900, -300], [-300, 900]]]
    return screen_mesh(tris, [2.0, 2.0, 2.0, 4.0, 8.0], 256, 256)


def two_spheres(n, table):
    """marching-cubes mesh (tests/mc_restate.py, the library's table) of two overlapping spheres, one partly in front of the other as
    the default camera sees them, on an n x (n + 1) x (n + 2) grid"""
    import mc_restate as M
    ax = tuple(np.linspace(-1.0, 1.0, n + k).astype(F32) for k in range(3))
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in ax], indexing="ij")
    sd = np.maximum(0.55 - np.sqrt((X + 0.25) ** 2 + (Y - 0.1) ** 2 + (Z - 0.3) ** 2),
                    0.5 - np.sqrt((X - 0.3) ** 2 + (Y + 0.15) ** 2 + (Z + 0.2) ** 2))
    return M.marching_cubes(sd.astype(F32), ax, 0.0, "ascent", table)


# (grid size, H, W) of the two-spheres cases: sizes off any tile, W != H, occlusion
SPHERE_CASES = [(34, 64, 64), (40, 80, 96), (28, 53, 37)]
