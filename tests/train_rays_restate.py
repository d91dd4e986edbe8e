"""numpy restatement of the training-batch sampler of include/dsnerf.h (dsn_train_rays / dsn_bound_mask), the whole rule:

the box mask as the union of the reference's six corner loops (on a segment, or winding number non-zero, exact integers); the three
classes as np.argwhere lists; the counter-hash draws; the reference's rounds with their quotas, the face draws left out when the
face class is empty; status and round count.  The rays and the box test come from oracle.camera_rays_np / camera_rays_h36m_np, the
formulas tests/golden/camera_rays*.npz pin (or from `rays`, e.g. the device's own whole-image call).
tests/golden/make_golden_train_rays.py runs the reference's my_sample_ray and sample_ray_h36m with fill_poly and draw_indices in
the place of cv2.fillPoly and np.random.randint."""
import numpy as np

LOOPS = ((0, 1, 3, 2), (4, 5, 7, 6, 5), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5))     # as the reference writes them
OK, EMPTY_CLASS, SHORT, BAD_CAMERA = 0, 1, 2, 3
MAX_ROUNDS, MAX_RAYS = 64, 65536
ZJU, H36M = "zju", "h36m"
M32 = np.uint64(0xFFFFFFFF)


# ---- box mask ----------------------------------------------------------------------------------------------------------------
def corners_3d(bounds):
    b = np.asarray(bounds, np.float64).reshape(2, 3)
    return np.array([[b[(t >> 2) & 1, 0], b[(t >> 1) & 1, 1], b[t & 1, 2]] for t in range(8)])       # get_bound_corners' order


def project_corners(K, R, T, bounds):
    """float64 (u, v) of the eight corners and their camera z (utils/rays_utils.py:5-14 project)"""
    K, R, T = np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)
    cam = corners_3d(bounds) @ R.T + T
    pix = cam @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return pix[:, :2] / pix[:, 2:], cam[:, 2], pix[:, 2]


def rounded_corners(K, R, T, bounds):
    """int64 [8,2] (x, y), or None where the rule calls the camera an argument error"""
    uv, z, w = project_corners(K, R, T, bounds)
    r = np.round(uv)                                                   # half to even
    if not (np.all(z > 0) and np.all(w > 0) and np.all(np.isfinite(r)) and np.all(np.abs(r) < 2.0 ** 29)):
        return None
    return r.astype(np.int64)


def half_integer_distance(K, R, T, bounds):
    """how far the projected corners stay from a rounding tie (fixtures keep this above 1e-6)"""
    uv = project_corners(K, R, T, bounds)[0]
    return float(np.abs(np.abs(uv - np.floor(uv)) - 0.5).min())


def loop_mask(pts, H, W):
    """bool [H,W]: the pixels of one loop - vertices pts [n,2] (x, y) integers, closed from the last to the first"""
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    out = np.zeros((H, W), bool)
    x0, y0 = max(int(pts[:, 0].min()), 0), max(int(pts[:, 1].min()), 0)
    x1, y1 = min(int(pts[:, 0].max()), W - 1), min(int(pts[:, 1].max()), H - 1)
    if x0 > x1 or y0 > y1:
        return out
    y, x = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
    wn = np.zeros(x.shape, np.int64)
    on = np.zeros(x.shape, bool)
    n = len(pts)
    for e in range(n):
        (ax, ay), (bx, by) = pts[e], pts[(e + 1) % n]
        cross = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
        on |= (cross == 0) & (x >= min(ax, bx)) & (x <= max(ax, bx)) & (y >= min(ay, by)) & (y <= max(ay, by))
        if ay <= by:
            wn += (ay <= y) & (by > y) & (cross > 0)
        else:
            wn -= (ay > y) & (by <= y) & (cross < 0)
    out[y0:y1 + 1, x0:x1 + 1] = on | (wn != 0)
    return out


def fill_poly(mask, pts, color):
    """cv2.fillPoly's place in the reference's get_bound_2d_mask: the loop rule above, in place"""
    for p in pts:
        mask[loop_mask(np.asarray(p).reshape(-1, 2), *mask.shape)] = color
    return mask


def bound_mask_from_corners(c, H, W):
    m = np.zeros((H, W), np.uint8)
    for loop in LOOPS:
        fill_poly(m, [c[list(loop)]], 1)
    return m


def bound_mask(K, R, T, bounds, H, W):
    c = rounded_corners(K, R, T, bounds)
    return np.zeros((H, W), np.uint8) if c is None else bound_mask_from_corners(c, H, W)


# ---- draws -------------------------------------------------------------------------------------------------------------------
def mix(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def hash32(seed, r, c, k):
    """h(seed, r, c, k) of the header; k may be an array"""
    base = mix(np.uint64((int(seed) + 0x9E3779B9 * (3 * int(r) + int(c))) & 0xFFFFFFFF))
    return mix(base ^ np.asarray(k, np.uint64))


def draw_indices(seed, r, c, n, count):
    """list entries of slots 0 ... n-1 of class c in round r: (h * count) >> 32"""
    return ((hash32(seed, r, c, np.arange(n, dtype=np.uint64)) * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def quotas(rem):
    n_body, n_face = rem * 6 // 10, rem * 5 // 100
    return n_body, n_face, rem - n_body - n_face


# ---- the batch ---------------------------------------------------------------------------------------------------------------
def whole_image_rays(K, R, T, bounds, H, W, convention):
    import oracle as O
    f = O.camera_rays_h36m_np if convention == H36M else O.camera_rays_np
    return f(K, R, T, bounds, H, W)


def classes(mask_a, mask_b, bound, convention):
    """flat pixel lists (row-major) of body, face, random"""
    a, b = np.asarray(mask_a).reshape(-1), np.asarray(bound).reshape(-1) == 1
    if convention == H36M:
        body, face, rand = b & (a == 1), np.asarray(mask_b).reshape(-1) == 2, b & (a != 100)
    else:
        body, face, rand = a != 0, a == 2, b
    return [np.flatnonzero(m) for m in (body, face, rand)]


def sample(img, K, R, T, bounds, mask_a, nrays, seed, convention=ZJU, mask_b=None, bound_mask_in=None, occupancy_src=None, rays=None):
    """the batch of dsn_train_rays as numpy arrays.  rays: (ray_o, ray_d, near, far, hit) over all pixels (default: the oracle's)."""
    H, W = np.asarray(img).shape[:2]
    assert 1 <= nrays <= MAX_RAYS and convention in (ZJU, H36M)
    n = int(nrays)
    out = {"ray_o": np.zeros((n, 3), np.float32), "ray_d": np.zeros((n, 3), np.float32), "near": np.zeros(n, np.float32),
           "far": np.zeros(n, np.float32), "coord": np.zeros((n, 2), np.int64), "rgb": np.zeros((n, 3), np.float32),
           "mask_at_box": np.zeros(n, bool), "rounds": 0, "occupancy": None if occupancy_src is None else np.zeros(n, np.uint8)}
    if bound_mask_in is None:
        c = rounded_corners(K, R, T, bounds)
        bound = np.zeros((H, W), np.uint8) if c is None else bound_mask_from_corners(c, H, W)
        out["bound_mask"] = bound
        if c is None:
            out["status"] = BAD_CAMERA
            return out
    else:
        bound = np.asarray(bound_mask_in, np.uint8).copy()
        out["bound_mask"] = bound
    lists = classes(mask_a, mask_b, bound, convention)
    count = [len(l) for l in lists]
    if count[0] == 0 or count[2] == 0:
        out["status"] = EMPTY_CLASS
        return out
    ray_o, ray_d, near, far, hit = rays if rays is not None else whole_image_rays(K, R, T, bounds, H, W, convention)
    hit = np.asarray(hit).reshape(-1).astype(bool)
    got, have, r = [], 0, 0
    while have < n and r < MAX_ROUNDS:
        n_body, n_face, n_rand = quotas(n - have)
        parts = [lists[0][draw_indices(seed, r, 0, n_body, count[0])]]
        if count[1] > 0:
            parts.append(lists[1][draw_indices(seed, r, 1, n_face, count[1])])
        parts.append(lists[2][draw_indices(seed, r, 2, n_rand, count[2])])
        cand = np.concatenate(parts)
        acc = cand[hit[cand]]
        got.append(acc)
        have += len(acc)
        r += 1
    p = np.concatenate(got)
    k = len(p)
    out["rounds"], out["status"] = r, OK if k == n else SHORT
    out["ray_o"][:k], out["ray_d"][:k] = np.asarray(ray_o)[p], np.asarray(ray_d)[p]
    out["near"][:k], out["far"][:k] = np.asarray(near)[p], np.asarray(far)[p]
    out["coord"][:k, 0], out["coord"][:k, 1] = p // W, p % W
    rgb = np.asarray(img).reshape(-1, 3)[p].astype(np.float32)
    if convention == H36M:
        rgb[bound.reshape(-1)[p] != 1] = 0
    out["rgb"][:k] = rgb
    out["mask_at_box"][:k] = True
    if occupancy_src is not None:
        out["occupancy"][:k] = np.asarray(occupancy_src, np.uint8).reshape(-1)[p]
    return out
