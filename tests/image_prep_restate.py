"""numpy restatement of the image-preparation rule of include/dsnerf.h (dsn_image_undistort, dsn_image_morph, dsn_image_resize,
dsn_image_prep): the undistortion map in float64 with one rounding per operation, the fixed-point bilinear taps with a zero border,
box erode / dilate with the anchor k // 2, the integer-factor resizes, and the two data sets' compositions in the reference's order
(dataloader/zju_mocap_dataset.py:94-123, :192-213; dataloader/h36m_dataset.py:75-96, :128-158, :182-184).  Written for clarity: whole
arrays, no tiles.  The kernels are held to these bits; the rule has the shape of OpenCV's fixed-point path, cv2's own bits are not
claimed."""
import numpy as np

TWO30 = float(2 ** 30)


def _coefficients(D):
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    if D.size not in (4, 5, 8):
        raise ValueError(f"D must have 4, 5 or 8 terms, got {D.size}")
    full = np.zeros(8, dtype=np.float64)
    full[:D.size] = D
    return full          # k1, k2, p1, p2, k3, k4, k5, k6


def undistort_map(K, D, H, W):
    """(iu, iv, ok): the map of every destination pixel in 1/32 pixel (int64), ok False for the outside pixels (iu = iv = 0 there)"""
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be [3, 3]")
    if K[0, 1] != 0:
        raise ValueError("a skew term K[0, 1] is not modelled")
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3, k4, k5, k6 = _coefficients(D)
    j = np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], (H, W))
    i = np.broadcast_to(np.arange(H, dtype=np.float64)[:, None], (H, W))
    with np.errstate(all="ignore"):
        x = (j - cx) / fx
        y = (i - cy) / fy
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        t = (2.0 * x) * y
        num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
        kr = num / den
        xd = (x * kr + p1 * t) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * t
        us = (fx * xd + cx) * 32.0
        vs = (fy * yd + cy) * 32.0
        ok = (np.abs(us) < TWO30) & (np.abs(vs) < TWO30)          # NaN and infinities fail
    iu = np.rint(np.where(ok, us, 0.0)).astype(np.int64)          # np.rint: halves to even
    iv = np.rint(np.where(ok, vs, 0.0)).astype(np.int64)
    return iu, iv, ok


def weights(ax, ay):
    """the four integer tap weights (w00, w01, w10, w11) of the phase (ax, ay) in 0 ... 31: they sum to 1024"""
    return (32 - ay) * (32 - ax), (32 - ay) * ax, ay * (32 - ax), ay * ax


def _taps(src, iu, iv, ok):
    """the four taps [H, W, C] (zero outside the image and for outside pixels) and their integer weights [H, W, 1]"""
    H, W = src.shape[:2]
    s = src.reshape(H, W, -1)
    sx, sy = iu >> 5, iv >> 5          # arithmetic shifts
    ws = weights(iu & 31, iv & 31)
    taps = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = sy + dy, sx + dx
        inside = ok & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = s[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        taps.append(np.where(inside[..., None], v, np.zeros((), dtype=s.dtype)))
    return taps, [w[..., None] for w in ws]


def remap(src, iu, iv, ok):
    """rule 2 on one image [H, W] or [H, W, C], uint8 or float32"""
    src = np.asarray(src)
    taps, ws = _taps(src, iu, iv, ok)
    if src.dtype == np.uint8:
        acc = sum(t.astype(np.int64) * w for t, w in zip(taps, ws))
        out = ((acc + 512) >> 10).astype(np.uint8)
    elif src.dtype == np.float32:
        f = [w.astype(np.float32) / np.float32(1024.0) for w in ws]
        with np.errstate(all="ignore"):
            out = ((taps[0] * f[0] + taps[1] * f[1]) + taps[2] * f[2]) + taps[3] * f[3]
        assert out.dtype == np.float32
    else:
        raise ValueError(f"uint8 or float32, got {src.dtype}")
    return out.reshape(src.shape)


def undistort(src, K, D):
    src = np.asarray(src)
    iu, iv, ok = undistort_map(K, D, src.shape[0], src.shape[1])
    return remap(src, iu, iv, ok)


def morph(m, k, dilate):
    """rule 3: max (dilate) or min over the k x k box anchored at (k // 2, k // 2); outside pixels do not take part"""
    m = np.asarray(m)
    if m.dtype != np.uint8 or m.ndim != 2:
        raise ValueError("uint8 [H, W]")
    if not 1 <= k <= 15:
        raise ValueError("k must be 1 ... 15")
    H, W = m.shape
    a = k // 2
    neutral = 0 if dilate else 255
    padded = np.full((H + k - 1, W + k - 1), neutral, dtype=np.uint8)
    padded[a:a + H, a:a + W] = m
    out = np.full((H, W), neutral, dtype=np.uint8)
    for dy in range(k):
        for dx in range(k):
            win = padded[dy:dy + H, dx:dx + W]          # = m(y - a + dy, x - a + dx)
            out = np.maximum(out, win) if dilate else np.minimum(out, win)
    return out


def dilate(m, k):
    return morph(m, k, True)


def erode(m, k):
    return morph(m, k, False)


def _check_factor(src, c):
    if c not in (1, 2, 4):
        raise ValueError("the factor must be 1, 2 or 4")
    if src.shape[0] % c or src.shape[1] % c:
        raise ValueError("H and W must be multiples of the factor")


def resize_nearest(src, c):
    src = np.asarray(src)
    _check_factor(src, c)
    return np.ascontiguousarray(src[::c, ::c])


def area_u8(s, c):
    """the rounding of a block sum of uint8 levels"""
    s = np.asarray(s, dtype=np.int64)
    if c == 1:
        return s
    if c == 2:
        return (s + 2) >> 2                         # half up
    return (s + 7 + ((s >> 4) & 1)) >> 4            # s / 16, half to even


def resize_area(src, c):
    src = np.asarray(src)
    _check_factor(src, c)
    if c == 1:
        return src.copy()
    H, W = src.shape[0] // c, src.shape[1] // c
    if src.dtype == np.uint8:
        s = np.zeros((H, W) + src.shape[2:], dtype=np.int64)
        for dy in range(c):
            for dx in range(c):
                s += src[dy::c, dx::c]
        return area_u8(s, c).astype(np.uint8)
    if src.dtype == np.float32:
        with np.errstate(all="ignore"):
            s = src[0::c, 0::c].copy()
            for q in range(1, c * c):          # row-major
                s = s + src[q // c::c, q % c::c]
            out = s * np.float32(1.0 / (c * c))
        assert out.dtype == np.float32
        return out
    raise ValueError(f"uint8 or float32, got {src.dtype}")


def zju_steps(img_u8, msk_cihp, K, D, c=2, border=5):
    """rule 5 step by step (one item): every intermediate, by name"""
    img_u8, msk_cihp = np.asarray(img_u8), np.asarray(msk_cihp)
    fg = (msk_cihp != 0).astype(np.uint8)
    fg_u = undistort(fg, K, D)
    msk_fg = dilate(fg_u, border)
    im = undistort(img_u8, K, D) * msk_fg[..., None]
    im_small = resize_area(im, c)
    return {"fg": fg, "fg_u": fg_u, "msk_fg_full": msk_fg, "im": im, "img_u8": im_small, "msk_fg": resize_nearest(msk_fg, c),
            "msk_cihp": resize_nearest(msk_cihp, c)}


def scaled_K(K, c):
    K = np.array(K, dtype=np.float64)
    K[..., :2, :] = K[..., :2, :] * (1.0 / c)
    return K


def prepare_zju(img_u8, msk_cihp, K, D, c=2, border=5, dtype=np.float64):
    """the ZJU item: {"img" [H, W, 3] float64 (or float32: rounded once more), "img_u8", "msk_fg", "msk_cihp", "K"}"""
    st = zju_steps(img_u8, msk_cihp, K, D, c, border)
    img = st["img_u8"].astype(np.float64) / 255.0
    return {"img": img.astype(dtype), "img_u8": st["img_u8"], "msk_fg": st["msk_fg"], "msk_cihp": st["msk_cihp"], "K": scaled_K(K, c)}


def dilate_per_tile(m, k, tile_h, tile_w):
    """what a tiled dilation WITHOUT halo would give (every tile dilated on its own): the mutant the seam tests are built against"""
    out = np.empty_like(m)
    for y in range(0, m.shape[0], tile_h):
        for x in range(0, m.shape[1], tile_w):
            out[y:y + tile_h, x:x + tile_w] = dilate(m[y:y + tile_h, x:x + tile_w], k)
    return out


def prepare_h36m(img_u8, msk, K, D, c=1, is_eval=False):
    """the Human3.6M item, the reference's order (h36m_dataset.py:75-96, :128-158, :182-184)"""
    img_u8, raw = np.asarray(img_u8), np.asarray(msk)
    img = img_u8.astype(np.float32) / np.float32(255.0)
    fg = (raw != 0).astype(np.uint8)
    m = fg.copy()
    if not is_eval:
        m[(dilate(fg, 5) - erode(fg, 5)) == 1] = 100
    img = undistort(img, K, D)
    m = undistort(m, K, D)
    orig = undistort(fg, K, D)
    cihp = undistort(raw, K, D)
    img = resize_area(img, c)
    m = resize_nearest(m, c)
    orig = resize_nearest(orig, c)
    img[orig == 0] = 0
    return {"img": img, "msk": m, "orig_msk": orig, "msk_cihp": cihp, "msk_cihp_eroded": erode(cihp, 10), "K": scaled_K(K, c)}
