"""The image-preparation rule of include/dsnerf.h without a GPU: the numpy restatement (tests/image_prep_restate.py) against closed
forms and scipy's grey morphology, the order of the ZJU pipeline against a run of the reference's own code, and the argument checks of
the library and its wrappers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import image_prep_restate as IP
from helpers import GOLDEN

K0 = np.array([[37.25, 0.0, 23.5], [0.0, 36.5, 19.75], [0.0, 0.0, 1.0]])


def shift_map(H, W, du32, dv32):
    """the map of a pure shift by (du32, dv32) / 32 pixel.  (With D = 0 the rule's map is the identity whatever K is - u = fx ((j - cx) /
    fx) + cx - so a shift cannot be crafted through cx alone; the closed forms below put it into the map itself.)"""
    iu = np.broadcast_to(32 * np.arange(W, dtype=np.int64)[None, :] + du32, (H, W))
    iv = np.broadcast_to(32 * np.arange(H, dtype=np.int64)[:, None] + dv32, (H, W))
    return iu, iv, np.ones((H, W), dtype=bool)


# ---- 1. map and taps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [K0, np.array([[1234.567, 0, 511.3], [0, 1233.9, 498.7], [0, 0, 1.0]])])
def test_zero_distortion_is_the_identity(K):
    rng = np.random.RandomState(0)
    H, W = 40, 48
    iu, iv, ok = IP.undistort_map(K, np.zeros(5), H, W)
    assert ok.all() and np.array_equal(iu, shift_map(H, W, 0, 0)[0]) and np.array_equal(iv, shift_map(H, W, 0, 0)[1])
    for src in (rng.randint(0, 256, (H, W)).astype(np.uint8), rng.randint(0, 256, (H, W, 3)).astype(np.uint8),
                rng.randn(H, W).astype(np.float32), rng.randn(H, W, 3).astype(np.float32)):
        out = IP.undistort(src, K, np.zeros(4))
        assert out.dtype == src.dtype and out.tobytes() == src.tobytes()


def test_half_pixel_shift_closed_forms():
    rng = np.random.RandomState(1)
    H, W = 9, 11
    src = rng.randint(0, 256, (H, W)).astype(np.uint8)
    s = src.astype(np.int64)
    right = np.concatenate([s[:, 1:], np.zeros((H, 1), np.int64)], axis=1)          # the tap past the last column reads 0
    down = np.concatenate([s[1:], np.zeros((1, W), np.int64)], axis=0)
    diag = np.concatenate([right[1:], np.zeros((1, W), np.int64)], axis=0)
    assert np.array_equal(IP.remap(src, *shift_map(H, W, 16, 0)), (s + right + 1) >> 1)
    assert np.array_equal(IP.remap(src, *shift_map(H, W, 0, 16)), (s + down + 1) >> 1)
    assert np.array_equal(IP.remap(src, *shift_map(H, W, 16, 16)), (s + right + down + diag + 2) >> 2)
    assert np.array_equal(IP.remap(src, *shift_map(H, W, 8, 0)), (3 * s + right + 2) >> 2)
    f = src.astype(np.float32)
    fr = right.astype(np.float32)
    assert np.array_equal(IP.remap(f, *shift_map(H, W, 16, 0)), f * np.float32(0.5) + fr * np.float32(0.5))
    # a whole-pixel shift moves the image and fills with 0
    assert np.array_equal(IP.remap(src, *shift_map(H, W, 32, -64))[2:, :-1], src[:-2, 1:])
    assert not IP.remap(src, *shift_map(H, W, 32, -64))[:2].any()


def test_weights_sum_to_1024_in_every_phase():
    ax, ay = np.meshgrid(np.arange(32), np.arange(32))
    w = IP.weights(ax, ay)
    assert all((v >= 0).all() for v in w) and np.all(sum(w) == 1024)
    assert IP.weights(0, 0) == (1024, 0, 0, 0) and IP.weights(31, 31) == (1, 31, 31, 961)


def test_outside_pixels_and_partial_taps():
    H, W = 6, 7
    src = np.full((H, W), 200, dtype=np.uint8)
    fsrc = np.full((H, W), 2.0, dtype=np.float32)
    # half a pixel beyond the last column: one tap inside, one outside -> half the level; a whole pixel beyond: 0
    assert np.all(IP.remap(src, *shift_map(H, W, 16, 0))[:, -1] == 100) and np.all(IP.remap(fsrc, *shift_map(H, W, 16, 0))[:, -1] == 1.0)
    assert np.all(IP.remap(src, *shift_map(H, W, -16, 0))[:, 0] == 100) and np.all(IP.remap(src, *shift_map(H, W, 0, -24))[0] == 50)
    assert np.all(IP.remap(src, *shift_map(H, W, 32, 0))[:, -1] == 0) and np.all(IP.remap(src, *shift_map(H, W, -33, 0))[:, 0] == 0)
    # NaN, infinite and huge maps are outside pixels: all taps zero
    for bad in (np.nan, np.inf, 1e300):
        K = K0.copy()
        K[0, 2] = bad
        iu, iv, ok = IP.undistort_map(K, np.zeros(4), H, W)
        assert not ok.any()
        assert not IP.undistort(src, K, np.zeros(4)).any() and not IP.undistort(fsrc, K, np.zeros(4)).any()
    # the 2^30 edge: u 32 = 2^30 is outside, the value below it is not
    K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    big = float(2 ** 25)          # x = j; xd = x kr with kr = 1 + k1 j^2
    for k1, inside in ((big - 1.0, False), (big - 1.5, True)):
        _, _, ok = IP.undistort_map(K, [k1, 0, 0, 0], 1, 2)          # j = 1: u = 1 + k1, u 32 = 2^30 or 2^30 - 16
        assert bool(ok[0, 1]) == inside and ok[0, 0]
    # a strong distortion sends a band of border pixels outside the image
    iu, iv, ok = IP.undistort_map(np.array([[30.0, 0, 24], [0, 30.0, 20], [0, 0, 1]]), [2.5, 0, 0, 0], 40, 48)
    out = IP.undistort(np.full((40, 48), 255, np.uint8), np.array([[30.0, 0, 24], [0, 30.0, 20], [0, 0, 1]]), [2.5, 0, 0, 0])
    assert ok.all() and (out[0] == 0).all() and (out[:, 0] == 0).all() and out[20, 24] == 255


def test_rint_ties_go_to_even():
    K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])          # row 0, column 1: x = 1, y = 0, u = 1 + k1 exactly
    for k1, want in ((1 / 64, 32), (3 / 64, 34), (5 / 64, 34), (7 / 64, 36), (-1 / 64, 32), (-3 / 64, 30)):
        iu, iv, ok = IP.undistort_map(K, [k1, 0, 0, 0], 1, 2)
        assert ok.all() and iu[0, 1] == want and iv[0, 1] == 0, (k1, iu)


def test_coefficient_counts():
    D8 = np.array([-0.3, 0.1, 1e-3, -2e-3, 0.02, 0.01, -0.02, 0.005])
    a = IP.undistort_map(K0, D8[:4], 20, 24)
    b = IP.undistort_map(K0, np.concatenate([D8[:4], [0.0]]), 20, 24)
    c = IP.undistort_map(K0, np.concatenate([D8[:4], np.zeros(4)]), 20, 24)
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c))
    assert not np.array_equal(IP.undistort_map(K0, D8, 20, 24)[0], IP.undistort_map(K0, D8[:5], 20, 24)[0])
    with pytest.raises(ValueError):
        IP.undistort_map(K0, D8[:6], 20, 24)
    Ks = K0.copy()
    Ks[0, 1] = 0.1
    with pytest.raises(ValueError):
        IP.undistort_map(Ks, D8, 20, 24)


# ---- 2. morphology ----------------------------------------------------------------------------------------------------------------------
# scipy.ndimage.grey_erosion(size=(k, k), origin=0) takes the window y - k // 2 ... y + k - 1 - k // 2: the rule's anchor.  Its
# grey_dilation mirrors the window, so for an even k it needs origin = -1 in both axes to reach k // 2 up / left; odd k: origin 0.
def scipy_morph(m, k, dilate):
    ndi = pytest.importorskip("scipy.ndimage")
    if dilate:
        return ndi.grey_dilation(m, size=(k, k), mode="constant", cval=0, origin=0 if k % 2 else -1)
    return ndi.grey_erosion(m, size=(k, k), mode="constant", cval=255, origin=0)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 10, 15])
@pytest.mark.parametrize("dilate", [True, False])
def test_morphology_against_scipy(k, dilate):
    rng = np.random.RandomState(k)
    for density in (0.01, 0.5, 0.99):
        m = (rng.rand(37, 53) < density).astype(np.uint8)
        assert np.array_equal(IP.morph(m, k, dilate), scipy_morph(m, k, dilate)), density
    labels = rng.randint(0, 20, (24, 31)).astype(np.uint8)          # label maps, values other than 0 / 1
    assert np.array_equal(IP.morph(labels, k, dilate), scipy_morph(labels, k, dilate))


@pytest.mark.parametrize("k", [2, 5, 10])
def test_morphology_edge_masks_and_anchor(k):
    H, W = 12, 14
    for v in (0, 255):
        m = np.full((H, W), v, np.uint8)
        assert np.array_equal(IP.dilate(m, k), m) and np.array_equal(IP.erode(m, k), m)          # the border takes no part
    a = k // 2
    for (y, x) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (6, 7)):
        m = np.zeros((H, W), np.uint8)
        m[y, x] = 1
        want = np.zeros((H, W), np.uint8)          # dst(y', x') sees src(y' - a ... y' + k - 1 - a): the pixel spreads a DOWN, k - 1 - a UP
        want[max(0, y - (k - 1 - a)):y + a + 1, max(0, x - (k - 1 - a)):x + a + 1] = 1
        assert np.array_equal(IP.dilate(m, k), want), (y, x)
        hole = 255 - 255 * m
        assert np.array_equal(IP.erode(hole.astype(np.uint8), k), (255 - 255 * want).astype(np.uint8))


# ---- 3. resizes --------------------------------------------------------------------------------------------------------------------------
def test_area_rounding_ties():
    # c = 2 rounds half up: block sums 4 q + 2 -> q + 1
    blocks = np.array([[0, 0, 1, 1], [1, 1, 2, 3], [255, 255, 255, 253], [2, 0, 0, 0]], dtype=np.uint8)          # sums 2, 7, 1018, 2
    src = blocks.reshape(4, 2, 2).transpose(1, 0, 2).reshape(2, 8)
    assert IP.resize_area(src, 2).tolist() == [[1, 2, 255, 1]]
    assert [int(IP.area_u8(s, 2)) for s in (1, 2, 3, 5, 6, 1020)] == [0, 1, 1, 1, 2, 255]
    # c = 4 rounds half to even: sums 16 q + 8 -> q for even q, q + 1 for odd q
    assert [int(IP.area_u8(s, 4)) for s in (7, 8, 9, 23, 24, 25, 40, 56, 4072, 4080)] == [0, 0, 1, 1, 2, 2, 2, 4, 254, 255]
    for s in range(0, 4081):
        assert int(IP.area_u8(s, 4)) == int(np.rint(s / 16.0)), s
    src = np.zeros((4, 8), np.uint8)
    src[0, 0], src[0, 4:8] = 8, (10, 10, 4, 0)          # sums 8 (tie -> 0) and 24 (tie -> 2)
    assert IP.resize_area(src, 4).tolist() == [[0, 2]]
    f = np.arange(32, dtype=np.float32).reshape(4, 8)
    assert IP.resize_area(f, 2).tolist() == [[4.5, 6.5, 8.5, 10.5], [20.5, 22.5, 24.5, 26.5]]
    # float32: the row-major order matters
    g = np.array([[1e8, 1.0], [-1e8, 1.0]], dtype=np.float32)
    assert IP.resize_area(g, 2)[0, 0] == np.float32(((np.float32(1e8) + np.float32(1)) + np.float32(-1e8)) + np.float32(1)) * np.float32(0.25)


def test_nearest_and_copy_and_bad_sizes():
    rng = np.random.RandomState(3)
    src = rng.randint(0, 256, (8, 12, 3)).astype(np.uint8)
    for c in (1, 2, 4):
        assert np.array_equal(IP.resize_nearest(src, c), src[::c, ::c])
    assert np.array_equal(IP.resize_area(src, 1), src)
    for bad in (np.zeros((7, 8), np.uint8), np.zeros((8, 10), np.uint8)):
        with pytest.raises(ValueError):
            IP.resize_area(bad, 4)
        with pytest.raises(ValueError):
            IP.resize_nearest(bad, 4)
    with pytest.raises(ValueError):
        IP.resize_area(src, 3)


# ---- 4. the ZJU item ---------------------------------------------------------------------------------------------------------------------
def zju_case(H=40, W=48, seed=5):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    cihp = np.zeros((H, W), np.uint8)
    cihp[H // 4:3 * H // 4, W // 3:2 * W // 3] = rng.randint(1, 20, (3 * H // 4 - H // 4, 2 * W // 3 - W // 3))
    cihp[rng.rand(H, W) < 0.02] = 7
    K = np.array([[0.9 * W, 0.0, W / 2 - 0.3], [0.0, 0.92 * W, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    D = np.array([-0.3, 0.12, 1.5e-3, -2e-3, 0.03])
    return img, cihp, K, D


@pytest.mark.parametrize("c", [1, 2, 4])
def test_prepare_zju_is_the_composition(c):
    img, cihp, K, D = zju_case()
    out = IP.prepare_zju(img, cihp, K, D, c=c, border=5)
    fg_u = IP.undistort((cihp != 0).astype(np.uint8), K, D)
    msk_fg = IP.dilate(fg_u, 5)
    im = IP.undistort(img, K, D) * msk_fg[..., None]
    assert np.array_equal(out["img_u8"], IP.resize_area(im, c)) and np.array_equal(out["msk_fg"], msk_fg[::c, ::c])
    # the RAW mask is handed through, not the undistorted one
    assert np.array_equal(out["msk_cihp"], cihp[::c, ::c])
    assert not np.array_equal(out["msk_cihp"], IP.undistort(cihp, K, D)[::c, ::c])
    assert out["img"].dtype == np.float64 and np.array_equal(out["img"], out["img_u8"] / 255.0)
    assert np.array_equal(out["K"][:2], K[:2] * (1.0 / c)) and np.array_equal(out["K"][2], K[2])
    assert set(np.unique(out["msk_fg"])) <= {0, 1} and out["msk_fg"].any() and not out["msk_fg"].all()
    assert not out["img_u8"][out["msk_fg"] == 0].any() if c == 1 else True


def test_division_by_255_for_all_levels():
    levels = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    K = np.array([[20.0, 0, 8], [0, 20.0, 8], [0, 0, 1]])
    ones = np.ones((16, 16), np.uint8)
    out64 = IP.prepare_zju(levels, ones, K, np.zeros(4), c=1, border=1)
    out32 = IP.prepare_zju(levels, ones, K, np.zeros(4), c=1, border=1, dtype=np.float32)
    assert out32["img"].dtype == np.float32
    for v in range(256):
        assert out64["img"][v // 16, v % 16, 0] == v / 255.0
        assert out32["img"][v // 16, v % 16, 0] == np.float32(v / 255.0)


def test_pipeline_order_is_the_references():
    """tests/golden/image_prep.npz (made by tests/golden/make_golden_image_prep.py): the reference's Mocap_Base.get_mask and the image
    lines of its __getitem__, run with cv2 replaced by shims built on this restatement.  ONLY THE ORDER of the operations comes from
    the reference here - which array is undistorted, dilated, multiplied, resized and divided, and which mask is handed on raw - not
    cv2's arithmetic."""
    path = os.path.join(GOLDEN, "image_prep.npz")
    g = np.load(path)
    for tag in ("half", "full"):
        c = int(g[f"{tag}_c"])
        out = IP.prepare_zju(g["img"], g["msk_cihp"], g["K"], g["D"], c=c, border=5)
        assert np.array_equal(out["img"], g[f"{tag}_img"]) and out["img"].dtype == g[f"{tag}_img"].dtype
        assert np.array_equal(out["msk_fg"], g[f"{tag}_msk_fg"])
        assert np.array_equal(out["msk_cihp"], g[f"{tag}_msk_cihp"])
        assert np.array_equal(out["K"], g[f"{tag}_K"])


# ---- 5. argument checks through the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    return dsnerf_amd._lib


def test_library_argument_checks(L):
    lib = L.lib()
    one, two = C.c_void_p(64), C.c_void_p(4096)          # (never dereferenced: every call below returns before anything is enqueued)

    def refused(name, msg, rc):
        assert rc != 0, (name, msg)
        err = lib.dsn_last_error()
        assert name in err and msg in err, (name, msg, err)

    und = lambda src=one, dst=two, K=one, D=one, nd=5, N=1, H=8, W=8, ch=1, dt=0: lib.dsn_image_undistort(src, dst, K, D, nd, N, H, W, ch, dt, None)
    refused(b"dsn_image_undistort", b"null", und(src=None))
    refused(b"dsn_image_undistort", b"null", und(K=None))
    refused(b"dsn_image_undistort", b"null", und(D=None))
    refused(b"dsn_image_undistort", b"must differ", und(dst=one))
    for nd in (0, 3, 6, 7, 9):
        refused(b"dsn_image_undistort", b"nd", und(nd=nd))
    refused(b"dsn_image_undistort", b"N must", und(N=-1))
    refused(b"dsn_image_undistort", b"H and W", und(H=0))
    refused(b"dsn_image_undistort", b"H and W", und(W=-3))
    refused(b"dsn_image_undistort", b"H and W", und(W=32769))
    refused(b"dsn_image_undistort", b"channels", und(ch=2))
    refused(b"dsn_image_undistort", b"dtype", und(dt=2))
    assert und(N=0, src=None, dst=None, K=None, D=None) == 0

    mor = lambda src=one, dst=two, N=1, H=8, W=8, k=5, op=0: lib.dsn_image_morph(src, dst, N, H, W, k, op, None)
    refused(b"dsn_image_morph", b"null", mor(dst=None))
    for k in (0, -1, 16):
        refused(b"dsn_image_morph", b"k must", mor(k=k))
    refused(b"dsn_image_morph", b"op must", mor(op=2))
    refused(b"dsn_image_morph", b"N must", mor(N=-2))
    refused(b"dsn_image_morph", b"H and W", mor(H=0))
    assert mor(N=0, src=None, dst=None) == 0

    res = lambda src=one, dst=two, N=1, H=8, W=8, ch=3, dt=0, c=2, mode=1: lib.dsn_image_resize(src, dst, N, H, W, ch, dt, c, mode, None)
    refused(b"dsn_image_resize", b"null", res(src=None))
    for c in (0, 3, 8, -2):
        refused(b"dsn_image_resize", b"c must", res(c=c))
    refused(b"dsn_image_resize", b"multiples", res(H=7))
    refused(b"dsn_image_resize", b"multiples", res(W=10, c=4))
    refused(b"dsn_image_resize", b"mode", res(mode=2))
    refused(b"dsn_image_resize", b"channels", res(ch=4))
    refused(b"dsn_image_resize", b"dtype", res(dt=7))
    refused(b"dsn_image_resize", b"4-byte", res(dt=1, src=C.c_void_p(66)))
    assert res(N=0, src=None, dst=None) == 0

    def prep(img=one, msk=two, K=one, D=one, nd=5, N=1, H=8, W=8, c=2, border=5, dt=2, out=two, u8=None, fg=None, ci=None):
        return lib.dsn_image_prep(img, msk, K, D, nd, N, H, W, c, border, dt, out, u8, fg, ci, None)
    for kw in ({"img": None}, {"msk": None}, {"K": None}, {"D": None}, {"out": None}):
        refused(b"dsn_image_prep", b"null", prep(**kw))
    refused(b"dsn_image_prep", b"nd", prep(nd=6))
    refused(b"dsn_image_prep", b"c must", prep(c=3))
    refused(b"dsn_image_prep", b"multiples", prep(H=6, c=4))
    for border in (0, 16):
        refused(b"dsn_image_prep", b"border", prep(border=border))
    refused(b"dsn_image_prep", b"out_dtype", prep(dt=0))
    refused(b"dsn_image_prep", b"aligned", prep(out=C.c_void_p(4100)))
    refused(b"dsn_image_prep", b"N must", prep(N=-1))
    refused(b"dsn_image_prep", b"N must", prep(N=65536))
    assert prep(N=0, img=None, msk=None, K=None, D=None, out=None) == 0


def test_wrapper_argument_checks(L):
    """dtype, shape, skew, coefficient count, box and factor are refused with ValueError before the device is asked for"""
    import dsnerf_amd.imageprep as P
    u8 = torch.zeros(1, 8, 8, dtype=torch.uint8)
    rgb = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    K, D = K0, np.zeros(5)
    skew = K0.copy()
    skew[0, 1] = 1e-9
    for call in (lambda: L.image_undistort(u8.to(torch.int32), K, D),          # dtype
                 lambda: L.image_undistort(torch.zeros(8, 8, dtype=torch.uint8), K, D),          # no leading N
                 lambda: L.image_undistort(torch.zeros(1, 8, 8, 2, dtype=torch.uint8), K, D),          # two channels
                 lambda: L.image_undistort(rgb.transpose(1, 2), K, D),          # not contiguous
                 lambda: L.image_undistort(np.zeros((1, 8, 8), np.uint8), K, D),          # not a tensor
                 lambda: L.image_undistort(u8, skew, D),
                 lambda: L.image_undistort(u8, K, np.zeros(6)),
                 lambda: L.image_undistort(u8, K[:2], D),
                 lambda: L.image_undistort(u8, np.stack([K, K]), D),          # two cameras, one image
                 lambda: L.image_morph(u8, 0, L.PREP_DILATE),
                 lambda: L.image_morph(u8, 16, L.PREP_ERODE),
                 lambda: L.image_morph(u8, 2.5, L.PREP_ERODE),
                 lambda: L.image_morph(u8, 5, 7),
                 lambda: L.image_morph(rgb, 5, L.PREP_DILATE),
                 lambda: L.image_morph(u8.float(), 5, L.PREP_DILATE),
                 lambda: L.image_resize(u8, 3, L.PREP_AREA),
                 lambda: L.image_resize(torch.zeros(1, 6, 8, dtype=torch.uint8), 4, L.PREP_AREA),
                 lambda: L.image_resize(u8, 2, 5),
                 lambda: L.image_resize(u8.double(), 2, L.PREP_AREA),
                 lambda: L.image_prep(rgb, u8, skew, D),
                 lambda: L.image_prep(rgb, u8, K, np.zeros(7)),
                 lambda: L.image_prep(rgb, torch.zeros(1, 8, 4, dtype=torch.uint8), K, D),
                 lambda: L.image_prep(u8, u8, K, D),
                 lambda: L.image_prep(rgb, u8, K, D, c=3),
                 lambda: L.image_prep(rgb, u8, K, D, border=0),
                 lambda: L.image_prep(rgb, u8, K, D, border=16),
                 lambda: L.image_prep(rgb, u8, K, D, dtype=torch.float16),
                 lambda: P.prepare_zju(rgb[0].numpy(), u8[0].numpy(), K, D, ratio=0.3),
                 lambda: P.resize_area(np.zeros((2, 2, 2, 2, 2), np.uint8), 2)):
        with pytest.raises(ValueError):
            call()
    Kt, Dt = L.prep_camera("test", K, D, 3)
    assert Kt.shape == (3, 3, 3) and Dt.shape == (3, 5) and Kt.dtype == torch.float64 and Kt.is_contiguous() and Dt.is_contiguous()
    assert np.array_equal(P.scaled_K(K, 2)[:2], K[:2] * 0.5) and np.array_equal(P.scaled_K(K, 2)[2], K[2])
    if not torch.cuda.is_available():          # no quiet host path: well-formed host tensors are refused, the missing device is an error
        with pytest.raises((ValueError, RuntimeError)):
            L.image_morph(u8, 5, L.PREP_DILATE)
        with pytest.raises(RuntimeError):
            P.dilate(u8[0].numpy(), 5)


# ---- 6. for users who have OpenCV ----------------------------------------------------------------------------------------------------------
def test_against_cv2_where_installed(capsys):
    """Compares the restatement with cv2 on the GPU tests' inputs and prints the count of differing pixels.  Asserted: the integer steps
    (morphology, nearest, area on uint8).  cv2.undistort's bits are NOT claimed - its map differs between versions and SIMD paths - so its
    count is recorded only."""
    cv2 = pytest.importorskip("cv2")
    img, cihp, K, D = zju_case()
    fg = (cihp != 0).astype(np.uint8)
    for k in (1, 2, 5, 10, 15):
        box = np.ones((k, k), np.uint8)
        assert np.array_equal(IP.dilate(fg, k), cv2.dilate(fg, box)), k
        assert np.array_equal(IP.erode(cihp, k), cv2.erode(cihp, box)), k
    for c in (2, 4):
        r = 1.0 / c
        assert np.array_equal(IP.resize_nearest(cihp, c), cv2.resize(cihp, (0, 0), fx=r, fy=r, interpolation=cv2.INTER_NEAREST))
        assert np.array_equal(IP.resize_area(img, c), cv2.resize(img, (0, 0), fx=r, fy=r, interpolation=cv2.INTER_AREA))
    with capsys.disabled():
        for name, src in (("uint8 image", img), ("mask", fg), ("float32 image", img.astype(np.float32) / np.float32(255))):
            diff = IP.undistort(src, K, D) != cv2.undistort(src, K, D)
            print(f"\nimage_prep vs cv2 {cv2.__version__} undistort, {name}: {int(diff.sum())} of {diff.size} values differ")
