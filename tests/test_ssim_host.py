"""The SSIM oracle (tests/ssim_oracle.py, the restatement of metrics.py:ssim_metric the device path is checked against) pinned
by closed forms that do not depend on it, and the host side of dsn_image_ssim's C ABI.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from ssim_oracle import C1, C2, bounding_rect, ssim_channel, ssim_metric


def _direct(X, Y):
    """SSIM of one channel by brute force: the mean over every whole 7 x 7 window of S from np.mean / np.var(ddof=1)"""
    H, W = X.shape
    out = []
    for i in range(H - 6):
        for j in range(W - 6):
            x, y = X[i:i + 7, j:j + 7].ravel(), Y[i:i + 7, j:j + 7].ravel()
            ux, uy = x.mean(), y.mean()
            vx, vy = x.var(ddof=1), y.var(ddof=1)
            vxy = ((x - ux) * (y - uy)).sum() / 48.0
            out.append((2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2)))
    return float(np.mean(out))


def test_constants_pin_the_dtype_range_quirk():
    # float64 input: skimage takes the data range from dtype_range[float64] = (-1, 1), so R = 2 (not 1)
    assert C1 == (0.01 * 2) ** 2 and C2 == (0.03 * 2) ** 2


def test_identical_images_give_exactly_one():
    rng = np.random.default_rng(1)
    img = rng.random((40, 33, 3))
    mask = np.zeros((40, 33), bool)
    mask[5:30, 4:25] = rng.random((25, 21)) < 0.8
    assert ssim_metric(img, img, mask) == 1.0


def test_constant_images():
    a, b = 0.3, 0.8
    H, W = 30, 40
    mask = np.zeros((H, W), bool)
    mask[4:20, 7:35] = True                        # the crop is exactly the set rectangle: constant a / b over all of it
    pred, gt = np.full((H, W, 3), a), np.full((H, W, 3), b)
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    assert abs(ssim_metric(pred, gt, mask) - want) < 1e-12


def test_checkerboard_pins_sample_covariance_and_c2():
    """x = m + d s and y = k - x on a +-1 checkerboard s: every 7 x 7 window holds 25 of the centre's sign and 24 of the other,
    so mean(s) = +-1/49 and the sample variance of s is (49/48)(1 - 1/49^2) = 50/49; vx = vy = -vxy = 50/49 d^2"""
    m, d, k = 0.5, 0.2, 0.9
    H, W = 19, 26
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    s = np.where((ii + jj) % 2 == 0, 1.0, -1.0)
    X = m + d * s
    Y = k - X

    def closed_form(v, c2):
        vals = []
        for i in range(3, H - 3):
            for j in range(3, W - 3):
                ux = m + d * s[i, j] / 49.0
                uy = k - ux
                vals.append((2 * ux * uy + C1) * (-2 * v + c2) / ((ux * ux + uy * uy + C1) * (2 * v + c2)))
        return float(np.mean(vals))

    want = closed_form(50.0 / 49.0 * d * d, C2)
    assert abs(ssim_channel(X, Y) - want) < 1e-12
    mask = np.ones((H, W), bool)
    assert abs(ssim_metric(np.stack([X] * 3, -1), np.stack([Y] * 3, -1), mask) - want) < 1e-12
    # the population covariance (no 49/48) or C2 of a data range 1 would be far off
    assert abs(closed_form((1 - 1 / 49.0 ** 2) * d * d, C2) - want) > 1e-4
    assert abs(closed_form(50.0 / 49.0 * d * d, 0.03 ** 2) - want) > 1e-4


def test_oracle_matches_brute_force_windows():
    rng = np.random.default_rng(2)
    X, Y = rng.random((17, 23)), rng.random((17, 23))
    assert abs(ssim_channel(X, Y) - _direct(X, Y)) < 1e-12


def test_width_seven_uses_one_window_per_row():
    rng = np.random.default_rng(3)
    H, W = 24, 30
    pred, gt = rng.random((H, W, 3)), rng.random((H, W, 3))
    mask = np.zeros((H, W), bool)
    mask[2:21, 9:16] = True                        # 7 wide, 19 high: 13 windows, one per interior row
    assert bounding_rect(mask) == (9, 2, 7, 19)
    want = np.mean([_direct(pred[2:21, 9:16, c], gt[2:21, 9:16, c]) for c in range(3)])
    assert abs(ssim_metric(pred, gt, mask) - want) < 1e-12


@pytest.mark.parametrize("case", ["width6", "height6", "single_pixel", "empty"])
def test_too_small_crops_raise(case):
    H, W = 20, 20
    mask = np.zeros((H, W), bool)
    if case == "width6":
        mask[2:15, 3:9] = True
    elif case == "height6":
        mask[4:10, 1:19] = True
    elif case == "single_pixel":
        mask[7, 7] = True
    img = np.full((H, W, 3), 0.5)
    with pytest.raises(ValueError):
        ssim_metric(img, img, mask)


def test_masked_out_pixels_inside_the_crop_are_zero():
    rng = np.random.default_rng(4)
    H, W = 26, 31
    pred, gt = rng.random((H, W, 3)), rng.random((H, W, 3))
    mask = rng.random((H, W)) < 0.6
    mask[:2] = False
    x, y, w, h = bounding_rect(mask)
    P, G = np.where(mask[..., None], pred, 0.0), np.where(mask[..., None], gt, 0.0)
    want = np.mean([_direct(P[y:y + h, x:x + w, c], G[y:y + h, x:x + w, c]) for c in range(3)])
    assert abs(ssim_metric(pred, gt, mask) - want) < 1e-12


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


def test_ssim_workspace_bytes(lib):
    assert lib.dsn_image_ssim_workspace_bytes(0, 512, 512) == 0
    assert lib.dsn_image_ssim_workspace_bytes(1, 0, 512) == 0
    assert lib.dsn_image_ssim_workspace_bytes(1, 512, 0) == 0
    assert lib.dsn_image_ssim_workspace_bytes(-1, 512, 512) == 0
    one = lib.dsn_image_ssim_workspace_bytes(1, 512, 512)
    assert one >= 3 * 8 * (512 // 16) * (512 // 32)              # one fp64 partial per (tile, channel)
    assert lib.dsn_image_ssim_workspace_bytes(16, 1024, 1024) >= 16 * 3 * 8 * (1024 // 16) * (1024 // 32)


def test_ssim_rejects_bad_arguments_by_name(lib):
    z, one = None, C.c_void_p(64)
    assert lib.dsn_image_ssim(z, z, z, z, 1, 8, 8, 0, z, z, z, z, z) != 0
    assert b"dsn_image_ssim" in lib.dsn_last_error() and b"null" in lib.dsn_last_error()
    # every output and the workspace are required
    assert lib.dsn_image_ssim(one, one, z, one, 1, 8, 8, 0, one, one, z, one, z) != 0
    assert b"dsn_image_ssim: null argument" in lib.dsn_last_error()
    # exactly one ground truth
    assert lib.dsn_image_ssim(one, z, z, one, 1, 8, 8, 0, one, one, one, one, z) != 0
    assert b"dsn_image_ssim" in lib.dsn_last_error() and b"ground-truth" in lib.dsn_last_error()
    assert lib.dsn_image_ssim(one, one, one, one, 1, 8, 8, 0, one, one, one, one, z) != 0
    assert b"ground-truth" in lib.dsn_last_error()
    for F, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -3), (70000, 8, 8)):
        assert lib.dsn_image_ssim(one, one, z, one, F, H, W, 0, one, one, one, one, z) != 0
        assert b"dsn_image_ssim: bad sizes" in lib.dsn_last_error()


def test_ssim_status_error_is_a_value_error():
    from dsnerf_amd import _lib
    e = _lib.ssim_status_error(_lib.SSIM_CROP_TOO_SMALL, (3, 4, 6, 20))
    assert isinstance(e, ValueError) and "6 x 20" in str(e)
    assert "empty" in str(_lib.ssim_status_error(_lib.SSIM_EMPTY_MASK, (0, 0, 0, 0)))
