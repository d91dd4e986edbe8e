"""The SSIM oracle (test infrastructure only): a float64 numpy / scipy restatement of the reference's metrics.py:23-38
ssim_metric, i.e. scikit-image 0.15 compare_ssim(img_pred, img_gt, multichannel=True) on the images that are zero outside
mask_at_box, cropped to cv2.boundingRect(mask_at_box).  scipy.ndimage.uniform_filter is the filter skimage calls."""
import numpy as np
from scipy.ndimage import uniform_filter

WIN = 7
DATA_RANGE = 2.0                 # skimage's dtype_range[np.float64] = (-1, 1)
C1 = (0.01 * DATA_RANGE) ** 2
C2 = (0.03 * DATA_RANGE) ** 2
COV_NORM = WIN * WIN / (WIN * WIN - 1.0)      # use_sample_covariance=True


def bounding_rect(mask):
    """cv2.boundingRect of a binary [H,W] image: (x, y, w, h) of the smallest rectangle holding every set pixel; (0, 0, 0, 0)
    for an empty mask"""
    ys, xs = np.nonzero(np.asarray(mask))
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def ssim_channel(X, Y):
    """compare_ssim of two 2-D float64 images (win_size 7, data range 2, sample covariance, no Gaussian weights)"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if np.any(np.asarray(X.shape) - WIN < 0):
        raise ValueError("win_size exceeds image extent.  If the input is a multichannel (color) image, set multichannel=True.")
    ux, uy = uniform_filter(X, size=WIN), uniform_filter(Y, size=WIN)
    uxx, uyy, uxy = uniform_filter(X * X, size=WIN), uniform_filter(Y * Y, size=WIN), uniform_filter(X * Y, size=WIN)
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (WIN - 1) // 2
    return S[pad:-pad, pad:-pad].mean()


def ssim_metric(pred, gt, mask_at_box):
    """metrics.py:23-38: pred, gt [H,W,3] (pred already clamped where the caller clamps), mask_at_box [H,W] or [H*W]"""
    gt = np.asarray(gt)
    H, W = gt.shape[:2]
    mask = np.asarray(mask_at_box).reshape(H, W) != 0
    img_pred = np.zeros((H, W, 3))
    img_pred[mask] = np.asarray(pred)[mask]
    img_gt = np.zeros((H, W, 3))
    img_gt[mask] = gt[mask]
    x, y, w, h = bounding_rect(mask)
    img_pred, img_gt = img_pred[y:y + h, x:x + w], img_gt[y:y + h, x:x + w]
    return float(np.mean([ssim_channel(img_pred[..., c], img_gt[..., c]) for c in range(3)]))
