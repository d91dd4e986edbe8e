"""The datasets' image preparation on the device: what the reference does with OpenCV between cv2.imread and the ray sampler
(dataloader/zju_mocap_dataset.py:84-123, :192-213; dataloader/h36m_dataset.py:88-93, :128-158, :182-184).

    undistort(x, K, D)   dilate(m, k)   erode(m, k)   resize_area(x, c)   resize_nearest(x, c)
    prepare_zju(img_u8, msk_cihp, K, D, ratio=0.5, border=5, dtype=torch.float64, want_u8=False)      one launch (dsn_image_prep)
    prepare_h36m(img_u8, msk, K, D, ratio=1.0, is_eval=False)                                           a composition of the calls above

The arithmetic is the rule written out in include/dsnerf.h (the shape of OpenCV's fixed-point path; cv2's own bits are not claimed)
and restated in tests/image_prep_restate.py.  Host arrays (numpy, CPU tensors) are uploaded once; device tensors are used as they
are; results stay on the device.  Every function takes one image or a batch with a leading N:

    [H, W]           one single-channel image          [N, H, W, 3]     a batch of three-channel images
    [H, W, 3]        one three-channel image           [N, H, W]        a batch of single-channel images (N x H x 3 masks: batch=True)

K: [3, 3] or [N, 3, 3]; D: [nd] or [N, nd] with nd = 4, 5 or 8 - host arrays preferably (they are checked on the host).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

TILE_W, TILE_H = _lib.PREP_TILE_W, _lib.PREP_TILE_H          # the full-resolution tile one workgroup owns (tests aim at its seams)


def _device(device=None):
    _lib.require_gpu()
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _batched(what, x, channels_ok, batch, device):
    """x as a contiguous device tensor with a leading N, and whether the caller gave a single image"""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dim() == 2:
        single = True
    elif x.dim() == 3:
        single = (3 in channels_ok and x.shape[2] == 3) if batch is None else not batch
    elif x.dim() == 4:
        single = False
    else:
        raise ValueError(f"{what}: an image is [H, W] or [H, W, 3], a batch [N, H, W] or [N, H, W, 3]; got {tuple(x.shape)}")
    if single:
        x = x.unsqueeze(0)
    if x.dim() == 4 and (3 not in channels_ok or x.shape[3] != 3):
        raise ValueError(f"{what}: got {tuple(x.shape)}; channels must be {' or '.join(str(c) for c in channels_ok)}")
    if not x.is_cuda:
        x = x.to(_device(device))
    return x.contiguous(), single


def _factor(what, ratio):
    c = {1.0: 1, 0.5: 2, 0.25: 4}.get(float(ratio))
    if c is None:
        raise ValueError(f"{what}: ratio must be 1, 0.5 or 0.25, got {ratio!r}")
    return c


def undistort(x, K, D, batch=None, device=None):
    """cv2.undistort(x, K, D)'s place: uint8 or float32, one or three channels."""
    x, single = _batched("undistort", x, (1, 3), batch, device)
    out = _lib.image_undistort(x, K, D)
    return out[0] if single else out


def _morph(what, m, k, op, device):
    m, single = _batched(what, m, (1,), None, device)
    out = _lib.image_morph(m, k, op)
    return out[0] if single else out


def dilate(m, k, device=None):
    """cv2.dilate(m, np.ones((k, k), np.uint8))'s place: uint8 [H, W] or [N, H, W], k = 1 ... 15."""
    return _morph("dilate", m, k, _lib.PREP_DILATE, device)


def erode(m, k, device=None):
    """cv2.erode(m, np.ones((k, k), np.uint8))'s place."""
    return _morph("erode", m, k, _lib.PREP_ERODE, device)


def resize_area(x, c, batch=None, device=None):
    """cv2.resize(x, (0, 0), fx=1/c, fy=1/c, interpolation=cv2.INTER_AREA)'s place for c = 1, 2, 4 dividing H and W."""
    x, single = _batched("resize_area", x, (1, 3), batch, device)
    out = _lib.image_resize(x, c, _lib.PREP_AREA)
    return out[0] if single else out


def resize_nearest(x, c, batch=None, device=None):
    """cv2.resize(..., interpolation=cv2.INTER_NEAREST)'s place for c = 1, 2, 4 dividing H and W."""
    x, single = _batched("resize_nearest", x, (1, 3), batch, device)
    out = _lib.image_resize(x, c, _lib.PREP_NEAREST)
    return out[0] if single else out


def scaled_K(K, c):
    """the reference's `K[:2] = K[:2] * ratio` on the host: float64 [.., 3, 3]"""
    K = np.array(torch.as_tensor(K).detach().cpu().numpy(), dtype=np.float64)
    K[..., :2, :] = K[..., :2, :] * (1.0 / c)
    return K


def prepare_zju(img_u8, msk_cihp, K, D, ratio=0.5, border=5, dtype=torch.float64, want_u8=False, device=None):
    """The ZJU data set's image work of one item or a batch (zju_mocap_dataset.py:94-123 with get_mask, :192-213) in one launch:
    img_u8 [H0, W0, 3] or [N, H0, W0, 3] and msk_cihp [H0, W0] or [N, H0, W0] uint8 as cv2.imread gives them ->
    {"img": [.., H, W, 3] in [0, 1] of `dtype`, "msk_fg", "msk_cihp": [.., H, W] uint8, "K": the scaled cameras (host, float64),
    "img_u8" with want_u8}: on the device, what Renderer.sample_batch(img, K, R, T, bounds, mask=msk_cihp, occupancy_from=msk_fg)
    takes.  msk_cihp is the RAW mask at the small size, as in the reference."""
    c = _factor("prepare_zju", ratio)
    img_u8, single = _batched("prepare_zju", img_u8, (3,), None, device)
    msk_cihp, msingle = _batched("prepare_zju", msk_cihp, (1,), None if single else True, img_u8.device)
    if single != msingle:
        raise ValueError("prepare_zju: img_u8 and msk_cihp must both be single items or both batches")
    img, u8, fg, ci = _lib.image_prep(img_u8, msk_cihp, K, D, c=c, border=border, dtype=dtype, want_u8=want_u8)
    Ks = scaled_K(K, c)
    out = {"img": img, "msk_fg": fg, "msk_cihp": ci, "K": Ks}
    if want_u8:
        out["img_u8"] = u8
    if single:
        out = {k: (v[0] if (torch.is_tensor(v) or v.ndim == 3) else v) for k, v in out.items()}
    return out


def prepare_h36m(img_u8, msk, K, D, ratio=1.0, is_eval=False, device=None):
    """The Human3.6M data set's image work of ONE item (h36m_dataset.py:128-158 with get_mask, :75-96, and :182-184) as a composition
    of the stand-alone calls, in the reference's order: img_u8 [H, W, 3] uint8 (cv2.imread), msk [H, W] uint8 (the label map of
    imageio.imread, at the image's size) ->
        get_mask      fg = (msk != 0); training: the 5 x 5 erode / dilate band of fg marked 100 in `msk`
        :128          img = float32(img_u8) / 255
        :139-142      undistort of img (float32), msk, orig_msk and the label map
        :148-152      area resize of img, nearest resize of msk and orig_msk by `ratio`
        :154          img[orig_msk == 0] = 0
        :182-184      the undistorted label map (full size, as the reference leaves it) eroded with a 10 x 10 box
    {"img" [h, w, 3] float32, "msk", "orig_msk" [h, w] uint8, "msk_cihp", "msk_cihp_eroded" [H, W] uint8, "K" (host, scaled)}."""
    c = _factor("prepare_h36m", ratio)
    img_u8, _ = _batched("prepare_h36m", img_u8, (3,), None, device)
    dev = img_u8.device
    raw, _ = _batched("prepare_h36m", msk, (1,), None, dev)
    if img_u8.dtype != torch.uint8 or raw.dtype != torch.uint8 or img_u8.shape[0] != 1 or tuple(raw.shape) != tuple(img_u8.shape[:3]):
        raise ValueError(f"prepare_h36m: one uint8 image [H, W, 3] and its uint8 label map [H, W]; got {tuple(img_u8.shape)}, {tuple(raw.shape)}")
    levels = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(dev)          # float32(v) / 255, from the host
    img = levels[img_u8.long()]
    fg = (raw != 0).to(torch.uint8)
    m = fg.clone()
    if not is_eval:
        band = (_lib.image_morph(fg, 5, _lib.PREP_DILATE) - _lib.image_morph(fg, 5, _lib.PREP_ERODE)) == 1
        m[band] = 100
    img = _lib.image_undistort(img, K, D)
    m = _lib.image_undistort(m, K, D)
    orig = _lib.image_undistort(fg, K, D)
    cihp = _lib.image_undistort(raw, K, D)
    img = _lib.image_resize(img, c, _lib.PREP_AREA)
    m = _lib.image_resize(m, c, _lib.PREP_NEAREST)
    orig = _lib.image_resize(orig, c, _lib.PREP_NEAREST)
    img = torch.where((orig == 0).unsqueeze(-1), torch.zeros((), dtype=torch.float32, device=dev), img)
    eroded = _lib.image_morph(cihp, 10, _lib.PREP_ERODE)
    return {"img": img[0], "msk": m[0], "orig_msk": orig[0], "msk_cihp": cihp[0], "msk_cihp_eroded": eroded[0], "K": scaled_K(K, c)}
