"""Golden record of the ZJU pipeline's ORDER (tests/golden/image_prep.npz), from the reference's own dataloader/zju_mocap_dataset.py:
Mocap_Base.get_mask and the image lines of Mocap_Base.__getitem__ are run as they are, with the modules cv2 and glob2 replaced by shims
whose imread hands out this script's arrays and whose undistort / dilate / resize are the numpy restatement
(tests/image_prep_restate.py).  What the record pins is therefore which array the reference undistorts, dilates, multiplies, resizes
and divides, in which order, and which mask it hands on raw - not cv2's arithmetic.  prepare_input and the ray sampler, which follow
the image lines, are replaced by recorders; nothing of the reference is copied into the repository.
Run where the reference is checked out:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_prep.py <reference dir>"""
import os, sys, types
import numpy as np
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import image_prep_restate as IP  # noqa: E402

REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DSN_REFERENCE", "")
if not os.path.isdir(os.path.join(REFERENCE, "dataloader")):
    sys.exit("usage: make_golden_image_prep.py <reference dir>")

FILES = {}          # path -> array, what imread hands out


def _resize(src, dsize, fx=None, fy=None, interpolation=None):
    assert dsize == (0, 0) and fx == fy and interpolation in (cv2.INTER_AREA, cv2.INTER_NEAREST)
    c = {1.0: 1, 0.5: 2, 0.25: 4}[fx]
    if src.ndim == 3 and src.shape[2] == 1:
        src = src[..., 0]          # cv2.resize drops a single channel's axis
    return IP.resize_area(src, c) if interpolation == cv2.INTER_AREA else IP.resize_nearest(src, c)


def _dilate(src, kernel):
    assert kernel.shape[0] == kernel.shape[1] and kernel.all()
    return IP.dilate(src, kernel.shape[0])


cv2 = types.ModuleType("cv2")
cv2.INTER_AREA, cv2.INTER_NEAREST = "area", "nearest"
cv2.imread = lambda path: FILES[path].copy()
cv2.undistort = lambda src, K, D: IP.undistort(src, np.asarray(K), np.asarray(D))
cv2.dilate = _dilate
cv2.resize = _resize
sys.modules["cv2"] = cv2
sys.modules["glob2"] = types.ModuleType("glob2")
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.join(REFERENCE, "dataloader"))
import zju_mocap_dataset as ZJU  # noqa: E402  (the module file itself: the package's __init__ pulls in the other data sets' imports)
from utils import rays_utils  # noqa: E402


def run_item(img, msk_cihp, K, D, ratio):
    """one __getitem__ of Mocap_Base on the arrays: (img, msk_fg, msk_cihp, K) as the reference hands them to its ray sampler"""
    H, W = img.shape[:2]
    FILES.clear()
    FILES["root/Camera_B1/000007.jpg"] = img
    FILES["root/mask_cihp/Camera_B1/000007.png"] = np.repeat(msk_cihp[..., None], 3, axis=2)          # a three-channel png, as on disk
    ds = ZJU.Mocap_Base.__new__(ZJU.Mocap_Base)
    ds.human, ds.ratio, ds.nrays, ds.mode = "CoreView_377", ratio, 16, "train"
    ds.all_img_path = ["root/Camera_B1/000007.jpg"]
    ds.cams = {"Camera_B1": {"K": K.tolist(), "dist": D.tolist(), "R": np.eye(3).tolist(), "T": [[0.0], [0.0], [3.0]]}}
    ds.prepare_input = lambda i: (np.zeros((24, 3)), np.zeros((4, 3), np.float32), np.zeros((2, 3), np.float32), -1, np.eye(3), np.zeros(3))
    seen = {}

    def recorder(img, K, R, T, bounds, msk, nrays):
        seen.update(img=img.copy(), K=np.array(K), msk_cihp=np.array(msk))
        h, w = img.shape[:2]
        coord = np.stack(np.mgrid[:h, :w], axis=-1).reshape(-1, 2)          # every pixel: `occupancy` then is msk_fg, row by row
        z = np.zeros((len(coord), 3))
        return z, z, z, z[:, 0], z[:, 0], coord, np.ones(len(coord), bool), np.ones((h, w), np.uint8)

    keep = rays_utils.my_sample_ray
    rays_utils.my_sample_ray = recorder
    try:
        ret = ds[0]
    finally:
        rays_utils.my_sample_ray = keep
    h, w = seen["img"].shape[:2]
    assert np.array_equal(ret["img"], seen["img"])
    return seen["img"], np.asarray(ret["occupancy"]).reshape(h, w), seen["msk_cihp"].reshape(h, w), seen["K"]


def main():
    rng = np.random.RandomState(20261020)
    H, W = 40, 48
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[:H, :W]
    msk = np.zeros((H, W), np.uint8)
    msk[((y - 19) / 13.0) ** 2 + ((x - 25) / 9.0) ** 2 <= 1.0] = 5
    msk[(msk != 0) & (y > 22)] = 1
    msk[3, 40] = 9          # a lone label near the border
    K = np.array([[0.9 * W, 0.0, W / 2 - 0.3], [0.0, 0.92 * W, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    D = np.array([-0.3, 0.12, 1.5e-3, -2e-3, 0.03])
    rec = {"img": img, "msk_cihp": msk, "K": K, "D": D}
    for tag, ratio in (("half", 0.5), ("full", 1)):
        out_img, msk_fg, msk_cihp, Ks = run_item(img, msk, K, D, ratio)
        rec.update({f"{tag}_c": np.int32(round(1 / ratio)), f"{tag}_img": out_img, f"{tag}_msk_fg": msk_fg.astype(np.uint8),
                    f"{tag}_msk_cihp": msk_cihp.astype(np.uint8), f"{tag}_K": Ks})
        print(tag, out_img.shape, out_img.dtype, int(msk_fg.sum()), int((msk_cihp != 0).sum()))
    np.savez_compressed(os.path.join(HERE, "image_prep.npz"), **rec)


if __name__ == "__main__":
    main()
