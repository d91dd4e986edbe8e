"""Golden vectors for the training-batch sampler (dsn_train_rays), from the reference's own utils/rays_utils.my_sample_ray and
utils/h36m_utils.sample_ray_h36m.  cv2 is stubbed: its fillPoly applies the union rule of include/dsnerf.h
(tests/train_rays_restate.fill_poly); np.random.randint is replaced for the duration of the call by the header's counter-hash draws,
keyed by call order (body, face unless the class is empty, random; round by round).  Everything else is the reference's code.
Run in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_rays.py"""
import os, sys, types
import numpy as np
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import train_rays_restate as TR  # noqa: E402

cv2 = types.ModuleType("cv2")
_last_mask = {}


def _fill_poly(mask, pts, color):
    TR.fill_poly(mask, pts, color)
    _last_mask["mask"] = mask.copy()          # after the sixth call: the box mask, before sample_ray_h36m takes msk == 100 out of it


cv2.fillPoly = _fill_poly
sys.modules["cv2"] = cv2
sys.path.insert(0, "/root/reference")
from utils import rays_utils, h36m_utils  # noqa: E402


class Draws:
    """np.random.randint(0, count, n) -> the header's draws of the class and round this call belongs to"""

    def __init__(self, seed, face_empty):
        self.seed, self.order, self.calls = seed, ((0, 2) if face_empty else (0, 1, 2)), 0

    def __call__(self, low, high, size):
        assert low == 0
        r, j = divmod(self.calls, len(self.order))
        self.calls += 1
        return TR.draw_indices(self.seed, r, self.order[j], size, high)


def camera(H, W, z, ang=0.4):
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0.05, 1, 0.02], [-np.sin(ang), 0, np.cos(ang)]])
    R, _ = np.linalg.qr(R)
    f = 0.35 * W          # a close, wide camera: near and far stay below 2, where the float32 comparisons of the tests are tightest
    K = np.array([[f, 0.3, W / 2 - 0.5], [0.0, f * 1.03, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    T = np.array([[0.1], [0.07], [z]])
    return K, R, T


def body_mask(H, W, cy, cx, ry, rx, face=True):
    y, x = np.mgrid[:H, :W]
    m = np.zeros((H, W), np.uint8)
    m[((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = 5           # some body-part label
    m[(m != 0) & (y > cy)] = 1
    if face:
        m[(m != 0) & (y < cy - 0.55 * ry)] = 2
    return m


rng = np.random.RandomState(7)
out = {}
ZJU_BOUNDS = np.array([[-0.55, -0.6, -0.3], [0.5, 0.55, 0.28]])
cases = [  # name, H, W, z, mask centre / radii, face, nrays, seed, image dtype
    ("zju", 40, 48, 1.0, (20, 24, 12, 9), True, 64, 11, np.float64),
    ("zju_half", 37, 53, 1.0, (18, 44, 12, 8), True, 200, 5, np.float32),          # half of the body lies beside the box: several rounds
    ("zju_noface", 40, 48, 1.0, (22, 22, 10, 8), False, 37, 3, np.float64),
]
for name, H, W, z, (cy, cx, ry, rx), face, nrays, seed, dt in cases:
    K, R, T = camera(H, W, z)
    assert TR.half_integer_distance(K, R, T, ZJU_BOUNDS) > 1e-6
    img = rng.rand(H, W, 3).astype(dt)
    msk = body_mask(H, W, cy, cx, ry, rx, face)
    draws, keep = Draws(seed, not (msk == 2).any()), np.random.randint
    np.random.randint = draws
    try:
        rgb, ray_o, ray_d, near, far, coord, mask_at_box, bound = rays_utils.my_sample_ray(img, K, R, T, ZJU_BOUNDS, msk, nrays)
    finally:
        np.random.randint = keep
    rounds = draws.calls // len(draws.order)
    e = TR.sample(img, K, R, T, ZJU_BOUNDS, msk, nrays, seed)
    assert e["status"] == TR.OK and e["rounds"] == rounds, (name, e["status"], e["rounds"], rounds)
    assert np.array_equal(e["coord"], coord) and np.array_equal(e["bound_mask"], bound) and np.array_equal(e["rgb"], rgb), name
    print(name, "rounds", rounds, "| near", float(np.abs(e["near"] - near).max()), "far", float(np.abs(e["far"] - far).max()),
          "| ray_d", float(np.abs(e["ray_d"] - ray_d).max()), "| body pixels whose ray meets the box",
          float(TR.whole_image_rays(K, R, T, ZJU_BOUNDS, H, W, TR.ZJU)[4].reshape(H, W)[msk != 0].mean()), "| box pixels", int(bound.sum()),
          "| near", float(near.min()), "far", float(far.max()))
    out.update({f"{name}:{k}": v for k, v in dict(
        K=K, R=R, T=T, bounds=ZJU_BOUNDS, img=img, mask=msk, nrays=np.int64(nrays), seed=np.int64(seed), rounds=np.int64(rounds),
        corners=TR.rounded_corners(K, R, T, ZJU_BOUNDS), coord=coord, rgb=rgb, ray_o=ray_o, ray_d=ray_d, near=near, far=far,
        mask_at_box=mask_at_box, bound_mask=bound).items()})

# ---- Human3.6M: msk with 100s (the border label the datasets give the mask's edge), msk_cihp with a face that leaves the box
H, W, nrays, seed = 37, 53, 100, 9
K, R, T = camera(H, W, 1.1, ang=-0.3)
bounds32 = h36m_utils.get_bounds(np.array([[-0.5, -0.55, -0.25], [0.45, 0.5, 0.23]]))
assert TR.half_integer_distance(K, R, T, bounds32) > 1e-6
img = rng.rand(H, W, 3).astype(np.float32)
cihp = body_mask(H, W, 16, 27, 14, 9, True)
msk = (cihp != 0).astype(np.uint8)
edge = msk.copy()
edge[1:-1, 1:-1] = msk[1:-1, 1:-1] & msk[:-2, 1:-1] & msk[2:, 1:-1] & msk[1:-1, :-2] & msk[1:-1, 2:]
msk[(msk == 1) & (edge == 0)] = 100
assert (msk == 100).any() and (msk == 1).any()
draws, keep = Draws(seed, not (cihp == 2).any()), np.random.randint
np.random.randint = draws
try:
    rgb, ray_o, ray_d, near, far, coord, mask_at_box = h36m_utils.sample_ray_h36m(img.copy(), msk.copy(), cihp.copy(), K, R, T, bounds32,
                                                                                   nrays, "train")
finally:
    np.random.randint = keep
bound = _last_mask["mask"]
rounds = draws.calls // len(draws.order)
e = TR.sample(img, K, R, T, bounds32, msk, nrays, seed, convention=TR.H36M, mask_b=cihp)
assert e["status"] == TR.OK and e["rounds"] == rounds, (e["status"], e["rounds"], rounds)
assert np.array_equal(e["coord"], coord) and np.array_equal(e["bound_mask"], bound) and np.array_equal(e["rgb"], rgb)
print("h36m rounds", rounds, "| near", float(np.abs(e["near"] - near).max()), "far", float(np.abs(e["far"] - far).max()),
      "| ray_d", float(np.abs(e["ray_d"] - ray_d).max()), "| msk==100 in box", int(((msk == 100) & (bound == 1)).sum()),
      "| face outside box", int(((cihp == 2) & (bound != 1)).sum()))
out.update({f"h36m:{k}": v for k, v in dict(
    K=K, R=R, T=T, bounds=bounds32, img=img, mask=msk, mask_b=cihp, nrays=np.int64(nrays), seed=np.int64(seed), rounds=np.int64(rounds),
    corners=TR.rounded_corners(K, R, T, bounds32), coord=coord, rgb=rgb, ray_o=ray_o, ray_d=ray_d, near=near, far=far,
    mask_at_box=mask_at_box, bound_mask=bound).items()})
np.savez_compressed(os.path.join(HERE, "train_rays.npz"), **out)
print("wrote train_rays.npz", os.path.getsize(os.path.join(HERE, "train_rays.npz")), "bytes")
