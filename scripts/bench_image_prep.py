#!/usr/bin/env python3
"""The ZJU item's image preparation on the device (imageprep.prepare_zju: dsn_image_prep, one launch) against a torch formulation of the
same steps on the same GPU in the same run, and against the call's byte floor.
    python scripts/bench_image_prep.py [--blocks 6] [--iters 30] [--out profiles/image_prep_bench.json]
1024 x 1024 uint8 frames with their label masks already on the device, ratio 0.5 (c = 2), border 5, float64 output, N = 1, 4 and 16
items per call; the cameras are host arrays, as a data set holds them (their upload is part of the call).
The torch formulation: the rule's map as float64 tensor ops, F.grid_sample (bilinear, zero padding) for the image and the foreground
mask, F.max_pool2d for the 5 x 5 dilation, the product, F.avg_pool2d, / 255 and strided slicing for the masks - float32 interpolation
instead of the rule's fixed-point taps: DIFFERENT BITS, a time reference only.  Its image is compared with the call's (mean absolute
difference in levels) before anything is timed.
HIP events around whole calls after a warm-up, the two variants in alternating blocks; medians with the quartiles.
Byte floor: the uint8 frame and mask read once, the float64 image and the two small masks written once, over the 8.0 TB/s of the HBM's
specification.  A host cv2 time is not taken: OpenCV is not a dependency of this repository."""
import argparse
import json
import os
import platform
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import dsnerf_amd  # noqa: E402,F401
from dsnerf_amd import imageprep  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def quartiles(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 5), "q25_ms": round(float(q[0]), 5), "q75_ms": round(float(q[2]), 5), "n": len(ms)}


def timed(fn, iters):
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(variants, blocks, iters, warmup=10):
    for fn in variants.values():
        timed(fn, warmup)
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            ms[k] += timed(fn, iters)
    return {k: quartiles(v) for k, v in ms.items()}


def torch_prepare(img_u8, msk, K, D, c, border):
    """the same steps as torch ops (grid_sample / max_pool2d / avg_pool2d / slicing): other bits, a time reference"""
    N, H, W = msk.shape
    dev = img_u8.device
    Kd = torch.as_tensor(K, dtype=torch.float64).to(dev).reshape(-1, 3, 3).expand(N, 3, 3)
    Dd = torch.as_tensor(D, dtype=torch.float64).to(dev).reshape(-1, 5).expand(N, 5)
    fx, fy, cx, cy = (Kd[:, 0, 0, None, None], Kd[:, 1, 1, None, None], Kd[:, 0, 2, None, None], Kd[:, 1, 2, None, None])
    k1, k2, p1, p2, k3 = (Dd[:, i, None, None] for i in range(5))
    j = torch.arange(W, dtype=torch.float64, device=dev)[None, None, :]
    i = torch.arange(H, dtype=torch.float64, device=dev)[None, :, None]
    x, y = (j - cx) / fx, (i - cy) / fy
    x2, y2 = x * x, y * y
    r2, t = x2 + y2, 2 * x * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    u = fx * (x * kr + p1 * t + p2 * (r2 + 2 * x2)) + cx
    v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * t) + cy
    grid = torch.stack([u * (2.0 / (W - 1)) - 1.0, v * (2.0 / (H - 1)) - 1.0], dim=-1).float()
    fg = (msk != 0).float()[:, None]
    fg_u = (F.grid_sample(fg, grid, mode="bilinear", padding_mode="zeros", align_corners=True) >= 0.5).float()
    a = border // 2
    msk_fg = F.max_pool2d(F.pad(fg_u, (a, border - 1 - a, a, border - 1 - a)), border, stride=1)
    im = F.grid_sample(img_u8.permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    im = torch.floor(im + 0.5) * msk_fg
    small = torch.floor(F.avg_pool2d(im, c) + 0.5) if c > 1 else im
    return {"img": small.permute(0, 2, 3, 1).double() / 255.0, "msk_fg": msk_fg[:, 0, ::c, ::c].to(torch.uint8).contiguous(),
            "msk_cihp": msk[:, ::c, ::c].contiguous()}


def byte_floor(N, H0, W0, c):
    H, W = H0 // c, W0 // c
    return N * (H0 * W0 * 3 + H0 * W0 + H * W * 3 * 8 + 2 * H * W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--counts", type=int, nargs="*", default=[1, 4, 16])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_prep_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    S, c, border = args.size, 2, 5
    K = np.array([[1.1 * S, 0.0, S / 2 - 3.3], [0.0, 1.1 * S, S / 2 + 4.1], [0.0, 0.0, 1.0]])
    D = np.array([-0.3, 0.12, 1.5e-3, -2e-3, 0.03])
    res = {"metric": "image_prep_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "size": S, "c": c, "border": border, "blocks": args.blocks, "iters_per_block": args.iters,
           "timing": "HIP events around each whole call, variants in alternating blocks after 10 warm-up calls each",
           "variants": {"call": "imageprep.prepare_zju(img_u8, msk_cihp, K, D, ratio=0.5): device frames, host cameras, one dsn_image_prep launch",
                        "torch": "the same steps as torch ops: float64 map, grid_sample x 2, max_pool2d, product, avg_pool2d, / 255, slicing "
                                 "(float32 interpolation: different bits, a time reference only)"},
           "byte_floor": "uint8 frame and mask read once, float64 image and two small masks written once, over 8.0 TB/s",
           "not_measured": "host cv2 (not installed), the upload of the frames, more than one GPU", "items": {}}
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[:S, :S]
    for N in args.counts:
        img = torch.from_numpy(rng.randint(0, 256, (N, S, S, 3)).astype(np.uint8)).to(dev)
        body = (((yy - S / 2) / (0.4 * S)) ** 2 + ((xx - S / 2) / (0.2 * S)) ** 2 <= 1.0).astype(np.uint8) * 5
        msk = torch.from_numpy(np.broadcast_to(body, (N, S, S)).copy()).to(dev)
        ours = imageprep.prepare_zju(img, msk, K, D, ratio=1.0 / c, border=border)
        theirs = torch_prepare(img, msk, K, D, c, border)
        diff_levels = float((ours["img"] - theirs["img"]).abs().mean() * 255.0)
        fg_differs = int((ours["msk_fg"] != theirs["msk_fg"]).sum())
        assert diff_levels < 1.0 and fg_differs < 0.01 * ours["msk_fg"].numel(), (diff_levels, fg_differs)
        assert torch.equal(ours["msk_cihp"], theirs["msk_cihp"])
        variants = {"call": lambda: imageprep.prepare_zju(img, msk, K, D, ratio=1.0 / c, border=border),
                    "torch": lambda: torch_prepare(img, msk, K, D, c, border)}
        alternate(variants, 1, 30)                        # not recorded: the clocks come up from idle during the first launches
        q = alternate(variants, args.blocks, args.iters)
        floor = byte_floor(N, S, S, c)
        floor_ms = 1e3 * floor / HBM_BYTES_PER_S
        q.update(mean_abs_difference_levels=round(diff_levels, 4), msk_fg_pixels_differing=fg_differs, byte_floor_bytes=floor,
                 byte_floor_ms=round(floor_ms, 5), call_over_floor=round(q["call"]["median_ms"] / floor_ms, 2),
                 torch_over_floor=round(q["torch"]["median_ms"] / floor_ms, 2),
                 torch_over_call=round(q["torch"]["median_ms"] / q["call"]["median_ms"], 3))
        res["items"][str(N)] = q
        del img, msk, ours, theirs
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
