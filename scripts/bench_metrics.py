#!/usr/bin/env python3
"""SSIM of test.py's evaluation loop on the device (dsn_image_ssim) against the float64 numpy / scipy restatement of metrics.py's
ssim_metric (tests/ssim_oracle.py) on the same inputs.
    python scripts/bench_metrics.py [--reps 20]
Body-shaped masks (a 512 x 512 frame's crop is about 307 x 256, as the reference's test frames), float64 ground truth as the
reference's batch["img"].  HIP-event time of _lib.image_ssim on one 512^2 and one 1024^2 frame and on a batch of 16 512^2 frames
(median per call); wall time of Renderer.image_metrics(ssim=True) from the call to the python floats (device image, host batch
as a DataLoader hands it over) next to image_metrics without ssim; the host restatement's wall time; the largest
|device - host| SSIM.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dsnerf_amd  # noqa: E402
from dsnerf_amd import _lib, synth  # noqa: E402
from ssim_oracle import bounding_rect, ssim_metric  # noqa: E402


def body_mask(H, W, seed):
    """an ellipse for the torso and two for the legs: bounding rectangle ~0.6 H x 0.5 W"""
    yy, xx = np.mgrid[0:H, 0:W] / np.array([H, W])[:, None, None]
    rng = np.random.default_rng(seed)
    dx = rng.uniform(-0.05, 0.05)
    m = ((yy - 0.4) / 0.2) ** 2 + ((xx - 0.5 - dx) / 0.25) ** 2 <= 1.0
    for side in (-1, 1):
        m |= ((yy - 0.65) / 0.15) ** 2 + ((xx - 0.5 - dx - 0.1 * side) / 0.06) ** 2 <= 1.0
    return m


def frame(H, W, seed):
    rng = np.random.default_rng(seed)
    pred = rng.random((H, W, 3), dtype=np.float32)
    gt = np.clip(pred * 0.9 + rng.normal(0, 0.05, (H, W, 3)), 0, 1)
    return pred, gt, body_mask(H, W, seed)


def event_ms(fn, reps):
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t)), float(np.max(t) - np.min(t))


def wall_ms(fn, reps):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.max(t) - np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    canon, faces = synth.make_body()
    cfg = SimpleNamespace(DATASETS=SimpleNamespace(SMPL_PATH="<synthetic>"),
                          MODEL=SimpleNamespace(sample_points_mode="GG", COARSE_RAY_SAMPLING=64, perturb=1.0, raw_noise_std=1.0, TYPE="nerf",
                                                FINE_RAY_SAMPLING=-1))
    net = dsnerf_amd.DualSpaceNeRF(cfg).to(dev)
    r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
    r.eval()
    res = {"metric": "ssim_on_device", "reps": args.reps, "ms": {}, "spread_ms": {}, "crop": {}, "max_abs_diff": 0.0}
    for hw in (512, 1024):
        pred, gt, mask = frame(hw, hw, hw)
        x, y, w, h = bounding_rect(mask)
        res["crop"][str(hw)] = f"{h}x{w}"
        P, G, M = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)
        call = lambda: _lib.image_ssim(P, G, M, clamp=True)
        for _ in range(3):
            call()
        res["ms"][f"image_ssim_{hw}"], res["spread_ms"][f"image_ssim_{hw}"] = event_ms(call, args.reps)
        dev_val = float(call()[0].cpu())
        batch = {"img": torch.from_numpy(gt)[None], "mask_at_box": torch.from_numpy(mask.reshape(-1))[None]}
        for ssim in (False, True):
            fn = lambda: r.image_metrics(P, batch, ssim=ssim)
            for _ in range(3):
                fn()
            key = f"image_metrics{'_ssim' if ssim else ''}_wall_{hw}"
            res["ms"][key], res["spread_ms"][key] = wall_ms(fn, args.reps)
        host = lambda: ssim_metric(np.clip(pred, 0, 1), gt, mask)
        host_val = host()
        res["ms"][f"host_restatement_{hw}"], res["spread_ms"][f"host_restatement_{hw}"] = wall_ms(host, args.host_reps)
        res["max_abs_diff"] = max(res["max_abs_diff"], abs(dev_val - host_val))
    F = args.batch
    frames = [frame(512, 512, 1000 + k) for k in range(F)]
    P = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
    G = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
    M = torch.from_numpy(np.stack([f[2] for f in frames])).to(dev)
    call = lambda: _lib.image_ssim(P, G, M, clamp=True)
    for _ in range(3):
        call()
    key = f"image_ssim_batch{F}_512"
    res["ms"][key], res["spread_ms"][key] = event_ms(call, args.reps)
    got = call()[0].cpu().numpy()
    k = F - 1
    res["max_abs_diff"] = max(res["max_abs_diff"], abs(float(got[k]) - ssim_metric(np.clip(frames[k][0], 0, 1), frames[k][1], frames[k][2])))
    res["ms"] = {k: round(v, 4) for k, v in res["ms"].items()}
    res["spread_ms"] = {k: round(v, 4) for k, v in res["spread_ms"].items()}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
