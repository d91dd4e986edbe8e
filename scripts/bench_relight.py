#!/usr/bin/env python3
"""Relighting sweep vs one render_view per light on the w4 bench frame (512 x 512 x 64, the converged checkpoint, early stop as the
Renderer plans it): the reference's vis_lighting.py renders every view under ten rotations of the light about the head.
    python scripts/bench_relight.py [--reps 7] [--hw 512]
For K = 1, 4 and 10 of those angles, alternated in one process after warm-up: HIP-event time of Renderer.render_view_lights(K lights)
and of K Renderer.render_view calls (device-resident batch and images), the median over --reps rounds; whether every light's images
are equal (torch.equal) between the two.  Prints one JSON line."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dsnerf_amd  # noqa: E402
from dsnerf_amd import synth  # noqa: E402
from benchlib.common import load_weights  # noqa: E402

HEAD = torch.tensor([[0.18649693, -0.14180326, 1.7103844]])          # vis_lighting.py:57


def angle2rot(angle):                                                # vis_lighting.py:86-91
    rad = np.pi * angle / 180
    return np.array([[np.cos(rad), -np.sin(rad)], [np.sin(rad), np.cos(rad)]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = args.hw
    S = args.samples
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon, seed=3)
    rays = synth.make_rays(H, W, xyz, fit_box=True)
    cfg = SimpleNamespace(DATASETS=SimpleNamespace(SMPL_PATH="<synthetic>"),
                          MODEL=SimpleNamespace(sample_points_mode="GG", COARSE_RAY_SAMPLING=S, perturb=1.0, raw_noise_std=1.0, TYPE="nerf",
                                                FINE_RAY_SAMPLING=-1))
    net = dsnerf_amd.DualSpaceNeRF(cfg)
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in load_weights(synth, args.weights).items()})
    net.to(dev)
    r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
    r.eval()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    batch = {"ray_o": T(rays["ray_o"])[None], "ray_d": T(rays["ray_d"])[None], "near": T(rays["near"])[None], "far": T(rays["far"])[None],
             "xyz": T(xyz)[None], "poses": T(synth.make_poses(seed=5))[None], "Th": torch.zeros(1, 1, 3, device=dev),
             "frame": torch.tensor([5]), "img": torch.zeros(1, H, W, 3, device=dev), "mask_at_box": torch.ones(1, H * W, dtype=torch.bool, device=dev)}
    lights = [{"rot": torch.Tensor(angle2rot(a)), "rot_center": HEAD} for a in range(0, 360, 36)]

    def views(K):
        out = []
        for lt in lights[:K]:
            net.set_rot_center(lt["rot_center"])
            net.set_rot(lt["rot"])
            out.append(r.render_view(dict(batch), device_output=True))
        net.rot = net.rot_center = None
        return out

    def sweep(K):
        return r.render_view_lights(dict(batch), lights[:K], device_output=True)

    def timed(fn, K):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        res = fn(K)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), res

    Ks = (1, 4, 10)
    for _ in range(args.warmup):
        for K in Ks:
            views(K)
            sweep(K)
    equal = True
    for K in Ks:
        v, s = views(K), sweep(K)
        # (bit patterns: disp is NaN where acc is 0)
        equal = equal and all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for x, y in zip(v, s) for k in x)
    t = {K: {"sweep": [], "views": []} for K in Ks}
    for _ in range(args.reps):
        for K in Ks:
            t[K]["views"].append(timed(views, K)[0])
            t[K]["sweep"].append(timed(sweep, K)[0])
    med = {K: {k: float(np.median(v)) for k, v in d.items()} for K, d in t.items()}
    res = {"metric": "relight_sweep", "frame": f"{H}x{W}x{S}", "weights": args.weights, "reps": args.reps,
           "early_stop": bool(r.last_frame_info.get("early_stop")), "images_equal": bool(equal),
           "ms": {str(K): {"sweep": round(m["sweep"], 3), "render_views": round(m["views"], 3),
                           "ratio": round(m["sweep"] / m["views"], 4)} for K, m in med.items()},
           "ms_per_extra_light": round((med[10]["sweep"] - med[1]["sweep"]) / 9.0, 4),
           "ms_per_render_view": round(med[10]["views"] / 10.0, 4),
           "spread_ms": {str(K): {k: round(float(np.max(v) - np.min(v)), 3) for k, v in d.items()} for K, d in t.items()},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
