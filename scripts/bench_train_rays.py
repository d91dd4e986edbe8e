#!/usr/bin/env python3
"""The training-batch sampler on the device (dsn_train_rays, Renderer.sample_batch) against the host.
    python scripts/bench_train_rays.py [--reps 30] [--out profiles/train_rays_bench.json]
Synthetic body at 512^2 / 4096 rays and 1024^2 / 8192 rays, both conventions: HIP-event time of _lib.train_rays (median per call and
spread, the image, masks and camera already on the device), the wall time of the numpy restatement of the same rule
(tests/train_rays_restate.py: whole-image float64 rays, box mask, argwhere lists, draws, rounds - what the datasets' my_sample_ray /
sample_ray_h36m do on the host), and Renderer.render (eval mode, wall time to the synchronised result) fed from a host batch, as a
DataLoader hands it over, against sample_batch(check=False) + render.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import dsnerf_amd  # noqa: E402
from dsnerf_amd import _lib, synth  # noqa: E402
import train_rays_restate as TR  # noqa: E402


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
    return float(np.median(t)), float(np.percentile(t, 75) - np.percentile(t, 25))


def wall_ms(fn, reps):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.percentile(t, 75) - np.percentile(t, 25))


def scene(hw, xyz):
    """camera in front of the posed body, its bounds as the datasets pad them, a body-shaped label map with a face and a border"""
    lo, hi = xyz.min(0) - 0.05, xyz.max(0) + 0.05
    f = 1.05 * hw
    K = np.array([[f, 0.0, hw / 2 - 0.5], [0.0, f, hw / 2 - 0.5], [0.0, 0.0, 1.0]])
    R = np.eye(3)
    T = np.array([0.013, 0.021, 3.0]) - (lo + hi) / 2
    bounds = np.stack([lo, hi]).astype(np.float32).astype(np.float64)
    y, x = np.mgrid[:hw, :hw] / float(hw)
    cihp = np.zeros((hw, hw), np.uint8)
    cihp[((y - 0.5) / 0.3) ** 2 + ((x - 0.5) / 0.12) ** 2 <= 1.0] = 5
    cihp[(cihp != 0) & (y < 0.28)] = 2
    msk = (cihp != 0).astype(np.uint8)
    rng = np.random.default_rng(hw)
    msk[(msk == 1) & (rng.random((hw, hw)) < 0.01)] = 100
    img = rng.random((hw, hw, 3), dtype=np.float32)
    return K, R, T, bounds, img, cihp, msk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_rays_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon)
    cfg = SimpleNamespace(DATASETS=SimpleNamespace(SMPL_PATH="<synthetic>"),
                          MODEL=SimpleNamespace(sample_points_mode="GG", COARSE_RAY_SAMPLING=64, perturb=1.0, raw_noise_std=1.0, TYPE="nerf",
                                                FINE_RAY_SAMPLING=-1))
    net = dsnerf_amd.DualSpaceNeRF(cfg).to(dev)
    r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
    r.eval()
    frame = {"xyz": torch.from_numpy(np.ascontiguousarray(xyz, np.float32))[None], "poses": torch.zeros(1, 24, 3),
             "frame": torch.tensor([0])}
    res = {"metric": "train_rays_on_device", "reps": args.reps, "ms": {}, "iqr_ms": {}, "rounds": {}}
    for hw, nrays in ((512, 4096), (1024, 8192)):
        K, R, T, bounds, img, cihp, msk = scene(hw, np.asarray(xyz, np.float64))
        d = lambda a: torch.from_numpy(a).to(dev)
        Dimg, Dcihp, Dmsk = d(img), d(cihp), d(msk)
        for conv in ("zju", "h36m"):
            mask, dmask, mb, dmb = (cihp, Dcihp, None, None) if conv == "zju" else (msk, Dmsk, cihp, Dcihp)
            ws = _lib.train_rays(Dimg, K, R, T, bounds, dmask, nrays, 0, convention=conv, mask_b=dmb)["workspace"]
            seed = [0]

            def call():
                seed[0] += 1
                return _lib.train_rays(Dimg, K, R, T, bounds, dmask, nrays, seed[0], convention=conv, mask_b=dmb, workspace=ws)

            for _ in range(3):
                out = call()
            assert int(out["status"]) == _lib.TRAIN_RAYS_OK, int(out["status"])
            key = f"{conv}_{hw}_{nrays}"
            res["rounds"][key] = int(out["rounds"])
            res["ms"]["device_" + key], res["iqr_ms"]["device_" + key] = event_ms(call, args.reps)
            host = lambda: TR.sample(img, K, R, T, bounds, mask, nrays, 1, convention=conv, mask_b=mb)
            e = host()
            assert e["status"] == TR.OK
            t = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                host()
                t.append(1e3 * (time.perf_counter() - t0))
            res["ms"]["host_numpy_" + key] = float(np.median(t))
            if conv == "zju":
                hb = {k: torch.from_numpy(np.ascontiguousarray(e[k]))[None] for k in ("ray_o", "ray_d", "near", "far")}
                from_host = lambda: r.render({**{k: v.clone() for k, v in hb.items()}, **frame})["coarse"]["color"]
                from_dev = lambda: r.render({**r.sample_batch(Dimg, K, R, T, bounds, dmask, nrays, 1, check=False), **frame})["coarse"]["color"]
                for fn in (from_host, from_dev):
                    for _ in range(3):
                        fn()
                res["ms"]["render_from_host_batch_" + key], res["iqr_ms"]["render_from_host_batch_" + key] = wall_ms(from_host, args.reps)
                res["ms"]["sample_batch_and_render_" + key], res["iqr_ms"]["sample_batch_and_render_" + key] = wall_ms(from_dev, args.reps)
    res["ms"] = {k: round(v, 4) for k, v in res["ms"].items()}
    res["iqr_ms"] = {k: round(v, 4) for k, v in res["iqr_ms"].items()}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
