#!/usr/bin/env python3
"""Visualizer3D.render_mesh on the device (dsn_raster_mesh): per-kernel device times on the w4 body's marching-cubes meshes.
    python scripts/bench_render_mesh.py [--res 256 512] [--size 1024] [--reps 15] [--warmup 3] [--thresholds 16 64 256 ...] [--out FILE]
Setup: the w4 weights, the synthetic SMPL-like body posed by synth.pose_body(canon, seed=3) (scripts/bench_mesh.py's), extract_mesh at
each resolution, the camera 2.5 in front of the mesh's bounding-box centre, --size x --size pixels.
Per mesh, after warm-up, HIP events around each kernel of one frame (dsn_raster_mesh_ex's phases, enqueued one by one on the same
workspace: clear, project, raster, raster_big, shade), around the whole call (dsn_raster_mesh, all kernels in one call) and around
extract_mesh on the same mesh; repeats alternate over the meshes and the thresholds; medians with the interquartile range.
Beside each kernel time: the bytes it must move at least - project reads 12 V and writes 16 V, raster reads 12 T of indices and
16 V of projected vertices once (the mesh term 12 V + 12 T the issue names is the call's input) and touches 8 H W of visibility
buffer, clear writes 8 H W, shade reads 8 H W and writes 11 H W - and the fraction of HBM bandwidth (8.0 TB/s peak; 6.29 TB/s is what a
float4 copy reaches) that this implies.  The raster kernels are not streaming kernels: each covered pixel centre costs a dependent
8-byte read and, when the key is smaller, one 64-bit unsigned atomic minimum; the rate of those atomics on this chip has not been
measured on its own (the guide's atomic figures are for float adds), the times below are what is known.
The big-triangle threshold: the frame time of every mesh, of coarse meshes of the same body (--ab-res: triangles of tens to thousands
of pixels) and of two triangles that fill the image, far and from close by (camera --close in front of the bounding box), for each
--thresholds value, alternated.  Writes one JSON document."""
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
from dsnerf_amd import _lib, synth  # noqa: E402
from benchlib.common import load_weights  # noqa: E402

HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29
PHASES = [("clear", _lib.RM_CLEAR), ("project", _lib.RM_PROJECT), ("raster", _lib.RM_RASTER), ("raster_big", _lib.RM_RASTER_BIG),
          ("shade", _lib.RM_SHADE)]


def stats(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thresholds", type=int, nargs="+", default=[4, 16, 64, 256, 1024, 1 << 30])
    ap.add_argument("--ab-res", type=int, nargs="+", default=[16, 32, 64], help="coarse meshes of the threshold A/B only")
    ap.add_argument("--close", type=float, default=0.6, help="camera distance of the close-up of the threshold A/B")
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_mesh_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon, seed=3)
    cfg = SimpleNamespace(DATASETS=SimpleNamespace(SMPL_PATH="<synthetic>"),
                          MODEL=SimpleNamespace(sample_points_mode="GG", COARSE_RAY_SAMPLING=64, perturb=1.0, raw_noise_std=1.0, TYPE="nerf",
                                                FINE_RAY_SAMPLING=-1))
    net = dsnerf_amd.DualSpaceNeRF(cfg)
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in load_weights(synth, args.weights).items()})
    net.to(dev)
    r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
    r.eval()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    batch = {"xyz": T(xyz)[None], "poses": T(synth.make_poses(seed=5))[None], "Th": torch.zeros(1, 1, 3, device=dev),
             "frame": torch.tensor([5])}
    S = args.size

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    meshes, poses, close, held = {}, {}, {}, {}
    for res in list(args.res + args.ab_res) + ["quad"]:
        if res == "quad":          # two triangles over the whole image of the far camera of the first mesh
            c = torch.tensor(poses[args.res[0]][:3, 3] - np.array([0.0, 0.0, 2.5]), dtype=torch.float32, device=dev)
            q = torch.tensor([[-3.0, -3.0, 0.0], [3.0, -3.0, 0.0], [3.0, 3.0, 0.0], [-3.0, 3.0, 0.0]], device=dev)
            m = {"verts": q + c, "faces": torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev)}
        else:
            m = r.extract_mesh(batch, res)
            if m is None:          # (a grid too coarse to cross the level)
                args.ab_res.remove(res)
                continue
        meshes[res] = m
        lo, hi = m["verts"].min(dim=0).values.cpu().numpy(), m["verts"].max(dim=0).values.cpu().numpy()
        for store, dist in ((poses, 2.5), (close, args.close)):
            p = np.eye(4)
            # (2.5 from the centre, as the reference's camera from the origin; the close-up: that far from the box's front face)
            p[:3, 3] = 0.5 * (lo + hi) + np.array([0.0, 0.0, (0.5 * (hi[2] - lo[2]) + dist) if store is close else dist])
            store[res] = p
        # one set of outputs and one workspace per mesh, used by every phase call (phases= returns them)
        held[res] = _lib.raster_mesh(m["verts"], m["faces"], camera_pose=poses[res], height=S, phases=31)

    def frame(res, pose, big=0):
        m = meshes[res]
        return _lib.raster_mesh(m["verts"], m["faces"], camera_pose=pose, height=S, big_pixels=big, phases=31, out=held[res])

    def phase(res, bit):
        m = meshes[res]
        return _lib.raster_mesh(m["verts"], m["faces"], camera_pose=poses[res], height=S, phases=bit, out=held[res])

    for _ in range(args.warmup):
        for res in args.res:
            frame(res, poses[res])
            frame(res, close[res])
            for _, bit in PHASES:
                phase(res, bit)
            r.extract_mesh(batch, res)
    t = {res: {k: [] for k in [n for n, _ in PHASES] + ["frame", "extract_mesh"]} for res in args.res}
    ab_keys = args.res + args.ab_res + ["quad"]
    ab = {res: {"far": {th: [] for th in args.thresholds}, "close": {th: [] for th in args.thresholds}} for res in ab_keys}
    for res in args.ab_res + ["quad"]:
        for th in args.thresholds:
            frame(res, poses[res], th)
            frame(res, close[res], th)
    for rep in range(args.reps):
        for res in args.res:
            for name, bit in PHASES:          # (in frame order: each kernel sees what the one before left)
                t[res][name].append(timed(lambda: phase(res, bit))[0])
            t[res]["frame"].append(timed(lambda: frame(res, poses[res]))[0])
            if rep < 3:
                t[res]["extract_mesh"].append(timed(lambda: r.extract_mesh(batch, res))[0])
        for res in ab_keys:
            for th in args.thresholds:
                ab[res]["far"][th].append(timed(lambda: frame(res, poses[res], th))[0])
                ab[res]["close"][th].append(timed(lambda: frame(res, close[res], th))[0])
    ab_stats = lambda res: {side: {str(th): stats(v) for th, v in ab[res][side].items()} for side in ("far", "close")}
    out = {}
    for res in args.res:
        V, Tn = int(meshes[res]["verts"].shape[0]), int(meshes[res]["faces"].shape[0])
        img = frame(res, poses[res])
        covered = int((img["face"] >= 0).sum())
        big_n = int(held[res]["_ws"][16 * V + 8 * S * S:16 * V + 8 * S * S + 4].view(torch.int32)[0])
        byts = {"clear": 8 * S * S, "project": 12 * V + 16 * V, "raster": 12 * Tn + 16 * V + 8 * S * S, "raster_big": 0,
                "shade": 8 * S * S + 11 * S * S, "frame": 12 * V + 12 * Tn + 8 * S * S + 11 * S * S}
        rows = {}
        for k, v in t[res].items():
            s = stats(v)
            if k in byts and byts[k]:
                tbs = byts[k] / (s["median_ms"] * 1e-3) / 1e12 if s["median_ms"] > 0 else 0.0
                s.update({"min_bytes": byts[k], "implied_TBps": round(tbs, 4), "frac_of_hbm_peak": round(tbs / HBM_PEAK_TBS, 4),
                          "frac_of_hbm_copy_rate": round(tbs / HBM_COPY_TBS, 4)})
            rows[k] = s
        out[str(res)] = {"verts": V, "faces": Tn, "image": [S, S], "covered_pixels": covered, "big_triangles_at_default_threshold": big_n,
                         "mesh_bytes_12V_12T": 12 * V + 12 * Tn, "vis_bytes_8HW": 8 * S * S, "ms": rows,
                         "threshold_ab_frame_ms": ab_stats(res)}
    coarse = {str(res): dict(faces=int(meshes[res]["faces"].shape[0]), threshold_ab_frame_ms=ab_stats(res)) for res in args.ab_res + ["quad"]}
    doc = {"metric": "render_mesh", "weights": args.weights, "reps": args.reps, "warmup": args.warmup, "image": [S, S],
           "default_big_pixels": _lib.RM_BIG_PIXELS, "close_up_camera_distance": args.close,
           "hbm_peak_TBps": HBM_PEAK_TBS, "hbm_float4_copy_TBps": HBM_COPY_TBS,
           "note": "times by HIP events around single enqueues (they include the launch); the rate of 64-bit unsigned-minimum atomics on "
                   "this chip has not been measured on its own; extract_mesh includes its one device-to-host read of the counts",
           "by_resolution": out, "threshold_ab_coarse_meshes": coarse, "device": torch.cuda.get_device_name(0)}
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
