#!/usr/bin/env python3
"""Mesh extraction of the posed w4 body (utils/visualizer.py Visualizer3D: get_grid_pred_batch + get_mesh_from_grid) on the device.
    python scripts/bench_mesh.py [--res 128 256 512] [--reps 3] [--render-view]
Setup: the w4 weights, the synthetic SMPL-like body posed by synth.pose_body(canon, seed=3), get_grid's axes at each resolution.  After
warm-up, alternated in one process, HIP-event medians over --reps rounds of
    density_grid   Renderer.density_grid (dsn_density_grid: grid points + warp + density-only split-fp16 kernel, in slabs)
    mc             marching cubes count + emit on that volume (_lib.marching_cubes: one device->host read of the counts)
    extract_mesh   Renderer.extract_mesh end to end
    chunk_loop     what users have today: w2l_without_lbs + query_volume in 100 000-point chunks (128 and 256 only)
plus grid points/s, evaluated (non-transparent) points, and the field's TFLOP/s on the evaluated points with the FLOPs counted from
the layer shapes below, as a fraction of the split-fp16 ceiling of the bench line (dense f16 MFMA peak / 3 products).
--render-view: one 512 x 512 x 64 render_view of the bench frame first (a kernel trace then holds k_field16's forward mode beside
the density-only kernel).  Prints one JSON line."""
import argparse
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dsnerf_amd  # noqa: E402
from dsnerf_amd import _lib, synth  # noqa: E402
from benchlib.common import PEAK_F16_MATRIX_TFLOPS, SPLIT_PRODUCTS, load_weights  # noqa: E402

# density-only trunk (model/spacenet.py:18-81): stage1.0 PE 63 -> 256 (its 24 code / pose columns are constant per frame: folded
# into the bias), three 256 -> 256, stage2.0 [256 + 63] -> 256, two 256 -> 256, density head 256 -> 1 = 425 728 multiply-adds (the
# reverse pass's count, benchlib FLOP_FIELD_REV_PER_SAMPLE).  2 FLOP per multiply-add.
LAYERS = [(63, 256), (256, 256), (256, 256), (256, 256), (256 + 63, 256), (256, 256), (256, 256), (256, 1)]
FLOP_DENSITY = 2 * sum(a * b for a, b in LAYERS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--loop-res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--render-view", action="store_true")
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
    if args.render_view:
        rays = synth.make_rays(512, 512, xyz, fit_box=True)
        vb = dict(batch, ray_o=T(rays["ray_o"])[None], ray_d=T(rays["ray_d"])[None], near=T(rays["near"])[None], far=T(rays["far"])[None],
                  img=torch.zeros(1, 512, 512, 3, device=dev), mask_at_box=torch.ones(1, 512 * 512, dtype=torch.bool, device=dev))
        r.render_view(vb, device_output=True)
        torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    axes = {res: r.grid_axes(batch["xyz"][0], res) for res in args.res}
    frame = int(batch["frame"][0])

    def chunk_loop(res):
        pts = torch.from_numpy(np.stack(np.meshgrid(*axes[res], indexing="ij"), -1).reshape(-1, 3)).float()
        out = []
        for i in range(0, pts.shape[0], 100000):
            p = pts[i:i + 100000].to(dev)
            can, tm = r.w2l_without_lbs(p.reshape(1, -1, 1, 3), batch, r.canonical_model)
            out.append(r.query_volume(can.reshape(1, -1, 3), torch.tensor([frame], device=dev), tm, batch))
        return torch.cat(out, 1)

    vols = {}
    for _ in range(args.warmup):
        for res in args.res:
            vols[res] = r.density_grid(batch, axes=axes[res])[1]
            _lib.marching_cubes(vols[res], axes[res], 0.5, "ascent")
            r.extract_mesh(batch, res, axes=axes[res])
            if res in args.loop_res:
                chunk_loop(res)
    t = {res: {"density_grid": [], "mc": [], "extract_mesh": [], "chunk_loop": []} for res in args.res}
    for _ in range(args.reps):
        for res in args.res:
            ms, (_, vol) = timed(lambda: r.density_grid(batch, axes=axes[res]))
            t[res]["density_grid"].append(ms)
            vols[res] = vol
            t[res]["mc"].append(timed(lambda: _lib.marching_cubes(vol, axes[res], 0.5, "ascent"))[0])
            t[res]["extract_mesh"].append(timed(lambda: r.extract_mesh(batch, res, axes=axes[res]))[0])
            del vol
            if res in args.loop_res:
                t[res]["chunk_loop"].append(timed(lambda: chunk_loop(res))[0])
    out = {}
    for res in args.res:
        nx, ny, nz = (len(a) for a in axes[res])
        n = nx * ny * nz
        vol = vols[res]
        n_eval = int((vol != 0).sum())          # (a non-transparent point whose density is exactly 0 is not counted)
        verts, faces_ = _lib.marching_cubes(vol, axes[res], 0.5, "ascent")
        med = {k: float(np.median(v)) for k, v in t[res].items() if v}
        ach = n_eval * FLOP_DENSITY / (med["density_grid"] * 1e-3) / 1e12
        peak = PEAK_F16_MATRIX_TFLOPS / SPLIT_PRODUCTS
        out[str(res)] = {"grid": [nx, ny, nz], "points": n, "evaluated_points": n_eval, "evaluated_fraction": round(n_eval / n, 4),
                         "verts": int(verts.shape[0]), "faces": int(faces_.shape[0]),
                         "ms": {k: round(v, 3) for k, v in med.items()},
                         "spread_ms": {k: round(float(np.max(v) - np.min(v)), 3) for k, v in t[res].items() if v},
                         "grid_points_per_s": round(n / (med["density_grid"] * 1e-3), 1),
                         "evaluated_points_per_s": round(n_eval / (med["density_grid"] * 1e-3), 1),
                         "field_tflops_on_evaluated_points": round(ach, 2), "frac_of_split_f16_ceiling": round(ach / peak, 4)}
        if "chunk_loop" in med:
            out[str(res)]["speedup_vs_chunk_loop"] = round(med["chunk_loop"] / med["density_grid"], 1)
    res = {"metric": "mesh_extraction", "weights": args.weights, "reps": args.reps, "level": 0.5, "gradient_direction": "ascent",
           "flop_per_evaluated_point": FLOP_DENSITY, "split_f16_ceiling_tflops": round(PEAK_F16_MATRIX_TFLOPS / SPLIT_PRODUCTS, 1),
           "by_resolution": out, "device": torch.cuda.get_device_name(0)}
    if args.render_view:
        # the first resolution's active points once more, through k_field16's forward mode (dsn_field_forward) and through the grid
        # (one slab): a kernel trace then holds both modes on the same points
        res0 = args.res[0]
        _, vol = r.density_grid(batch, axes=axes[res0], slab_points=math.prod(len(a) for a in axes[res0]))
        pts = torch.from_numpy(np.stack(np.meshgrid(*axes[res0], indexing="ij"), -1).reshape(-1, 3)).float().to(dev)
        w = _lib.warp(r.scene, pts, None, 1, want_dir=False)
        x_act = w["x_c"][~w["transparent"].bool()].contiguous()
        ms_fwd = timed(lambda: _lib.field_forward(r.scene, r.net.packed(dev), x_act))[0]
        res["same_points"] = {"res": res0, "points": int(x_act.shape[0]), "field_forward_call_ms": round(ms_fwd, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
