#!/usr/bin/env python3
"""Mesh extraction of the posed w4 body, dense grid against the coarse-to-fine grid (Renderer.extract_mesh(coarse=...), the rule of
include/dsnerf.h), on the device.
    python scripts/bench_mesh_hier.py [--res 256 512 1024] [--coarse 4] [--dilate 1] [--reps 5] [--sweep] [--out profiles/mesh_hier_bench.json]
Setup as scripts/bench_mesh.py: the w4 weights, the synthetic SMPL-like body posed by synth.pose_body(canon, seed=3), get_grid's axes at
each resolution, level 0.5.  After warm-up the dense and the hierarchical calls ALTERNATE in one process; HIP-event medians and
quartiles over --reps rounds of
    dense.density_grid / dense.mc / dense.extract_mesh      the dense path as it is (the yardstick: this script's own run of it)
    hier.coarse, hier.mark_list, hier.listed, hier.assemble, hier.mc      the stages of the hierarchical path
    hier.extract_mesh                                       Renderer.extract_mesh(coarse=..., dilate=...) end to end
plus evaluated_points / points, leaks, the hidden points (inside masks of the dense and the assembled volume of the same run) and
whether the two meshes (vertices, faces, normals) are bit-identical.  --sweep adds the evaluated fraction, leaks and hidden points
for factors 2, 4, 8 and 1 - 4 rings at every resolution that ran.  A resolution whose dense volume, marching-cubes workspace and
density slab do not fit beside the rest of the device memory is skipped and says so.  Prints one JSON line; --out also writes it."""
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

LEVEL = 0.5


def quart(v):
    q1, med, q3 = (float(x) for x in np.percentile(np.asarray(v, np.float64), [25, 50, 75]))
    return {"median": round(med, 3), "q1": round(q1, 3), "q3": round(q3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--coarse", type=int, default=4)
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sweep", action="store_true", help="also: evaluated fraction, leaks and hidden points for factors 2, 4, 8 x 1 - 4 rings")
    ap.add_argument("--out", default=None)
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
    packed = r.net.packed(dev)
    c, dil = args.coarse, args.dilate

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def hier_stages(axes, t=None):
        """_lib.density_grid_hier's chain, stage by stage (the scene's frame state is set by the dense call in front of it)"""
        x, y, z = _lib._axes_dev(axes, dev)
        shape = (x.numel(), y.numel(), z.numel())
        ix, iy, iz = (torch.from_numpy(a).to(dev) for a in _lib.grid_hier_axes(shape, c))

        def coarse_pass():
            lin = ((ix[:, None, None] * shape[1] + iy[None, :, None]) * shape[2] + iz[None, None, :]).to(torch.int32)
            return _lib.density_points(r.scene, packed, (x, y, z), lin.reshape(-1)).reshape(lin.shape).contiguous()

        def mark_list(coarse):
            ws, counts = _lib.grid_hier_mark(coarse, shape, c, dil, LEVEL)
            counts = [int(v) for v in counts.cpu()]
            return ws, counts, _lib.grid_hier_list(ws, shape, c, counts[2])

        ms0, coarse = timed(coarse_pass)
        ms1, (ws, counts, index) = timed(lambda: mark_list(coarse))
        ms2, values = timed(lambda: _lib.density_points(r.scene, packed, (x, y, z), index))
        ms3, (vol, leaks) = timed(lambda: _lib.grid_hier_assemble(coarse, shape, c, LEVEL, ws, index, values))
        del ws, index, values
        ms4, mesh = timed(lambda: _lib.marching_cubes(vol, axes, LEVEL, "ascent", want_normals=True))
        if t is not None:
            for k, ms in zip(("coarse", "mark_list", "listed", "assemble", "mc"), (ms0, ms1, ms2, ms3, ms4)):
                t["hier." + k].append(ms)
        return vol, counts, int(leaks.cpu()), mesh

    out = {}
    for res in args.res:
        axes = r.grid_axes(batch["xyz"][0], res)
        shape = tuple(len(a) for a in axes)
        n = shape[0] * shape[1] * shape[2]
        if n >= 1 << 31:
            out[str(res)] = {"grid": list(shape), "points": n, "skipped": "2^31 grid points or more"}
            continue
        # dense volume + the assembled one beside it (the comparison) + marching cubes' workspace + the density slab
        need = 2 * 4 * n + _lib.lib().dsn_mc_workspace_bytes(*shape) + _lib.lib().dsn_density_grid_workspace_bytes(
            max(shape[1] * shape[2], min(_lib.DENSITY_GRID_SLAB_POINTS, n))) + (1 << 30)
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            out[str(res)] = {"grid": list(shape), "points": n, "skipped": f"needs {need >> 20} MiB, {free >> 20} MiB free"}
            continue
        keys = ["dense.density_grid", "dense.mc", "dense.extract_mesh", "hier.coarse", "hier.mark_list", "hier.listed", "hier.assemble",
                "hier.mc", "hier.extract_mesh"]
        t = {k: [] for k in keys}
        for rep in range(args.warmup + args.reps):
            tt = t if rep >= args.warmup else {k: [] for k in keys}
            ms, (_, dense) = timed(lambda: r.density_grid(batch, axes=axes))
            tt["dense.density_grid"].append(ms)
            ms, dense_mesh = timed(lambda: _lib.marching_cubes(dense, axes, LEVEL, "ascent", want_normals=True))
            tt["dense.mc"].append(ms)
            vol, counts, leaks, hier_mesh = hier_stages(axes, tt)
            if rep == args.warmup + args.reps - 1:
                hidden = int(((dense > LEVEL) != (vol > LEVEL)).sum())
                same = all(a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(dense_mesh, hier_mesh))
                nv, nf = int(dense_mesh[0].shape[0]), int(dense_mesh[1].shape[0])
            del dense, vol, dense_mesh, hier_mesh
            tt["dense.extract_mesh"].append(timed(lambda: r.extract_mesh(batch, res, level=LEVEL, axes=axes, normals=True))[0])
            ms, m = timed(lambda: r.extract_mesh(batch, res, level=LEVEL, axes=axes, normals=True, coarse=c, dilate=dil))
            tt["hier.extract_mesh"].append(ms)
            info = m["grid_info"]
            del m
        out[str(res)] = {"grid": list(shape), "points": n, "evaluated_points": counts[2], "evaluated_fraction": round(counts[2] / n, 5),
                         "core_cells": counts[0], "active_cells": counts[1], "leaks": leaks, "hidden_points": hidden,
                         "meshes_bit_identical": bool(same), "verts": nv, "faces": nf,
                         "extract_mesh_attempts": info["attempts"], "extract_mesh_fell_back": info["fell_back"],
                         "extract_mesh_dilate": info["dilate"], "ms": {k: quart(v) for k, v in t.items()}}
        torch.cuda.empty_cache()
    sweep = {}
    if args.sweep:      # the stages driven by a gather from the dense volume of the same run (the values are the same bits either way)
        for res in args.res:
            if "skipped" in out[str(res)]:
                continue
            axes, dense = r.density_grid(batch, resolution=res)
            flat = dense.reshape(-1)
            for cc in (2, 4, 8):
                for rr in (1, 2, 3, 4):
                    vol, info = _lib.density_grid_hier(None, None, axes, LEVEL, factor=cc, dilate=rr, evaluate=lambda index: flat[index.long()])
                    sweep[f"{res}/c{cc}/r{rr}"] = {"evaluated_fraction": round(info["evaluated_points"] / info["points"], 4),
                                                   "leaks": info["leaks"], "hidden_points": int(((dense > LEVEL) != (vol > LEVEL)).sum())}
                    del vol
            del dense, flat
            torch.cuda.empty_cache()
    res = {"metric": "mesh_extraction_coarse_to_fine", "weights": args.weights, "reps": args.reps, "level": LEVEL, "coarse": c,
           "dilate": dil, "gradient_direction": "ascent", "normals": True, "by_resolution": out, "sweep": sweep, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
