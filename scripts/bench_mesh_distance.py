#!/usr/bin/env python3
"""The distance between two meshes on the device (dsn_mesh_dist_build / _query / _reduce, dsn_mesh_sample_surface): device times on the w4
body's marching-cubes meshes.
    python scripts/bench_mesh_distance.py [--res 256 512] [--target 200000] [--taubin 5] [--samples 1000000] [--reps 9] [--warmup 2]
                                          [--out FILE]
Setup: scripts/bench_mesh_simplify.py's - the w4 weights, the synthetic SMPL-like body posed by synth.pose_body(canon, seed=3), extract_mesh
at each resolution (the dense mesh).  Three comparisons per resolution, both directions each:
  simplified   visualizer.simplify_mesh(dense, target_vertices=--target) against the dense mesh
  smoothed     visualizer.smooth_mesh(dense, iterations=--taubin) against the dense mesh
  coarse       extract_mesh(coarse=4, dilate=1, max_dilate=1) - the coarse-to-fine extraction with one ring - against the dense mesh
Per direction, after warm-up, HIP events around single enqueues on one workspace; medians with the interquartile range:
  build        dsn_mesh_dist_build over the target mesh (its nine launches)
  query        dsn_mesh_dist_query of the source mesh's vertices, all three outputs
  reduce       dsn_mesh_dist_reduce
  sample + query   --samples area-weighted surface samples of the source (dsn_mesh_sample_surface) and their query
points_per_s = queries over the query's median.  byte_floor: queries x 12 B in and 20 B out plus the target once (12 V + 12 T bytes) over
the HBM peak (8 TB/s); hbm_fraction = that floor over the measured query time - the achieved share of the peak if the kernel moved
nothing else, which it does (the cell lists, and every candidate's corners once per query that looks at it).  The figures of
visualizer.mesh_distance (one call, with its allocations and its host read) are recorded beside the times.  Runs on the GPU only.
Writes one JSON document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dsnerf_amd  # noqa: E402,F401
from dsnerf_amd import _lib, visualizer  # noqa: E402
from bench_mesh_simplify import scene, stats, timed  # noqa: E402

HBM_PEAK = 8.0e12


def direction(src, dst, samples, reps, warmup):
    """times of one direction: the points of src against the surface of dst"""
    sv, sf = src
    dv, df = dst
    n = sv.shape[0]
    index = _lib.mesh_dist_build(dv, df)
    state = {"ws": index["ws"], "counts": index["counts"]}
    out = _lib.mesh_dist_query(index, sv)
    spts = _lib.mesh_sample_surface(sv, sf, samples, 0, want_face=False)[0]
    sout = _lib.mesh_dist_query(index, spts)
    t = {k: [] for k in ("build", "query", "reduce", "sample", "sample_query")}
    for rep in range(warmup + reps):
        row = {"build": timed(lambda: _lib.mesh_dist_build(dv, df, check=False, state=state, box=(index["box"][:3], index["box"][3:])))[0],
               "query": timed(lambda: _lib.mesh_dist_query(index, sv, out=out))[0],
               "reduce": timed(lambda: _lib.mesh_dist_reduce(out["dist2"]))[0],
               "sample": timed(lambda: _lib.mesh_sample_surface(sv, sf, samples, 0, want_face=False))[0],
               "sample_query": timed(lambda: _lib.mesh_dist_query(index, spts, out=sout))[0]}
        if rep >= warmup:
            for k, v in row.items():
                t[k].append(v)
    rows = {k: stats(v) for k, v in t.items()}
    V, T = dv.shape[0], df.shape[0]

    def rate(count, ms):
        floor = (32.0 * count + 12.0 * V + 12.0 * T) / HBM_PEAK * 1e3
        return {"points": count, "points_per_s": round(count / (ms * 1e-3)), "byte_floor_ms": round(floor, 4), "hbm_fraction": round(floor / ms, 4)}
    info = index["info"]
    return {"queries": n, "target_verts": V, "target_faces": T, "grid": dict(info, mean_list=round(info["listed_pairs"] / max(info["cells"], 1), 2)),
            "workspace_bytes": index["nbytes"], "ms": rows, "vertices": rate(n, rows["query"]["median_ms"]),
            "samples": rate(samples, rows["sample_query"]["median_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--target", type=int, default=200000)
    ap.add_argument("--taubin", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_distance_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    r, batch = scene(args.weights, dev)
    out = {}
    for res in args.res:
        dense = r.extract_mesh(batch, res)
        others = {"simplified": visualizer.simplify_mesh(dense, target_vertices=args.target),
                  "smoothed": visualizer.smooth_mesh(dense, iterations=args.taubin),
                  "coarse": r.extract_mesh(batch, res, coarse=4, dilate=1, max_dilate=1)}
        dm = (dense["verts"], dense["faces"])
        for name, other in others.items():
            om = (other["verts"], other["faces"])
            figures = visualizer.mesh_distance(om, dm)
            entry = {"figures": figures, "other_to_dense": direction(om, dm, args.samples, args.reps, args.warmup),
                     "dense_to_other": direction(dm, om, args.samples, args.reps, args.warmup)}
            if name == "coarse":
                entry["grid_info"] = {k: v for k, v in other.get("grid_info", {}).items() if isinstance(v, (int, float, bool))}
            print(f"res {res} {name}: {json.dumps(entry)}", file=sys.stderr, flush=True)
            out[f"{res}/{name}"] = entry
    doc = {"metric": "mesh_distance", "weights": args.weights, "reps": args.reps, "warmup": args.warmup, "hbm_peak_bytes_per_s": HBM_PEAK,
           "target_vertices": args.target, "taubin_pairs": args.taubin, "samples": args.samples,
           "note": "times by HIP events around single enqueues (they include the launches: build = 9, query = 1, reduce = 2, sample = 5); "
                   "byte_floor_ms = (32 B per query + 12 V + 12 T of the target) over the HBM peak, hbm_fraction = byte_floor_ms over the "
                   "query's median; figures: visualizer.mesh_distance(other, dense), vertices of each against the surface of the other",
           "by_resolution_and_comparison": out, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
