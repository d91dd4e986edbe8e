#!/usr/bin/env python3
"""A bound mesh under other poses on the device: device times on the w4 body's marching-cubes meshes.
    python scripts/bench_mesh_pose.py [--res 256 512] [--poses 1 8] [--reps 15] [--warmup 3] [--out FILE]
Setup: scripts/bench_mesh_attr.py's - the w4 weights, the synthetic body posed by synth.pose_body(canon, seed=3), extract_mesh with
normals at each resolution.  The mesh is bound once (Renderer.bind_mesh: dsn_warp in slabs + dsn_mesh_bind_normals, timed as one whole
call with its allocations); the targets are synth.pose_body(canon, seed=7 + k) for k < P.  After warm-up, HIP events around single
enqueues on buffers allocated once; repeats alternate over the meshes and over what is timed; medians with the interquartile range.
  pose / pose_normals   dsn_mesh_pose without and with the covectors: two launches (P x Fb face records, then one thread per vertex)
  stretch               dsn_mesh_stretch of the posed vertices against the bound mesh
  per pose              the same divided by P, beside the byte floor of the vertex pass - 28 B of binding read once per vertex plus
                        12 B (24 B with normals) written per vertex and pose; the face records (64 B x P x Fb) stay in L2 and are
                        not counted - as an implied bandwidth and its fraction of the HBM peak (8.0 TB/s; 6.29 TB/s is what a float4
                        copy reaches)
  extract_mesh          Renderer.extract_mesh(normals=True) of the same body at the same resolution, wall clock around a synchronised
                        call: the only way to get the surface in a second pose without the binding
Writes one JSON document."""
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
import dsnerf_amd  # noqa: E402
from dsnerf_amd import _lib, synth  # noqa: E402
from benchlib.common import load_weights  # noqa: E402

HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29


def stats(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "n": len(v)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--poses", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_pose_bench.json"))
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
    Pmax = max(args.poses)
    targets = T(np.stack([synth.pose_body(canon, seed=7 + k) for k in range(Pmax)]))
    bfaces = T(faces.astype(np.int32))
    Vb, Fb = canon.shape[0], faces.shape[0]
    L, P_ = _lib.lib(), _lib._ptr

    ctx = {}
    for res in args.res:
        r.extract_mesh(batch, res, normals=True)          # warm-up of the extraction path
        extract_ms, mesh = wall(lambda: r.extract_mesh(batch, res, normals=True))
        r.bind_mesh(batch, mesh)
        bind_ms, b = wall(lambda: r.bind_mesh(batch, mesh))
        N, Tn = mesh["verts"].shape[0], mesh["faces"].shape[0]
        c = SimpleNamespace(mesh=mesh, b=b, N=N, T=Tn, extract_ms=extract_ms, bind_ms=bind_ms,
                            out_v=torch.empty(Pmax, N, 3, device=dev), out_n=torch.empty(Pmax, N, 3, device=dev),
                            st=torch.empty(Pmax, Tn, device=dev), status=torch.zeros(1, dtype=torch.int32, device=dev),
                            ws=_lib._scratch(L.dsn_mesh_pose_workspace_bytes(Pmax, Fb), dev))
        ctx[res] = c

    def pose(c, P, normals):
        b = c.b
        assert L.dsn_mesh_pose(P_(targets), P, Vb, P_(bfaces), Fb, P_(b["face_idx"]), P_(b["uv"]), P_(b["h"]), P_(b["cov"]) if normals else None,
                               c.N, P_(c.out_v), P_(c.out_n) if normals else None, P_(c.status), P_(c.ws), _lib._stream()) == 0

    def stretch(c, P):
        assert L.dsn_mesh_stretch(P_(c.mesh["verts"]), P_(c.out_v), P, c.N, P_(c.mesh["faces"]), c.T, P_(c.st), _lib._stream()) == 0

    keys = [(k, P) for P in args.poses for k in ("pose", "pose_normals", "stretch")]
    t = {res: {k: [] for k in keys} for res in args.res}
    for rep in range(args.warmup + args.reps):
        for res in args.res if rep % 2 == 0 else args.res[::-1]:
            c = ctx[res]
            for P in args.poses:
                row = {("pose", P): timed(lambda: pose(c, P, False))[0], ("pose_normals", P): timed(lambda: pose(c, P, True))[0],
                       ("stretch", P): timed(lambda: stretch(c, P))[0]}
                if rep >= args.warmup:
                    for k, v in row.items():
                        t[res][k].append(v)
    out = {}
    for res in args.res:
        c = ctx[res]
        assert int(c.status.cpu()[0]) == 0
        entry = {"verts": c.N, "faces": c.T, "valid_share": round(float(c.b["valid"].float().mean()), 4),
                 "extract_mesh_wall_ms": round(c.extract_ms, 2), "bind_mesh_wall_ms": round(c.bind_ms, 2), "ms": {}}
        for (k, P), v in t[res].items():
            s = stats(v)
            s["per_pose_ms"] = round(s["median_ms"] / P, 4)
            if k != "stretch":
                byts = c.N * (28 + (24 if k == "pose_normals" else 12) * P)
                tbs = byts / (s["median_ms"] * 1e-3) / 1e12
                s.update({"min_bytes": byts, "implied_TBps": round(tbs, 4), "frac_of_hbm_peak": round(tbs / HBM_PEAK_TBS, 4)})
                s["extract_mesh_over_pose"] = round(c.extract_ms / max(s["per_pose_ms"], 1e-6), 1)
            entry["ms"][f"{k}_P{P}"] = s
        out[str(res)] = entry
    doc = {"metric": "mesh_pose", "weights": args.weights, "reps": args.reps, "warmup": args.warmup, "body": {"verts": Vb, "faces": Fb},
           "hbm_peak_TBps": HBM_PEAK_TBS, "hbm_float4_copy_TBps": HBM_COPY_TBS,
           "note": "device times by HIP events around single enqueues (they include the launches: two for dsn_mesh_pose, one for "
                   "dsn_mesh_stretch); min_bytes = N (28 + 12 or 24 per pose), the face records are not counted; extract_mesh and bind_mesh: "
                   "one synchronised whole call each, wall clock, after one warm-up call",
           "by_resolution": out, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
