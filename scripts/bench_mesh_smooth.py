#!/usr/bin/env python3
"""Smoothing an extracted mesh on the device (dsn_mesh_smooth) and normals from its faces (dsn_mesh_vertex_normals): device times on the
w4 body's marching-cubes meshes.
    python scripts/bench_mesh_smooth.py [--res 256 512] [--reps 15] [--warmup 3] [--out FILE]
Setup: scripts/bench_mesh_simplify.py's - the w4 weights, the synthetic SMPL-like body posed by synth.pose_body(canon, seed=3), the density
grid and extract_mesh at each resolution.  After warm-up, HIP events around single enqueues on one workspace; repeats alternate over the
cases; medians with the interquartile range.
  lists             the vertex -> corner lists: zero, count, rank + scan, fill (DSN_SM_COUNT | DSN_SM_SCAN | DSN_SM_FILL)
  step              one umbrella step on lists that are there (DSN_SM_STEP, one factor)
  ten_pairs_steps   twenty steps (ten Taubin pairs) on lists that are there
  ten_pairs_call    dsn_mesh_smooth whole: lists and twenty steps
  normals_kernel    the normals' gather on lists that are there (DSN_SM_NORMALS)
  normals_call      dsn_mesh_vertex_normals whole: lists and the gather
  whole_smooth_mesh _lib.mesh_smooth with its bounding-box reduction, its allocations and the read of the counts
  whole_vertex_normals  _lib.mesh_vertex_normals with its bounding-box reduction (six floats read for the shift) and its allocations
Two yardsticks from the same run.  step_byte_floor_ms: what one step must move over the HBM peak (8 TB/s) - the positions read and written
once, the row lengths and offsets, the entries: (12 + 12 + 12) V + 24 T bytes; the neighbours' positions are counted as cache hits.
torch: the obvious formulation on the same GPU - float32, the six directed index pairs of every face built once (torch_lists), then per
step acc.index_add_(0, i, x[j]) and x + f (acc / n - x) (torch_step; torch_ten_pairs: twenty of them).  Its sums are float atomics: the
result depends on the arrival order, and its largest difference from the device rule's is recorded, not asserted.  Writes one JSON
document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from dsnerf_amd import _lib  # noqa: E402
from bench_mesh_simplify import scene, stats, timed  # noqa: E402

HBM_PEAK = 8.0e12
LISTS = _lib.SM_COUNT | _lib.SM_SCAN | _lib.SM_FILL
PAIRS = [0.5, -0.53] * 10


def torch_lists(faces, V):
    f = faces.long()
    i = torch.cat([f[:, 0], f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2]])
    j = torch.cat([f[:, 1], f[:, 2], f[:, 2], f[:, 0], f[:, 0], f[:, 1]])
    n = torch.zeros(V, device=faces.device).index_add_(0, i, torch.ones(i.shape[0], device=faces.device))
    return i, j, n.clamp_(min=1.0)[:, None]


def torch_steps(x, lists, factors):
    i, j, n = lists
    for f in factors:
        acc = torch.zeros_like(x).index_add_(0, i, x[j])
        x = x + f * (acc / n - x)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    r, batch = scene(args.weights, dev)
    ctx = {}
    for res in args.res:
        mesh = r.extract_mesh(batch, res)
        verts, faces = mesh["verts"], mesh["faces"]
        V, T = verts.shape[0], faces.shape[0]
        origin, k = _lib.mesh_smooth_scale(_lib._finite_box(verts))
        nbytes = _lib.lib().dsn_mesh_smooth_workspace_bytes(V, T)
        state = {"ws": _lib._scratch(nbytes, dev), "counts": torch.empty(4, dtype=torch.int64, device=dev),
                 "out": torch.empty(V, 3, dtype=torch.float32, device=dev)}
        ctx[res] = dict(verts=verts, faces=faces, V=V, T=T, origin=origin, k=k, nbytes=nbytes, state=state,
                        shift=_lib._mesh_cc_inputs(verts, faces)[4],
                        nstate={"ws": state["ws"], "out": torch.empty(V, 3, dtype=torch.float32, device=dev)})
        print(f"res {res}: V {V} T {T} k {k} workspace {nbytes} bytes", file=sys.stderr, flush=True)

    def smooth(c, factors, phases=0):
        return _lib.mesh_smooth(c["verts"], c["faces"], factors, origin=c["origin"], scale_exp=c["k"], phases=phases, state=c["state"])

    def normals(c, phases=0):          # (the library call alone: _lib.mesh_vertex_normals reduces the bounding box for the shift first)
        st = c["nstate"]
        _lib._check(_lib.lib().dsn_mesh_vertex_normals_ex(_lib._ptr(c["verts"]), _lib._ptr(c["faces"]), c["V"], c["T"], c["shift"], _lib._ptr(st["ws"]),
                                                          c["nbytes"], _lib._ptr(st["out"]), phases, _lib._stream()), "dsn_mesh_vertex_normals")
        return st["out"]

    keys = ["lists", "step", "ten_pairs_steps", "ten_pairs_call", "normals_kernel", "normals_call", "whole_smooth_mesh", "whole_vertex_normals",
            "torch_lists",
            "torch_step", "torch_ten_pairs"]
    cases = list(ctx)
    t = {case: {kk: [] for kk in keys} for case in cases}
    for rep in range(args.warmup + args.reps):
        for case in cases if rep % 2 == 0 else cases[::-1]:
            c, row = ctx[case], {}
            row["lists"] = timed(lambda: smooth(c, [], LISTS))[0]
            row["step"] = timed(lambda: smooth(c, [0.5], _lib.SM_STEP))[0]
            row["ten_pairs_steps"] = timed(lambda: smooth(c, PAIRS, _lib.SM_STEP))[0]
            row["ten_pairs_call"] = timed(lambda: smooth(c, PAIRS))[0]
            row["normals_call"] = timed(lambda: normals(c))[0]
            row["normals_kernel"] = timed(lambda: normals(c, _lib.SM_NORMALS))[0]
            row["whole_smooth_mesh"] = timed(lambda: _lib.mesh_smooth(c["verts"], c["faces"], PAIRS, info={}))[0]
            row["whole_vertex_normals"], wn = timed(lambda: _lib.mesh_vertex_normals(c["verts"], c["faces"]))
            assert torch.equal(wn.view(torch.int32), c["nstate"]["out"].view(torch.int32))
            row["torch_lists"], lists = timed(lambda: torch_lists(c["faces"], c["V"]))
            row["torch_step"] = timed(lambda: torch_steps(c["verts"], lists, [0.5]))[0]
            row["torch_ten_pairs"], c["torch_out"] = timed(lambda: torch_steps(c["verts"], lists, PAIRS))
            del lists
            if rep >= args.warmup:
                for kk, v in row.items():
                    t[case][kk].append(v)
    out = {}
    for res in cases:
        c = ctx[res]
        rows = {kk: stats(v) for kk, v in t[res].items()}
        floor_ms = (36.0 * c["V"] + 24.0 * c["T"]) / HBM_PEAK * 1e3
        info = {}
        whole = _lib.mesh_smooth(c["verts"], c["faces"], PAIRS, info=info).clone()
        by_phase = smooth(c, PAIRS, _lib.SM_STEP)          # (on the lists the last whole call of the loop left)
        assert torch.equal(whole.view(torch.int32), by_phase.view(torch.int32))
        diff = float((whole - c["torch_out"]).abs().max())
        out[str(res)] = {"verts": c["V"], "faces": c["T"], "scale_exp": c["k"], "workspace_bytes": c["nbytes"],
                         "counts": {n: info[n] for n in _lib.MESH_SMOOTH_COUNTS}, "step_byte_floor_ms": round(floor_ms, 4),
                         "step_over_floor": round(rows["step"]["median_ms"] / floor_ms, 1),
                         "torch_step_over_step": round(rows["torch_step"]["median_ms"] / rows["step"]["median_ms"], 2),
                         "torch_ten_pairs_over_ten_pairs_call": round(rows["torch_ten_pairs"]["median_ms"] / rows["ten_pairs_call"]["median_ms"], 2),
                         "max_abs_difference_from_torch_float32": diff, "ms": rows}
    doc = {"metric": "mesh_smooth", "weights": args.weights, "reps": args.reps, "warmup": args.warmup, "hbm_peak_bytes_per_s": HBM_PEAK,
           "factors": PAIRS,
           "note": "times by HIP events around single enqueues (they include the launches: lists = 6, a step = 1, normals = 1); "
                   "step_byte_floor_ms = (36 V + 24 T) bytes over the HBM peak, neighbour positions counted as cache hits; whole_smooth_mesh "
                   "is _lib.mesh_smooth with its bounding-box reduction, its allocations and the read of the counts, whole_vertex_normals "
                   "_lib.mesh_vertex_normals with its bounding-box reduction and its allocations; torch_*: float32 "
                   "index_add_ on the same GPU in the same run, lists = the six directed index pairs per face and the valences",
           "by_resolution": out, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
