#!/usr/bin/env python3
"""Simplifying an extracted mesh on the device (vertex clustering, dsn_mesh_simplify_*): device times on the w4 body's marching-cubes meshes.
    python scripts/bench_mesh_simplify.py [--res 256 512] [--targets 50000 200000] [--reps 15] [--warmup 3] [--no-host]
                                          [--parent-lib FILE] [--rounds 3] [--out FILE]
Setup: scripts/bench_mesh_cc.py's - the w4 weights, the synthetic SMPL-like body posed by synth.pose_body(canon, seed=3), the density
grid and extract_mesh at each resolution.  Per mesh and target vertex count the cell comes from _lib.mesh_target_search; then, after
warm-up, HIP events around single enqueues on one workspace; repeats alternate over the cases; medians with the interquartile range.
  count / emit      dsn_mesh_simplify_count and dsn_mesh_simplify_emit, every kernel of each
  kernels           the phases of dsn_mesh_simplify_count_ex / dsn_mesh_simplify_emit_ex one by one, in order, on the same workspace
                    (zero, mark, rank, sum, pick, faces, keep + scan, emit vertices, emit faces)
  cells             dsn_mesh_simplify_cells: what one probe of the target search enqueues
  whole call        _lib.mesh_simplify with a given cell: the bounding-box reduction, both phases, the device->host reads, the allocations
  target search     _lib.mesh_target_search: 12 probes, each with its allocation and its 8-byte read
Two yardsticks from the same run: byte_floor_ms, one read of verts plus two reads of faces over the HBM peak (8 TB/s), and host, the
numpy restatement of the rule (tests/mesh_simplify_restate.py) on the same mesh, wall clock; the device result is checked against it.
extract_mesh: the time of Renderer.extract_mesh (keywords off) with this build and, with --parent-lib, with another build of the library
(the parent commit's), each in `rounds` fresh processes that alternate; the spread between processes of one build is recorded beside
the difference between the builds.  Writes one JSON document."""
import argparse
import json
import os
import subprocess
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

PHASES = [("zero", _lib.SP_ZERO), ("mark", _lib.SP_MARK), ("rank", _lib.SP_RANK), ("sum", _lib.SP_SUM), ("pick", _lib.SP_PICK),
          ("faces", _lib.SP_FACES), ("keep_scan", _lib.SP_KEEP), ("emit_verts", _lib.SP_EMIT_VERTS), ("emit_faces", _lib.SP_EMIT_FACES)]
COUNT_PHASES = 127
HBM_PEAK = 8.0e12


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


def scene(weights, dev):
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon, seed=3)
    cfg = SimpleNamespace(DATASETS=SimpleNamespace(SMPL_PATH="<synthetic>"),
                          MODEL=SimpleNamespace(sample_points_mode="GG", COARSE_RAY_SAMPLING=64, perturb=1.0, raw_noise_std=1.0, TYPE="nerf",
                                                FINE_RAY_SAMPLING=-1))
    net = dsnerf_amd.DualSpaceNeRF(cfg)
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in load_weights(synth, weights).items()})
    net.to(dev)
    r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
    r.eval()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    batch = {"xyz": T(xyz)[None], "poses": T(synth.make_poses(seed=5))[None], "Th": torch.zeros(1, 1, 3, device=dev),
             "frame": torch.tensor([5])}
    return r, batch


def extract_only(args):
    """child process: extract_mesh times of the library DSNERF_LIB names (or the tree's), one JSON line"""
    if os.environ.get("DSNERF_LIB"):
        # a build from before dsn_mesh_simplify_*: the binding sets their prototypes when it loads the library; extract_mesh with the
        # keywords off calls none of them
        import ctypes

        class Older(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if name.startswith("dsn_mesh_simplify"):
                        return SimpleNamespace()
                    raise
        ctypes.CDLL = Older
    dev = torch.device("cuda:0")
    r, batch = scene(args.weights, dev)
    out = {}
    for res in args.res:
        ts = []
        for rep in range(args.warmup + args.reps):
            ms, mesh = timed(lambda: r.extract_mesh(batch, res))
            if rep >= args.warmup:
                ts.append(ms)
        out[str(res)] = dict(stats(ts), verts=int(mesh["verts"].shape[0]), faces=int(mesh["faces"].shape[0]))
    print("EXTRACT " + json.dumps(out))


def extract_compare(args):
    """extract_mesh with this build and the parent's, in fresh processes that alternate"""
    builds = [("this", None)] + ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else [])
    runs = {name: [] for name, _ in builds}
    for rnd in range(args.rounds):
        for name, lib in builds if rnd % 2 == 0 else builds[::-1]:
            env = dict(os.environ)
            env.pop("DSNERF_LIB", None)
            if lib:
                env["DSNERF_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--extract-only", "--weights", args.weights, "--reps", str(max(args.reps // 3, 3)),
                   "--warmup", "2", "--res"] + [str(x) for x in args.res]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise RuntimeError(f"extract_mesh child ({name}) failed:\n{p.stderr[-2000:]}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("EXTRACT ")][-1]
            runs[name].append(json.loads(line[len("EXTRACT "):]))
            print(f"extract_mesh, {name} build, process {rnd + 1} of {args.rounds}: {line}", file=sys.stderr, flush=True)
    out = {}
    for res in args.res:
        row = {}
        for name, _ in builds:
            med = [x[str(res)]["median_ms"] for x in runs[name]]
            row[name] = {"process_medians_ms": med, "median_ms": round(float(np.median(med)), 4), "spread_ms": round(float(max(med) - min(med)), 4),
                         "verts": runs[name][0][str(res)]["verts"], "faces": runs[name][0][str(res)]["faces"]}
        if "parent" in row:
            row["this_minus_parent_ms"] = round(row["this"]["median_ms"] - row["parent"]["median_ms"], 4)
            row["within_spread"] = bool(abs(row["this_minus_parent_ms"]) <= max(row["this"]["spread_ms"], row["parent"]["spread_ms"]))
            assert (row["this"]["verts"], row["this"]["faces"]) == (row["parent"]["verts"], row["parent"]["faces"])
        out[str(res)] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--targets", type=int, nargs="+", default=[50000, 200000])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libdsnerf_hip.so of the parent commit: extract_mesh is timed with both builds")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--extract-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify_bench.json"))
    args = ap.parse_args()
    if args.extract_only:
        return extract_only(args)
    extract = extract_compare(args)          # (children first: this process has not opened the GPU yet)
    dev = torch.device("cuda:0")
    r, batch = scene(args.weights, dev)
    L, P = _lib.lib(), _lib._ptr

    ctx = {}
    for res in args.res:
        mesh = r.extract_mesh(batch, res)
        verts, fcs = mesh["verts"], mesh["faces"]
        V, Tn = verts.shape[0], fcs.shape[0]
        box = _lib._finite_box(verts)
        for target in args.targets:
            info = {}
            cell = _lib.mesh_target_search(verts, target, info=info)
            origin, g = _lib.mesh_simplify_grid(box, cell)
            cf, g3 = _lib._mesh_simplify_check_grid(cell, origin, g)
            nbytes = L.dsn_mesh_simplify_workspace_bytes(V, Tn, g3)
            c = SimpleNamespace(verts=verts, faces=fcs, V=V, T=Tn, cell=cf, origin=origin, g=g, g3=g3, n=info["n"], nbytes=nbytes,
                                ws=_lib._scratch(nbytes, dev), counts=torch.empty(7, dtype=torch.int64, device=dev),
                                vc=torch.empty(V, dtype=torch.int32, device=dev), outK=torch.empty(1, dtype=torch.int64, device=dev))
            assert L.dsn_mesh_simplify_count(P(verts), P(fcs), V, Tn, origin.ctypes.data, cf, g3, P(c.ws), nbytes, P(c.vc), P(c.counts),
                                             _lib._stream()) == 0, L.dsn_last_error()
            c.k = [int(x) for x in c.counts.cpu()]
            assert c.k[6] == 0 and c.k[0] <= target
            c.ov = torch.empty(c.k[0], 3, device=dev)
            c.of = torch.empty(c.k[1], 3, dtype=torch.int32, device=dev)
            c.src = torch.empty(c.k[0], dtype=torch.int32, device=dev)
            ctx[(res, target)] = c
            print(f"res {res} target {target}: V {V} T {Tn} n {c.n} g {g} counts {c.k}", file=sys.stderr, flush=True)

    def count(c, phases=0):
        assert L.dsn_mesh_simplify_count_ex(P(c.verts), P(c.faces), c.V, c.T, c.origin.ctypes.data, c.cell, c.g3, P(c.ws), c.nbytes, P(c.vc),
                                            P(c.counts), phases, _lib._stream()) == 0

    def emit(c, phases=0):
        assert L.dsn_mesh_simplify_emit_ex(P(c.verts), P(c.faces), c.V, c.T, c.g3, P(c.ws), c.nbytes, c.k[0], c.k[1], P(c.ov), P(c.of), P(c.src),
                                           phases, _lib._stream()) == 0

    def cells(c):
        assert L.dsn_mesh_simplify_cells(P(c.verts), c.V, c.origin.ctypes.data, c.cell, c.g3, P(c.ws), c.nbytes, P(c.outK), _lib._stream()) == 0

    keys = ["count", "emit", "cells", "whole_call", "target_search"] + [k for k, _ in PHASES]
    cases = list(ctx)
    t = {case: {k: [] for k in keys} for case in cases}
    for rep in range(args.warmup + args.reps):
        for case in cases if rep % 2 == 0 else cases[::-1]:
            c, row = ctx[case], {}
            row["cells"] = timed(lambda: cells(c))[0]          # (before the phases: it writes the head of the same workspace)
            row["count"] = timed(lambda: count(c))[0]
            row["emit"] = timed(lambda: emit(c))[0]
            for name, bit in PHASES:          # in order, on the workspace the phases before left
                row[name] = timed((lambda: count(c, bit)) if bit & COUNT_PHASES else (lambda: emit(c, bit)))[0]
            row["whole_call"] = timed(lambda: _lib.mesh_simplify(c.verts, c.faces, c.cell))[0]
            row["target_search"] = timed(lambda: _lib.mesh_target_search(c.verts, case[1]))[0]
            if rep >= args.warmup:
                for k, v in row.items():
                    t[case][k].append(v)
    out = {}
    for case in cases:
        res, target = case
        c = ctx[case]
        rows = {k: stats(v) for k, v in t[case].items()}
        rows["kernels_sum"] = {"median_ms": round(sum(rows[k]["median_ms"] for k, _ in PHASES), 4)}
        floor_ms = (12.0 * c.V + 2 * 12.0 * c.T) / HBM_PEAK * 1e3
        entry = {"verts": c.V, "faces": c.T, "target_vertices": target, "n": c.n, "cell": c.cell, "g": c.g, "out_verts": c.k[0], "out_faces": c.k[1],
                 "live_faces": c.k[2], "duplicates_dropped": c.k[3], "workspace_bytes": c.nbytes, "byte_floor_ms": round(floor_ms, 4),
                 "count_plus_emit_over_floor": round((rows["count"]["median_ms"] + rows["emit"]["median_ms"]) / floor_ms, 1), "ms": rows}
        # the phases one by one left the same result as the whole call
        ov, of, src, vc = _lib.mesh_simplify(c.verts, c.faces, c.cell)
        assert torch.equal(ov.view(torch.int32), c.ov.view(torch.int32)) and torch.equal(of, c.of) and torch.equal(src, c.src) and torch.equal(vc, c.vc)
        if not args.no_host:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import mesh_simplify_restate as R
            t0 = time.perf_counter()
            hv, hf = c.verts.cpu().numpy(), c.faces.cpu().numpy()
            t1 = time.perf_counter()
            want = R.simplify(hv, hf, np.float32(c.cell), c.origin, c.g)
            t2 = time.perf_counter()
            assert want["counts"].tolist() == c.k and np.array_equal(want["cluster_source"], c.src.cpu().numpy())
            assert np.array_equal(want["faces"], c.of.cpu().numpy()) and np.array_equal(want["vertex_cluster"], c.vc.cpu().numpy())
            print(f"host restatement {case}: {(t2 - t1) * 1e3:.0f} ms", file=sys.stderr, flush=True)
            entry["host"] = {"copy_to_host_ms": round((t1 - t0) * 1e3, 2), "numpy_ms": round((t2 - t1) * 1e3, 2), "threads": torch.get_num_threads()}
        out[f"{res}/{target}"] = entry
    doc = {"metric": "mesh_simplify", "weights": args.weights, "reps": args.reps, "warmup": args.warmup, "hbm_peak_bytes_per_s": HBM_PEAK,
           "note": "times by HIP events around single enqueues (they include the launches: count = 10, emit = 2, cells = 5); byte_floor_ms = "
                   "(12 V + 24 T) bytes over the HBM peak; whole_call is _lib.mesh_simplify with its allocations, its bounding-box reduction "
                   "and its two device->host reads; target_search is 12 probes; host: one run, wall clock, the numpy restatement; "
                   "extract_mesh: medians of fresh processes that alternate between the builds, spread = max - min over a build's processes",
           "by_resolution_and_target": out, "extract_mesh": extract, "parent_lib": bool(args.parent_lib),
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
