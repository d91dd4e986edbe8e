#!/usr/bin/env python3
"""The largest connected component of an extracted mesh on the device: device times on the w4 body's marching-cubes meshes.
    python scripts/bench_mesh_cc.py [--res 256 512] [--reps 15] [--warmup 3] [--no-host] [--out FILE]
Setup: scripts/bench_mesh_attr.py's - the w4 weights, the synthetic SMPL-like body posed by synth.pose_body(canon, seed=3), the density
grid and extract_mesh at each resolution.  Per mesh, after warm-up, HIP events around single enqueues on one workspace; repeats
alternate over the meshes and over what is timed; medians with the interquartile range.  The floor under every figure is one empty
launch (empty_launch_ms: dsn_mesh_cc_label on a mesh without vertices and faces, select phase only - one one-block kernel).
  label / emit      dsn_mesh_cc_label and dsn_mesh_cc_emit, every kernel of each
  kernels           the phases of dsn_mesh_cc_label_ex / dsn_mesh_cc_emit_ex one by one, in order, on the same workspace
                    (init, unite, flatten, sums, select, count + scan, emit vertices, emit faces)
  whole call        _lib.largest_component: the bounding-box reduction, both phases, the device->host reads and the allocations
  marching cubes    dsn_mc_count + dsn_mc_emit on the same volume, for scale
  host              the numpy / scipy restatement of the same rule on the same mesh (scipy.sparse.csgraph.connected_components over the
                    faces' edges, float32 areas, a bincount), wall clock, the device->host copy of the mesh stated apart
The device result is checked against the host's: the same labels, the same kept vertices and faces.  Writes one JSON document."""
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

PHASES = [("init", _lib.CC_INIT), ("unite", _lib.CC_UNITE), ("flatten", _lib.CC_FLATTEN), ("sums", _lib.CC_SUMS), ("select", _lib.CC_SELECT),
          ("count_scan", _lib.CC_COUNT), ("emit_verts", _lib.CC_EMIT_VERTS), ("emit_faces", _lib.CC_EMIT_FACES)]
LABEL_PHASES = 63


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


def host_largest(verts, faces):
    """the rule on the host with scipy: labels (smallest index of the component, -1 unused), kept vertex and face masks"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    V = verts.shape[0]
    f = faces.astype(np.int64)
    ok = ((f >= 0) & (f < V)).all(axis=1)
    fv = f[ok]
    g = coo_matrix((np.ones(2 * fv.shape[0], np.int8), (np.concatenate([fv[:, 0], fv[:, 0]]), np.concatenate([fv[:, 1], fv[:, 2]]))), shape=(V, V))
    comp = connected_components(g, directed=False)[1]
    first = np.full(comp.max() + 1, V, np.int64)
    np.minimum.at(first, comp, np.arange(V))
    used = np.zeros(V, bool)
    used[fv.reshape(-1)] = True
    lab = np.where(used, first[comp], -1)
    a, b, c = verts[fv[:, 0]], verts[fv[:, 1]], verts[fv[:, 2]]
    e1, e2 = b - a, c - a
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    d = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    area = np.bincount(lab[fv[:, 0]], weights=np.where(np.isfinite(d), d, 0).astype(np.float64), minlength=V)
    winner = int(np.argmax(area))
    keep_f = ok.copy()
    keep_f[ok] = lab[fv[:, 0]] == winner
    return lab.astype(np.int32), lab == winner, keep_f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_cc_bench.json"))
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
    L, P = _lib.lib(), _lib._ptr

    ctx = {}
    for res in args.res:
        axes, vol = r.density_grid(batch, resolution=res)
        x, y, z = _lib._axes_dev(axes, dev)
        nx, ny, nz = vol.shape
        verts, fcs = _lib.marching_cubes(vol, axes, 0.5, "ascent")
        V, Tn = verts.shape[0], fcs.shape[0]
        _, _, _, _, shift = _lib._mesh_cc_inputs(verts, fcs)
        nbytes = L.dsn_mesh_cc_workspace_bytes(V, Tn)
        c = SimpleNamespace(axes=axes, vol=vol, x=x, y=y, z=z, verts=verts, faces=fcs, V=V, T=Tn, shift=shift, nbytes=nbytes,
                            ws=_lib._scratch(nbytes, dev), counts=torch.empty(6, dtype=torch.int64, device=dev),
                            labels=torch.empty(V, dtype=torch.int32, device=dev),
                            mcws=_lib._scratch(L.dsn_mc_workspace_bytes(nx, ny, nz), dev), mccounts=torch.empty(2, dtype=torch.int64, device=dev),
                            mcv=torch.empty(V, 3, device=dev), mcf=torch.empty(Tn, 3, dtype=torch.int32, device=dev))
        assert L.dsn_mesh_cc_label(P(verts), P(fcs), V, Tn, shift, P(c.ws), nbytes, P(c.labels), P(c.counts), _lib._stream()) == 0
        c.n = [int(k) for k in c.counts.cpu()]
        c.ov = torch.empty(c.n[2], 3, device=dev)
        c.of = torch.empty(c.n[3], 3, dtype=torch.int32, device=dev)
        c.src = torch.empty(c.n[2], dtype=torch.int32, device=dev)
        ctx[res] = c

    def label(c, phases=0):
        assert L.dsn_mesh_cc_label_ex(P(c.verts), P(c.faces), c.V, c.T, c.shift, P(c.ws), c.nbytes, P(c.labels), P(c.counts), phases,
                                      _lib._stream()) == 0

    def emit(c, phases=0):
        assert L.dsn_mesh_cc_emit_ex(P(c.verts), P(c.faces), c.V, c.T, P(c.ws), c.nbytes, c.n[2], c.n[3], P(c.ov), P(c.of), P(c.src), phases,
                                     _lib._stream()) == 0

    def mc(c):
        nx, ny, nz = c.vol.shape
        st = _lib._stream()
        assert L.dsn_mc_count(P(c.vol), nx, ny, nz, 0.5, P(c.mcws), P(c.mccounts), st) == 0
        assert L.dsn_mc_emit(P(c.vol), nx, ny, nz, P(c.x), P(c.y), P(c.z), 0.5, 1, P(c.mcws), c.V, c.T, P(c.mcv), P(c.mcf), st) == 0

    tiny_ws = _lib._scratch(L.dsn_mesh_cc_workspace_bytes(0, 0), dev)
    tiny_counts = torch.empty(6, dtype=torch.int64, device=dev)
    empty = lambda: L.dsn_mesh_cc_label_ex(None, None, 0, 0, 0, P(tiny_ws), tiny_ws.numel(), None, P(tiny_counts), _lib.CC_SELECT, _lib._stream())
    keys = ["label", "emit", "whole_call", "marching_cubes"] + [k for k, _ in PHASES]
    t = {res: {k: [] for k in keys} for res in args.res}
    floor = []
    for rep in range(args.warmup + args.reps):
        rec = rep >= args.warmup
        for res in args.res if rep % 2 == 0 else args.res[::-1]:
            c, row = ctx[res], {}
            row["label"] = timed(lambda: label(c))[0]
            row["emit"] = timed(lambda: emit(c))[0]
            for name, bit in PHASES:          # in order, on the workspace the phases before left
                row[name] = timed((lambda: label(c, bit)) if bit & LABEL_PHASES else (lambda: emit(c, bit)))[0]
            row["marching_cubes"] = timed(lambda: mc(c))[0]
            row["whole_call"] = timed(lambda: _lib.largest_component(c.verts, c.faces))[0]
            if rec:
                for k, v in row.items():
                    t[res][k].append(v)
        if rec:
            floor.append(timed(empty)[0])
    out = {}
    for res in args.res:
        c = ctx[res]
        rows = {k: stats(v) for k, v in t[res].items()}
        for k in ("label", "emit", "unite", "sums"):
            rows[k]["ns_per_face"] = round(rows[k]["median_ms"] * 1e6 / max(c.T, 1), 4)
        rows["kernels_sum"] = {"median_ms": round(sum(rows[k]["median_ms"] for k, _ in PHASES), 4)}
        entry = {"grid": list(c.vol.shape), "verts": c.V, "faces": c.T, "area_shift": c.shift, "components": c.n[0], "winner": c.n[1],
                 "kept_verts": c.n[2], "kept_faces": c.n[3], "workspace_bytes": c.nbytes, "ms": rows}
        # the phases one by one left the same result as the whole calls
        ov, of, src = _lib.largest_component(c.verts, c.faces)
        assert torch.equal(ov, c.ov) and torch.equal(of, c.of) and torch.equal(src, c.src)
        if not args.no_host:
            t0 = time.perf_counter()
            hv, hf = c.verts.cpu().numpy(), c.faces.cpu().numpy()
            t1 = time.perf_counter()
            lab, keep_v, keep_f = host_largest(hv, hf)
            t2 = time.perf_counter()
            assert np.array_equal(lab, c.labels.cpu().numpy())
            assert np.array_equal(np.flatnonzero(keep_v), c.src.cpu().numpy()) and int(keep_f.sum()) == c.n[3]
            entry["host"] = {"copy_to_host_ms": round((t1 - t0) * 1e3, 2), "scipy_ms": round((t2 - t1) * 1e3, 2),
                             "threads": torch.get_num_threads()}
        out[str(res)] = entry
    doc = {"metric": "mesh_cc", "weights": args.weights, "reps": args.reps, "warmup": args.warmup, "empty_launch_ms": stats(floor),
           "note": "times by HIP events around single enqueues (they include the launches: empty_launch_ms is the floor of one); label = 8 "
                   "launches, emit = 2; whole_call is _lib.largest_component with its allocations, its bounding-box reduction and its two "
                   "device->host reads; host: one run, wall clock, scipy.sparse.csgraph on the faces' edges plus numpy areas",
           "by_resolution": out, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
