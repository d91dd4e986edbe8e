#!/usr/bin/env python3
"""Mesh normals, field attributes and the coloured preview on the device: device times on the w4 body's marching-cubes meshes.
    python scripts/bench_mesh_attr.py [--res 256 512] [--size 1024] [--reps 15] [--warmup 3] [--parent-lib FILE] [--out FILE]
Setup: scripts/bench_render_mesh.py's - the w4 weights, the synthetic SMPL-like body posed by synth.pose_body(canon, seed=3), the
density grid and extract_mesh at each resolution, the camera 2.5 in front of the mesh's bounding-box centre, --size x --size pixels.
Per mesh, after warm-up, HIP events around single enqueues; repeats alternate over the meshes and over the variants compared;
medians with the interquartile range.  The floor under every figure is one empty launch: the events around the enqueue of a
one-block kernel (the clear of a 1 x 1 image), stated as empty_launch_ms.
  marching cubes   dsn_mc_count (k_mc_count + the scan), dsn_mc_emit (k_mc_emit) and dsn_mc_normals (k_mc_normals) on the same volume
                   and workspace
  mesh_attributes  dsn_warp / dsn_field (essence and gradient) / dsn_shade on the first min(V, 2^22) vertices (one slab), per call and
                   per vertex, and Renderer.mesh_attributes on the whole mesh; beside them dsn_density_grid's time per grid point
  preview          the flat grey preview (dsn_raster_mesh), the smooth preview, the smooth preview with the albedo as colours, and
                   the unlit painted colour, alternated
  --parent-lib     a libdsnerf_hip.so built from the parent commit: its dsn_raster_mesh on the same buffers, alternated with this
                   tree's in the same run (the flat path must not get slower)
Writes one JSON document."""
import argparse
import ctypes as C
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
from benchlib.common import load_weights  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_attr_bench.json"))
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
    L = _lib.lib()
    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.dsn_raster_mesh.argtypes = L.dsn_raster_mesh.argtypes
        assert not hasattr(parent, "dsn_raster_mesh_attr"), "--parent-lib: that library already has dsn_raster_mesh_attr"
    packed = r.net.packed(dev)
    origin = torch.tensor(r.MESH_VIEW_ORIGIN, device=dev)

    ctx = {}
    for res in args.res:
        axes, vol = r.density_grid(batch, resolution=res)
        t_grid = [timed(lambda: r.density_grid(batch, axes=axes))[0] for _ in range(3)]
        x, y, z = _lib._axes_dev(axes, dev)
        nx, ny, nz = vol.shape
        mcws = _lib._scratch(L.dsn_mc_workspace_bytes(nx, ny, nz), dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        mesh = r.extract_mesh(batch, axes=axes, normals=True, attributes=("albedo", "colour"))
        V, Tn = mesh["verts"].shape[0], mesh["faces"].shape[0]
        lo, hi = mesh["verts"].min(dim=0).values.cpu().numpy(), mesh["verts"].max(dim=0).values.cpu().numpy()
        pose = np.eye(4)
        pose[:3, 3] = 0.5 * (lo + hi) + np.array([0.0, 0.0, 2.5])
        n1 = min(V, 1 << 22)
        v1 = mesh["verts"][:n1].contiguous()
        d1 = (v1 - origin).contiguous()
        c = SimpleNamespace(axes=axes, vol=vol, x=x, y=y, z=z, mcws=mcws, counts=counts, mesh=mesh, V=V, T=Tn, pose=pose, n1=n1, v1=v1, d1=d1,
                            t_grid=t_grid, verts=torch.empty(V, 3, device=dev), faces=torch.empty(Tn, 3, dtype=torch.int32, device=dev),
                            normals=torch.empty(V, 3, device=dev))
        c.flat = _lib.raster_mesh(mesh["verts"], mesh["faces"], camera_pose=pose, height=S, phases=31)
        c.attr = {k: _lib.raster_mesh(mesh["verts"], mesh["faces"], camera_pose=pose, height=S, phases=31, **kw)
                  for k, kw in self_variants(mesh).items()}
        c.cam = _lib.raster_camera(pose, math.pi / 3, S, S)
        c.light = np.array([30.0, math.cos(math.pi / 16), math.cos(math.pi / 6), 0.3], dtype=np.float32)
        c.wsb = L.dsn_raster_workspace_bytes(V, Tn, S, S)
        ctx[res] = c

    def mc(c, which):
        nx, ny, nz = c.vol.shape
        P, st = _lib._ptr, _lib._stream()
        if which == "count":
            return L.dsn_mc_count(P(c.vol), nx, ny, nz, 0.5, P(c.mcws), P(c.counts), st)
        if which == "emit":
            return L.dsn_mc_emit(P(c.vol), nx, ny, nz, P(c.x), P(c.y), P(c.z), 0.5, 1, P(c.mcws), c.V, c.T, P(c.verts), P(c.faces), st)
        return L.dsn_mc_normals(P(c.vol), nx, ny, nz, P(c.x), P(c.y), P(c.z), 0.5, 1, P(c.mcws), c.V, P(c.normals), st)

    def stage(c, which, keep):
        if which == "warp":
            keep["w"] = _lib.warp(r.scene, c.v1, c.d1, 1, want_dir=True, want_active=True)
        elif which == "field":
            w = keep["w"]
            keep["f"] = _lib.field(r.scene, packed, w["x_c"], active=(w["active_list"], w["active_count"]))
        else:
            w, (sg, ess, gr) = keep["w"], keep["f"]
            _lib.shade(r.scene, packed, w["x_c"], gr, c.v1, c.d1, ess, 1, active=(w["active_list"], w["active_count"]))

    def preview(c, which):
        m = c.mesh
        if which == "flat":
            return _lib.raster_mesh(m["verts"], m["faces"], camera_pose=c.pose, height=S, phases=31, out=c.flat)
        return _lib.raster_mesh(m["verts"], m["faces"], camera_pose=c.pose, height=S, phases=31, out=c.attr[which], **self_variants(m)[which])

    def flat_raw(c, lib):
        m, P = c.mesh, _lib._ptr
        pose, fx, fy = c.cam
        rc = lib.dsn_raster_mesh(P(m["verts"]), c.V, P(m["faces"]), c.T, pose.ctypes.data, fx, fy, 0.05, c.light.ctypes.data, S, S,
                                 P(c.flat["face"]), P(c.flat["depth"]), P(c.flat["color"]), P(c.flat["_ws"]), c.wsb, _lib._stream())
        assert rc == 0

    tiny = _lib.raster_mesh(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), height=1, phases=_lib.RM_CLEAR)
    empty = lambda: _lib.raster_mesh(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), height=1,
                                     phases=_lib.RM_CLEAR, out=tiny)
    variants = ["flat"] + list(self_variants(ctx[args.res[0]].mesh))
    keys = ["mc_count", "mc_emit", "mc_normals", "warp", "field", "shade", "mesh_attributes"] + ["preview_" + v for v in variants]
    keys += ["flat_this_tree", "flat_parent"] if parent else []
    t = {res: {k: [] for k in keys} for res in args.res}
    floor = []
    for rep in range(args.warmup + args.reps):
        rec = rep >= args.warmup
        for res in args.res:
            c, keep, row = ctx[res], {}, {}
            for which in ("count", "emit", "normals"):
                row["mc_" + which] = timed(lambda: mc(c, which))[0]
            for which in ("warp", "field", "shade"):
                row[which] = timed(lambda: stage(c, which, keep))[0]
            if rep < args.warmup + 3:
                row["mesh_attributes"] = timed(lambda: r.mesh_attributes(batch, c.mesh["verts"]))[0]
            for v in variants:
                row["preview_" + v] = timed(lambda: preview(c, v))[0]
            if parent:
                for name, lib in (("flat_this_tree", L), ("flat_parent", parent)) if rep % 2 == 0 else (("flat_parent", parent), ("flat_this_tree", L)):
                    row[name] = timed(lambda: flat_raw(c, lib))[0]
            if rec:
                for k, v in row.items():
                    t[res][k].append(v)
        if rec:
            floor.append(timed(empty)[0])
    out = {}
    for res in args.res:
        c = ctx[res]
        rows = {k: stats(v) for k, v in t[res].items() if v}
        for k in ("warp", "field", "shade"):
            rows[k]["ns_per_vertex"] = round(rows[k]["median_ms"] * 1e6 / c.n1, 3)
        rows["mesh_attributes"]["ns_per_vertex"] = round(rows["mesh_attributes"]["median_ms"] * 1e6 / c.V, 3)
        for k in ("mc_count", "mc_emit", "mc_normals"):
            rows[k]["ns_per_grid_point"] = round(rows[k]["median_ms"] * 1e6 / c.vol.numel(), 4)
        rows["mc_normals"]["ns_per_vertex"] = round(rows["mc_normals"]["median_ms"] * 1e6 / c.V, 3)
        g = stats(c.t_grid)
        g["ns_per_grid_point"] = round(g["median_ms"] * 1e6 / c.vol.numel(), 3)
        rows["density_grid"] = g
        # the outputs are the same whichever way they were made
        chk = _lib.marching_cubes(c.vol, c.axes, 0.5, "ascent", want_normals=True)
        assert torch.equal(chk[2], c.normals) and torch.equal(chk[0], c.verts) and torch.equal(c.mesh["normals"], c.normals)
        out[str(res)] = {"grid": list(c.vol.shape), "verts": c.V, "faces": c.T, "stage_vertices": c.n1, "image": [S, S],
                         "covered_pixels": int((preview(c, "flat")["face"] >= 0).sum()), "ms": rows}
    doc = {"metric": "mesh_attr", "weights": args.weights, "reps": args.reps, "warmup": args.warmup, "image": [S, S],
           "empty_launch_ms": stats(floor),
           "note": "times by HIP events around single enqueues (they include the launch: empty_launch_ms is the floor); mesh_attributes "
                   "is the host composition, its own allocations and per-slab copies included; the stage calls allocate their outputs "
                   "inside the timed region as mesh_attributes does",
           "parent_library_compared": bool(parent), "by_resolution": out, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


def self_variants(mesh):
    """the attribute previews compared with the flat one: keyword arguments of _lib.raster_mesh"""
    return {"smooth": dict(vertex_normals=mesh["normals"], smooth=True),
            "smooth_albedo": dict(vertex_normals=mesh["normals"], vertex_colors=mesh["albedo"], smooth=True),
            "unlit_colour": dict(vertex_normals=mesh["normals"], vertex_colors=mesh["colour"], smooth=True, lit=False)}


if __name__ == "__main__":
    main()
