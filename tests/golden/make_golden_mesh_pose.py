"""Golden vectors for the bound-mesh rule (dsn_mesh_pose, include/dsnerf.h) from the reference's own functions:
utils/geo_utils.py:181-200 project_point2mesh (the binding: uv, h of a point in the frame of its nearest posed face) and :138-156
barycentric_map2can (the record evaluated on another mesh), in torch float32 and float64.  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mesh_pose.py

Three bodies (synth.make_body: lattice and SMPL-like tessellation; make_small_body), each in two poses (synth.pose_body seeds 3 and 7,
different translations); points on the posed surface and 3 cm to either side of it, and a share pushed out until the reference's mask
(utils/render_utils.py:103-109) calls them transparent; the nearest face by centroid, brute force.  The fixture holds, per point, the
three vertices of its face in the source pose, the other pose and the canonical pose, the point, a unit normal, (uv, h, transparent)
and the reference's float32 outputs on the other pose and on the canonical mesh.  mesh_pose_spread.json: the largest float32 - float64
differences of tests/mesh_pose_restate.py's positions and normals on these inputs, which tests/test_mesh_pose_host.py recomputes.
Data only.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
spec = importlib.util.spec_from_file_location("synth", os.path.join(ROOT, "dual-space-nerf_amd", "synth.py"))
synth = importlib.util.module_from_spec(spec)
spec.loader.exec_module(synth)
import ref_harness as rh  # noqa: E402
import mesh_pose_restate as MP  # noqa: E402

CASES = (("lattice", 700, 401), ("smpl_like", 900, 411), ("small", 400, 421))


def spread(c):
    """what mesh_pose_spread.json records for one case of the fixture (c: a dict of its arrays, keys without the case prefix): the largest
    |float32 - float64| of the restatement's positions (on the other pose; also in units of 2^-24 (|m0| + |u||v20| + |v||v10| + |h|)) and
    normals (bound on the source pose, posed on the other), and the float32 round trip back onto the source pose against the point"""
    n = c["pts"].shape[0]
    faces, fi = np.arange(3 * n).reshape(n, 3), np.arange(n)
    src, dst = c["tri_src"].reshape(-1, 3), c["tri_dst"].reshape(-1, 3)
    out = {}
    v32, n32, _ = MP.pose(dst[None], faces, fi, c["uv"], c["h"], MP.bind_normals(src, faces, fi, c["normal"]))
    v64, n64, _ = MP.pose(dst[None], faces, fi, c["uv"], c["h"], MP.bind_normals(src, faces, fi, c["normal"], np.float64), np.float64)
    d = np.abs(v32[0].astype(np.float64) - v64[0])
    t = c["tri_dst"].astype(np.float64)
    u, v, h = (np.abs(a.astype(np.float64)) for a in (c["uv"][:, 0:1], c["uv"][:, 1:2], c["h"][:, None]))
    scale = 2.0 ** -24 * (np.abs(t[:, 0]) + u * np.abs(t[:, 2] - t[:, 0]) + v * np.abs(t[:, 1] - t[:, 0]) + h)
    out["position"] = float(d.max())
    out["position_units"] = float((d / scale).max())
    out["normal"] = float(np.abs(n32[0].astype(np.float64) - n64[0]).max())
    back, _, _ = MP.pose(src[None], faces, fi, c["uv"], c["h"])
    out["roundtrip"] = float(np.abs(back[0].astype(np.float64) - c["pts"].astype(np.float64)).max())
    return out


def case(name, canon, faces, n_pts, seed):
    import torch
    rh.install_shims()
    from utils.geo_utils import barycentric_map2can, project_point2mesh
    src = synth.pose_body(canon, seed=3)
    dst = synth.pose_body(canon, seed=7, trans=(-0.3, 0.25, 0.6))
    F = faces.shape[0]
    f = (synth.hash_uniform(n_pts, seed) * F).astype(np.int64) % F
    b = synth.hash_uniform(2 * n_pts, seed + 1).reshape(n_pts, 2).astype(np.float64)
    flip = b.sum(axis=1) > 1
    b[flip] = 1.0 - b[flip]
    tri = src[faces[f]].astype(np.float64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    # offsets along the face normal: on the surface, +-3 cm, and every eighth point 15 cm out (the mask's |h| > 0.1)
    off = np.array([0.0, 0.03, -0.03])[np.arange(n_pts) % 3]
    off[np.arange(n_pts) % 8 == 7] = 0.15
    pts = (tri[:, 0] + b[:, 0:1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:2] * (tri[:, 2] - tri[:, 0]) + off[:, None] * nrm).astype(np.float32)
    cent = src[faces].astype(np.float64).mean(axis=1)
    near = np.empty(n_pts, np.int64)
    for s in range(0, n_pts, 256):      # nearest face by centroid, brute force
        near[s:s + 256] = ((pts[s:s + 256, None, :].astype(np.float64) - cent[None]) ** 2).sum(-1).argmin(axis=1)
    nv = synth.hash_normal(3 * n_pts, seed + 2).reshape(n_pts, 3).astype(np.float64)
    normal = (nv / np.linalg.norm(nv, axis=1, keepdims=True)).astype(np.float32)
    out = {"pts": pts, "face": near.astype(np.int32), "normal": normal,
           "tri_src": src[faces[near]], "tri_dst": dst[faces[near]], "tri_can": canon[faces[near]]}
    for dt, tag in ((torch.float32, ""), (torch.float64, "64")):
        p = torch.from_numpy(pts).to(dt)
        m = {k: torch.from_numpy(out[k]).to(dt) for k in ("tri_src", "tri_dst", "tri_can")}
        uv, h = project_point2mesh(p, m["tri_src"])
        out["uv" + tag], out["h" + tag] = uv.numpy(), h.numpy()
        out["out_dst" + tag] = barycentric_map2can(uv, h, m["tri_dst"]).numpy()
        out["out_can" + tag] = barycentric_map2can(uv, h, m["tri_can"]).numpy()
        out["out_src" + tag] = barycentric_map2can(uv, h, m["tri_src"]).numpy()
    uv, h = out["uv"], out["h"]
    out["transparent"] = ((uv > 5).any(axis=1) | (uv < -4).any(axis=1) | (np.abs(h) > 0.1)).astype(np.uint8)
    assert 0 < int(out["transparent"].sum()) < n_pts
    rec = spread(out)
    rec.update(points=int(n_pts), transparent=int(out["transparent"].sum()),
               reference_position=float(np.abs(out["out_dst"].astype(np.float64) - out["out_dst64"]).max()),
               reference_roundtrip=float(np.abs(out["out_src"].astype(np.float64) - pts.astype(np.float64)).max()))
    for k in ("uv64", "h64", "out_dst64", "out_can64", "out_src64", "out_src"):
        del out[k]
    print(name, rec)
    return {name + ":" + k: v for k, v in out.items()}, rec


def main():
    bodies = {"lattice": synth.make_body(), "smpl_like": synth.make_body(nonuniform=True), "small": synth.make_small_body()}
    arrays, records = {}, {}
    for name, n_pts, seed in CASES:
        a, records[name] = case(name, bodies[name][0], bodies[name][1], n_pts, seed)
        arrays.update(a)
    path = os.path.join(HERE, "mesh_pose.npz")
    np.savez_compressed(path, **arrays)
    print(f"mesh_pose.npz {os.path.getsize(path) / 1024:.0f} KiB")
    what = ("per case of tests/golden/mesh_pose.npz: position / normal = the largest |float32 - float64| between the two restatements of "
            "dsn_mesh_pose (tests/mesh_pose_restate.py) on the fixture's other pose, position_units = the same in units of "
            "2^-24 (|m0| + |u||v20| + |v||v10| + |h|), roundtrip = the float32 restatement posed back onto the source pose against the "
            "point; recomputed and checked by tests/test_mesh_pose_host.py.  reference_* = the same figures of the reference's own "
            "torch functions (float32 against float64, end to end), for orientation.")
    with open(os.path.join(HERE, "mesh_pose_spread.json"), "w") as fh:
        json.dump({"what": what, "cases": records}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
