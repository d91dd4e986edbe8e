#!/usr/bin/env python3
"""The body model on the device (dsn_body_pose: SMPL parameters -> posed vertices, joint transforms and bounds for P poses in one
call) against the same arithmetic written as torch ops on the same GPU in the same run, and against the call's byte floor.
    python scripts/bench_body_pose.py [--blocks 6] [--iters 30] [--out profiles/body_pose_bench.json]
V = 6890 with posedirs, Rh and Th; P = 1, 8, 64 and 512 poses per call; outputs xyz, A and bounds (what BodyModel.pose returns by
default).  The torch formulation is the usual SMPL layer: batched Rodrigues and the 23-step chain over the kinematic tree in float64
(as the rule has them), pose feature @ posedirs, weights @ A, the rigid part, Rh / Th, amin / amax - every op on the device, nothing
copied.  Its results are compared with the call's before anything is timed.
HIP events around every iteration after a warm-up, the two variants in alternating blocks; medians with the quartiles.
Byte floor: what the call must move at least - posedirs and weights once per block of 8 poses (the vertex kernel's pose block), the
float32 outputs once - over the 8.0 TB/s of the HBM's specification; the 17 MB of posedirs stay in the 256 MB Infinity Cache between
pose blocks, so the floor is the floor of a cold call."""
import argparse
import json
import os
import platform
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import dsnerf_amd  # noqa: E402
from dsnerf_amd import synth  # noqa: E402
from dsnerf_amd.body import BodyModel  # noqa: E402
import body_pose_restate as BP  # noqa: E402  (the synthetic model and SMPL's parent table)

HBM_BYTES_PER_S = 8.0e12
POSE_BLOCK = 8


def quartiles(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 5), "q25_ms": round(float(q[0]), 5), "q75_ms": round(float(q[2]), 5), "n": len(ms)}


def timed(fn, iters):
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(variants, blocks, iters, warmup=10):
    for fn in variants.values():
        timed(fn, warmup)
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            ms[k] += timed(fn, iters)
    return {k: quartiles(v) for k, v in ms.items()}


def rodrigues_torch(p):
    """[N,3] float64 -> [N,3,3]: utils/h36m_utils.py:210-229 as torch ops"""
    angle = torch.linalg.norm(p + 1e-8, dim=1, keepdim=True)
    r = p / angle
    c, s = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    z = torch.zeros_like(r[:, 0])
    K = torch.stack([z, -r[:, 2], r[:, 1], r[:, 2], z, -r[:, 0], -r[:, 1], r[:, 0], z], dim=1).reshape(-1, 3, 3)
    return torch.eye(3, dtype=p.dtype, device=p.device)[None] + s * K + (1 - c) * torch.bmm(K, K)


def make_torch_pose(bm, parents, pad=0.05):
    vs, w, pd = bm.v_shaped, bm.weights, bm.posedirs
    J = bm.joints.double()
    rel = J.clone()
    rel[1:] = J[1:] - J[torch.as_tensor(parents[1:].astype(np.int64), device=J.device)]
    eye = torch.eye(3, dtype=torch.float64, device=J.device)
    V = vs.shape[0]

    def pose(poses, Rh, Th):
        P = poses.shape[0]
        R = rodrigues_torch(poses.double().reshape(-1, 3)).reshape(P, 24, 3, 3)
        T = torch.zeros(P, 24, 4, 4, dtype=torch.float64, device=poses.device)
        T[:, :, :3, :3] = R
        T[:, :, :3, 3] = rel
        T[:, :, 3, 3] = 1.0
        chain = [T[:, 0]]
        for i in range(1, 24):
            chain.append(torch.bmm(chain[int(parents[i])], T[:, i]))
        G = torch.stack(chain, dim=1)
        A = G.clone()
        A[..., :3, 3] = G[..., :3, 3] - (G[..., :3, :3] @ J[None, :, :, None])[..., 0]
        A = A.float()
        pf = (R[:, 1:] - eye).reshape(P, 207).float()
        vp = vs[None] + (pf @ pd).reshape(P, V, 3)
        Tv = (w @ A.reshape(P, 24, 16)).reshape(P, V, 4, 4)
        xs = (Tv[..., :3, :3] @ vp[..., None])[..., 0] + Tv[..., :3, 3]
        xyz = xs @ rodrigues_torch(Rh.double()).float().transpose(1, 2) + Th[:, None]
        bounds = torch.stack([xyz.amin(dim=1) - pad, xyz.amax(dim=1) + pad], dim=1)
        return {"xyz": xyz, "A": A, "bounds": bounds}
    return pose


def byte_floor(V, P):
    blocks = -(-P // POSE_BLOCK)
    read = blocks * 4 * (207 * 3 * V + 24 * V) + 4 * (3 * V + 72) + 4 * P * (72 + 6)
    write = 4 * P * (3 * V + 24 * 16 + 6)
    return read + write


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--counts", type=int, nargs="*", default=[1, 8, 64, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_pose_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    canon, _ = synth.make_body()
    vt, w, Jr, sd, pd = BP.make_model(canon)
    bm = BodyModel(vt, w, BP.SMPL_PARENTS, J_regressor=Jr, shapedirs=sd, posedirs=pd, device=dev)
    bm.set_shape((synth.hash_normal(10, 77) * np.float32(0.8)).astype(np.float32))
    torch_pose = make_torch_pose(bm, BP.SMPL_PARENTS)
    res = {"metric": "body_pose_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "V": int(bm.V), "blocks": args.blocks, "iters_per_block": args.iters,
           "timing": "HIP events around each iteration, variants in alternating blocks after 10 warm-up iterations each",
           "variants": {"call": "BodyModel.pose(poses, Rh, Th, pad='h36m'): one dsn_body_pose call (three launches), outputs xyz, A, bounds",
                        "torch": "the same arithmetic as torch ops (float64 Rodrigues and 23-step chain, pf @ posedirs, weights @ A, rigid "
                                 "part, Rh / Th, amin / amax), same outputs"},
           "byte_floor": "posedirs + weights once per block of 8 poses, inputs and float32 outputs once, over 8.0 TB/s", "poses": {}}
    for P in args.counts:
        poses = torch.from_numpy(np.stack([synth.make_poses(1000 + i) for i in range(P)])).to(dev)
        Rh = torch.from_numpy((synth.hash_normal(3 * P, 11) * np.float32(0.7)).reshape(P, 3)).to(dev)
        Th = torch.from_numpy((synth.hash_normal(3 * P, 12) * np.float32(0.9)).reshape(P, 3)).to(dev)
        ours = bm.pose(poses, Rh, Th, pad="h36m", slab=P)
        theirs = torch_pose(poses, Rh, Th)
        diff = {k: float((ours[k] - theirs[k]).abs().max()) for k in ("xyz", "A", "bounds")}
        assert max(diff.values()) < 2e-5, diff            # two float32 orders of the same sums
        variants = {"call": lambda: bm.pose(poses, Rh, Th, pad="h36m", slab=P), "torch": lambda: torch_pose(poses, Rh, Th)}
        alternate(variants, 1, 50)                        # not recorded: the clocks come up from idle during the first launches
        q = alternate(variants, args.blocks, args.iters)
        floor_ms = 1e3 * byte_floor(bm.V, P) / HBM_BYTES_PER_S
        q.update(max_abs_difference=diff, byte_floor_bytes=byte_floor(bm.V, P), byte_floor_ms=round(floor_ms, 5),
                 call_over_floor=round(q["call"]["median_ms"] / floor_ms, 2), torch_over_call=round(q["torch"]["median_ms"] / q["call"]["median_ms"], 3),
                 call_not_above_torch=bool(q["call"]["median_ms"] <= q["torch"]["median_ms"]))
        res["poses"][str(P)] = q
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
