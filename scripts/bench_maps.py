#!/usr/bin/env python3
"""What the decomposition maps cost, and whether the frames that do not ask for them got slower: the w4 bench frame (512 x 512 x 64,
the converged checkpoint, early stop as the Renderer plans it).
    python scripts/bench_maps.py [--frames 20] [--parent-root DIR [--rounds 3]] [--out profiles/maps_bench.json]
After warm-up, alternated frame by frame inside one process, HIP-event time of
    (a) Renderer.render_view                       (b) Renderer.render_view_maps, all three maps
    (c) Renderer.render_view_lights, vis_lighting.py's ten angles      (d) render_view_maps with the same ten lights
(device-resident batch and images), --frames frames each: medians, (b) - (a) and (d) - (c) per frame with their spread.
--parent-root DIR: a checkout of the PARENT commit with its library built (git archive HEAD~ | tar -x -C DIR; python DIR/__graft_entry__.py).
(a) is then measured again in fresh processes, --rounds times this tree and DIR alternated (this script with --view-only --root ...,
which needs nothing the parent lacks): "existing frames did not get slower" = this tree's median inside the spread of the parent's
process medians, measured in this very run.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def angle2rot(angle):                                                # vis_lighting.py:86-91
    rad = np.pi * angle / 180
    return np.array([[np.cos(rad), -np.sin(rad)], [np.sin(rad), np.cos(rad)]])


def setup(root, hw, S, weights):
    sys.path.insert(0, root)
    import torch
    import dsnerf_amd
    from dsnerf_amd import synth
    from benchlib.common import load_weights
    dev = torch.device("cuda:0")
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon, seed=3)
    rays = synth.make_rays(hw, hw, xyz, fit_box=True)
    cfg = SimpleNamespace(DATASETS=SimpleNamespace(SMPL_PATH="<synthetic>"),
                          MODEL=SimpleNamespace(sample_points_mode="GG", COARSE_RAY_SAMPLING=S, perturb=1.0, raw_noise_std=1.0, TYPE="nerf",
                                                FINE_RAY_SAMPLING=-1))
    net = dsnerf_amd.DualSpaceNeRF(cfg)
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in load_weights(synth, weights).items()})
    net.to(dev)
    r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
    r.eval()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    batch = {"ray_o": T(rays["ray_o"])[None], "ray_d": T(rays["ray_d"])[None], "near": T(rays["near"])[None], "far": T(rays["far"])[None],
             "xyz": T(xyz)[None], "poses": T(synth.make_poses(seed=5))[None], "Th": torch.zeros(1, 1, 3, device=dev),
             "frame": torch.tensor([5]), "img": torch.zeros(1, hw, hw, 3, device=dev),
             "mask_at_box": torch.ones(1, hw * hw, dtype=torch.bool, device=dev)}
    return torch, r, batch


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4),
            "iqr": round(float(np.quantile(v, 0.75) - np.quantile(v, 0.25)), 4), "n": int(v.size)}


def view_only(args):
    """(a) alone, in this process, from the tree at args.root: one JSON line"""
    torch, r, batch = setup(args.root, args.hw, args.samples, args.weights)
    fn = lambda: r.render_view(dict(batch), device_output=True)
    for _ in range(args.warmup + 2):
        fn()
    t = [timed(torch, fn) for _ in range(args.frames)]
    print(json.dumps({"root": args.root, "render_view_ms": stats(t), "early_stop": bool(r.last_frame_info.get("early_stop"))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--view-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.view_only:
        return view_only(args)
    torch, r, batch = setup(args.root, args.hw, args.samples, args.weights)
    head = torch.tensor([[0.18649693, -0.14180326, 1.7103844]])          # vis_lighting.py:57
    lights = [{"rot": torch.Tensor(angle2rot(a)), "rot_center": head} for a in range(0, 360, 36)]
    variants = {
        "a_render_view": lambda: r.render_view(dict(batch), device_output=True),
        "b_render_view_maps": lambda: r.render_view_maps(dict(batch), device_output=True),
        "c_render_view_lights_10": lambda: r.render_view_lights(dict(batch), lights, device_output=True),
        "d_render_view_maps_10": lambda: r.render_view_maps(dict(batch), lights=lights, device_output=True),
    }
    for _ in range(args.warmup + 2):
        for fn in variants.values():
            fn()
    info = {}
    t = {k: [] for k in variants}
    for _ in range(args.frames):
        for k, fn in variants.items():
            t[k].append(timed(torch, fn))
            info[k] = {"early_stop": bool(r.last_frame_info.get("early_stop")), "density_screen": bool(r.last_frame_info.get("density_screen")),
                       "rendered_again_in_one_pass": bool(r.last_frame_info.get("rendered_again_in_one_pass", False))}
    # the maps' own cost, frame by frame (the variants of one round ran back to back)
    b_a = np.asarray(t["b_render_view_maps"]) - np.asarray(t["a_render_view"])
    d_c = np.asarray(t["d_render_view_maps_10"]) - np.asarray(t["c_render_view_lights_10"])
    res = {"metric": "decomposition_maps", "frame": f"{args.hw}x{args.hw}x{args.samples}", "weights": args.weights,
           "frames_each": args.frames, "timer": "HIP events around each call, synchronised before", "plan": info,
           "ms": {k: stats(v) for k, v in t.items()},
           "maps_cost_ms": {"b_minus_a": stats(b_a), "d_minus_c": stats(d_c), "d_minus_c_per_light": round(float(np.median(d_c)) / 10.0, 4)},
           "device": torch.cuda.get_device_name(0)}
    if args.parent_root:
        runs = {"this": [], "parent": []}
        ok = True
        for _ in range(args.rounds):
            for who, root in (("this", args.root), ("parent", args.parent_root)):
                if not ok:
                    break
                cmd = [sys.executable, os.path.abspath(__file__), "--view-only", "--root", root, "--hw", str(args.hw), "--samples",
                       str(args.samples), "--weights", args.weights, "--frames", str(args.frames), "--warmup", str(args.warmup)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:      # (nothing more is started on the GPU after a process that failed)
                    ok = False
                    res["parent_comparison_error"] = {"who": who, "returncode": p.returncode, "stderr": p.stderr[-400:]}
                    break
                runs[who].append(json.loads(p.stdout.strip().splitlines()[-1]))
        if ok:
            med = {w: [x["render_view_ms"]["median"] for x in v] for w, v in runs.items()}
            lo, hi = min(med["parent"]), max(med["parent"])
            res["render_view_vs_parent"] = {
                "processes_each": args.rounds, "this_process_medians_ms": med["this"], "parent_process_medians_ms": med["parent"],
                "this_median_ms": round(float(np.median(med["this"])), 4), "parent_median_ms": round(float(np.median(med["parent"])), 4),
                "parent_spread_ms": round(hi - lo, 4),
                "parent_frame_iqr_ms": [x["render_view_ms"]["iqr"] for x in runs["parent"]],
                "this_within_parent_spread": bool(float(np.median(med["this"])) <= hi + 1e-9)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
