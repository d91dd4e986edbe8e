#!/usr/bin/env python3
"""The training step's draws on the device (dsn_train_draws, Renderer.draws = "device") against the host path (Renderer._draws: the
CPU default generator into a page-locked ring, one upload).
    python scripts/bench_draws.py [--blocks 6] [--iters 40] [--step-iters 20] [--out profiles/train_draws_bench.json]
1. dsn_train_draws alone at 8192 x 64 (both arrays): device time between HIP events, beside the floor of its 8 bytes per value at
   the HBM write rate the file names, and beside the same call at 1 x 4 (what the two events cost around any launch).
2. The host's wall time inside Renderer._draws (host path) and inside Renderer._device_draws, device idle before each call.
3. The whole 8192 x 64 training step of benchlib/train.py's recipe (render, MSE, backward, Adam) from the w4 parameters with either
   source of the draws, in the same process: HIP events around every step, and - the steps of a block enqueued back to back with one
   wait at its end, as a trainer runs them - the block's wall time per step.
The variants run in alternating blocks after a warm-up; medians with the quartiles.  Clocks (rocm-smi --showclocks, read only)
before and after, the device and the host go into the file."""
import argparse
import json
import os
import platform
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

HBM_TBS = 8.0          # what the byte floor is priced at: the HBM peak, as in the other records of profiles/


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k or "mclk" in k or "fclk" in k}
    except Exception as e:      # (the numbers stand without it; the file says that the clocks could not be read)
        return {"unavailable": repr(e)[:200]}


def quartiles(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 5), "q25_ms": round(float(q[0]), 5), "q75_ms": round(float(q[2]), 5), "n": len(ms)}


def timed(fn, iters, mode="device"):
    """mode "device": device time of fn() between two HIP events per iteration; "host": the wall time the host spends inside fn() with
    the device idle before it; "pipelined": `iters` calls enqueued back to back, one wait at the end - wall time per call (one figure)"""
    out = []
    if mode == "pipelined":
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return [1e3 * (time.perf_counter() - t0) / iters]
    for _ in range(iters):
        if mode == "host":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            out.append(1e3 * (time.perf_counter() - t0))
            continue
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(variants, blocks, iters, warmup=10, mode="device"):
    """variants: {name: fn()}; alternating blocks of `iters` timed iterations each -> {name: quartiles}"""
    for fn in variants.values():
        timed(fn, warmup, mode)
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            ms[k] += timed(fn, iters, mode)
    return {k: quartiles(v) for k, v in ms.items()}


def compare(q, a="host", b="device"):
    q[f"{b}_minus_{a}_ms"] = round(q[b]["median_ms"] - q[a]["median_ms"], 5)
    q["outside_the_quartiles"] = bool(q[b]["q75_ms"] < q[a]["q25_ms"] or q[b]["q25_ms"] > q[a]["q75_ms"])
    return q


def _cfg(S=64):
    return SimpleNamespace(DATASETS=SimpleNamespace(SMPL_PATH="<synthetic>"),
                           MODEL=SimpleNamespace(sample_points_mode="GG", COARSE_RAY_SAMPLING=S, perturb=1.0, raw_noise_std=1.0, TYPE="nerf",
                                                 FINE_RAY_SAMPLING=-1))


def make_renderer(dev, S, canon, faces, draws):
    net = dsnerf_amd.DualSpaceNeRF(_cfg(S))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in load_weights(synth, "w4").items()})
    net = net.to(dev)
    r = dsnerf_amd.Renderer(net, None, _cfg(S), torch.from_numpy(canon), body_data={"f": faces}, device=dev)
    r.train()
    r.draws = draws
    r.seed_draws(233)
    return r


def kernel_alone(dev, R, S):
    out = (torch.empty(R, S, device=dev), torch.empty(R, S, device=dev))
    step = [0]

    def run():
        _lib.train_draws(R, S, 233, step[0], out=out)
        step[0] += 1

    tiny = (torch.empty(1, 4, device=dev), torch.empty(1, 4, device=dev))
    # (one thread's work: what lies between two HIP events around ANY launch of this kernel - the floor the full size is read against)
    return {"dsn_train_draws": run, "dsn_train_draws_1x4": lambda: _lib.train_draws(1, 4, 233, 0, out=tiny)}


def draws_alone(dev, R, S, canon, faces):
    rs = {k: make_renderer(dev, S, canon, faces, k) for k in ("host", "device")}
    return {"host": lambda: rs["host"]._draws(R, S), "device": lambda: rs["device"]._device_draws(R, S)}


def training_step(dev, canon, faces, S=64, R=8192, hw=512):
    """benchlib/train.py's step (zero_grad, render, MSE, backward, step on one synthetic batch, w4 parameters)"""
    xyz = synth.pose_body(canon, seed=3)
    rays = synth.make_rays(hw, hw, xyz, fit_box=True)
    sel = np.linspace(0, hw * hw - 1, R).astype(np.int64)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    batch = {"ray_o": T(rays["ray_o"][sel])[None], "ray_d": T(rays["ray_d"][sel])[None], "near": T(rays["near"][sel])[None],
             "far": T(rays["far"][sel])[None], "xyz": T(xyz)[None], "poses": T(synth.make_poses(seed=5))[None],
             "Th": torch.zeros(1, 1, 3, device=dev), "frame": torch.tensor([5])}
    target = T(synth.hash_uniform(R * 3, 77).reshape(R, 3).astype(np.float32))
    variants, last = {}, {}
    for name in ("host", "device"):
        r = make_renderer(dev, S, canon, faces, name)
        opt = dsnerf_amd.optim.Adam(r.net.parameters(), lr=5e-4, net=r.net)

        def step(r=r, opt=opt, name=name):
            opt.zero_grad()
            out = r.render(batch)["coarse"]
            loss = torch.nn.functional.mse_loss(out["color"], target)
            loss.backward()
            opt.step()
            last[name] = loss.detach()

        variants[name] = step
    training_step.last = last
    return variants


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_draws_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    torch.manual_seed(233)
    R, S = args.rays, args.samples
    res = {"metric": "train_draws_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "host_threads": torch.get_num_threads(), "cpu_quota_cores": _lib.cpu_quota_cores(), "rays": R,
           "samples": S, "blocks": args.blocks, "iters_per_block": args.iters, "step_iters_per_block": args.step_iters,
           "timing": "HIP events around each iteration (host: perf_counter around the call, device idle before; pipelined: a block's "
                     "steps enqueued back to back, one wait at its end, wall time per step), variants in alternating blocks after a warm-up",
           "variants": {"host": "Renderer.draws = 'host': torch.rand / torch.randn from the CPU default generator into a page-locked ring, "
                                "one upload, two device clones",
                        "device": "Renderer.draws = 'device': one dsn_train_draws launch"},
           "clocks_before": clocks()}
    canon, faces = synth.make_body()
    variants = kernel_alone(dev, R, S)
    alternate(variants, 2, 200)               # not recorded: the clocks come up from idle during the first few hundred launches
    q = alternate(variants, args.blocks, args.iters)
    nbytes = 8 * R * S
    q["bytes_written"] = nbytes
    q["byte_floor_ms_at_%g_TB_s" % HBM_TBS] = round(1e3 * nbytes / (HBM_TBS * 1e12), 5)
    q["achieved_GB_s"] = round(nbytes / (1e-3 * q["dsn_train_draws"]["median_ms"]) / 1e9, 1)
    res["kernel_device"] = q
    res["draws_host_wall"] = compare(alternate(draws_alone(dev, R, S, canon, faces), args.blocks, args.iters, mode="host"))
    variants = training_step(dev, canon, faces, S, R)
    res["training_step_w4_device_events"] = compare(alternate(variants, args.blocks, args.step_iters, warmup=8))
    q = compare(alternate(variants, 2 * args.blocks, args.step_iters, warmup=8, mode="pipelined"))
    q["last_loss"] = {k: float(v) for k, v in training_step.last.items()}
    res["training_step_w4_pipelined_wall"] = q
    res["clocks_after"] = clocks()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
