#!/usr/bin/env python3
"""The optimizer step on the device (dsnerf_amd.optim.Adam: dsn_adam_step, one launch for all tensors, the packed image rebuilt behind
it) against torch.optim.Adam followed by the re-pack net.packed() then has to do, on the same parameters and gradients.
    python scripts/bench_adam.py [--blocks 6] [--iters 40] [--step-iters 20] [--out profiles/adam_bench.json]
    python scripts/bench_adam.py --count torch|fused [--count-what opt|step]       (a fixed number of iterations of one variant and
                                                                     nothing else: run under rocprofv3 --kernel-trace --stats to count launches)
1. opt.step() and the net.packed() that follows it, alone, on the w4 parameters with fixed gradients: device time between HIP events,
   and the host's wall time inside the two calls (nothing synchronises inside them).
2. The whole 8192 x 64 training step of benchlib/train.py's recipe (render, MSE, backward, step) from the w4 parameters with either
   optimizer, in the same process.
HIP events around every iteration after a warm-up, the variants in alternating blocks; medians with the quartiles.  Clocks
(rocm-smi --showclocks, read only) before and after, the device and the host go into the file."""
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
from dsnerf_amd import synth  # noqa: E402
from benchlib.common import load_weights  # noqa: E402


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


def timed(fn, iters, host=False):
    """device time of fn() between two HIP events per iteration - or, host=True, the wall time the host spends inside fn() with the
    device idle before it"""
    out = []
    for _ in range(iters):
        if host:
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


def alternate(variants, blocks, iters, warmup=10, host=False):
    """variants: {name: fn()}; alternating blocks of `iters` timed iterations each -> {name: quartiles}"""
    for fn in variants.values():
        timed(fn, warmup, host)
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            ms[k] += timed(fn, iters, host)
    return {k: quartiles(v) for k, v in ms.items()}


def make_optimizer(name, net, lr=5e-4):
    if name == "torch":
        return torch.optim.Adam(net.parameters(), lr=lr)
    return dsnerf_amd.optim.Adam(net.parameters(), lr=lr, net=net)


def make_net(cfg, dev):
    net = dsnerf_amd.DualSpaceNeRF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in load_weights(synth, "w4").items()})
    return net.to(dev)


def _cfg(S=64):
    return SimpleNamespace(DATASETS=SimpleNamespace(SMPL_PATH="<synthetic>"),
                           MODEL=SimpleNamespace(sample_points_mode="GG", COARSE_RAY_SAMPLING=S, perturb=1.0, raw_noise_std=1.0, TYPE="nerf",
                                                 FINE_RAY_SAMPLING=-1))


def optimizer_alone(dev):
    """opt.step() + net.packed() with gradients that stay in place (what trainer.py:80 and the next render's first call amount to)"""
    variants = {}
    for name in ("torch", "fused"):          # each variant owns its parameters
        net = make_net(_cfg(), dev)
        rng = np.random.RandomState(3)
        for p in net.parameters():
            p.grad = torch.from_numpy((1e-3 * rng.randn(*p.shape)).astype(np.float32)).to(dev)
        opt = make_optimizer(name, net)
        net.packed()

        def run(net=net, opt=opt):
            opt.step()
            net.packed()

        variants[name] = run
    return variants


def training_step(dev, S=64, R=8192, hw=512):
    """benchlib/train.py's step (zero_grad, render, MSE, backward, step on one synthetic batch, w4 parameters)"""
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon, seed=3)
    rays = synth.make_rays(hw, hw, xyz, fit_box=True)
    sel = np.linspace(0, hw * hw - 1, R).astype(np.int64)
    cfg = _cfg(S)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    batch = {"ray_o": T(rays["ray_o"][sel])[None], "ray_d": T(rays["ray_d"][sel])[None], "near": T(rays["near"][sel])[None],
             "far": T(rays["far"][sel])[None], "xyz": T(xyz)[None], "poses": T(synth.make_poses(seed=5))[None],
             "Th": torch.zeros(1, 1, 3, device=dev), "frame": torch.tensor([5])}
    target = T(synth.hash_uniform(R * 3, 77).reshape(R, 3).astype(np.float32))
    variants, last = {}, {}
    for name in ("torch", "fused"):
        net = make_net(cfg, dev)
        r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
        r.train()
        opt = make_optimizer(name, net)

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_bench.json"))
    ap.add_argument("--count", choices=["torch", "fused"], help="run --count-iters iterations of this variant and exit (for a kernel trace)")
    ap.add_argument("--count-what", choices=["opt", "step"], default="opt")
    ap.add_argument("--count-iters", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    torch.manual_seed(233)
    if args.count:
        variants = optimizer_alone(dev) if args.count_what == "opt" else training_step(dev)
        timed(variants[args.count], args.count_iters)       # (the first step allocates the moments: difference two counts to drop the set-up)
        torch.cuda.synchronize()
        print(json.dumps({"counted": args.count, "what": args.count_what, "iterations": args.count_iters}))
        return
    res = {"metric": "adam_step_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "blocks": args.blocks, "iters_per_block": args.iters, "step_iters_per_block": args.step_iters,
           "timing": "HIP events around each iteration (host: perf_counter around the calls, device idle before), variants in alternating "
                     "blocks after 10 warm-up iterations each",
           "variants": {"torch": "torch.optim.Adam(net.parameters()) then net.packed() (version counters compared, 33 tensors re-packed)",
                        "fused": "dsnerf_amd.optim.Adam(net.parameters(), net=net) then net.packed() (finds the image current)"},
           "clocks_before": clocks()}
    variants = optimizer_alone(dev)
    alternate(variants, 2, 200)               # not recorded: the clocks come up from idle during the first few hundred launches
    q = alternate(variants, args.blocks, args.iters)
    q["torch_over_fused"] = round(q["torch"]["median_ms"] / q["fused"]["median_ms"], 3)
    res["step_and_packed_device"] = q
    q = alternate(variants, args.blocks, args.iters, host=True)
    q["torch_over_fused"] = round(q["torch"]["median_ms"] / q["fused"]["median_ms"], 3)
    res["step_and_packed_host_wall"] = q
    variants = training_step(dev)
    q = alternate(variants, args.blocks, args.step_iters, warmup=8)
    q["fused_minus_torch_ms"] = round(q["fused"]["median_ms"] - q["torch"]["median_ms"], 5)
    q["outside_the_quartiles"] = bool(q["fused"]["q75_ms"] < q["torch"]["q25_ms"] or q["fused"]["q25_ms"] > q["torch"]["q75_ms"])
    q["last_loss"] = {k: float(v) for k, v in training_step.last.items()}
    res["training_step_8192x64_w4"] = q
    res["clocks_after"] = clocks()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
