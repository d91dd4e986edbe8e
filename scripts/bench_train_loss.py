#!/usr/bin/env python3
"""The trainer's loss on the device (dsnerf_amd.loss: dsn_train_loss / dsn_train_loss_grad) against the torch-op chain that the
reference's utils/loss.py + metrics.psnr amount to, on the same tensors.
    python scripts/bench_train_loss.py [--blocks 6] [--iters 40] [--step-iters 20] [--out profiles/train_loss_bench.json]
    python scripts/bench_train_loss.py --count torch|fused [--count-what loss|step]     (a fixed number of iterations of one variant and
                                                                     nothing else: run under rocprofv3 --kernel-trace --stats to count launches)
1. The loss with its backward alone at R = 8192 (the trainer's batch) and R = 512^2 (a frame's rays): loss_fn(coarse, batch), the
   per-step psnr, sum, backward() down to the seeds of color and acc_map.  Both kinds, LOSSwMask on, float32 targets, uint8 occupancy.
2. The whole 8192 x 64 training step from the w4 parameters (benchlib/train.py's step with LOSSwMask and the per-step psnr, as
   trainer.py:66-84 has them), the loss in torch ops against the loss from dsnerf_amd.loss, in the same process.
HIP events around every iteration after a warm-up, the variants in alternating blocks; medians with the quartiles.  Clocks
(rocm-smi --showclocks, read only) before and after, the device and the host go into the file."""
import argparse
import json
import os
import platform
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dsnerf_amd  # noqa: E402
from dsnerf_amd import synth  # noqa: E402
from benchlib.common import load_weights  # noqa: E402

F = torch.nn.functional


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k or "mclk" in k or "fclk" in k}
    except Exception as e:      # (the numbers stand without it; the file says that the clocks could not be read)
        return {"unavailable": repr(e)[:200]}


def torch_op_loss(kind, coarse, batch):
    """utils/loss.py:11-49 with LOSSwMask, trainer.py:73-76's sum and :83's psnr (metrics.py:8-21), op by op"""
    target = batch["rgb"].reshape(-1, 3).cuda()
    loss_rgb = (F.mse_loss if kind == "L2" else F.smooth_l1_loss)(coarse["color"], target)
    acc_map = coarse["acc_map"]
    occupancy = batch["occupancy"].reshape(-1).cuda()
    acc_map[occupancy == 1] = 1
    loss1 = {"loss_rgb": loss_rgb, "loss_mask": 0.1 * F.l1_loss(acc_map, occupancy)}
    loss = 0
    for key in loss1:
        loss += loss1[key]
    psnr = -10 * torch.log10(torch.mean((coarse["color"] - target) ** 2))
    return loss, psnr


def fused_loss(loss_fn, coarse, batch):
    loss1 = loss_fn(coarse, batch)
    loss = 0
    for key in loss1:
        loss += loss1[key]
    return loss, loss_fn.last["psnr"]


class _Source(torch.autograd.Function):
    """stands for the renderer: hands out (color, acc_map) as the non-leaf outputs of a node whose backward takes the seeds and does
    nothing, so that only the loss and its backward are between the events"""

    @staticmethod
    def forward(ctx, w, color, acc):
        ctx.set_materialize_grads(False)
        return color.clone(), acc.clone()

    @staticmethod
    def backward(ctx, g_color, g_acc):
        _Source.seen = (g_color, g_acc)
        return None, None, None


def quartiles(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 5), "q25_ms": round(float(q[0]), 5), "q75_ms": round(float(q[2]), 5), "n": len(ms)}


def timed(fn, setup, iters):
    out = []
    for _ in range(iters):
        state = setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(state)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(variants, setup, blocks, iters, warmup=10):
    """variants: {name: fn(state)}; alternating blocks of `iters` timed iterations each -> {name: quartiles}"""
    for fn in variants.values():
        timed(fn, setup, warmup)
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            ms[k] += timed(fn, setup, iters)
    return {k: quartiles(v) for k, v in ms.items()}


def loss_alone(R, kind, dev):
    rng = np.random.RandomState(R % 1000 + (kind == "L1"))
    t = rng.rand(R, 3).astype(np.float32)
    color = torch.from_numpy((t + 0.6 * rng.randn(R, 3)).astype(np.float32)).to(dev)
    acc = torch.from_numpy(rng.rand(R).astype(np.float32)).to(dev)
    batch = {"rgb": torch.from_numpy(t).to(dev)[None], "occupancy": torch.from_numpy((rng.rand(R) < 0.5).astype(np.uint8)).to(dev)[None]}
    w = torch.zeros((), device=dev, requires_grad=True)
    loss_fn = dsnerf_amd.loss.make_loss(SimpleNamespace(MODEL=SimpleNamespace(LOSS=kind, LOSSwMask=True)))

    def setup():
        c, a = _Source.apply(w, color, acc)
        return {"color": c, "acc_map": a}

    def run_torch(coarse):
        loss, _ = torch_op_loss(kind, coarse, batch)
        loss.backward()

    def run_fused(coarse):
        loss, _ = fused_loss(loss_fn, coarse, batch)
        loss.backward()

    return {"torch": run_torch, "fused": run_fused}, setup


def training_step(dev, kind="L2", S=64, R=8192, hw=512):
    """benchlib/train.py's step (render + loss + backward + Adam on one synthetic batch, w4 parameters) with LOSSwMask and the psnr"""
    canon, faces = synth.make_body()
    sd = load_weights(synth, "w4")
    xyz = synth.pose_body(canon, seed=3)
    rays = synth.make_rays(hw, hw, xyz, fit_box=True)
    sel = np.linspace(0, hw * hw - 1, R).astype(np.int64)
    cfg = SimpleNamespace(DATASETS=SimpleNamespace(SMPL_PATH="<synthetic>"),
                          MODEL=SimpleNamespace(sample_points_mode="GG", COARSE_RAY_SAMPLING=S, perturb=1.0, raw_noise_std=1.0, TYPE="nerf",
                                                FINE_RAY_SAMPLING=-1, LOSS=kind, LOSSwMask=True))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    batch = {"ray_o": T(rays["ray_o"][sel])[None], "ray_d": T(rays["ray_d"][sel])[None], "near": T(rays["near"][sel])[None],
             "far": T(rays["far"][sel])[None], "xyz": T(xyz)[None], "poses": T(synth.make_poses(seed=5))[None],
             "Th": torch.zeros(1, 1, 3, device=dev), "frame": torch.tensor([5]),
             "rgb": T(synth.hash_uniform(R * 3, 77).reshape(R, 3).astype(np.float32))[None],
             "occupancy": T((synth.hash_uniform(R, 78) > 0.5).astype(np.uint8))[None]}
    variants, last = {}, {}
    for name in ("torch", "fused"):          # each variant trains its own copy of the parameters
        net = dsnerf_amd.DualSpaceNeRF(cfg)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        net.to(dev)
        r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
        r.train()
        opt = torch.optim.Adam(net.parameters(), lr=5e-4)
        loss_fn = dsnerf_amd.loss.make_loss(cfg)

        def step(_, r=r, opt=opt, loss_fn=loss_fn, name=name):
            opt.zero_grad()
            coarse = r.render(batch)["coarse"]
            loss, psnr = torch_op_loss(kind, coarse, batch) if name == "torch" else fused_loss(loss_fn, coarse, batch)
            loss.backward()
            opt.step()
            last[name] = (loss.detach(), psnr.detach())

        variants[name] = step
    training_step.last = last
    return variants, (lambda: None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_loss_bench.json"))
    ap.add_argument("--count", choices=["torch", "fused"], help="run --count-iters iterations of this variant and exit (for a kernel trace)")
    ap.add_argument("--count-what", choices=["loss", "step"], default="loss")
    ap.add_argument("--count-iters", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    torch.manual_seed(233)
    if args.count:
        variants, setup = loss_alone(8192, "L2", dev) if args.count_what == "loss" else training_step(dev)
        timed(variants[args.count], setup, args.count_iters)
        torch.cuda.synchronize()
        print(json.dumps({"counted": args.count, "what": args.count_what, "iterations": args.count_iters}))
        return
    res = {"metric": "train_loss_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "blocks": args.blocks, "iters_per_block": args.iters, "step_iters_per_block": args.step_iters,
           "timing": "HIP events around each iteration, variants in alternating blocks after 10 warm-up iterations each",
           "clocks_before": clocks(), "loss_and_backward": {}, "training_step_8192x64_w4": {}}
    variants, setup = loss_alone(8192, "L2", dev)
    alternate(variants, setup, 2, 200)               # not recorded: the clocks come up from idle during the first few hundred launches
    for R in (8192, 512 * 512):
        for kind in ("L2", "L1"):
            variants, setup = loss_alone(R, kind, dev)
            q = alternate(variants, setup, args.blocks, args.iters)
            q["torch_over_fused"] = round(q["torch"]["median_ms"] / q["fused"]["median_ms"], 3)
            res["loss_and_backward"][f"R{R}_{kind}"] = q
    variants, setup = training_step(dev)
    q = alternate(variants, setup, args.blocks, args.step_iters, warmup=8)
    q["fused_minus_torch_ms"] = round(q["fused"]["median_ms"] - q["torch"]["median_ms"], 5)
    q["outside_the_quartiles"] = bool(q["fused"]["q75_ms"] < q["torch"]["q25_ms"] or q["fused"]["q25_ms"] > q["torch"]["q75_ms"])
    q["last_loss_psnr"] = {k: [float(v) for v in training_step.last[k]] for k in variants}
    res["training_step_8192x64_w4"] = q
    res["clocks_after"] = clocks()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
