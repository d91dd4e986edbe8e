#!/usr/bin/env python3
"""test.py's two LPIPS distances on the device (dsnerf_amd.lpips / dsn_lpips: csrc/dsn_lpips.hip) against the same arithmetic as torch
ops (F.conv2d, F.max_pool2d, float32, the framework's convolution library) on the same GPU in the same run.
    python scripts/bench_lpips.py [--blocks 4] [--iters 8] [--out profiles/lpips_bench.json]
Whole calls on device stacks: 512 x 512 and 1024 x 1024, F = 1 and 16 frames, alex and vgg; float32 BGR prediction and float64 ground
truth in, F float64 distances out (no host copy in either variant).  Hash-generated He-scaled weights (the timing does not depend on
the values; the two variants are compared before anything is timed).
HIP events around whole calls after a warm-up, the two variants in alternating blocks; medians with the quartiles.
Recorded beside the times: the exact multiply-accumulate count of the convolutions (two images per frame), what fraction of the
split-fp16 matrix ceiling the whole call reaches (2 MAC flops over 2500 / 3 = 833 TFLOP/s, as benchlib/roofline.py counts), and the
convolution kernel's share of the call's kernel time (torch.profiler's device activity; null where it records none)."""
import argparse
import json
import os
import platform
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import dsnerf_amd  # noqa: E402
from dsnerf_amd import _lib  # noqa: E402
from dsnerf_amd.synth import hash_uniform  # noqa: E402

SPLIT_CEILING_TFLOPS = 2500.0 / 3.0
# (Cin, Cout, k, stride, pad, tap) | (k, stride)
ARCH = {
    "alex": [(3, 64, 11, 4, 2, 0), (3, 2), (64, 192, 5, 1, 2, 1), (3, 2), (192, 384, 3, 1, 1, 2), (384, 256, 3, 1, 1, 3), (256, 256, 3, 1, 1, 4)],
    "vgg": [(3, 64, 3, 1, 1, None), (64, 64, 3, 1, 1, 0), (2, 2), (64, 128, 3, 1, 1, None), (128, 128, 3, 1, 1, 1), (2, 2),
            (128, 256, 3, 1, 1, None), (256, 256, 3, 1, 1, None), (256, 256, 3, 1, 1, 2), (2, 2),
            (256, 512, 3, 1, 1, None), (512, 512, 3, 1, 1, None), (512, 512, 3, 1, 1, 3), (2, 2),
            (512, 512, 3, 1, 1, None), (512, 512, 3, 1, 1, None), (512, 512, 3, 1, 1, 4)],
}


def make_weights(net, seed=11):
    conv, lin = [], []
    for i, op in enumerate(o for o in ARCH[net] if len(o) == 6):
        cin, cout, k = op[:3]
        he = np.sqrt(2.0 / (cin * k * k))
        w = ((2.0 * hash_uniform(cout * cin * k * k, seed + 101 * i).astype(np.float64) - 1.0) * np.sqrt(3.0) * he).astype(np.float32)
        b = ((2.0 * hash_uniform(cout, seed + 101 * i + 50).astype(np.float64) - 1.0) * 0.05).astype(np.float32)
        conv.append((torch.from_numpy(w.reshape(cout, cin, k, k)), torch.from_numpy(b)))
    for l, c in enumerate(_lib.LPIPS_TAP_CHANNELS[net]):
        lin.append(torch.from_numpy(hash_uniform(c, seed + 7000 + l).astype(np.float32)))
    return conv, lin


def macs_per_image(net, H, W):
    total, h, w = 0, H, W
    for op in ARCH[net]:
        if len(op) == 6:
            cin, cout, k, s, p, _ = op
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
            total += h * w * cout * cin * k * k
        else:
            h, w = (h - op[0]) // op[1] + 1, (w - op[0]) // op[1] + 1
    return total


def torch_lpips(net, conv, lin, img, gt):
    """the rule of include/dsnerf.h as torch ops in float32 (what the lpips package runs): [F,H,W,3] BGR stacks -> [F] float32"""
    shift = torch.tensor([-0.030, -0.088, -0.188], device=img.device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=img.device).view(1, 3, 1, 1)
    x = torch.cat([img, gt.float()]).permute(0, 3, 1, 2)
    x = ((2.0 * x - 1.0).flip(1) - shift) / scale
    taps, ci = [None] * 5, 0
    for op in ARCH[net]:
        if len(op) == 6:
            x = torch.relu(F.conv2d(x, conv[ci][0], conv[ci][1], stride=op[3], padding=op[4]))
            ci += 1
            if op[5] is not None:
                taps[op[5]] = x
        else:
            x = F.max_pool2d(x, op[0], op[1])
    n, total = img.shape[0], 0.0
    for f, w in zip(taps, lin):
        f = f / (torch.sqrt((f * f).sum(1, keepdim=True)) + 1e-10)
        total = total + (w.view(1, -1, 1, 1) * (f[:n] - f[n:]) ** 2).sum(1).mean((1, 2))
    return total


def quartiles(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4), "q75_ms": round(float(q[2]), 4), "n": len(ms)}


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


def alternate(variants, blocks, iters, warmup=3):
    for fn in variants.values():
        timed(fn, warmup)
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            ms[k] += timed(fn, iters)
    return {k: quartiles(v) for k, v in ms.items()}


def conv_share(fn):
    """the convolution kernel's share of the call's kernel time, from torch.profiler's device activity (None where it records none)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        conv = whole = 0.0
        for e in prof.events():
            if "k_lpips" in e.name:
                t = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
                whole += t
                conv += t if "k_lpips_conv" in e.name else 0.0
        return round(conv / whole, 4) if whole > 0 else None
    except Exception:          # noqa: BLE001  (the share is a by-product: the times stand without it)
        return None


def write(res, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-share", dest="share", action="store_false", help="skip the profiler pass that gives the convolution kernel's share")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--nets", nargs="*", default=["alex", "vgg"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    res = {"metric": "lpips_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "blocks": args.blocks, "iters_per_block": args.iters,
           "timing": "HIP events around each whole call, variants in alternating blocks after 3 warm-up calls each",
           "variants": {"call": "_lib.lpips(net, packed, img, gt): device stacks in, float64 distances on the device out",
                        "torch": "the same rule as torch ops in float32 (F.conv2d, F.max_pool2d, the framework's convolution library)"},
           "split_fp16_ceiling_tflops": round(SPLIT_CEILING_TFLOPS, 1), "workspace_cap_bytes": _lib.LPIPS_WORKSPACE_CAP,
           "not_measured": "the lpips package itself (not installed), the upload of the ground truth, more than one GPU", "items": {}}
    for net in args.nets:
        conv, lin = make_weights(net)
        packed = _lib.lpips_pack(net, conv, lin, dev)
        conv_d = [(w.to(dev), b.to(dev)) for w, b in conv]
        lin_d = [w.to(dev) for w in lin]
        for S in args.sizes:
            for n in args.frames:
                u = torch.from_numpy(hash_uniform(n * S * S * 3, 5).reshape(n, S, S, 3)).to(dev)
                v = torch.from_numpy(hash_uniform(n * S * S * 3, 6).reshape(n, S, S, 3)).to(dev)
                gt = (0.5 + 0.5 * torch.sin(torch.arange(S, device=dev, dtype=torch.float32) * 0.05).view(1, S, 1, 1) * u).double()
                img = torch.clamp(gt.float() + 0.3 * (2.0 * v - 1.0), 0.0, 1.0)
                del u, v
                ours, _, status = _lib.lpips(net, packed, img, gt)
                with torch.no_grad():
                    theirs = torch_lpips(net, conv_d, lin_d, img, gt)
                rel = float(((ours - theirs.double()).abs() / theirs.double()).max())
                assert int(status.abs().sum()) == 0 and rel < 1e-4, (net, S, n, rel)

                def call():
                    return _lib.lpips(net, packed, img, gt)

                def ref():
                    with torch.no_grad():
                        return torch_lpips(net, conv_d, lin_d, img, gt)

                variants = {"call": call, "torch": ref}
                alternate(variants, 1, 3)                 # not recorded: the clocks come up from idle during the first launches
                q = alternate(variants, args.blocks, args.iters)
                macs = 2 * n * macs_per_image(net, S, S)
                q.update(macs=macs, relative_difference_of_the_variants=float(f"{rel:.3e}"),
                         call_tflops=round(2e-9 * macs / q["call"]["median_ms"], 2),
                         call_fraction_of_split_ceiling=round(2e-9 * macs / q["call"]["median_ms"] / SPLIT_CEILING_TFLOPS, 4),
                         torch_tflops=round(2e-9 * macs / q["torch"]["median_ms"], 2),
                         call_over_torch=round(q["call"]["median_ms"] / q["torch"]["median_ms"], 3),
                         frames_per_chunk=_lib._lpips_chunk(net, n, S, S))
                res["items"][f"{net}_{S}_F{n}"] = q
                print(f"{net} {S} F={n}: {json.dumps(q)}", flush=True)
                write(res, args.out)
                q["conv_kernel_share_of_call"] = conv_share(call) if args.share else None
                write(res, args.out)
                del img, gt, ours, theirs
                torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
