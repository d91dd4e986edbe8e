#!/usr/bin/env python3
"""Baseline JPEG on the device (dsnerf_amd.jpeg.encode_device: dsn_jpeg_encode) against the path a user has without it, and against
the call's byte floor.
    python scripts/bench_jpeg.py [--blocks 5] [--iters 20] [--out profiles/jpeg_bench.json]
    python scripts/bench_jpeg.py --kernels 20          (only 20 calls at 512 x 512, F = 1: for a kernel trace)
Frames: float32 [F, S, S, 3] on the device, S = 512 and 1024, F = 1 and 16, quality 95, 4:2:0 - a frame rendered from the w4 parameters
(repeated F times; at 1024 the 512 frame enlarged bilinearly on the device) and a uniform-noise frame, the encoder's worst case.
    call      jpeg.encode_device(frames): HIP events around the whole call, nothing copied back
    stages    _lib.jpeg_coefficients and _lib.jpeg_scan alone (HIP events): the split of the call into its two halves
    encode    jpeg.encode(frames): wall time including the two device->host copies, F files as bytes
    host      what a user does today: frames.cpu(), * 255, round, uint8, Pillow's encoder (libjpeg-turbo) per frame: WALL time on the
              host, a time reference of another kind (one CPU thread, a copy of 12 bytes per pixel first); skipped without Pillow
The variants run in alternating blocks after a warm-up; medians with the quartiles.  Byte floor of the call: 12 bytes per pixel read,
the int16 coefficients written and read once, the files written, over the 8.0 TB/s of the HBM's specification.
Not measured: a cv2.imwrite time (OpenCV is not a dependency), more than one GPU, the disk."""
import argparse
import io
import json
import os
import platform
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import dsnerf_amd  # noqa: E402
from dsnerf_amd import _lib, jpeg, synth  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def quartiles(ms):
    q = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 5), "q25_ms": round(float(q[0]), 5), "q75_ms": round(float(q[2]), 5), "n": len(ms)}


def timed_events(fn, iters):
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def timed_wall(fn, iters):
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return out


def alternate(variants, blocks, iters, warmup=5):
    for fn, timer, div in variants.values():
        timer(fn, warmup)
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for k, (fn, timer, div) in variants.items():
            ms[k] += timer(fn, max(2, iters // div))
    return {k: quartiles(v) for k, v in ms.items()}


def rendered_frame(hw, S, weights):
    """coarse_color [hw, hw, 3] float32 of the synthetic body from the given parameters, on the device"""
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
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    batch = {"ray_o": T(rays["ray_o"])[None], "ray_d": T(rays["ray_d"])[None], "near": T(rays["near"])[None], "far": T(rays["far"])[None],
             "xyz": T(xyz)[None], "poses": T(synth.make_poses(seed=5))[None], "Th": torch.zeros(1, 1, 3, device=dev),
             "frame": torch.tensor([5]), "img": torch.zeros(1, hw, hw, 3, device=dev),
             "mask_at_box": torch.ones(1, hw * hw, dtype=torch.bool, device=dev)}
    return r.render_view(batch, device_output=True)["coarse_color"].to(torch.float32).contiguous()


def host_path(frames, quality):
    from PIL import Image
    a = frames.cpu().numpy()
    out = []
    for f in a:
        lv = np.clip(np.rint(f * np.float32(255.0)), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(lv[..., ::-1]).save(b, "JPEG", quality=quality, subsampling=2, optimize=False)
        out.append(b.getvalue())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    q = args.quality
    base = rendered_frame(512, 64, args.weights)
    if args.kernels:
        x = base[None].contiguous()
        for _ in range(args.kernels):
            jpeg.encode_device(x, quality=q)
        torch.cuda.synchronize()
        return
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = None
    res = {"metric": "jpeg_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "pillow": pillow, "quality": q, "subsampling": "420", "blocks": args.blocks,
           "iters_per_block": args.iters,
           "timing": "call / stages: HIP events around each whole call; encode / host: wall time with a device synchronisation on both "
                     "sides; variants in alternating blocks after 5 warm-up calls each (host: a quarter of the iterations)",
           "variants": {"call": "jpeg.encode_device(frames): dsn_jpeg_encode, results stay on the device",
                        "coefficients": "_lib.jpeg_coefficients alone", "scan": "_lib.jpeg_scan alone on those coefficients",
                        "encode": "jpeg.encode(frames): the call plus two device->host copies, F files as bytes",
                        "host": "frames.cpu(), x 255, rint, uint8, Pillow (libjpeg-turbo) per frame on one CPU thread: a time reference "
                                "of another kind"},
           "byte_floor": "12 B per pixel read, int16 coefficients written and read once, the files written, over 8.0 TB/s",
           "not_measured": "cv2.imwrite (OpenCV is not installed), more than one GPU, the disk", "items": {}}
    gen = torch.Generator(dev).manual_seed(1)
    for S in (512, 1024):
        img = base if S == 512 else torch.nn.functional.interpolate(base.permute(2, 0, 1)[None], size=(S, S), mode="bilinear",
                                                                    align_corners=False)[0].permute(1, 2, 0).contiguous()
        noise = torch.rand(S, S, 3, device=dev, generator=gen)
        for content, frame in (("rendered_" + args.weights, img), ("noise", noise)):
            for F in (1, 16):
                x = frame[None].expand(F, S, S, 3).contiguous()
                files = jpeg.encode(x, quality=q)
                if pillow:
                    assert files == host_path(x[:1], q) * F, "the device's file is not Pillow's"
                coef, st = _lib.jpeg_coefficients(x, _lib.JPEG_420, q)
                variants = {"call": (lambda: jpeg.encode_device(x, quality=q), timed_events, 1),
                            "coefficients": (lambda: _lib.jpeg_coefficients(x, _lib.JPEG_420, q), timed_events, 1),
                            "scan": (lambda: _lib.jpeg_scan(coef, S, S, _lib.JPEG_420, q, status_in=st), timed_events, 1),
                            "encode": (lambda: jpeg.encode(x, quality=q), timed_wall, 1)}
                if pillow:
                    variants["host"] = (lambda: host_path(x, q), timed_wall, 4)
                alternate(variants, 1, 8)                  # not recorded: the clocks come up from idle during the first launches
                r = alternate(variants, args.blocks, args.iters)
                nb = _lib.jpeg_blocks(S, S, _lib.JPEG_420)
                floor = F * (S * S * 12 + 2 * nb * 128) + sum(len(f) for f in files)
                floor_ms = 1e3 * floor / HBM_BYTES_PER_S
                r.update(file_bytes=len(files[0]), byte_floor_bytes=floor, byte_floor_ms=round(floor_ms, 5),
                         call_over_floor=round(r["call"]["median_ms"] / floor_ms, 2), equals_pillow=bool(pillow))
                if pillow:
                    r["host_over_encode"] = round(r["host"]["median_ms"] / r["encode"]["median_ms"], 2)
                res["items"][f"{S}_{content}_F{F}"] = r
                del x, coef, st
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
