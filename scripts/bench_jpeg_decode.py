#!/usr/bin/env python3
"""Baseline JPEG decoding on the device (dsnerf_amd.jpeg.decode: dsn_jpeg_decode) against the path a user has without it.
    python scripts/bench_jpeg_decode.py [--blocks 5] [--iters 20] [--out profiles/jpeg_decode_bench.json]
    python scripts/bench_jpeg_decode.py --kernels 20          (only 20 calls at 1024 x 1024, F = 1: for a kernel trace)
Files: quality 95, 4:2:0, S = 512 and 1024, F = 1 and 16 - a frame rendered from the w4 parameters (at 1024 the 512 frame enlarged
bilinearly on the device) and a uniform-noise frame, written by the project's own encoder (byte for byte Pillow's files).  Every frame
is compared with Pillow's decode of the same file before anything is timed (skipped without Pillow).
    call      _lib.jpeg_decode on files that are in HBM already (JpegdBatch built before): HIP events around the whole call, which
              includes its one status copy per group of rounds
    decode    jpeg.decode(files): wall time from `bytes` on the host to the uint8 tensor on the device - header parsing, the upload of
              the file bytes and the descriptors, the call, the status copy
    host      what a user does today: Pillow's decode (libjpeg-turbo) per file on one CPU thread, then the upload of the pixels: WALL
              time, a time reference of another kind; skipped without Pillow
    bits      the call at subseq_bits 512 / 1024 / 2048 on the 1024 x 1024 rendered frame, F = 1: the default is the lowest median
The variants run in alternating blocks after a warm-up; medians with the quartiles.  `rounds`: the synchronisation rounds the frames
took.  Not measured: the ZJU-MoCap and Human3.6M files themselves (they are not on these machines; who wrote them, with which sampling,
tables and restart settings, is unknown), a cv2.imread time (OpenCV is not a dependency), more than one GPU, the disk."""
import argparse
import io
import json
import os
import platform
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
from bench_jpeg import alternate, rendered_frame, timed_events, timed_wall  # noqa: E402
from dsnerf_amd import _lib, jpeg  # noqa: E402


def host_path(files, dev):
    from PIL import Image
    return torch.stack([torch.from_numpy(np.asarray(Image.open(io.BytesIO(f)))) for f in files]).to(dev)


def batch_of(files):
    return _lib.JpegdBatch(files, [_lib.jpeg_parse(f)[0] for f in files])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    q = args.quality
    base = rendered_frame(512, 64, args.weights)
    big = torch.nn.functional.interpolate(base.permute(2, 0, 1)[None], size=(1024, 1024), mode="bilinear",
                                          align_corners=False)[0].permute(1, 2, 0).contiguous()
    if args.kernels:
        b = batch_of(jpeg.encode(big[None], quality=q))
        ws = b.workspace()
        for _ in range(args.kernels):
            _lib.jpeg_decode(b, workspace=ws)
        torch.cuda.synchronize()
        return
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = None
    res = {"metric": "jpeg_decode_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "pillow": pillow, "quality": q, "subsampling": "420", "blocks": args.blocks,
           "iters_per_block": args.iters, "default_subseq_bits": _lib.JPEGD_SUBSEQ_BITS, "rounds_per_group": _lib.JPEGD_ROUNDS,
           "timing": "call: HIP events around each whole call (its status copy included); decode / host: wall time with a device "
                     "synchronisation on both sides; variants in alternating blocks after 5 warm-up calls each (host: a quarter of the "
                     "iterations)",
           "variants": {"call": "_lib.jpeg_decode(batch): dsn_jpeg_decode on files already in HBM, pixels stay on the device",
                        "decode": "jpeg.decode(files): parse, upload of the file bytes, the call, the status copy",
                        "host": "Pillow (libjpeg-turbo) per file on one CPU thread, then the upload of the pixels: a time reference of "
                                "another kind"},
           "not_measured": "the ZJU-MoCap and Human3.6M files themselves (not on these machines; their writer, sampling, tables and "
                           "restart settings are unknown), cv2.imread (OpenCV is not installed), more than one GPU, the disk",
           "items": {}}
    gen = torch.Generator(dev).manual_seed(1)
    for S in (512, 1024):
        img = base if S == 512 else big
        noise = torch.rand(S, S, 3, device=dev, generator=gen)
        for content, frame in (("rendered_" + args.weights, img), ("noise", noise)):
            one = jpeg.encode(frame[None], quality=q)
            for F in (1, 16):
                files = one * F
                batch = batch_of(files)
                ws = batch.workspace()
                out, st, rd, host = _lib.jpeg_decode(batch, workspace=ws)
                assert not host[0].any(), "a frame came back with a status bit"
                if pillow:
                    assert torch.equal(out, host_path(files, dev).flip(-1)), "the device's pixels are not Pillow's"
                variants = {"call": (lambda: _lib.jpeg_decode(batch, workspace=ws), timed_events, 1),
                            "decode": (lambda: jpeg.decode(files), timed_wall, 1)}
                if pillow:
                    variants["host"] = (lambda: host_path(files, dev), timed_wall, 4)
                alternate(variants, 1, 8)                  # not recorded: the clocks come up from idle during the first launches
                r = alternate(variants, args.blocks, args.iters)
                r.update(file_bytes=len(files[0]), pixel_bytes=S * S * 3, rounds=int(host[1].max()), equals_pillow=bool(pillow))
                if pillow:
                    r["host_over_decode"] = round(r["host"]["median_ms"] / r["decode"]["median_ms"], 2)
                res["items"][f"{S}_{content}_F{F}"] = r
    batch = batch_of(jpeg.encode(big[None], quality=q))
    ws = batch.workspace()
    variants = {str(b): ((lambda b=b: _lib.jpeg_decode(batch, b, workspace=ws)), timed_events, 1) for b in (512, 1024, 2048)}
    alternate(variants, 1, 8)
    r = alternate(variants, args.blocks, args.iters)
    for b in (512, 1024, 2048):
        r[str(b)]["rounds"] = int(_lib.jpeg_decode(batch, b, workspace=ws)[3][1].max())
    res["subseq_bits_1024_rendered_F1"] = r
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
