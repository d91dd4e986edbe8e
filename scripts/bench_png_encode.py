#!/usr/bin/env python3
"""PNG encoding on the device (dsnerf_amd.png: dsn_png_encode) against the path a user has without it.
    python scripts/bench_png_encode.py [--blocks 3] [--iters 10] [--out profiles/png_encode_bench.json]
Frames: the rendered synthetic body (weights w4) and uniform noise at 512 x 512 and 1024 x 1024, F = 1 and 16, float32 B, G, R in HBM.
Every file is decoded to its levels (png.decode on the device against the levels computed by torch) before anything is timed.
    call      png.encode_device(frames): HIP events around the whole call - filter, Adler-32, matches, codes, emission, scan, compaction,
              container; the files stay on the device
    encode    png.encode(frames): wall time, the call plus its two device->host copies, F files as bytes
    host1 / host   a time reference OF ANOTHER KIND: frames.cpu(), x 255, rint, uint8, then Pillow's PNG writer per frame on ONE CPU thread at
              compress_level 1 / at its default (6): WALL time
    set       test.py's five files of one frame as Renderer.save_test_views encodes them (colour and ground truth, the two maps as
              three equal channels, the pair side by side: three encoder calls), wall time without the disk
The variants run in alternating blocks after a warm-up; medians with the quartiles.  Sizes: the file against zlib on the SAME filtered
bytes (level 1 with Z_RLE, level 6, level 6 restarted at every chunk) and against Pillow's default file.  The chunk sweep (4, 8, 16 and
32 KiB) reports time and size; DSN_PNGE_CHUNK_DEFAULT was chosen from it.  Not measured: cv2.imwrite (OpenCV is not installed), more than
one GPU, the disk."""
import argparse
import io
import json
import os
import platform
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
from bench_jpeg import HBM_BYTES_PER_S, alternate, rendered_frame, timed_events, timed_wall  # noqa: E402
from dsnerf_amd import _lib, png  # noqa: E402


def levels_of(x):
    return torch.clamp(torch.round(x * 255.0), 0, 255).to(torch.uint8)


def host_path(frames, level):
    from PIL import Image
    out = []
    for f in frames.cpu().numpy():
        lv = np.clip(np.rint(f * np.float32(255.0)), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        kw = {} if level is None else {"compress_level": level}
        Image.fromarray(lv[..., ::-1] if lv.ndim == 3 else lv).save(b, "PNG", **kw)
        out.append(b.getvalue())
    return out


def zlib_sizes(raw, chunk):
    """sizes of zlib streams of the same filtered bytes"""
    rle = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return {"zlib1_rle": len(rle.compress(raw) + rle.flush()), "zlib6": len(zlib.compress(raw, 6)),
            "zlib6_per_chunk": sum(len(zlib.compress(raw[i:i + chunk], 6)) for i in range(0, len(raw), chunk))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--weights", default="w4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = None
    base = rendered_frame(512, 64, args.weights)
    C0 = _lib.PNGE_CHUNK_DEFAULT
    res = {"metric": "png_encode_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "pillow": pillow, "chunk_default": C0, "blocks": args.blocks, "iters_per_block": args.iters,
           "timing": "call: HIP events around each whole call; encode / host1 / host / set: wall time with a device synchronisation on both "
                     "sides; variants in alternating blocks after 5 warm-up calls each (host1 / host: an eighth of the iterations)",
           "variants": {"call": "png.encode_device(frames): dsn_png_encode, results stay on the device",
                        "encode": "png.encode(frames): the call plus two device->host copies, F files as bytes",
                        "host1": "frames.cpu(), levels, Pillow's PNG writer per frame on one CPU thread, compress_level 1: a time reference of "
                                 "another kind", "host": "the same at Pillow's default level",
                        "set": "the five files of one frame in save_test_views' three encoder calls, without the disk"},
           "byte_floor": "12 B per pixel read, the raw stream and its 2 B per byte match records written and read once, the files written, "
                         "over 8.0 TB/s",
           "not_measured": "cv2.imwrite (OpenCV is not installed), more than one GPU, the disk", "items": {}, "chunk_sweep": {}}
    gen = torch.Generator(dev).manual_seed(1)
    for S in (512, 1024):
        img = base if S == 512 else torch.nn.functional.interpolate(base.permute(2, 0, 1)[None], size=(S, S), mode="bilinear",
                                                                    align_corners=False)[0].permute(1, 2, 0).contiguous()
        noise = torch.rand(S, S, 3, device=dev, generator=gen)
        for content, frame in (("rendered_" + args.weights, img), ("noise", noise)):
            for F in (1, 16):
                x = frame[None].expand(F, S, S, 3).contiguous()
                files = png.encode(x)
                assert torch.equal(png.decode(files), levels_of(x)), "a file does not decode to its levels"
                variants = {"call": (lambda: png.encode_device(x), timed_events, 1), "encode": (lambda: png.encode(x), timed_wall, 1)}
                if pillow:
                    variants["host1"] = (lambda: host_path(x, 1), timed_wall, 8)
                    variants["host"] = (lambda: host_path(x, None), timed_wall, 8)
                alternate(variants, 1, 8, warmup=2)          # not recorded: the clocks come up from idle during the first launches
                r = alternate(variants, args.blocks, args.iters, warmup=2)
                raw = _lib.png_filter(x[:1], _lib.PNGE_COLOUR)[0][0].cpu().numpy().tobytes()
                floor = F * (S * S * 12 + 2 * 3 * len(raw)) + sum(len(f) for f in files)
                floor_ms = 1e3 * floor / HBM_BYTES_PER_S
                r.update(file_bytes=len(files[0]), raw_bytes=len(raw), byte_floor_bytes=floor, byte_floor_ms=round(floor_ms, 5),
                         call_over_floor=round(r["call"]["median_ms"] / floor_ms, 2), **zlib_sizes(raw, C0))
                if pillow:
                    r["pillow_default_bytes"] = len(host_path(x[:1], None)[0])
                    r["pillow_level1_bytes"] = len(host_path(x[:1], 1)[0])
                    r["host_over_encode"] = round(r["host"]["median_ms"] / r["encode"]["median_ms"], 2)
                    r["host1_over_encode"] = round(r["host1"]["median_ms"] / r["encode"]["median_ms"], 2)
                res["items"][f"{S}_{content}_F{F}"] = r
                if content != "noise":
                    sweep = {}
                    for C in (4096, 8192, 16384, 32768):
                        one = png.encode(x[:1], chunk=C)
                        assert torch.equal(png.decode(one), levels_of(x[:1]))
                        t = alternate({"call": (lambda C=C: png.encode_device(x, chunk=C), timed_events, 1)}, args.blocks, args.iters, warmup=2)
                        sweep[str(C)] = {"call": t["call"], "file_bytes": len(one[0])}
                    res["chunk_sweep"][f"{S}_{content}_F{F}"] = sweep
                del x
        # test.py's five files of one frame
        depth, acc = img[..., 0].contiguous(), img[..., 1].contiguous()
        flat, maps, pair = torch.stack([img, noise * 0.5]), torch.stack([depth, acc]), torch.cat([img, noise * 0.5], 1)[None].contiguous()

        def five():
            return png.encode(flat) + png.encode(maps, replicate=True) + png.encode(pair)
        got = five()
        assert torch.equal(png.decode(got[4]), levels_of(pair[0])) and torch.equal(png.decode(got[2])[..., 0], levels_of(depth))
        res["items"][f"{S}_test_views_set"] = dict(alternate({"set": (five, timed_wall, 1)}, args.blocks, args.iters, warmup=2),
                                                   file_bytes=[len(f) for f in got])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
