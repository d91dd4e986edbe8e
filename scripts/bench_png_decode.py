#!/usr/bin/env python3
"""PNG decoding on the device (dsnerf_amd.png: dsn_png_decode) against the path a user has without it.
    python scripts/bench_png_decode.py [--blocks 3] [--iters 12] [--out profiles/png_decode_bench.json]
Files: the three 1024 x 1024 label maps of tests/golden/png_pillow.npz (blobs of small labels, the masks' own shape, written by
Pillow as grey, palette and three-channel), 1 file and batches of 4, 16 and 64.  Every frame is compared with the recorded Pillow
pixels before anything is timed.
    call      _lib.png_decode(batch, first_channel=True) on files that are in HBM already (PngBatch built before): HIP events around the
              whole call - gather, inflate, Adler-32, unfilter, pixels; nothing is copied back
    stages    each stage alone on the workspace the call left (HIP events): where the time goes
    decode    png.decode_device(files, first_channel=True): wall time from `bytes` on the host to the uint8 mask on the device - chunk
              walk and CRCs, the upload of the file bytes and tables, the call
    host      what a user does today: Pillow's decode per file on ONE CPU thread, then the upload of the decoded mask: WALL time, the
              baseline (the parent commit has no device path); skipped without Pillow
The variants run in alternating blocks after a warm-up; medians with the quartiles.  Reported beside them: the inflated bytes per second
of one wave (raw bytes / the inflate stage's median at F = 1) and the smallest measured batch at which `call` is below `host`.
Not measured: the data sets' own mask files (they are not on these machines), cv2.imread / imageio (not installed), more than one GPU,
the disk."""
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
from bench_jpeg import alternate, timed_events, timed_wall  # noqa: E402
from dsnerf_amd import _lib, png  # noqa: E402

STAGES = (("gather", _lib.PNG_GATHER), ("inflate", _lib.PNG_INFLATE), ("adler", _lib.PNG_ADLER_STAGE), ("unfilter", _lib.PNG_UNFILTER),
          ("pixels", _lib.PNG_PIXELS))


def host_path(files, dev):
    from PIL import Image
    out = []
    for f in files:
        a = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[..., 2]          # cv2.imread(path)[..., 0]: the blue channel
        out.append(torch.from_numpy(np.ascontiguousarray(a)))
    return torch.stack(out).to(dev)


def batch_of(files):
    parsed = [_lib.png_parse(f) for f in files]
    return _lib.PngBatch(files, [p[0] for p in parsed], [p[1] for p in parsed])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no device, no number"
    dev = torch.device("cuda:0")
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = None
    G = np.load(os.path.join(ROOT, "tests", "golden", "png_pillow.npz"))
    res = {"metric": "png_decode_on_device", "device": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "hip": torch.version.hip, "pillow": pillow, "blocks": args.blocks, "iters_per_block": args.iters,
           "timing": "call / stages: HIP events around each whole call; decode / host: wall time with a device synchronisation on both "
                     "sides; variants in alternating blocks after 5 warm-up calls each (host: a quarter of the iterations)",
           "variants": {"call": "_lib.png_decode(batch, first_channel=True): dsn_png_decode on files already in HBM, the mask stays on the device",
                        "decode": "png.decode_device(files, first_channel=True): parse, upload of the file bytes and tables, the call",
                        "host": "Pillow per file on one CPU thread, then the upload of the decoded mask: the baseline"},
           "not_measured": "the data sets' own mask files (not on these machines), cv2.imread and imageio (not installed), more than one "
                           "GPU, the disk",
           "items": {}}
    for kind in ("L", "P", "RGB"):
        key = f"mask_{kind}_1024"
        one = G[f"png_{key}"].tobytes()
        want = G[f"rgb_{key}"][..., 2] if f"rgb_{key}" in G.files else G[f"px_{key}"] if G[f"px_{key}"].ndim == 2 else G[f"px_{key}"][..., 2]
        even = None
        for F in (1, 4, 16, 64):
            files = [one] * F
            batch = batch_of(files)
            ws = batch.workspace()
            out, st = _lib.png_decode(batch, "bgr", True, workspace=ws)
            assert not st.cpu().numpy().any(), "a frame came back with a status bit"
            assert all(np.array_equal(o, want) for o in out.cpu().numpy()), "the device's pixels are not Pillow's"
            variants = {"call": (lambda: _lib.png_decode(batch, "bgr", True, workspace=ws), timed_events, 1),
                        "decode": (lambda: png.decode_device(files, first_channel=True), timed_wall, 1)}
            for name, bit in STAGES:
                variants[name] = ((lambda bit=bit: _lib.png_decode(batch, "bgr", True, stages=bit, workspace=ws, out=out, status=st)), timed_events, 1)
            if pillow:
                variants["host"] = (lambda: host_path(files, dev), timed_wall, 4)
            alternate(variants, 1, 4)                      # not recorded: the clocks come up from idle during the first launches
            r = alternate(variants, args.blocks, args.iters)
            r.update(file_bytes=len(one), raw_bytes=batch.raw_bytes, stream_bytes=batch.max_stream)
            r["inflate_bytes_per_s_per_wave"] = round(batch.raw_bytes / (1e-3 * r["inflate"]["median_ms"]))
            if pillow:
                r["host_over_call"] = round(r["host"]["median_ms"] / r["call"]["median_ms"], 3)
                if even is None and r["call"]["median_ms"] < r["host"]["median_ms"]:
                    even = F
            res["items"][f"{kind}_F{F}"] = r
        res["items"][f"{kind}_break_even_batch"] = even          # the smallest of 1, 4, 16, 64 at which the call is below the host path; None: none
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
