"""Writes tests/golden/lpips_golden.json and lpips_errors.json from the restatement alone (tests/lpips_restate.py; CPU, a minute):

    python tests/golden/make_golden_lpips.py

lpips_golden.json: per net and case "HxW" (lpips_restate.SIZES and 512x512) the float64 distance and per-tap terms of
make_pair(H, W, seed) - an image and the same image plus hash noise of amplitude 0.3 - with make_weights(net).
lpips_errors.json: per net, what the restatement's float32 twin differs from float64 by, pooled (maximum) over the cases: per tap
max|f32 - f64| / max|f64| over both images, and the scalar's relative error.  The GPU tests' bars are multiples of these."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_restate as R  # noqa: E402

BIG = (512, 512)


def case_seed(net, H, W):
    return 1000 + 7 * H + W + (0 if net == "alex" else 500)


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    golden, errors = {}, {}
    for net in ("alex", "vgg"):
        w = R.make_weights(net)
        golden[net] = {}
        tap_err, scalar_err = [0.0] * 5, 0.0
        for H, W in R.SIZES[net] + [BIG]:
            seed = case_seed(net, H, W)
            img, gt = R.make_pair(H, W, seed)
            t64 = [R.features(net, w, s[None], torch.float64) for s in (img, gt)]
            t32 = [R.features(net, w, s[None], torch.float32) for s in (img, gt)]
            out64, lay64 = R.head(t64[0], t64[1], w["lin"])
            out32, _ = R.head(t32[0], t32[1], w["lin"])
            for l in range(5):
                for a, b in zip(t32, t64):
                    tap_err[l] = max(tap_err[l], float((a[l].double() - b[l]).abs().max() / b[l].abs().max()))
            scalar_err = max(scalar_err, abs(float(out32[0]) - float(out64[0])) / float(out64[0]))
            golden[net][f"{H}x{W}"] = {"seed": seed, "out": float(out64[0]), "layers": [float(v) for v in lay64[0]],
                                       "max_activation": max(float(t.max()) for t in t64[0] + t64[1])}
            print(net, H, W, float(out64[0]), flush=True)
        errors[net] = {"tap": tap_err, "scalar": scalar_err}
    with open(os.path.join(HERE, "lpips_golden.json"), "w") as f:
        json.dump(golden, f, indent=1)
    with open(os.path.join(HERE, "lpips_errors.json"), "w") as f:
        json.dump(errors, f, indent=1)
    print(json.dumps(errors, indent=1))


if __name__ == "__main__":
    main()
