"""Shared helpers for the test-suite (test infrastructure only)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:      # (conftest.py does this for pytest; the probe scripts import helpers directly)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
CASES = ["small_eval", "small_train", "small_novel", "small_rot", "full_eval"]
# the same stage / end-to-end cases on two more parameter sets (tests/golden/make_golden.py --other-weights):
#   _w2: TRAINED by the real reference (tests/golden/make_weights_w2.py; weights_w2.npz) - larger, non-uniform layer scales
#   _w3: hash-generated with init gain 3.5 - |sigma| ~ 1e3, |d sigma/dx| ~ 2e5, activations ~ 1e2
#   _w4: CONVERGED on the full-size synthetic body by this repo's HIP trainer on the MI355X (scripts/train_w4.py, 24 000 steps,
#        held-out PSNR 26-27 dB; weights_w4.npz) - a bimodal field (sigma in [-316, 1013]: << 0 outside, >> 0 inside), acc 0 / 1
W_CASES = ["small_eval_w2", "small_train_w2", "full_eval_w2", "small_eval_w3", "small_train_w3", "full_eval_w3",
           "small_eval_w4", "small_train_w4", "full_eval_w4"]
# the SMPL-like body (synth.make_body(nonuniform=True): dense caps at head / hands / feet) through the real reference
# (tests/golden/make_golden.py --nonuniform): rays of the regular grid + the rays passing closest to the hands and the head
NU_CASES = ["full_eval_nu", "full_eval_nu_w4"]
ALL_CASES = CASES + W_CASES + NU_CASES


from cases import GOLDEN, code_for, load, state  # noqa: E402,F401  (oracle/cases.py: shared with __graft_entry__.smoke())


def ref_tol(g, key, base, rel=4e-6):
    """absolute tolerance on array `key` of a golden case: `base` (the bar: 1e-4 on sigma / RGB), or `rel` x the largest
    magnitude in the array where float32 itself is coarser than the bar.  rel = 4e-6: two independent float32
    implementations of the network (the reference and the C oracle, same inputs) differ by 0.3e-6 .. 1.4e-6 of max |sigma|
    on all three parameter sets (measured: sigma 8e-6 at |sigma| <= 9, 2.7e-5 at 64, 1.5e-3 at 1400) - the float32-vs-float64
    companions of the fixtures are NOT a usable floor here, they differ in the canonical points themselves."""
    m = float(np.abs(g[key]).max())
    return base if m <= 100.0 else max(base, rel * m)     # the bar itself wherever the magnitudes leave float32 room for it


def light_kw(g):
    kw = {}
    if "light_center" in g.files:
        kw["light_shift"] = g["light_center"] - g["Th"]
    if "rot" in g.files:
        kw["rot"] = g["rot"]
        kw["rot_center"] = g["rot_center"][0, :2]
    return kw


def per_point_dirs(g):
    S = int(g["S"])
    return np.repeat(g["ray_d"][:, None, :], S, 1).reshape(-1, 3)


def workspace_arrays(ws, N):
    """per-sample arrays of a render workspace of N = R x S samples, by dsn_carve's layout (csrc/dsn_api.hip): transparent, x_c, sigma,
    n_w, colour - clones, as torch tensors on the workspace's device"""
    import torch
    al = lambda n: (n + 255) // 256 * 256      # noqa: E731
    b = ws.buf
    p = 8192 + al(4 * N)
    out = {"transparent": b[p:p + N].clone()}
    p += al(N) + al(4 * N)
    out["x_c"] = b[p:p + 12 * N].view(torch.float32).reshape(N, 3).clone()
    p += al(12 * N)
    out["sigma"] = b[p:p + 4 * N].view(torch.float32).clone()
    p += al(4 * N)
    out["n_w"] = b[p:p + 12 * N].view(torch.float32).reshape(N, 3).clone()
    p += 12 * N
    out["colour"] = b[p:p + 12 * N].view(torch.float32).reshape(N, 3).clone()
    return out


def maxdiff(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.nanmax(np.abs(a - b))) if a.size else 0.0
