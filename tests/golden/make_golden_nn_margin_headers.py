"""The grid headers the device builds for the meshes of tests/nn_margin_cases.py (nn_margin_headers.json).  Needs an MI355X:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nn_margin_headers.py

k_grid_params derives a level's cell size from the centroid box and the face count through cbrtf, which the device's library and the
host's round differently in the last place for about half of the inputs, so the cases are built on recorded headers.  They depend on
the placeholder mesh alone (nn_margin_cases.placeholder_mesh: the body + the final number of appended faces, all inside the body's
centroid box) - the probes placed later do not move the box.  Per body and level: lo [3], cell, inv_cell as float32 bit patterns,
n [3], and the face count F.  tests/test_gpu_nn_margins.py asserts that the device still builds exactly these.  Data only.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import nn_cases as N                      # noqa: E402
import nn_margin_cases as M               # noqa: E402
from helpers import state                 # noqa: E402


def main():
    from dsnerf_amd import _lib, synth
    dev = "cuda:0"
    pk = _lib.PackedParams(dev).update({k: torch.from_numpy(v) for k, v in state().items()})
    out = {}
    for nonuniform in (False, True):
        _, _, _, canon, xyz, faces = M.placeholder_mesh(nonuniform)
        sc = _lib.Scene(torch.from_numpy(canon), torch.from_numpy(faces), dev)
        sc.set_frame(pk, torch.from_numpy(xyz), torch.from_numpy(synth.make_poses()), 5)
        rec = {}
        for lv in N.LEVELS:
            h = N.read_header(sc, lv)
            assert h["ok"] == 1, (lv, h)
            rec[lv] = dict(lo=[int(x) for x in h["lo"].view(np.uint32)], cell=int(np.float32(h["cell"]).view(np.uint32)),
                           inv_cell=int(np.float32(h["inv_cell"]).view(np.uint32)), n=[int(x) for x in h["n"]], F=int(faces.shape[0]))
        out["nonuniform" if nonuniform else "uniform"] = rec
    with open(os.path.join(HERE, "nn_margin_headers.json"), "w") as f:
        f.write(json.dumps(out, separators=(",", ":")) + "\n")
    print("wrote nn_margin_headers.json")


if __name__ == "__main__":
    main()
