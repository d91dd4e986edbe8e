"""the cameras of tests/golden/camera_rays_edges.npz (tests/golden/make_golden_rays.py) and the bars both camera-ray test files use"""
import os

import numpy as np

import camera_rays_restate as CR
from helpers import GOLDEN

EDGES = np.load(os.path.join(GOLDEN, "camera_rays_edges.npz"))
NAMES = [str(n) for n in EDGES["names"]]
CONVENTIONS = (CR.ZJU, CR.H36M)


def camera(name, convention):
    g = EDGES
    return (g[f"{name}:K"], g[f"{name}:R"], g[f"{name}:T"], g[f"{name}:{convention}:bounds"], int(g[f"{name}:H"]), int(g[f"{name}:W"]))


def recorded(name, convention):
    return tuple(EDGES[f"{name}:{convention}:{k}"] for k in ("ray_o", "ray_d", "near", "far", "mask"))


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def within_bars(a, b):
    """the bars of test_gpu_stages.py::test_camera_rays: no value further than 1 float32 ulp of the array's largest magnitude from
    the reference, and fewer than 1 % of the values different at all (the adjugate against numpy's LU inverse)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.size == 0 or not np.abs(b).max() > 0:
        return np.array_equal(a, b)
    ulp = float(np.spacing(np.float32(np.abs(b).max())))
    return float(np.abs(a.astype(np.float64) - b).max()) <= ulp and np.mean(a != b) < 0.01
