"""TEST INFRASTRUCTURE: the decomposition maps of dsn_render_rays_maps restated in float64 numpy from per-sample arrays (the role
mc_restate.py and ssim_oracle.py play for their features).

With w [R,S] the compositing weights (utils/nerf_net_utils.py:18-51), e [R,S,3] the essence, n [R,S,3] the unit world normal and
L [K,R,S] the light factor ELU + 1 of K lights, summed over the listed samples (`listed` [R,S] bool; None: every sample):

    albedo[r]     = sum_i w_i e_i            [R,3]
    normal[r]     = sum_i w_i n_i            [R,3]   (not renormalised)
    shading[k][r] = sum_i w_i L_{k,i}        [K,R]
    color[k][r]   = sum_i w_i L_{k,i} e_i    [K,R,3]

A sample that is not listed contributes 0 whatever its arrays hold (NaN and inf included: the arrays of a frame hold rubbish there).
"""
import numpy as np


def listed_samples(sigma, transparent):
    """the one-pass shading list of a frame: not transparent and sigma > 0"""
    sigma = np.asarray(sigma, np.float64)
    return (sigma > 0) & ~np.asarray(transparent).astype(bool).reshape(sigma.shape)


def maps(weights, essence, n_w, light, listed=None):
    w = np.asarray(weights, np.float64)
    R, S = w.shape
    e = np.asarray(essence, np.float64).reshape(R, S, 3)
    n = np.asarray(n_w, np.float64).reshape(R, S, 3)
    L = np.asarray(light, np.float64).reshape(-1, R, S)
    on = np.ones((R, S), bool) if listed is None else np.asarray(listed).astype(bool).reshape(R, S)
    w = np.where(on, w, 0.0)
    e = np.where(on[..., None], e, 0.0)
    n = np.where(on[..., None], n, 0.0)
    L = np.where(on[None], L, 0.0)
    return {
        "albedo": (w[..., None] * e).sum(1),
        "normal": (w[..., None] * n).sum(1),
        "shading": (w[None] * L).sum(2),
        "color": (w[None, ..., None] * L[..., None] * e[None]).sum(2),
    }


def weighed_max(essence, light, listed):
    """(largest |e| over the channels, largest L) of the listed samples - what out_max reports for a one-pass frame; (0, 0) for none"""
    on = np.asarray(listed).astype(bool).reshape(-1)
    e = np.abs(np.asarray(essence, np.float64).reshape(-1, 3))[on]
    L = np.asarray(light, np.float64).reshape(-1, on.size)[:, on]
    return (float(e.max()) if e.size else 0.0, float(L.max()) if L.size else 0.0)
