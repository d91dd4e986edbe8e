"""The CPU oracle's PER-ROW cotangents of the training backward (test infrastructure; no GPU needed).

oracle/train_oracle.py::render returns the graph nodes of the colour head and the lighting MLP; oracle_rows() takes
torch.autograd.grad of  L = sum(cotangent * output)  with respect to those nodes and to the 33 parameters in ONE backward, in
float32 or float64, so that every per-row array the device keeps in its gradient workspace (_lib.grad_rows) has a float64 twin.

Which node each device array is the cotangent of (read off csrc/dsn_train.hip):

  device array   node of the oracle          why
  d_sig [N]      sigma_node [N,1]            k_t_composite_adjoint*: ds = 0 on transparent rows and where raw <= 0 - the density head's
                                             output, in front of the transparent mask, the noise and the ReLU of the compositor
  d_col [N,3]    colour                      k_t_composite_adjoint*: w * d_rgb
  d_ess [N,3]    essence                     k_t_colour_adjoint: wl * d_col
  d_pre [N]      pre [N,1]                   k_t_colour_adjoint: (ess . d_col) * ELU'(pre) - in front of the ELU
  d_hl2 [N,128]  hl2_pre                     k_t_wcolsum<1>: hl2 > 0 ? d_pre * W4 : 0 - BEHIND the ReLU mask, i.e. the cotangent of the
                                             second layer's pre-activation (its column sum is lights_encoding.2.bias)
  d_hl1 [N,128]  hl1_pre                     lin16 / lin<EPI_MASK>: hl1 > 0 ? d_hl2 W2 : 0 - likewise, of the first layer's
  d_xl  [N,9]    li = (n_w, x_w, view)       k_t_light_first_bwd: d_hl1 W0; d_xl[:, :3] = d n_w (columns 3..8 reach no parameter)
  d_rr  [N,128]  rr_pre                      k_t_wcolsum<3>: rr > 0 ? d_ess W_rgb3 : 0 - behind the ReLU mask
  u     [N,3]    grad_sigma                  k_t_normal_adjoint: (d n_w / d g)^T d n_w - g reaches the loss through the normal only
  forward rows: sig = sigma_node, ess = essence, g = grad_sigma, n_w, xl = li, hl1 / hl2 / rr (after their ReLUs), pre, wl, col = colour,
  h6 = the trunk's last layer (after its ReLU).

So  sum d_pre = lights_encoding.4.bias,  d_pre^T hl2 = lights_encoding.4.weight,  d_hl2^T hl1 = lights_encoding.2.weight,
d_hl1^T li = lights_encoding.0.weight,  d_ess^T rr = rgb_net.3.weight,  d_rr^T h6 = rgb_net.1.weight,  sum d_sig =
density_net.0.bias (tests/test_row_cotangents_host.py holds the oracle to these in float64).

The cases are slices of the golden gradient fixtures, with the cotangents and the disparity rule of
test_gpu_train.oracle_case_errors (which takes both from here)."""
import functools

import numpy as np
import torch

import train_oracle as TO
from helpers import load, state

OUT_KEYS = ("color", "disp_map", "acc_map", "depth_map", "weights")
# device array -> oracle node (see the table above)
COTANGENT_NODES = {"d_sig": "sigma_node", "d_col": "colour", "d_ess": "essence", "d_pre": "pre", "d_hl2": "hl2_pre", "d_hl1": "hl1_pre",
                   "d_xl": "li", "d_rr": "rr_pre", "u": "grad_sigma"}
FORWARD_NODES = {"sig": "sigma_node", "ess": "essence", "g": "grad_sigma", "n_w": "n_w", "xl": "li", "hl1": "hl1", "hl2": "hl2",
                 "pre": "pre", "wl": "wl", "col": "colour", "rr": "rr", "h6": "h6"}
# the arrays the set-aside rule looks at and the device is judged on
COMPARED = ("d_sig", "d_col", "d_ess", "d_pre", "d_hl2", "d_hl1", "d_xl", "u", "pre", "n_w", "col")
# (weight, bias) <- (cotangent rows, input rows): the products of the lighting MLP and the colour head
PRODUCTS = {"lighting_mlp.lights_encoding.4": ("d_pre", "hl2"), "lighting_mlp.lights_encoding.2": ("d_hl2", "hl1"),
            "lighting_mlp.lights_encoding.0": ("d_hl1", "xl"), "nerf.rgb_net.3": ("d_ess", "rr"), "nerf.rgb_net.1": ("d_rr", "h6")}
LIGHT_TENSORS = tuple(f"lighting_mlp.lights_encoding.{k}.{w}" for k in (0, 2, 4) for w in ("weight", "bias"))

ROW_REL, ROW_FLOOR = 1e-3, 1e-6      # a row is "off" beyond 1e-3 of its own magnitude AND 1e-6 of the array's largest row magnitude
SET_ASIDE_CAP = 5e-3                 # share of the live rows the float32 oracle may be off on
# the named cases: (fixture, rays, samples, noise)
CASES = {"37x64": ("full_train_grads_s200", 37, 64, True), "37x100": ("full_train_grads_s200", 37, 100, True),
         "37x100-nonoise": ("full_train_grads_s200", 37, 100, False), "37x129": ("full_train_grads_s200", 37, 129, True),
         "128x128": ("full_train_grads_s200", 128, 128, True), "w4-128x128": ("full_train_grads_w4_s128", 128, 128, True)}


def load_case(name):
    """a gradient fixture as a dict.  The compact S > 64 cases (make_golden_grads.py --samples) keep only what cannot be regenerated:
    their body, 128 rays of the 32 x 32 view, targets and draws are rebuilt here from the seeds as the generator made them, and the
    draws are checked against the sums it kept"""
    g = dict(load(name).items())
    if "ray_o" in g:
        return g
    from dsnerf_amd import synth
    R, S, seed = int(g["rays"]), int(g["S"]), int(g["seed"])
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon)
    rays = synth.make_rays(32, 32, xyz, fit_box=True)
    sel = np.arange(0, 1024, 8)[:R]
    g.update(canonical_vertex=canon, faces=faces.astype(np.int32), xyz=xyz, poses=synth.make_poses(),
             ray_o=rays["ray_o"][sel], ray_d=rays["ray_d"][sel], near=rays["near"][sel], far=rays["far"][sel],
             target_rgb=synth.hash_uniform(R * 3, 91).reshape(R, 3).astype(np.float32),
             occupancy=(synth.hash_uniform(R, 92) > 0.5).astype(np.float32))
    torch.manual_seed(seed)                     # (the reference's draws: jitter, then noise, from the CPU generator)
    g["jitter"] = torch.rand(1, R, S).numpy()[0]
    g["noise"] = (torch.randn(R, S) * float(g["raw_noise_std"])).numpy()
    assert float(g["jitter"].astype(np.float64).sum()) == float(g["jitter_sum"])
    assert float(g["noise"].astype(np.float64).sum()) == float(g["noise_sum"])
    return g


def sliced_case(name, nrays, nsamp):
    """load_case(name) cut to its first nrays rays / nsamp samples per ray (None = all)"""
    g = load_case(name)
    if nrays is not None:                      # a ray count that is no multiple of the 32-point wave tiles / 128-point blocks
        for k in ("ray_o", "ray_d", "near", "far", "render:z_vals", "noise", "jitter"):
            g[k] = g[k][:nrays]
    if nsamp is not None:                      # 37 x 21 = 777 samples: not a multiple of 16 (the weight-gradient kernels' ragged tail)
        for k in ("render:z_vals", "noise", "jitter"):
            g[k] = np.ascontiguousarray(g[k][:, :nsamp])
    return g


def output_cotangents(R, S):
    """a float32 cotangent on every output of the render (colour, disp, acc, depth, weights); the disparity's is finished by
    oracle_loss, which knows the rays that hit something"""
    rng = np.random.default_rng(4)
    return {k: rng.standard_normal(s).astype(np.float32) for k, s in
            (("color", (R, 3)), ("disp_map", (R,)), ("acc_map", (R,)), ("depth_map", (R,)), ("weights", (R, S)))}


def oracle_loss(out, cot, hit=None):
    """L = sum(cotangent * output) of an oracle render; disparity only where the ray hit something (NaN elsewhere, as the reference):
    cot["disp_map"] is scaled by 1e-2 on those rays and zeroed on the others, IN PLACE.  hit (bool [R], optional): the rays that
    count as hit, else those with acc > 1e-3 in this run.  -> (L, hit)"""
    dt = out["color"].dtype
    ok = out["acc_map"].detach() > 1e-3 if hit is None else torch.as_tensor(hit)
    cot["disp_map"] = np.where(ok.numpy(), cot["disp_map"] * 1e-2, 0.0).astype(np.float32)
    L = sum((torch.from_numpy(cot[k]).to(dt) * out[k]).sum() for k in ("color", "acc_map", "depth_map", "weights"))
    L = L + (torch.from_numpy(cot["disp_map"]).to(dt)[ok] * out["disp_map"][ok]).sum()
    return L, ok


def _oracle_params(sd, dtype):
    """float64 everywhere but the pose MLP, whose input the reference computes in float32 (as train_oracle.loss_and_grads)"""
    return {k: torch.from_numpy(np.array(v)).to(dtype if not k.startswith("pose_mlp") else torch.float32).requires_grad_(True)
            for k, v in sd.items()}


def _run(name, g, z, noise, dtype, hit):
    params = _oracle_params(state(name), dtype)
    R, S = z.shape
    out = TO.render(params, g, jitter_z=z, noise=noise, dtype=dtype)
    cot = output_cotangents(R, S)
    L, ok = oracle_loss(out, cot, hit)
    names = list(params)
    nodes = list(COTANGENT_NODES.values())
    got = torch.autograd.grad(L, [out[k] for k in nodes] + [params[k] for k in names], allow_unused=True)
    f64 = lambda t, like: (torch.zeros_like(like) if t is None else t).detach().double().numpy()      # noqa: E731
    N = R * S
    rows = {k: out[v].detach().double().numpy().reshape(N, -1) for k, v in FORWARD_NODES.items()}
    cots = {k: f64(t, out[v]).reshape(N, -1) for (k, v), t in zip(COTANGENT_NODES.items(), got)}
    for d in (rows, cots):
        for k in d:
            if d[k].shape[1] == 1 and k in ("sig", "pre", "wl", "d_sig", "d_pre"):
                d[k] = d[k].reshape(N)
    grads = {k: f64(t, params[k]) for k, t in zip(names, got[len(nodes):])}
    return {"rows": rows, "cot": cots, "grads": grads, "cotangents": cot, "hit": ok.numpy().copy(),
            "transparent": out["transparent"].numpy().reshape(N).copy(), "z": z, "noise": noise, "g": g, "R": R, "S": S}


_CACHE = {}


def oracle_rows(name, nrays, nsamp, noise, dtype, z=None):
    """One oracle forward + backward of a sliced gradient case -> dict of float64 numpy (kept per case: do not write into it):
      rows        forward rows by device-array name (FORWARD_NODES), [N] or [N,k]
      cot         per-row cotangents by device-array name (COTANGENT_NODES)
      grads       the 33 parameter gradients
      cotangents  the float32 cotangents of the outputs, as the device takes them; hit: the rays whose disparity counts
      transparent [N] bool; z, noise (None when off), g (the sliced case), R, S
    noise: bool - the case's density noise on or off.  z (optional): other sample depths than the fixture's (the device's own, when
    its training forward sampled them).  The rays whose disparity counts are those of the FLOAT32 run in either dtype: the device is
    handed one set of cotangents."""
    zkey = None if z is None else np.ascontiguousarray(z, np.float32).tobytes()
    key = (name, nrays, nsamp, bool(noise), dtype, zkey)
    if key not in _CACHE:
        g = sliced_case(name, nrays, nsamp)
        zz = np.ascontiguousarray(g["render:z_vals"] if z is None else z, np.float32)
        nz = g["noise"] if noise and float(g["raw_noise_std"]) > 0 else None
        hit = None if dtype == torch.float32 else oracle_rows(name, nrays, nsamp, noise, torch.float32, z)["hit"]
        _CACHE[key] = _run(name, g, zz, nz, dtype, hit)
    return _CACHE[key]


# ---- the comparison rules (tests/test_row_cotangents_host.py, tests/test_gpu_row_cotangents.py) -----------------------------------
def rows2(a):
    a = np.asarray(a, np.float64)
    return a.reshape(a.shape[0], -1)


def off_rows(a, ref, rows):
    """bool per entry of `rows`: row of `a` further from `ref`'s than ROW_REL of that row's magnitude AND than ROW_FLOOR of the
    largest row magnitude of `ref` over `rows` (magnitudes: Euclidean norms of the float64 rows)"""
    a, ref = rows2(a)[rows], rows2(ref)[rows]
    if not len(rows):
        return np.zeros(0, bool)
    mag = np.linalg.norm(ref, axis=1)
    diff = np.linalg.norm(a - ref, axis=1)
    with np.errstate(invalid="ignore"):
        return ~(diff <= ROW_REL * mag) & ~(diff <= ROW_FLOOR * mag.max())      # (a non-finite row is off)


def oracle_array(o, k):
    return o["cot"][k] if k in o["cot"] else o["rows"][k]


def set_aside(o32, o64, rows):
    """the rows (bool per entry of `rows`) on which the float32 oracle is off its float64 run in ANY compared array, and per array"""
    per = {k: off_rows(oracle_array(o32, k), oracle_array(o64, k), rows) for k in COMPARED}
    return np.logical_or.reduce(list(per.values())) if len(rows) else np.zeros(0, bool), per


def oracle_live_rows(o):
    """rows with a non-zero cotangent in an oracle run: what the device's second list holds"""
    return np.flatnonzero((np.abs(rows2(o["cot"]["d_col"])).max(1) > 0) | (np.abs(o["cot"]["d_sig"]) > 0))


def rel_rows(a, ref, rows):
    a, ref = rows2(a)[rows], rows2(ref)[rows]
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-300))


def products(arr, rows, dtype=np.float64):
    """the ten weight / bias gradients of PRODUCTS and density_net.0.bias summed over `rows` of the arrays `arr` (by device-array
    name): float64 numpy, or - dtype = torch.float32 - plain float32 matmuls of the same arrays (the yardstick of a float32 sum)"""
    out = {}
    if dtype is torch.float32:
        T = lambda a: torch.from_numpy(np.ascontiguousarray(rows2(a)[rows], np.float32))      # noqa: E731
        for k, (dy, x) in PRODUCTS.items():
            y = T(arr[dy])
            out[k + ".weight"] = (y.t() @ T(arr[x])).double().numpy()
            out[k + ".bias"] = (y.t() @ torch.ones(len(rows), 1)).double().numpy().reshape(-1)
        out["nerf.density_net.0.bias"] = (T(arr["d_sig"]).t() @ torch.ones(len(rows), 1)).double().numpy().reshape(-1)
        return out
    for k, (dy, x) in PRODUCTS.items():
        y = rows2(arr[dy])[rows]
        out[k + ".weight"] = y.T @ rows2(arr[x])[rows]
        out[k + ".bias"] = y.sum(0)
    out["nerf.density_net.0.bias"] = rows2(arr["d_sig"])[rows].sum(0)
    return out
