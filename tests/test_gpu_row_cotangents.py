"""The training backward ROW BY ROW against the float64 oracle (tests/row_cotangents.py).

Every other training test compares parameter tensors - sums over thousands of rows, judged by a relative L2 - and the judge of
test_backward_matches_oracle_all_cotangents is the oracle in float32, which with density noise and S >= 100 is itself 1e-4 from its
float64 run on the lighting MLP's tensors.  Here the per-row arrays the backward leaves in its workspace (_lib.grad_rows: the
adjoints of compositing and of the colour product, the lighting MLP's three data gradients, the normal map's adjoint) are compared
with autograd of the float64 oracle on the rows of the device's own second list, and the weight-gradient products are compared with
float64 sums of the device's own rows.

A row is SET ASIDE when the float32 oracle itself is off its float64 run there (row_cotangents.off_rows; decided by the two oracle
runs alone, at most 0.5 % of the live rows): single noise-only samples far outside the body on which any float32 evaluation of the
normal map scatters.  On the rows that are kept the device gets the suite's outlier budget (2e-3 of the rows) and, without those, a
relative L2 of 3 x the float32 oracle's own + 2e-6 per array.

Cases (row_cotangents.CASES; noise on unless said): 37 x 64 (k_t_composite_adjoint_w<1>, one stream), 37 x 100 (w<2> with idle lanes
in the second chunk), 37 x 100 without noise, 37 x 129 (one thread per ray; two streams), 128 x 128 (two full chunks), the converged
field at 128 x 128 (opaque rays: factors of 1e-10 under suffix / f).  37 x 100 and the converged field run once more through the
training forward + the cached backward, where k_light16 leaves hl1 / hl2 / pre.

Each run prints one `row_cotangents:` line (profiles/row_cotangent_errors.txt is that output).

What these tests found when they first ran: on the converged field `u` was more than 1e-3 off on 3 962 of 9 041
rows - k_t_lin16 scaled its fp16 split by the batch-wide magnitude, now by the row's own - and lights_encoding.4.bias at 37 x 64 was
2.7e-6 from the float64 sum of the device's rows (bar 2.4e-6) - k_t_wcolsum's float32 chain, now a double.  The tensor-level gap of
the noisy S >= 100 cases (3.8e-4 on the lighting weights at 37 x 100, still there and recorded in the printed line) is one or two
noise-only rows per case with a hidden unit on its ReLU kink, inside the outlier budget of B."""
import numpy as np
import pytest
import torch

import row_cotangents as RC
from cases import make_batch, make_renderer, rel, state

pytestmark = pytest.mark.gpu

RUNS = [(cid, False) for cid in RC.CASES] + [("37x100", True), ("w4-128x128", True)]
IDS = [cid + ("-cached" if cached else "") for cid, cached in RUNS]
OUTLIER_SHARE = 2e-3          # the suite's outlier budget (test_field)
FACTOR, FLOOR = 3.0, 2e-6     # helpers.ref_tol's factor on the reference's own error; test_gpu_train.FLOOR
_RUNS = {}


def device_run(cid, cached):
    """one backward of the case on the device -> dict(rows: the workspace's per-row arrays as numpy, grads: {tensor: float64},
    o32 / o64: the two oracle runs on the same samples and cotangents); kept per run"""
    key = (cid, cached)
    if key in _RUNS:
        return _RUNS[key]
    from dsnerf_amd import _lib
    name, R, S, noise_on = RC.CASES[cid]
    g = RC.sliced_case(name, R, S)
    r = make_renderer(g, name)
    r._set_frame(make_batch(g))
    dev = r.device
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    params = {k: T(v) for k, v in state(name).items()}
    packed = _lib.PackedParams(dev).update(params)
    ws = _lib.GradWorkspace(dev)
    noise = g["noise"] if noise_on and float(g["raw_noise_std"]) > 0 else None
    z = None
    if cached:      # the training forward samples the rays itself: the oracles run on ITS depths
        out = _lib.render_rays(r.scene, packed, _lib.RenderWorkspace(dev), T(g["ray_o"]), T(g["ray_d"]), T(g["near"].copy()),
                               T(g["far"].copy()), S, torch.linspace(0.0, 1.0, steps=S).to(dev), T(g["jitter"]), T(noise),
                               skip_transparent=False, train_cache=ws)
        z = out["z_vals"].cpu().numpy()
        if np.array_equal(z, g["render:z_vals"]):
            z = None
    o32 = RC.oracle_rows(name, R, S, noise_on, torch.float32, z)
    o64 = RC.oracle_rows(name, R, S, noise_on, torch.float64, z)
    cot = o32["cotangents"]
    grads = _lib.render_rays_grad(r.scene, params, T(g["poses"]), int(g["frame"]), False, T(g["ray_o"]), T(g["ray_d"]), T(o32["z"]),
                                  T(noise), T(cot["color"]), T(cot["disp_map"]), T(cot["acc_map"]), T(cot["depth_map"]),
                                  T(cot["weights"]), ws=ws, packed=packed, cached=cached)
    rows = {k: v.cpu().numpy() for k, v in _lib.grad_rows(ws, R, S).items()}
    assert _lib.grad_range_overflow(ws, R, S) == 0
    assert _lib.grad_row_counts(ws, R, S) == (len(rows["list1"]), len(rows["list2"]))
    _RUNS[key] = {"rows": rows, "grads": {k: v.double().cpu().numpy() for k, v in zip(_lib.PARAM_ORDER, grads)}, "o32": o32, "o64": o64,
                  "noise": noise, "N": R * S}
    return _RUNS[key]


@pytest.mark.parametrize("cid,cached", RUNS, ids=IDS)
def test_row_lists_hold_exactly_the_rows_with_a_cotangent(cid, cached):
    """A.  list1 = every row but transparent ones with noise <= 0; list2 ascending and unique, a row is on it exactly when the device's
    own d_sig / d_col row is non-zero, none of its rows is off list1; and a row the float64 oracle gives a non-zero cotangent that
    the device leaves off carries less than float32's smallest normal (x 4, x the largest output cotangent): it cannot register in a
    float32 sum"""
    D = device_run(cid, cached)
    w, o64, N = D["rows"], D["o64"], D["N"]
    l1, l2 = w["list1"].astype(np.int64), w["list2"].astype(np.int64)
    for lst in (l1, l2):
        assert np.all(np.diff(lst) > 0) and (not len(lst) or (lst[0] >= 0 and lst[-1] < N))
    nz = D["noise"].reshape(-1) > 0 if D["noise"] is not None else np.zeros(N, bool)
    assert np.array_equal(l1, np.flatnonzero((w["transparent"] == 0) | nz))
    assert np.array_equal(l2, np.flatnonzero((w["d_sig"] != 0) | (w["d_col"] != 0).any(1)))
    assert np.isin(l2, l1).all()
    assert len(l2) > 0
    lost = np.setdiff1d(RC.oracle_live_rows(o64), l2)
    cmax = max(1.0, max(float(np.abs(v).max()) for v in D["o32"]["cotangents"].values()))
    big = 0.0
    if len(lost):
        big = max(float(np.abs(o64["cot"]["d_col"][lost]).max()), float(np.abs(o64["cot"]["d_sig"][lost]).max()))
    print(f"row_lists: {IDS[RUNS.index((cid, cached))]}: list1 {len(l1)}, list2 {len(l2)}, float64 live rows off list2 {len(lost)} (largest {big:.1e})")
    assert big <= 4 * 2.0 ** -126 * cmax, (len(lost), big)


def tensor_level(D, keep):
    """D (recorded, not asserted): the six lighting tensors' largest distance from the float64 parameter gradients - the device's and the
    float32 oracle's, as returned, and without the set-aside rows (products over the kept rows of each side's OWN rows against the
    float64 oracle's products over the same rows)"""
    o32, o64 = D["o32"], D["o64"]
    full_dev = max(rel(D["grads"][k], o64["grads"][k]) for k in RC.LIGHT_TENSORS)
    full_o32 = max(rel(o32["grads"][k], o64["grads"][k]) for k in RC.LIGHT_TENSORS)
    P64 = RC.products({**o64["cot"], **o64["rows"]}, keep)
    Pd = RC.products(D["rows"], keep)
    P32 = RC.products({**o32["cot"], **o32["rows"]}, keep)
    kept_dev = max(rel(Pd[k], P64[k]) for k in RC.LIGHT_TENSORS)
    kept_o32 = max(rel(P32[k], P64[k]) for k in RC.LIGHT_TENSORS)
    return full_dev, full_o32, kept_dev, kept_o32


@pytest.mark.parametrize("cid,cached", RUNS, ids=IDS)
def test_rows_match_the_float64_oracle(cid, cached):
    """B.  on the rows of the device's second list: at most 0.5 % set aside by the two oracle runs; on the others every compared array
    finite, at most 2e-3 of the rows off (1e-3 of the row, 1e-6 of the array), and without those a relative L2 within 3 x the float32
    oracle's own + 2e-6; on the set-aside rows finite values (their error is printed)"""
    D = device_run(cid, cached)
    w, o32, o64 = D["rows"], D["o32"], D["o64"]
    live = w["list2"].astype(np.int64)
    aside, _ = RC.set_aside(o32, o64, live)
    keep, out = live[~aside], live[aside]
    body = w["transparent"][keep] == 0
    fails, parts = [], []
    for k in RC.COMPARED:
        ref = RC.oracle_array(o64, k)
        finite = bool(np.isfinite(RC.rows2(w[k])[live]).all())
        off = RC.off_rows(w[k], ref, keep)
        good = keep[~off]
        e_dev, e_o32 = RC.rel_rows(w[k], ref, good), RC.rel_rows(RC.oracle_array(o32, k), ref, good)
        bar = FACTOR * e_o32 + FLOOR
        gb, gn = good[body[~off]], good[~body[~off]]
        parts.append(f"{k} {e_dev:.1e}/{bar:.1e} (body {RC.rel_rows(w[k], ref, gb):.1e}, noise-only {RC.rel_rows(w[k], ref, gn):.1e}, off {int(off.sum())}"
                     + (f", aside {RC.rel_rows(w[k], ref, out):.1e}" if len(out) else "") + ")")
        if not finite:
            fails.append((k, "not finite"))
        if off.sum() > OUTLIER_SHARE * len(keep):
            fails.append((k, "rows off", int(off.sum()), len(keep)))
        if not e_dev <= bar:
            fails.append((k, "relative L2", e_dev, bar))
    fd, fo, kd, ko = tensor_level(D, keep)
    print(f"row_cotangents: {IDS[RUNS.index((cid, cached))]}: list2 {len(live)} (body {int(body.sum())}, noise-only {int((~body).sum())} kept),"
          f" set aside {len(out)}; device/bar per array: " + "; ".join(parts)
          + f"; lighting tensors vs float64: device {fd:.1e}, float32 oracle {fo:.1e}; kept rows only: device {kd:.1e}, float32 oracle {ko:.1e}")
    assert len(out) <= RC.SET_ASIDE_CAP * len(live), (len(out), len(live))
    assert not fails, fails


@pytest.mark.parametrize("cid,cached", RUNS, ids=IDS)
def test_products_match_float64_sums_of_the_device_rows(cid, cached):
    """C.  the gradients of lights_encoding.4 / .2 / .0, rgb_net.3 and rgb_net.1 (weight and bias) and density_net.0.bias against the
    same products summed in float64 over list2 from the arrays the device left - the product kernels (k_t_wcolsum, k_t_wgrad16q,
    k_t_wgrad / wgrad_mfma) apart from the conditioning of the rows.  Yardstick: the product in plain float32 (torch matmul of the
    same arrays); bar: 3 x that + 2e-6"""
    D = device_run(cid, cached)
    live = D["rows"]["list2"].astype(np.int64)
    P64 = RC.products(D["rows"], live)
    P32 = RC.products(D["rows"], live, torch.float32)
    fails, parts = [], []
    for k, want in P64.items():
        got = D["grads"][k]
        assert got.shape == want.shape, (k, got.shape, want.shape)
        e, y = rel(got, want), rel(P32[k], want)
        parts.append(f"{k.replace('lighting_mlp.lights_encoding', 'le').replace('nerf.', '')} {e:.1e}/{FACTOR * y + FLOOR:.1e}")
        if not (np.isfinite(got).all() and e <= FACTOR * y + FLOOR):
            fails.append((k, e, y))
    print(f"row_products: {IDS[RUNS.index((cid, cached))]}: rows {len(live)}; device/bar: " + "; ".join(parts))
    assert not fails, fails
