"""tests/field_restate.py (the float64 restatement of the field and lighting networks that test_gpu_tiles.py judges the kernels by)
pinned before anything is judged by it - against the reference's own float64 and float32 runs (tests/golden/*.npz) and against
closed forms.  No GPU.

Light edits (light centre, rotation: small_novel / small_rot) are left out: light64 restates LightingMLP.forward, the edits move the
world point in DualSpaceNeRF.forward before that call (model/spacenet.py:254-265) and light64 does not take them.
"""
import numpy as np
import pytest

import field_restate as FR
from helpers import load, maxdiff, per_point_dirs, ref_tol, state

CASES = ["full_eval", "full_eval_w4", "small_eval_w3"]


def unit_dirs(g):
    d = per_point_dirs(g).astype(np.float64)       # the float32 ray directions, cast up; normalised as model/spacenet.py:102 does
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


@pytest.mark.parametrize("name", CASES)
def test_field64_against_the_reference_in_float64(name):
    """field64 at the reference's float64 canonical points vs its float64 outputs: 1e-6 of the largest magnitude on sigma and essence,
    1e-9 on d sigma/dx.
    Measured (sigma, largest |sigma|, essence, gradient): full_eval 5.3e-8 / 9.2 / 3e-9 / 0; full_eval_w4 1.6e-5 / 1013 / 1.2e-7 / 0;
    small_eval_w3 2.3e-4 / 947 / 3.4e-5 / 0.
    The residue on sigma and essence is the POSE CODE, and not its precision: the reference's float64 run keeps the pose MLP in
    float32 too (spacenet.py:223), but evaluates it on the quaternion repeated once per point (:229-236), and torch's batched float32
    product rounds differently from the single-row one (pose code: 3.0e-8 / 1.5e-8 / 4.8e-7 apart on the three cases).  Confirmed by
    feeding field64 the batched code: sigma, essence and gradient then agree with the goldens to the last bit (0.0 on all three cases; printed
    below and not asserted, since it rests on the host BLAS rounding the batched product as the machine that made the goldens did).
    The gradient agrees exactly either way: it sees the pose code only through the relu masks."""
    g, sd = load(name), state(name)
    big = lambda k: float(np.abs(g[k]).max())       # noqa: E731
    sig, ess, gr = FR.field64(g["x_c_f64"], sd, g["poses"], int(g["frame"]))
    figures = (maxdiff(sig, g["sigma_f64"]), big("sigma_f64"), maxdiff(ess, g["essence_f64"]), big("essence_f64"),
               maxdiff(gr, g["grad_sigma_f64"]), big("grad_sigma_f64"))
    print(name, "sigma %.3g of %.3g, essence %.3g of %.3g, grad %.3g of %.3g" % figures)
    assert figures[0] <= 1e-6 * figures[1], figures
    assert figures[2] <= 1e-6 * figures[3], figures
    assert figures[4] <= 1e-9 * figures[5], figures
    assert np.array_equal(FR.pose_code(sd, g["poses"]).numpy(), g["pose_feat"])       # the single-row code IS the golden's
    # the stated cause: with the code of the batched pose MLP the residue is gone
    batched = FR.pose_code(sd, g["poses"], rows=g["x_c_f64"].shape[0])
    sig_b, ess_b, gr_b = FR.field64(g["x_c_f64"], sd, g["poses"], int(g["frame"]), pose=batched)
    resid = (maxdiff(sig_b, g["sigma_f64"]), maxdiff(ess_b, g["essence_f64"]), maxdiff(gr_b, g["grad_sigma_f64"]))
    print(name, "with the batched pose code: sigma %.3g, essence %.3g, grad %.3g" % resid)


@pytest.mark.parametrize("name", CASES)
def test_field64_against_the_reference_in_float32(name):
    """field64 at the golden's float32 points vs the reference's float32 sigma / essence: inside the project's bar (helpers.ref_tol).
    Measured on full_eval: sigma 5.9e-6, essence 4.4e-7; full_eval_w4: 5.7e-4 (bar 4.1e-3), 4.4e-6; small_eval_w3: 1.1e-3 (3.8e-3),
    2.0e-4 (8.8e-4)."""
    g, sd = load(name), state(name)
    sig, ess, _ = FR.field64(g["x_c"], sd, g["poses"], int(g["frame"]))
    figures = (maxdiff(sig, g["sigma"]), ref_tol(g, "sigma", 1e-4), maxdiff(ess, g["essence"]), ref_tol(g, "essence", 1e-4))
    print(name, "sigma %.3g (bar %.3g), essence %.3g (bar %.3g)" % figures)
    assert figures[0] <= figures[1] and figures[2] <= figures[3], figures


@pytest.mark.parametrize("name", CASES)
def test_light64_against_the_reference(name):
    """light64 on the golden's n_w, world points, unit view directions and essence vs the reference's float32 colour: 1e-5, relative
    to the colour magnitude where that is above 1 (test_shade's bar).  Measured: 1.4e-7, 1.7e-7, 2.3e-4 at |colour| = 1632."""
    g, sd = load(name), state(name)
    col, fac = FR.light64(g["n_w"], g["pts"].reshape(-1, 3), unit_dirs(g), g["essence"], sd)
    bar = 1e-5 * max(1.0, float(np.abs(g["colour"]).max()))
    print(name, "colour %.3g (bar %.3g)" % (maxdiff(col, g["colour"]), bar))
    assert maxdiff(col, g["colour"]) <= bar
    assert fac.shape == (g["n_w"].shape[0],) and np.all(fac > 0)          # ELU + 1 > 0
    assert np.array_equal(col, fac[:, None] * g["essence"].astype(np.float64))


def test_closed_forms():
    """all weights zero, biases kept: sigma is the density bias, d sigma/dx exactly zero, the essence rgb_net.3's bias (relu of the
    bias below it feeds zero weights), and colour = (ELU(b) + 1) x essence for the lighting MLP's output bias b, on either side of 0"""
    g = load("small_eval")
    sd = {k: (np.zeros_like(v) if k.endswith(".weight") and not k.startswith("nerf.embedding") else np.array(v, np.float32))
          for k, v in state().items()}
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((257, 3)) * 20.0).astype(np.float32)
    sig, ess, gr = FR.field64(x, sd, g["poses"], int(g["frame"]))
    assert np.array_equal(sig, np.full(257, np.float64(sd["nerf.density_net.0.bias"][0])))
    assert np.array_equal(gr, np.zeros((257, 3)))
    assert np.array_equal(ess, np.broadcast_to(sd["nerf.rgb_net.3.bias"].astype(np.float64), (257, 3)))
    e = rng.random((257, 3)).astype(np.float32)
    for b in (-0.75, 0.0, 1.25):
        sd["lighting_mlp.lights_encoding.4.bias"] = np.array([b], np.float32)
        col, fac = FR.light64(x, x, x, e, sd)
        want = (b if b > 0 else np.expm1(b)) + 1.0
        assert np.allclose(fac, want, rtol=1e-14, atol=0) and np.allclose(col, want * e.astype(np.float64), rtol=1e-14, atol=0)


def test_field64_gradient_is_the_derivative():
    """autograd's d sigma/dx against central differences of field64's own sigma in float64 (away from relu kinks the field is smooth:
    the median over the points is what is judged)"""
    g, sd = load("small_eval"), state()
    x = g["x_c"][~g["transparent"]][:64].astype(np.float64)
    _, _, gr = FR.field64(x, sd, g["poses"], int(g["frame"]))
    h = 1e-7
    num = np.zeros_like(gr)
    for c in range(3):
        d = np.zeros(3)
        d[c] = h
        num[:, c] = (FR.field64(x + d, sd, g["poses"], int(g["frame"]))[0] - FR.field64(x - d, sd, g["poses"], int(g["frame"]))[0]) / (2 * h)
    rel = np.linalg.norm(num - gr, axis=-1) / np.maximum(np.linalg.norm(gr, axis=-1), 1.0)
    assert np.median(rel) < 1e-6, float(np.median(rel))
