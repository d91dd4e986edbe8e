"""The rule of dsn_train_loss / dsn_train_loss_grad (include/dsnerf.h) as restated in tests/train_loss_restate.py: against the
reference's own utils/loss.py run (tests/golden/train_loss.npz), against closed forms that do not depend on it, and the host side
of the two entry points' C ABI.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import train_loss_restate as LR
from helpers import GOLDEN

F32_HALF_ULP = 2.0 ** -24          # one rounding of a float64 value to float32
SEED_BAR = 2.0 ** -22              # the reference's own 2 ulp (measured, make_golden_train_loss.py) x 2: one rounding on each side


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "train_loss.npz"))
    cases = {}
    for name in g["cases"]:
        c = {k.split(":", 1)[1]: g[k] for k in g.files if k.startswith(name + ":")}
        R = int(c["R"])
        c["color"], c["acc"] = g[f"in{R}:color"], g[f"in{R}:acc"]
        c["target"] = g[f"in{R}:target32" if str(c["target_dtype"]) == "float32" else f"in{R}:target64"]
        c["occ"] = g[f"in{R}:occ_u8" if str(c["occ_dtype"]) == "uint8" else f"in{R}:occ_f32"]
        cases[str(name)] = c
    return cases


def check_against_reference(c, got, g_color, g_acc, acc_after):
    """losses (float64 or float32 values), seeds and the overwritten acc of one fixture case against the reference's"""
    assert abs(float(got["loss_rgb"]) - float(c["loss_rgb"])) <= (float(c["dev_rgb"]) + F32_HALF_ULP) * abs(float(c["loss_rgb"]))
    if bool(c["mask"]):
        assert abs(float(got["loss_mask"]) - float(c["loss_mask"])) <= (float(c["dev_mask"]) + F32_HALF_ULP) * abs(float(c["loss_mask"]))
        assert np.array_equal(acc_after, c["acc_after"])
    else:
        assert float(got["loss_mask"]) == 0.0
    if bool(c["has_grad"]):
        ref = c["color_grad"].astype(np.float64)
        assert np.array_equal(g_color == 0, ref == 0)
        assert (np.abs(g_color.astype(np.float64) - ref) <= SEED_BAR * np.abs(ref)).all()
        if bool(c["mask"]):
            ref = c["acc_grad"].astype(np.float64)
            assert np.array_equal(g_acc == 0, ref == 0)
            assert (np.abs(g_acc.astype(np.float64) - ref) <= SEED_BAR * np.abs(ref)).all()
            assert (g_acc[c["occ"] == 1] == 0).all() and (ref[c["occ"] == 1] == 0).all()


def test_fixture_covers_what_it_should(golden):
    assert {int(c["R"]) for c in golden.values()} == {1, 63, 257, 8192}
    assert {str(c["kind"]) for c in golden.values()} == {"L2", "L1"}
    assert {bool(c["mask"]) for c in golden.values()} == {True, False}
    assert any(str(c["occ_dtype"]) == "float32" for c in golden.values())
    for c in golden.values():      # the reference returns float64 with a float64 target (and its backward raises there: losses only)
        assert str(c["loss_dtype"]) == str(c["target_dtype"]) and c["loss_rgb"].dtype == np.dtype(str(c["target_dtype"]))
        assert bool(c["has_grad"]) == (str(c["target_dtype"]) == "float32" or str(c["kind"]) == "L1")
        if bool(c["mask"]):
            assert c["loss_mask"].dtype == np.float32
    assert any(str(c["target_dtype"]) == "float64" and bool(c["has_grad"]) for c in golden.values())


def test_restatement_matches_the_reference(golden):
    for name, c in golden.items():
        occ = c["occ"] if bool(c["mask"]) else None
        kind = LR.KINDS[str(c["kind"])]
        e = LR.forward(c["color"], c["target"], c["acc"], occ, kind)
        g_color, g_acc = LR.grad(c["color"], c["target"], c["acc"], occ, kind, 1.0, 1.0)
        assert g_color.dtype == np.float32 and g_acc.dtype == np.float32
        check_against_reference(c, e, g_color, g_acc, e["acc"])
        quiet = LR.forward(c["color"], c["target"], c["acc"], occ, kind, overwrite=False)
        assert np.array_equal(quiet["acc"], c["acc"]) and quiet["loss_mask"] == e["loss_mask"]


def test_closed_forms():
    rng = np.random.RandomState(3)
    R = 37
    t = rng.rand(R, 3).astype(np.float32)
    for kind in (LR.L2, LR.SMOOTH_L1):
        e = LR.forward(t, t, kind=kind)                      # d = 0
        assert e["loss_rgb"] == 0.0 and e["mse"] == 0.0 and e["psnr"] == np.inf and e["loss_mask"] == 0.0
        assert not LR.grad(t, t, kind=kind, up_rgb=1.0)[0].any()
        assert e["acc"] is None and LR.grad(t, t, kind=kind, up_rgb=1.0)[1] is None
    zero = np.zeros((R, 3), np.float32)
    for dv in (0.25, -0.5, 2.0, -3.0):                       # constant d (exact in binary)
        c = np.full((R, 3), dv, np.float32)
        e = LR.forward(c, zero, kind=LR.L2)
        assert e["loss_rgb"] == dv * dv and e["mse"] == dv * dv and np.isclose(e["psnr"], -10 * np.log10(dv * dv), rtol=1e-15)
        assert np.array_equal(LR.grad(c, zero, kind=LR.L2, up_rgb=1.0)[0], np.full((R, 3), np.float32((1.0 / (3 * R)) * (2 * dv))))
        e = LR.forward(c, zero, kind=LR.SMOOTH_L1)
        assert e["loss_rgb"] == (0.5 * dv * dv if abs(dv) < 1 else abs(dv) - 0.5) and e["mse"] == dv * dv
        want = np.float32((0.5 / (3 * R)) * (dv if abs(dv) < 1 else np.sign(dv)))
        assert np.array_equal(LR.grad(c, zero, kind=LR.SMOOTH_L1, up_rgb=0.5)[0], np.full((R, 3), want))
    # |d| exactly 1 and the float32 neighbours of 1 either side: 0.5 d d below, |d| - 0.5 from 1 on; the seed is d below, sign(d) from 1 on
    below, above = np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))
    d = np.array([[1.0, -1.0, below], [-below, above, -above]], np.float32)
    e = LR.forward(d, np.zeros_like(d), kind=LR.SMOOTH_L1)
    b, a = float(below), float(above)
    assert np.isclose(e["loss_rgb"], sum([0.5, 0.5, 0.5 * b * b, 0.5 * b * b, a - 0.5, a - 0.5]) / 6.0, rtol=1e-15)
    g = LR.grad(d, np.zeros_like(d), kind=LR.SMOOTH_L1, up_rgb=1.0)[0]
    s = 1.0 / 6.0
    assert np.array_equal(g.reshape(-1), np.array([s, -s, s * b, s * -b, s, -s]).astype(np.float32))
    # the mask term: acc == occ gives sign 0, occupancy 1 gives exactly 0 and acc = 1, other labels keep their value
    acc = np.array([0.0, 0.25, 0.5, 2.0, 0.7, 3.0], np.float32)
    occ = np.array([0, 0, 1, 2, 1, 2], np.uint8)
    c = np.zeros((6, 3), np.float32)
    e = LR.forward(c, c, acc, occ)
    assert e["loss_mask"] == 0.1 * ((0.0 + 0.25 + 0.0 + 0.0 + 0.0 + 1.0) / 6.0)
    assert np.array_equal(e["acc"], np.array([0.0, 0.25, 1.0, 2.0, 1.0, 3.0], np.float32))
    g_acc = LR.grad(c, c, acc, occ, up_mask=1.0)[1]
    m = np.float32(0.1 / 6.0)
    assert np.array_equal(g_acc, np.array([0.0, m, 0.0, 0.0, 0.0, m], np.float32)) and not np.signbit(g_acc).any()
    assert np.array_equal(LR.grad(c, c, acc, occ, up_mask=None)[1], np.zeros(6, np.float32))
    accf = np.array([0.2, 0.9], np.float32)
    e = LR.forward(c[:2], c[:2], accf, np.array([0.5, 1.0], np.float32))      # a float occupancy that is neither 0 nor 1
    assert np.isclose(e["loss_mask"], 0.1 * (0.5 - float(np.float32(0.2))) / 2.0, rtol=1e-15) and e["acc"][1] == 1.0 and e["acc"][0] == accf[0]
    assert np.array_equal(LR.grad(c[:2], c[:2], accf, np.array([0.5, 1.0], np.float32), up_mask=2.0)[1], np.array([-np.float32(2.0 * 0.05), 0.0], np.float32))
    # occupancy all 1 / all 0
    acc = rng.rand(R).astype(np.float32)
    e = LR.forward(t, t, acc, np.ones(R, np.uint8))
    assert e["loss_mask"] == 0.0 and (e["acc"] == 1.0).all() and not LR.grad(t, t, acc, np.ones(R, np.uint8), up_mask=1.0)[1].any()
    e = LR.forward(t, t, acc, np.zeros(R, np.uint8))
    assert np.isclose(e["loss_mask"], 0.1 * acc.astype(np.float64).mean(), rtol=1e-14) and np.array_equal(e["acc"], acc)
    assert np.array_equal(LR.grad(t, t, acc, np.zeros(R, np.uint8), up_mask=1.0)[1], np.full(R, np.float32(0.1 / R)))
    # NaN in, NaN out
    c = t.copy()
    c[5, 1] = np.nan
    acc_n = acc.copy()
    acc_n[3] = np.nan
    for kind in (LR.L2, LR.SMOOTH_L1):
        e = LR.forward(c, t, acc_n, np.zeros(R, np.uint8), kind)
        assert all(np.isnan(e[k]) for k in ("loss_rgb", "loss_mask", "mse", "psnr"))
        g_color, g_acc = LR.grad(c, t, acc_n, np.zeros(R, np.uint8), kind, 1.0, 1.0)
        assert np.isnan(g_color[5, 1]) and np.isnan(g_color).sum() == 1 and np.isnan(g_acc[3]) and np.isnan(g_acc).sum() == 1
    e = LR.forward(t, t, acc_n, np.ones(R, np.uint8))           # a NaN acc under occupancy 1 is never read
    assert e["loss_mask"] == 0.0
    # R = 0
    e = LR.forward(np.zeros((0, 3), np.float32), np.zeros((0, 3)), np.zeros(0, np.float32), np.zeros(0, np.uint8))
    assert all(np.isnan(e[k]) for k in ("loss_rgb", "loss_mask", "mse", "psnr"))
    assert LR.forward(np.zeros((0, 3), np.float32), np.zeros((0, 3)))["loss_mask"] == 0.0
    assert LR.grad(np.zeros((0, 3), np.float32), np.zeros((0, 3)))[0].shape == (0, 3)


def test_upstream_gradients_scale_in_the_headers_order():
    rng = np.random.RandomState(4)
    R = 65
    c, t = rng.randn(R, 3).astype(np.float32), rng.rand(R, 3)
    acc, occ = rng.rand(R).astype(np.float32), (rng.rand(R) < 0.5).astype(np.uint8)
    u, v = np.float32(0.1), np.float32(-0.3)
    g_color, g_acc = LR.grad(c, t, acc, occ, LR.L2, u, v)
    d = c.astype(np.float64) - t
    assert np.array_equal(g_color, ((np.float64(u) * (1.0 / (3.0 * R))) * (2.0 * d)).astype(np.float32))
    sign = np.sign(acc.astype(np.float64) - occ)
    assert np.array_equal(g_acc, np.where(occ == 1, 0.0, (np.float64(v) * (0.1 / R)) * sign).astype(np.float32))


def test_c_abi_argument_checks():
    import dsnerf_amd
    L = dsnerf_amd._lib
    lib = L.lib()
    assert {"dsn_train_loss_workspace_bytes", "dsn_train_loss", "dsn_train_loss_grad"} <= set(L.EXPORTS)
    assert lib.dsn_abi_version() == 8
    assert (L.LOSS_L2, L.LOSS_SMOOTH_L1, L.LOSS_SHARE) == (LR.L2, LR.SMOOTH_L1, LR.SHARE)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dsnerf.h")).read()
    assert f"#define DSN_LOSS_SHARE {LR.SHARE} " in header and "#define DSN_LOSS_L2 0" in header and "#define DSN_LOSS_SMOOTH_L1 1" in header
    wsb = lib.dsn_train_loss_workspace_bytes
    assert wsb(-1) == 0 and wsb(1 << 31) == 0
    assert 0 < wsb(0) <= 512 and wsb(8192) >= 3 * 8 * (8192 // LR.SHARE) and wsb(8192) < 4096
    assert wsb((1 << 20) + 37) >= 3 * 8 * (((1 << 20) + 37 + LR.SHARE - 1) // LR.SHARE) and wsb((1 << 20) + 37) < 1 << 17
    one, z = C.c_void_p(256), None

    def fwd(color=one, t32=one, t64=z, acc=one, o8=one, o32=z, R=4, kind=0, out4=one, ws=one):
        return lib.dsn_train_loss(color, t32, t64, acc, o8, o32, R, kind, 1, out4, ws, z)

    def bwd(color=one, t32=one, t64=z, acc=one, o8=one, o32=z, R=4, kind=0, g_color=one):
        return lib.dsn_train_loss_grad(color, t32, t64, acc, o8, o32, R, kind, one, one, g_color, one, z)

    for call, name, extra in ((fwd, b"dsn_train_loss:", (dict(out4=z), dict(ws=z))), (bwd, b"dsn_train_loss_grad:", (dict(g_color=z),))):
        for kw, msg in ((dict(kind=2), b"unknown kind"), (dict(kind=-1), b"unknown kind"), (dict(t64=one), b"exactly one target"),
                        (dict(t32=z), b"exactly one target"), (dict(acc=z), b"needs acc"), (dict(acc=z, o8=z, o32=one), b"needs acc"),
                        (dict(o32=one), b"at most one occupancy"), (dict(R=-1), b"R must be"), (dict(R=1 << 31), b"R must be"),
                        (dict(color=z), b"null argument")) + tuple((kw, b"null argument") for kw in extra):
            assert call(**kw) != 0, (name, kw)
            err = lib.dsn_last_error()
            assert name in err and msg in err, (kw, err)
