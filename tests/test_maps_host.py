"""Host side of the decomposition maps (dsn_render_rays_maps, dsn_composite_maps, Renderer.render_view_maps) that needs no GPU: the
float64 restatement against closed forms, the light-factor fixture against the golden cases it belongs to, and the argument checks of
the new entry points (every one of them runs before the device is touched)."""
import ctypes as C
import os

import numpy as np
import pytest

import maps_restate as MR
from helpers import ALL_CASES, GOLDEN, load

EVAL_CASES = [c for c in ALL_CASES if "train" not in c]


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


# ---- the restatement ----
def test_one_opaque_sample_gives_its_own_values():
    R, S = 3, 8
    rng = np.random.default_rng(0)
    e, n, L = rng.uniform(0, 2, (R, S, 3)), rng.normal(size=(R, S, 3)), rng.uniform(0.1, 3, (2, R, S))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    w = np.zeros((R, S))
    hit = [2, 5, 7]
    w[np.arange(R), hit] = 1.0
    m = MR.maps(w, e, n, L)
    for r in range(R):
        assert np.array_equal(m["albedo"][r], e[r, hit[r]]) and np.array_equal(m["normal"][r], n[r, hit[r]])
        for k in range(2):
            assert m["shading"][k, r] == L[k, r, hit[r]]
            assert np.allclose(m["color"][k, r], L[k, r, hit[r]] * e[r, hit[r]], rtol=1e-15)
    assert m["albedo"].shape == (R, 3) and m["shading"].shape == (2, R) and m["color"].shape == (2, R, 3)


def test_unlisted_samples_contribute_nothing_whatever_they_hold():
    R, S = 2, 6
    rng = np.random.default_rng(1)
    w = rng.uniform(0, 0.2, (R, S))
    e, n, L = rng.uniform(0, 2, (R, S, 3)), rng.normal(size=(R, S, 3)), rng.uniform(0.1, 3, (1, R, S))
    listed = rng.uniform(size=(R, S)) > 0.5
    e2, n2, L2 = e.copy(), n.copy(), L.copy()
    e2[~listed], n2[~listed], L2[0][~listed] = np.nan, np.inf, -np.inf            # rubbish off the list
    a, b = MR.maps(w, e, n, L, listed), MR.maps(w, e2, n2, L2, listed)
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.isfinite(b[k]).all(), k
    none = MR.maps(w, e2, n2, L2, np.zeros((R, S), bool))                        # all transparent: zeros
    assert all(float(np.abs(v).max()) == 0.0 for v in none.values())
    assert MR.weighed_max(e2, L2, np.zeros((R, S), bool)) == (0.0, 0.0)
    em, lm = MR.weighed_max(e, L, listed)
    assert em == np.abs(e[listed]).max() and lm == L[0][listed].max()
    sg = np.array([[1.0, -2.0, 0.0, 3.0]])
    assert MR.listed_samples(sg, np.array([0, 0, 0, 1])).tolist() == [[True, False, False, False]]


def test_normal_map_is_no_longer_than_acc():
    rng = np.random.default_rng(2)
    R, S = 50, 16
    alpha = rng.uniform(0, 0.6, (R, S))
    T = np.cumprod(np.concatenate([np.ones((R, 1)), 1 - alpha], 1), 1)[:, :-1]
    w = alpha * T
    n = rng.normal(size=(R, S, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    m = MR.maps(w, np.ones((R, S, 3)), n, np.ones((1, R, S)))
    acc = w.sum(1)
    assert (np.linalg.norm(m["normal"], axis=-1) <= acc * (1 + 1e-12)).all()
    assert np.allclose(m["albedo"], acc[:, None]) and np.allclose(m["shading"][0], acc)      # e = 1, L = 1: every map is acc


# ---- the fixture ----
def test_light_fixture_covers_the_eval_cases():
    z = np.load(os.path.join(GOLDEN, "maps_light.npz"))
    assert sorted(z.files) == sorted("light:" + c for c in EVAL_CASES)
    assert os.path.getsize(os.path.join(GOLDEN, "maps_light.npz")) < (1 << 20)


@pytest.mark.parametrize("name", EVAL_CASES)
def test_light_factor_times_essence_is_the_colour(name):
    """L of the fixture x the case's essence = the case's colour (model/spacenet.py:185-186), at test_shade's bar"""
    g = load(name)
    L = np.load(os.path.join(GOLDEN, "maps_light.npz"))["light:" + name]
    assert L.dtype == np.float32 and L.shape == (g["essence"].shape[0],) and np.isfinite(L).all()
    assert (L > 0).all()                                                       # ELU + 1
    err = np.abs(L[:, None].astype(np.float64) * g["essence"] - g["colour"]).max()
    bar = 1e-5 * max(1.0, float(np.abs(g["colour"]).max()))
    assert err <= bar, (name, err, bar)
    # and the four sums of the restatement agree with the case's own rgb_map where the colour is used
    S = int(g["S"])
    m = MR.maps(g["weights"], g["essence"], g["n_w"], L)
    assert np.abs(m["color"][0] - g["rgb_map"]).max() <= 2e-6 * max(1.0, float(np.abs(g["rgb_map"]).max())), name
    assert m["shading"].shape == (1, g["weights"].shape[0]) and g["weights"].shape[1] == S


# ---- the ABI ----
def test_maps_entry_points_are_exported(lib):
    import dsnerf_amd
    for n in ("dsn_render_maps_scratch_bytes", "dsn_render_rays_maps", "dsn_composite_maps", "dsn_shade_factor"):
        assert hasattr(lib, n) and n in dsnerf_amd._lib.EXPORTS
    assert lib.dsn_abi_version() == 8


def test_maps_scratch_bytes(lib):
    f, f3 = lib.dsn_render_maps_scratch_bytes, lib.dsn_render_lights_scratch_bytes
    R, S = 512 * 512, 64
    assert f(0, S, 1, 10) == 0 and f(R, 0, 1, 10) == 0 and f(R, S, 0, 10) == 0 and f(R, S, 1, -1) == 0
    assert f(R, S, 1, R * S + 1) == 0
    one = f(R, S, 1, 1_000_000)
    assert one == 16 * 1_000_000 and one % 256 == 0                            # 4 floats per shaded sample and light
    assert f(R, S, 10, 1_000_000) == 10 * one
    assert f(R, S, 1, 0) == 256 == f3(R, S, 1, 0)
    assert 3 * f(R, S, 7, 2_000_000) == 4 * f3(R, S, 7, 2_000_000)


def _render(lib, R=64, S=64, flags=1, lights=1, n_lights=1, jitter=None, noise=None, scratch=1, scratch_bytes=1 << 20, null=(),
            workspace=256):
    """dsn_render_rays_maps with fake non-null pointers"""
    p = C.c_void_p(256)
    a = {k: (None if k in null else p) for k in ("scene", "packed", "ray_o", "ray_d", "near", "far", "t_vals", "out_rgb", "out_disp",
                                                 "out_acc", "out_depth", "albedo", "normal", "shading", "max")}
    return lib.dsn_render_rays_maps(a["scene"], 1, 1, a["packed"], a["ray_o"], a["ray_d"], a["near"], a["far"], R, S, a["t_vals"],
                                    jitter, noise, flags, C.c_void_p(256) if lights else None, n_lights, a["out_rgb"], a["out_disp"],
                                    a["out_acc"], a["out_depth"], None, None, a["albedo"], a["normal"], a["shading"], a["max"],
                                    C.c_void_p(workspace) if workspace else None, C.c_size_t(0),
                                    C.c_void_p(256) if scratch else None, C.c_size_t(scratch_bytes), None, 0, None)


@pytest.mark.parametrize("case,words", [
    (dict(null=("scene",)), b"null argument"),
    (dict(null=("out_acc",)), b"null output"),
    (dict(lights=0), b"null argument"),
    (dict(scratch=0), b"null argument"),
    (dict(workspace=0), b"null argument"),
    (dict(R=0), b"empty ray batch"),
    (dict(n_lights=0), b"n_lights"),
    (dict(jitter=C.c_void_p(256)), b"no jitter"),
    (dict(noise=C.c_void_p(256)), b"no noise"),
    (dict(flags=0), b"DSN_SKIP_TRANSPARENT"),
    (dict(flags=1 | 4), b"DSN_FIELD_FP32"),
    (dict(flags=1 | 256), b"DSN_PHASE_"),
    (dict(flags=1 | 1024), b"DSN_PHASE_"),
    (dict(S=32), b"S must be 64 or 128"),
    (dict(workspace=264), b"16-byte aligned"),
    (dict(scratch_bytes=16), b"light_scratch is too small"),
])
def test_render_rays_maps_rejects_bad_arguments(lib, case, words):
    assert _render(lib, **case) != 0
    err = lib.dsn_last_error()
    assert b"dsn_render_rays_maps" in err and words in err, err


def _composite(lib, null=(), R=4, S=4):
    p = C.c_void_p(256)
    a = {k: (None if k in null else p) for k in ("essence", "n_w", "factor", "sigma", "z_vals", "ray_d", "albedo", "normal", "shading",
                                                 "weights", "max")}
    return lib.dsn_composite_maps(a["essence"], a["n_w"], a["factor"], a["sigma"], None, a["z_vals"], a["ray_d"], R, S, a["albedo"],
                                  a["normal"], a["shading"], a["weights"], a["max"], None)


@pytest.mark.parametrize("case,words", [
    (dict(null=("sigma",)), b"null argument"),
    (dict(null=("z_vals",)), b"null argument"),
    (dict(null=("ray_d",)), b"null argument"),
    (dict(R=0), b"empty ray batch"),
    (dict(S=0), b"empty ray batch"),
    (dict(null=("albedo", "normal", "shading", "weights", "max")), b"no output"),
    (dict(null=("essence", "max")), b"without its source"),
    (dict(null=("n_w",)), b"without its source"),
    (dict(null=("factor", "max")), b"without its source"),
    (dict(null=("factor", "shading")), b"out_max needs"),
])
def test_composite_maps_rejects_bad_arguments(lib, case, words):
    assert _composite(lib, **case) != 0
    err = lib.dsn_last_error()
    assert b"dsn_composite_maps" in err and words in err, err


def test_shade_factor_rejects_bad_arguments(lib):
    z, p, i64 = None, C.c_void_p(256), C.c_int64
    assert lib.dsn_shade_factor(z, 1, 1, z, z, z, z, z, z, i64(0), 1, z, z, z, z, z, z, 0, z) != 0
    assert b"dsn_shade_factor" in lib.dsn_last_error() and b"null argument" in lib.dsn_last_error()
    assert lib.dsn_shade_factor(p, 1, 1, p, p, p, p, p, p, i64(8), 4, z, z, z, p, p, z, 0, z) != 0           # no factor array
    assert b"null argument" in lib.dsn_last_error()
    assert lib.dsn_shade_factor(p, 1, 1, p, p, p, p, p, p, i64(8), 4, z, z, z, p, p, p, 4, z) != 0           # DSN_FIELD_FP32
    assert b"dsn_shade_factor" in lib.dsn_last_error() and b"DSN_FIELD_FP32" in lib.dsn_last_error()
    assert lib.dsn_shade_factor(p, 1, 1, p, p, p, p, p, p, i64(8), 4, p, z, z, p, p, p, 0, z) != 0           # a list without its count
    assert b"go together" in lib.dsn_last_error()


# ---- the Python surface ----
def test_renderer_maps_checks_come_before_any_device_work():
    import dsnerf_amd
    from types import SimpleNamespace
    fake = SimpleNamespace(net=SimpleNamespace(training=False), skip_transparent=True)
    with pytest.raises(ValueError, match="unknown maps"):
        dsnerf_amd.Renderer.render_view_maps(fake, {}, maps=("albedo", "depth"))
    with pytest.raises(ValueError, match="no maps"):
        dsnerf_amd.Renderer.render_view_maps(fake, {}, maps=())
    with pytest.raises(ValueError, match="no lights"):
        dsnerf_amd.Renderer.render_view_maps(fake, {}, lights=[])
    fake.net.training = True
    with pytest.raises(RuntimeError, match="eval mode"):
        dsnerf_amd.Renderer.render_view_maps(fake, {})
    fake.net.training = False
    fake.skip_transparent = False
    with pytest.raises(RuntimeError, match="skip_transparent"):
        dsnerf_amd.Renderer.render_view_maps(fake, {}, lights=[{}])


def test_maps_bound_follows_the_threshold(lib):
    from dsnerf_amd import _lib
    lib.dsn_early_stop_eps_scaled.restype = C.c_float
    assert _lib.MAPS == ("albedo", "shading", "normal")
    for S, c in ((64, 1.0), (128, 2.64), (64, 468.0)):
        eps = lib.dsn_early_stop_eps_scaled(S, C.c_float(c))
        assert _lib.maps_bound(S, eps, 1.0) == (S + 1) * (eps + 2.0 ** -22)
        assert _lib.maps_bound(S, eps, 3.5) == pytest.approx(3.5 * _lib.maps_bound(S, eps, 1.0), rel=1e-15)
        # for values up to the colour scale the threshold was computed with, the maps move by less than the colour bar's 1e-4
        assert _lib.maps_bound(S, eps, c) < 1e-4 * max(1.0, c)
