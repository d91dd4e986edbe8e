"""Host side of the relighting sweep (dsn_render_rays_lights, Renderer.render_view_lights) that needs no GPU: the light records
agree with what DualSpaceNeRF.frame_args hands to dsn_set_frame, the new entry points check their arguments before touching the
device, and the scratch size follows the number of lights and of shaded samples."""
import ctypes as C

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


def _net():
    import dsnerf_amd
    from test_gpu_render import make_cfg
    return dsnerf_amd.DualSpaceNeRF(make_cfg(64))


def _record_from_frame_args(net, batch):
    """the 12 floats dsn_set_frame would put into the frame state for the net's light edits (dsn_geom.hip k_pose_setup)"""
    _, ls, rot, rc = net.frame_args(batch)
    rec = np.zeros(12, np.float32)
    if ls is not None:
        rec[0] = 1.0
        rec[1:4] = ls.reshape(-1)[:3].to(torch.float32).numpy()
    if rot is not None and rc is not None:
        rec[4] = 1.0
        rec[5:9] = rot.reshape(-1)[:4].to(torch.float32).numpy()
        rec[9:11] = rc.reshape(-1)[:2].to(torch.float32).numpy()
    return rec


LC = torch.tensor([0.35, 0.05, 1.4])
ANG = np.pi * 108 / 180
ROT = torch.tensor([[np.cos(ANG), -np.sin(ANG)], [np.sin(ANG), np.cos(ANG)]])          # (float64, as vis_lighting.py's angle2rot)
RC = torch.tensor([[0.18649693, -0.14180326, 1.7103844]])


@pytest.mark.parametrize("which", ["neither", "shift", "rotation", "both"])
def test_light_records_agree_with_frame_args(which):
    from dsnerf_amd import _lib
    net = _net()
    batch = {"Th": torch.tensor([0.2, -0.1, 1.0]).reshape(1, 1, 3)}
    light = {}
    if which in ("shift", "both"):
        net.set_light_center(LC)
        light["light_center"] = LC
    if which in ("rotation", "both"):
        net.set_rot_center(RC)
        net.set_rot(ROT)
        light["rot"], light["rot_center"] = ROT, RC
    want = _record_from_frame_args(net, batch)
    for th in (batch["Th"][0], batch["Th"][0].reshape(-1, 3).mean(0)):      # Th itself or its mean
        got = _lib.light_records([light], th, "cpu")
        assert got.shape == (1, 12) and got.dtype == torch.float32
        assert np.array_equal(got[0].numpy(), want), (got, want)


def test_light_records_stack_and_reject_half_a_rotation():
    from dsnerf_amd import _lib
    th = torch.tensor([0.2, -0.1, 1.0])
    recs = _lib.light_records([{}, {"light_center": LC}, {"rot": ROT, "rot_center": RC}], th, "cpu")
    assert recs.shape == (3, 12)
    assert recs[0].abs().sum() == 0 and recs[1, 0] == 1 and recs[1, 4] == 0 and recs[2, 0] == 0 and recs[2, 4] == 1
    with pytest.raises(ValueError):
        _lib.light_records([{"rot": ROT}], th, "cpu")
    with pytest.raises(ValueError):
        _lib.light_records([{"rot_center": RC}], th, "cpu")
    with pytest.raises(ValueError):
        _lib.light_records([{"centre": LC}], th, "cpu")
    with pytest.raises(ValueError):
        _lib.light_records([], th, "cpu")


def test_sweep_entry_points_are_exported(lib):
    import dsnerf_amd
    for n in ("dsn_render_lights_scratch_bytes", "dsn_render_rays_lights"):
        assert hasattr(lib, n) and n in dsnerf_amd._lib.EXPORTS


def test_scratch_bytes(lib):
    f = lib.dsn_render_lights_scratch_bytes
    R, S = 512 * 512, 64
    assert f(0, S, 1, 10) == 0 and f(R, 0, 1, 10) == 0 and f(R, S, 0, 10) == 0 and f(R, S, 1, -1) == 0
    assert f(R, S, 1, R * S + 1) == 0                             # more shaded samples than samples
    one = f(R, S, 1, 1_000_000)
    assert one >= 12 * 1_000_000 and one % 256 == 0
    assert f(R, S, 10, 1_000_000) >= 10 * 12 * 1_000_000 > one
    assert f(R, S, 10, 2_000_000) > f(R, S, 10, 1_000_000)
    assert f(R, S, 4, 1_000_000) < f(R, S, 10, 1_000_000)


def _call(lib, R=64, S=64, flags=1, lights=1, n_lights=1, jitter=None, noise=None, scratch=1, scratch_bytes=1 << 20, null=()):
    """dsn_render_rays_lights with fake non-null pointers (every check runs before the device is touched)"""
    p = C.c_void_p(256)
    a = {k: (None if k in null else p) for k in ("scene", "packed", "ray_o", "ray_d", "near", "far", "t_vals", "out_rgb", "out_disp",
                                                 "out_acc", "out_depth", "workspace")}
    return lib.dsn_render_rays_lights(a["scene"], 1, 1, a["packed"], a["ray_o"], a["ray_d"], a["near"], a["far"], R, S, a["t_vals"],
                                      jitter, noise, flags, C.c_void_p(256) if lights else None, n_lights, a["out_rgb"], a["out_disp"],
                                      a["out_acc"], a["out_depth"], None, None, a["workspace"], C.c_size_t(0),
                                      C.c_void_p(256) if scratch else None, C.c_size_t(scratch_bytes), None, 0, None)


@pytest.mark.parametrize("case,words", [
    (dict(null=("scene",)), b"null argument"),
    (dict(null=("out_rgb",)), b"null output"),
    (dict(lights=0), b"null argument"),
    (dict(scratch=0), b"null argument"),
    (dict(R=0), b"empty ray batch"),
    (dict(n_lights=0), b"n_lights"),
    (dict(jitter=C.c_void_p(256)), b"no jitter"),
    (dict(noise=C.c_void_p(256)), b"no noise"),
    (dict(flags=0), b"DSN_SKIP_TRANSPARENT"),
    (dict(flags=1 | 4), b"DSN_FIELD_FP32"),
    (dict(flags=1 | 256), b"DSN_PHASE_"),
    (dict(flags=1 | 1024), b"DSN_PHASE_"),
    (dict(S=32), b"S must be 64 or 128"),
    (dict(scratch_bytes=16), b"light_scratch is too small"),
])
def test_render_rays_lights_rejects_bad_arguments(lib, case, words):
    assert _call(lib, **case) != 0
    err = lib.dsn_last_error()
    assert b"dsn_render_rays_lights" in err and words in err, err


def test_renderer_sweep_needs_eval_mode_and_lights():
    """the Renderer's checks come before any device work (the Renderer itself needs a GPU: its methods are called unbound here)"""
    import dsnerf_amd
    from types import SimpleNamespace
    fake = SimpleNamespace(net=SimpleNamespace(training=False), skip_transparent=True)
    with pytest.raises(ValueError, match="no lights"):
        dsnerf_amd.Renderer.render_view_lights(fake, {}, [])
    fake.net.training = True
    with pytest.raises(RuntimeError, match="eval mode"):
        dsnerf_amd.Renderer.render_view_lights(fake, {}, [{}])
    fake.net.training = False
    fake.skip_transparent = False
    with pytest.raises(RuntimeError, match="skip_transparent"):
        dsnerf_amd.Renderer.render_view_lights(fake, {}, [{}])
