"""GPU tests of the relighting sweep (dsn_render_rays_lights / Renderer.render_view_lights): one geometry / field / normal pass, K
lights.  Every light's image must be BIT-IDENTICAL to render_view with that light set on the net - same early-stop plan, same density
screen, same colour scale - and the reference's vis_lighting.py loop (ten rotations of the light about the head) must match on the
bench frame."""
import numpy as np
import pytest
import torch

from helpers import maxdiff, state
from test_gpu_round2 import _oracle_subset, full_frame, renderer_with

pytestmark = pytest.mark.gpu
KEYS = ("coarse_color", "coarse_disp", "coarse_acc", "coarse_depth")
HEAD = torch.tensor([[0.18649693, -0.14180326, 1.7103844]])          # vis_lighting.py:57


def angle2rot(angle):                                                # vis_lighting.py:86-91
    rad = np.pi * angle / 180
    return np.array([[np.cos(rad), -np.sin(rad)], [np.sin(rad), np.cos(rad)]])


def five_lights():
    rot = torch.Tensor(angle2rot(72))
    return [{}, {"light_center": torch.tensor([0.35, 0.05, 1.4])}, {"rot": rot, "rot_center": HEAD},
            {"light_center": torch.tensor([-0.3, 0.4, 0.9]), "rot": torch.Tensor(angle2rot(252)), "rot_center": HEAD},
            {"light_center": torch.tensor([6.0, -4.0, 9.0])}]


def set_light(net, lt):
    net.light_center = lt["light_center"].cuda() if "light_center" in lt else None
    net.rot = lt["rot"].cuda() if "rot" in lt else None
    net.rot_center = lt["rot_center"].cuda() if "rot_center" in lt else None


def references(r, batch, lights, **kw):
    """render_view per light with the light set on the net (then cleared)"""
    out = []
    for lt in lights:
        set_light(r.net, lt)
        out.append({k: v.clone() for k, v in r.render_view(dict(batch), device_output=True, **kw).items()})
    set_light(r.net, {})
    return out


def same_bits(a, b):
    """torch.equal on the bit patterns (disp is NaN where acc is 0, like the reference's)"""
    return torch.equal(a.to(b.device).contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_same(got, want, keys=KEYS):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        for k in keys:
            assert same_bits(a[k], b[k]), (i, k, float((a[k].to(b[k].device) - b[k]).abs().nan_to_num().max()))


def warm(r, batch):
    r.render_view(dict(batch))       # probe frame (early-stop statistics, colour scale) + screen calibration; synchronised
    r._read_stop_probe(wait=True)    # (what the next frame would pick up: the colour scale is set from here on)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("screen", [True, False])
def test_sweep_is_bit_identical_per_light(early_stop, screen):
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, density_screen=screen)
    r.early_stop = early_stop
    r.eval()
    warm(r, batch)
    lights = five_lights()
    want = references(r, batch, lights)
    got = r.render_view_lights(dict(batch), lights, device_output=True)
    assert_same(got, want)
    info = r.last_frame_info
    assert info["lights"] == 5 and info["early_stop"] == early_stop and not info["rendered_again_in_one_pass"]
    # the light edits reach the pixels: the shifted lights differ from the plain one
    assert not torch.equal(got[0]["coarse_color"], got[1]["coarse_color"])
    assert not torch.equal(got[0]["coarse_color"], got[4]["coarse_color"])


def test_bench_frame_vis_lighting_angles():
    """the w4 bench frame (512 x 512 x 64), vis_lighting.py's ten angles about the head: each equals its render_view; two of them
    against the oracle on 768 rays (colour and weights, 1e-4)"""
    from dsnerf_amd import _lib
    canon, faces, batch = full_frame(hw=512)
    sd = state("x_w4")
    r = renderer_with(sd, canon, faces, density_screen=False)
    r.eval()
    warm(r, batch)
    lights = [{"rot": torch.Tensor(angle2rot(a)), "rot_center": HEAD} for a in range(0, 360, 36)]
    want = references(r, batch, lights)
    got = r.render_view_lights(dict(batch), lights, device_output=True)
    assert_same(got, want)
    assert r.last_frame_info["lights"] == 10
    # two angles against the oracle: the per-ray sweep in one pass (colour of every light, the shared weights)
    S, sel = 64, np.linspace(0, 512 * 512 - 1, 768).astype(np.int64)
    r._set_frame(batch)
    pk = r.net.packed(r.device)
    o, d = r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0])
    n, f = r._dev(batch["near"][0]).clone(), r._dev(batch["far"][0]).clone()
    two = [lights[3], lights[7]]
    out = _lib.render_rays_lights(r.scene, pk, _lib.RenderWorkspace(r.device), o, d, n, f, S, r._t_vals(S),
                                  _lib.light_records(two, None, r.device))
    si = torch.from_numpy(sel).cuda()
    for k, lt in enumerate(two):
        e = _oracle_subset(batch, canon, faces, sd, S, sel, sd["nerf.embedding.weight"][5], rot=lt["rot"].numpy(),
                           rot_center=HEAD.numpy()[0, :2])
        assert maxdiff(out["color"][k][si].cpu().numpy(), e["color"]) < 1e-4
        assert maxdiff(out["weights"][si].cpu().numpy(), e["weights"]) < 1e-4


def test_group_boundaries():
    """K = 1 and K = 2 G + 1 lights with the scratch sized for G = 2 lights: three groups, the same per-light pixels as one light at
    a time and as render_view"""
    from dsnerf_amd import _lib
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, density_screen=False)
    r.early_stop = False
    r.eval()
    warm(r, batch)
    lights = five_lights()
    want = references(r, batch, lights)
    pk = r.net.packed(r.device)
    S = 64
    o, d = r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0])
    n0, f0 = r._dev(batch["near"][0]), r._dev(batch["far"][0])
    ws = _lib.RenderWorkspace(r.device)
    recs = _lib.light_records(lights, batch["Th"][0], r.device)
    r.scene.set_frame(pk, r._dev(batch["xyz"][0]), r._dev(batch["poses"][0]), 5, False, None, None, None)
    r._frame_src = None

    def sweep(rows, **kw):
        return _lib.render_rays_lights(r.scene, pk, ws, o, d, n0.clone(), f0.clone(), S, r._t_vals(S), recs[rows].contiguous(), **kw)

    singles = [sweep(slice(k, k + 1)) for k in range(5)]
    n_shaded = int(ws.buf[:256].view(torch.int32)[_lib.CNT_POS])
    assert n_shaded > 0
    two = 2 * 12 * n_shaded + 12                      # holds two lights' colours, not three
    grouped = sweep(slice(0, 5), scratch_bytes=two)
    mask = r._dev(batch["mask_at_box"][0], torch.uint8)
    for k in range(5):
        assert torch.equal(grouped["color"][k], singles[k]["color"][0]), k
        img = _lib.image_scatter(dict(singles[k], color=singles[k]["color"][0]), mask, 160, 160)
        assert torch.equal(img["coarse_color"], want[k]["coarse_color"]), k
    for key in ("disp_map", "acc_map", "depth_map", "weights", "z_vals"):
        assert same_bits(grouped[key], singles[0][key]), key
    with pytest.raises(RuntimeError, match="light_scratch is too small"):
        sweep(slice(0, 5), scratch_bytes=12 * n_shaded - 256)


def test_hand_over_renders_the_sweep_again_in_one_pass():
    """w4 with the early-stop colour scale forced down to 1: the sliced sweep weighs colours above it (this checkpoint's probe frame
    reaches 1.32 -> scale 2.64), warns, is rendered again in one pass, and each image equals a one-pass render_view of its light"""
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state("x_w4"), canon, faces, density_screen=False)
    r.early_stop = True
    r.eval()
    warm(r, batch)
    pk = r.net.packed(r.device)
    assert pk.colour_scale > 1.0
    lights = five_lights()[:3]
    pk.set_early_stop_colour_scale(min(1.0, 0.4 * pk.colour_scale))      # (below the largest colour: scale = 2 x that)
    with pytest.warns(UserWarning, match="rendered again in one pass"):
        got = r.render_view_lights(dict(batch), lights, device_output=True)
    assert r.last_frame_info["rendered_again_in_one_pass"] and r.last_frame_info["lights"] == 3
    assert not r.last_frame_info["early_stop"] and pk.colour_scale > 1.0
    r.early_stop = False
    assert_same(got, references(r, batch, lights))


def test_record_overflow_pass(monkeypatch):
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, density_screen=False)
    r.eval()
    warm(r, batch)
    lights = five_lights()
    full = r.render_view_lights(dict(batch), lights, device_output=True)
    monkeypatch.setenv("DSN_RECORD_CAP", "5000")
    capped = r.render_view_lights(dict(batch), lights, device_output=True)
    assert_same(capped, full)


def test_no_side_effects_and_errors():
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, density_screen=False)
    r.eval()
    lc = torch.tensor([0.1, 0.2, 1.1])
    r.net.set_light_center(lc)
    held = r.net.light_center
    warm(r, batch)
    before = r.render_view(dict(batch))
    got = r.render_view_lights(dict(batch), five_lights())
    assert r.net.light_center is held and torch.equal(held.cpu(), lc) and r.net.rot is None and r.net.rot_center is None
    after = r.render_view(dict(batch))
    for k in KEYS:
        assert same_bits(before[k], after[k]), k
    assert all(set(g) == set(KEYS) and g["coarse_color"].device.type == "cpu" for g in got)
    with pytest.raises(ValueError):
        r.render_view_lights(dict(batch), [])
    r.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        r.render_view_lights(dict(batch), [{}])
