"""GPU tests of the relighting sweep (dsn_render_rays_lights / Renderer.render_view_lights): one geometry / field / normal pass, K
lights.  Every light's image must be BIT-IDENTICAL to render_view with that light set on the net - same early-stop plan, same density
screen, same colour scale - and the reference's vis_lighting.py loop (ten rotations of the light about the head) must match on the
bench frame.  Both compositor widths are covered: S = 64 (k_composite16_multi<4>) and S = 128 (k_composite16_multi<8>) - bit identity,
group boundaries and the oracle.  The oracle also pins light-centre shifts, rotations and combined edits on the default and the w3
parameters, independently of render_view (which shares the sweep's arithmetic).  Chunked sweeps (the [K, R, 3] colours joined along
the ray axis), an empty shading list and ray counts that are not multiples of the compositor's 16 rays per workgroup (R = 5, 37)
complete it."""
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
    group_boundaries(64, 2)


@pytest.mark.parametrize("scratch_lights", [2, 5])
def test_group_boundaries_at_128_samples(scratch_lights):
    """the same at S = 128 (k_composite16_multi<8>): scratch for two lights (groups of 2, 2, 1) and for all five (one group)"""
    group_boundaries(128, scratch_lights)


def group_boundaries(S, scratch_lights):
    from dsnerf_amd import _lib
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, S=S, density_screen=False)
    r.early_stop = False
    r.eval()
    warm(r, batch)
    lights = five_lights()
    want = references(r, batch, lights)
    pk = r.net.packed(r.device)
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
    scratch = scratch_lights * 12 * n_shaded + 12      # holds `scratch_lights` lights' colours, not one more
    grouped = sweep(slice(0, 5), scratch_bytes=scratch)
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


@pytest.mark.parametrize("early_stop", [True, False])
def test_sweep_is_bit_identical_per_light_at_128_samples(early_stop):
    """S = 128 (k_composite16_multi<8>, k_composite16<false, 8> in render_view): the five lights, each image equal to render_view's"""
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, S=128)
    r.early_stop = early_stop
    r.eval()
    warm(r, batch)
    lights = five_lights()
    want = references(r, batch, lights)
    got = r.render_view_lights(dict(batch), lights, device_output=True)
    assert_same(got, want)
    info = r.last_frame_info
    assert info["lights"] == 5 and info["early_stop"] == early_stop and not info["rendered_again_in_one_pass"]
    assert not torch.equal(got[0]["coarse_color"], got[1]["coarse_color"])


def edit_lights():
    """a light-centre shift, a rotation about the head and the two combined"""
    return [{"light_center": torch.tensor([0.35, 0.05, 1.4])}, {"rot": torch.Tensor(angle2rot(72)), "rot_center": HEAD},
            {"light_center": torch.tensor([-0.3, 0.4, 0.9]), "rot": torch.Tensor(angle2rot(252)), "rot_center": HEAD}]


@pytest.mark.parametrize("wname", ["", "x_w3"])
@pytest.mark.parametrize("S", [64, 128])
def test_sweep_matches_oracle_per_light(S, wname):
    """one sweep of three light edits on a 256 x 256 frame against the oracle on 768 rays spread over it: z_vals bit for bit, every
    light's colour and the shared weights / acc within 1e-4 (w3 - |sigma| ~ 1e3, colours in the hundreds: the colour within 2e-5 x its
    largest magnitude, as test_gpu_render grants the one-light frame)"""
    from dsnerf_amd import _lib
    hw = 256
    canon, faces, batch = full_frame(hw=hw)
    sd = state(wname or None)
    r = renderer_with(sd, canon, faces, S=S, density_screen=False)
    r.eval()
    r._set_frame(batch)
    pk = r.net.packed(r.device)
    o, d = r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0])
    n, f = r._dev(batch["near"][0]).clone(), r._dev(batch["far"][0]).clone()
    lights = edit_lights()
    out = _lib.render_rays_lights(r.scene, pk, _lib.RenderWorkspace(r.device), o, d, n, f, S, r._t_vals(S),
                                  _lib.light_records(lights, batch["Th"][0], r.device))
    sel = np.linspace(0, hw * hw - 1, 768).astype(np.int64)
    si = torch.from_numpy(sel).cuda()
    th = batch["Th"][0].reshape(-1, 3).mean(0).numpy()
    code = sd["nerf.embedding.weight"][5]
    for k, lt in enumerate(lights):
        kw = {}
        if "light_center" in lt:
            kw["light_shift"] = lt["light_center"].numpy() - th
        if "rot" in lt:
            kw.update(rot=lt["rot"].numpy(), rot_center=lt["rot_center"].numpy()[0, :2])
        e = _oracle_subset(batch, canon, faces, sd, S, sel, code, **kw)
        tol = 1e-4 if not wname else 2e-5 * float(np.abs(e["color"]).max())
        print(k, "colour %.1e (bar %.1e)" % (maxdiff(out["color"][k][si].cpu().numpy(), e["color"]), tol),
              "weights %.1e" % maxdiff(out["weights"][si].cpu().numpy(), e["weights"]))
        assert float(np.abs(e["color"]).max()) > 0.05 and float(e["acc_map"].max()) > 0.05
        assert maxdiff(out["color"][k][si].cpu().numpy(), e["color"]) < tol, (k, maxdiff(out["color"][k][si].cpu().numpy(), e["color"]), tol)
        if k == 0:
            assert np.array_equal(out["z_vals"][si].cpu().numpy(), e["z_vals"])
            assert maxdiff(out["weights"][si].cpu().numpy(), e["weights"]) < 1e-4
            assert maxdiff(out["acc_map"][si].cpu().numpy(), e["acc_map"]) < 1e-4
    # the edits reach the pixels
    assert not torch.equal(out["color"][0], out["color"][1]) and not torch.equal(out["color"][1], out["color"][2])


@pytest.mark.parametrize("S", [64, 128])
def test_chunked_sweep_equals_chunked_render_view(S):
    """render_view_lights(chunk=c) with a chunk that does not divide the 25 600 rays: the per-chunk colours are joined along the ray
    axis of the [K, R, 3] sweep output (Renderer._render_chunks, color_axis=1); each light equals render_view(chunk=c)"""
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, S=S)
    r.eval()
    warm(r, batch)
    lights = five_lights()
    chunk = 7000
    want = references(r, batch, lights, chunk=chunk)
    got = r.render_view_lights(dict(batch), lights, chunk=chunk, device_output=True)
    assert_same(got, want)
    assert not torch.equal(got[0]["coarse_color"], got[4]["coarse_color"])


def test_sweep_with_an_empty_shading_list():
    """rays that never come near the body (as test_gpu_render.test_all_transparent_frame): the shading list is empty, the sweep still
    runs (per_light == 0 in dsn_render_rays_lights), every light gives zero colour, acc 0, NaN disparity - render_view's images"""
    from dsnerf_amd import _lib
    hw = 8
    R = hw * hw
    canon, faces, batch = full_frame(hw=hw)
    o = np.tile(np.array([[5.0, 5.0, 5.0]], np.float32), (R, 1))
    d = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (R, 1))
    batch.update(ray_o=torch.from_numpy(o)[None], ray_d=torch.from_numpy(d)[None], near=torch.full((1, R), 1.0),
                 far=torch.full((1, R), 2.0))
    r = renderer_with(state(), canon, faces, density_screen=False)
    r.early_stop = False
    r.eval()
    lights = five_lights()
    want = references(r, batch, lights)
    got = r.render_view_lights(dict(batch), lights, device_output=True)
    assert int(r._ws.buf[:256].view(torch.int32)[_lib.CNT_POS]) == 0       # (nothing on the shading list)
    assert_same(got, want)
    for g in got:
        assert float(g["coarse_color"].abs().max()) == 0.0 and float(g["coarse_acc"].abs().max()) == 0.0
        assert bool(torch.isnan(g["coarse_disp"]).all())


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("R", [5, 37])
def test_ragged_ray_counts_equal_single_light_renders(R, S):
    """R = 5 (fewer rays than the compositor's 16 per workgroup) and R = 37 (two full workgroups and a partial one) through
    _lib.render_rays_lights: each light's colours and the shared outputs equal _lib.render_rays with that light set, bit for bit"""
    from dsnerf_amd import _lib
    hw = 160
    canon, faces, batch = full_frame(hw=hw)
    r = renderer_with(state(), canon, faces, S=S, density_screen=False)
    r.eval()
    pk = r.net.packed(r.device)
    ws = _lib.RenderWorkspace(r.device)
    # R - 1 rays that hit the body, spread over it, and one that misses it
    r._set_frame(batch)
    acc = _lib.render_rays(r.scene, pk, ws, r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0]), r._dev(batch["near"][0]).clone(),
                           r._dev(batch["far"][0]).clone(), S, r._t_vals(S))["acc_map"].cpu()
    hit, miss = torch.nonzero(acc > 0.5)[:, 0], torch.nonzero(acc == 0)[:, 0]
    sel = torch.cat([hit[torch.from_numpy(np.linspace(0, len(hit) - 1, R - 1).astype(np.int64))], miss[:1]])
    o, d = r._dev(batch["ray_o"][0][sel]), r._dev(batch["ray_d"][0][sel])
    n0, f0 = r._dev(batch["near"][0][sel]), r._dev(batch["far"][0][sel])
    lights = five_lights()
    singles = []
    for lt in lights:
        set_light(r.net, lt)
        r._set_frame(batch)
        singles.append({k: v.clone() for k, v in _lib.render_rays(r.scene, pk, ws, o, d, n0.clone(), f0.clone(), S, r._t_vals(S)).items()})
    set_light(r.net, {})
    r.scene.set_frame(pk, r._dev(batch["xyz"][0]), r._dev(batch["poses"][0]), 5, False, None, None, None, fine_only=True)
    r._frame_src = None
    sweep = _lib.render_rays_lights(r.scene, pk, ws, o, d, n0.clone(), f0.clone(), S, r._t_vals(S),
                                    _lib.light_records(lights, batch["Th"][0], r.device))
    assert sweep["color"].shape == (5, R, 3)
    assert float(singles[0]["acc_map"][:-1].min()) > 0.5 and float(singles[0]["acc_map"][-1]) == 0.0
    for k in range(5):
        assert same_bits(sweep["color"][k], singles[k]["color"]), (k, float((sweep["color"][k] - singles[k]["color"]).abs().max()))
    for key in ("disp_map", "acc_map", "depth_map", "weights", "z_vals"):
        assert same_bits(sweep[key], singles[0][key]), key
    assert not torch.equal(sweep["color"][0], sweep["color"][1])
