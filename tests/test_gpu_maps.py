"""GPU tests of the decomposition maps (dsn_render_rays_maps / dsn_composite_maps / dsn_shade_factor, Renderer.render_view_maps): the
albedo, shading and normal maps of a view from the frame's own pass.

  albedo[r] = sum w_i e_i     normal[r] = sum w_i n_i (not renormalised)     shading[k][r] = sum w_i L_{k,i}

over the frame's shading list, w the compositing weights.  Checked stage by stage and end to end against the float64 restatement
(maps_restate.py) of the REFERENCE's per-sample arrays (the golden cases + tests/golden/maps_light.npz), against the C oracle on the
w4 bench frame, for bit identity with render_view / render_view_lights, for invariance under the grouping of the lights, chunking
and ray counts, and - with early stop - against the bound the call reports (last_frame_info["maps_bound"]).

Bars (none of them measured on the code under test): stage parity 2e-6 max(1, max|map|) - test_composite's bar for rgb_map, the same
sums; the light factor 1e-5 max(1, max L) - test_shade's; end to end 1e-4 max(1, max|map|) for albedo and shading - the project's
colour bar with test_composite's scaling - and 1e-4 absolute for the normal map; with early stop each grows by the call's maps_bound
and by nothing else.  The S = 16 golden cases take the stage entries only: the frame entry is the 16-lane compositor's (S = 64 / 128).
"""
import os

import numpy as np
import pytest
import torch

import maps_restate as MR
import oracle as O
from helpers import ALL_CASES, GOLDEN, load, maxdiff, state
from test_gpu_relight import HEAD, KEYS, angle2rot, assert_same, five_lights, same_bits, warm
from test_gpu_round2 import _oracle_subset, full_frame, renderer_with
from test_gpu_stages import T, W, ctx, scene_for  # noqa: F401  (ctx: the module fixture of the stage tests)

pytestmark = pytest.mark.gpu
EVAL_CASES = [c for c in ALL_CASES if "train" not in c]
S64_CASES = [c for c in EVAL_CASES if c.startswith("full_")]
MAPS = ("albedo", "shading", "normal")


def light_of(name):
    return np.load(os.path.join(GOLDEN, "maps_light.npz"))["light:" + name]


def big(a):
    return max(1.0, float(np.abs(a).max()))


def reference_maps(g, name):
    """the restatement from the reference's per-sample arrays of a golden case (its one-pass shading list: sigma > 0, not transparent)"""
    listed = MR.listed_samples(g["sigma"].reshape(g["weights"].shape), g["transparent"].reshape(g["weights"].shape))
    return MR.maps(g["weights"], g["essence"], g["n_w"], light_of(name), listed), listed


# ------------------------------------------------------------------------------------------------------------------------
# 1. stage parity
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EVAL_CASES)
def test_composite_maps_stage(ctx, name):
    g = load(name)
    dev = ctx["dev"]
    R, S = g["weights"].shape
    L = light_of(name)
    tm = T(g["transparent"].reshape(R, S).astype(np.uint8), dev)
    alb, nrm, shd, w, mx = ctx["lib"].composite_maps(T(g["essence"], dev), T(g["n_w"], dev), T(L, dev), T(g["sigma"], dev), tm,
                                                     T(g["z_vals"], dev), T(g["ray_d"], dev))
    want, listed = reference_maps(g, name)
    got = {"albedo": alb.cpu().numpy(), "normal": nrm.cpu().numpy(), "shading": shd.cpu().numpy()[None]}
    for k in MAPS:
        err, bar = maxdiff(got[k], want[k]), 2e-6 * big(want[k])
        print(name, k, "%.2e (bar %.2e)" % (err, bar))
        assert err < bar, (name, k, err, bar)
    assert maxdiff(w.cpu().numpy(), g["weights"]) < 2e-6
    # the two maxima are those of the listed samples, exactly (the kernel only compares)
    em, lm = MR.weighed_max(g["essence"], L, listed)
    assert float(mx[0]) == np.float32(em) and float(mx[1]) == np.float32(lm), (mx, em, lm)
    # rubbish off the list never reaches a product
    e2, n2, L2 = g["essence"].copy(), g["n_w"].copy(), L.copy()
    off = ~listed.reshape(-1)
    e2[off], n2[off], L2[off] = np.nan, np.inf, np.nan
    again = ctx["lib"].composite_maps(T(e2, dev), T(n2, dev), T(L2, dev), T(g["sigma"], dev), tm, T(g["z_vals"], dev), T(g["ray_d"], dev))
    for a, b in zip(again, (alb, nrm, shd, w, mx)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["full_eval", "full_eval_w3"])
def test_composite_maps_wave_form_on_unaligned_arrays(ctx, name):
    """S = 64 arrays that are not 16-byte aligned take the one-wave-per-ray form (what every S other than 64 / 128 takes): the same
    maps at the stage bar, the same maxima"""
    g = load(name)
    dev = ctx["dev"]
    R, S = g["weights"].shape
    L = light_of(name)

    def shifted(a):      # a copy of the array that starts 4 bytes into an allocation
        t = T(a, dev).reshape(-1)
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
        buf[1:].copy_(t)
        return buf[1:].reshape(a.shape)

    tm = T(g["transparent"].reshape(R, S).astype(np.uint8), dev)
    args = (T(g["essence"], dev), T(g["n_w"], dev), T(L, dev))
    a16 = ctx["lib"].composite_maps(*args, T(g["sigma"], dev), tm, T(g["z_vals"], dev), T(g["ray_d"], dev))
    sg, zv = shifted(g["sigma"]), shifted(g["z_vals"])
    assert sg.data_ptr() % 16 != 0 and zv.data_ptr() % 16 != 0
    aw = ctx["lib"].composite_maps(*args, sg, tm, zv, T(g["ray_d"], dev))
    want, _ = reference_maps(g, name)
    for got, k in ((aw[0], "albedo"), (aw[1], "normal"), (aw[2][None], "shading")):
        assert maxdiff(got.cpu().numpy(), want[k]) < 2e-6 * big(want[k]), (name, k)
    assert torch.equal(aw[4], a16[4])
    assert maxdiff(aw[3].cpu().numpy(), g["weights"]) < 2e-6


@pytest.mark.parametrize("name", EVAL_CASES)
def test_shade_returns_the_light_factor(ctx, name):
    g = load(name)
    dev, S = ctx["dev"], int(g["S"])
    sc = scene_for(ctx, g, name)
    a = (sc, W(ctx, name)["packed"], T(g["x_c"], dev), T(g["grad_sigma"], dev), T(g["pts"], dev), T(g["ray_d"], dev), T(g["essence"], dev), S)
    idx, n_w, col = ctx["lib"].shade(*a)
    idx2, n_w2, col2, fac = ctx["lib"].shade(*a, want_factor=True)
    assert torch.equal(idx, idx2) and torch.equal(n_w, n_w2) and same_bits(col, col2)
    L = light_of(name)
    err, bar = maxdiff(fac.cpu().numpy(), L), 1e-5 * big(L)
    print(name, "factor %.2e (bar %.2e)" % (err, bar))
    assert err < bar, (name, err, bar)
    # the colour is the factor times the essence, in one float32 product
    assert same_bits(col2, fac[:, None] * T(g["essence"], dev))
    with pytest.raises(ValueError):
        ctx["lib"].shade(*a, want_factor=True, fp32=True)


# ------------------------------------------------------------------------------------------------------------------------
# 2. end to end on the golden rays
# ------------------------------------------------------------------------------------------------------------------------
def golden_frame(ctx, name):
    g = load(name)
    dev, _lib = ctx["dev"], ctx["lib"]
    sd = state(name)
    pk = _lib.PackedParams(dev).update({k: torch.from_numpy(v) for k, v in sd.items()})      # (its own: the colour scale is set on it)
    sc = _lib.Scene(torch.from_numpy(g["canonical_vertex"]), torch.from_numpy(g["faces"].astype(np.int64)), dev)
    sc.set_frame(pk, torch.from_numpy(g["xyz"]), torch.from_numpy(g["poses"]), int(g["frame"]))
    S = int(g["S"])
    ws = _lib.RenderWorkspace(dev)
    recs = _lib.light_records([{}], None, dev)

    def call(**kw):
        return _lib.render_rays_maps(sc, pk, ws, T(g["ray_o"], dev), T(g["ray_d"], dev), T(g["near"].copy(), dev), T(g["far"].copy(), dev),
                                     S, torch.linspace(0.0, 1.0, steps=S).to(dev), recs, **kw)
    return g, pk, sc, ws, call


@pytest.mark.parametrize("screen", [False, True])
@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("name", S64_CASES)
def test_golden_rays_end_to_end(ctx, name, early_stop, screen):
    _lib = ctx["lib"]
    g, pk, sc, ws, call = golden_frame(ctx, name)
    S = int(g["S"])
    if screen:
        screen = bool(pk.calibrate_screen(sc)["safe"])      # (an unsafe margin is +inf: the screen would drop nothing)
    one = call(screen=screen)
    want, listed = reference_maps(g, name)
    bound = {k: 0.0 for k in MAPS}
    out = one
    if early_stop:
        # the threshold's colour scale as the Renderer sets it: headroom x the largest colour a one-pass frame weighed
        cmax = float(ws.buf[:256].view(torch.float32)[_lib.CNT_COLOUR_MAX])
        pk.set_early_stop_colour_scale(_lib.EARLY_STOP_COLOUR_HEADROOM * cmax)
        out = call(screen=screen, early_stop=True)
        eps = _lib.early_stop_eps(S, pk.colour_scale)
        mx = out["maps_max"].cpu().numpy()
        bound = {"albedo": _lib.maps_bound(S, eps, mx[0]), "shading": _lib.maps_bound(S, eps, mx[1]), "normal": _lib.maps_bound(S, eps, 1.0)}
    got = {k: out[k].cpu().numpy() for k in MAPS}
    for k in MAPS:
        bar = (1e-4 if k == "normal" else 1e-4 * big(want[k])) + bound[k]
        err = maxdiff(got[k], want[k])
        print(name, "early_stop", early_stop, "screen", screen, k, "%.2e (bar %.2e, of it the early-stop bound %.2e)" % (err, bar, bound[k]))
        assert err < bar, (name, k, err, bar, int(np.abs(got[k].reshape(want[k].shape) - want[k]).max(-1).argmax()))
    colour_bound = _lib.maps_bound(S, _lib.early_stop_eps(S, pk.colour_scale), pk.colour_scale) if early_stop else 0.0
    assert maxdiff(out["color"][0].cpu().numpy(), g["rgb_map"]) < 1e-4 * big(g["rgb_map"]) + colour_bound
    if not early_stop:
        # out_max: an upper bound of every |e| / L that entered a sum, and attained - against the reference's arrays on its list
        em, lm = MR.weighed_max(g["essence"], light_of(name), listed)
        mx = one["maps_max"].cpu().numpy()
        assert abs(mx[0] - em) < 1e-4 * max(1.0, em) and abs(mx[1] - lm) < 1e-4 * max(1.0, lm), (mx, em, lm)
        assert float(np.abs(g["essence"]).max()) > 0 and int(listed.sum()) > 0


# ------------------------------------------------------------------------------------------------------------------------
# 3. bit identity with what exists
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("screen", [True, False])
def test_maps_call_has_render_views_bits(early_stop, screen):
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, density_screen=screen)
    r.early_stop = early_stop
    r.eval()
    warm(r, batch)
    for setup in ("plain", "light_center", "rot"):
        if setup == "light_center":
            r.net.set_light_center(torch.tensor([0.35, 0.05, 1.4]))
        if setup == "rot":
            r.net.set_rot_center(HEAD)
            r.net.set_rot(torch.Tensor(angle2rot(72)))
        want = {k: v.clone() for k, v in r.render_view(dict(batch), device_output=True).items()}
        got = r.render_view_maps(dict(batch), device_output=True)
        assert set(got) == set(KEYS) | set(MAPS)
        assert_same([got], [want])
        info = r.last_frame_info
        assert info["maps"] == list(MAPS) and info["lights"] == 1 and info["early_stop"] == early_stop
        assert ("maps_bound" in info) == early_stop and not info["rendered_again_in_one_pass"]
        assert got["albedo"].shape == (160, 160, 3) and got["shading"].shape == (160, 160, 1) and got["normal"].shape == (160, 160, 3)
        assert float(got["albedo"].abs().max()) > 0.05 and float(got["normal"].abs().max()) > 0.05
    # a light edit moves the shading and the colour, not the albedo or the normal (same geometry, same field)
    r.net.light_center = r.net.rot = r.net.rot_center = None
    plain = r.render_view_maps(dict(batch), device_output=True)
    assert same_bits(plain["albedo"], got["albedo"]) and same_bits(plain["normal"], got["normal"])
    assert not torch.equal(plain["shading"], got["shading"])


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("screen", [True, False])
def test_maps_sweep_has_render_view_lights_bits(early_stop, screen):
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, density_screen=screen)
    r.early_stop = early_stop
    r.eval()
    warm(r, batch)
    lights = five_lights()
    want = [{k: v.clone() for k, v in img.items()} for img in r.render_view_lights(dict(batch), lights, device_output=True)]
    got = r.render_view_maps(dict(batch), lights=lights, device_output=True)
    assert_same(got, want)
    assert all(g["albedo"] is got[0]["albedo"] and g["normal"] is got[0]["normal"] for g in got)
    assert not torch.equal(got[0]["shading"], got[1]["shading"])
    assert r.last_frame_info["lights"] == 5 and r.last_frame_info["maps"] == list(MAPS)
    # a subset of the maps: the same bits for what is asked, nothing else in the dicts
    only = r.render_view_maps(dict(batch), lights=lights, maps=("shading",), device_output=True)
    assert set(only[0]) == set(KEYS) | {"shading"}
    assert_same(only, want)
    for a, b in zip(only, got):
        assert same_bits(a["shading"], b["shading"])


def frame_call(r, batch, S, lights, sel=None):
    """_lib.render_rays_maps / render_rays_lights on (a selection of) a frame's rays with the scene set as a sweep sets it"""
    from dsnerf_amd import _lib
    pk = r.net.packed(r.device)
    pick = (lambda t: t) if sel is None else (lambda t: t[sel])
    o, d = r._dev(pick(batch["ray_o"][0])), r._dev(pick(batch["ray_d"][0]))
    n0, f0 = r._dev(pick(batch["near"][0])), r._dev(pick(batch["far"][0]))
    recs = _lib.light_records(lights, batch["Th"][0], r.device)
    r.scene.set_frame(pk, r._dev(batch["xyz"][0]), r._dev(batch["poses"][0]), 5, False, None, None, None)
    r._frame_src = None
    ws = _lib.RenderWorkspace(r.device)

    def maps(rows=slice(None), **kw):
        return _lib.render_rays_maps(r.scene, pk, ws, o, d, n0.clone(), f0.clone(), S, r._t_vals(S), recs[rows].contiguous(), **kw)

    def sweep(rows=slice(None), **kw):
        return _lib.render_rays_lights(r.scene, pk, ws, o, d, n0.clone(), f0.clone(), S, r._t_vals(S), recs[rows].contiguous(), **kw)
    return maps, sweep, ws


@pytest.mark.parametrize("early_stop", [True, False])
def test_all_null_maps_equal_the_sweep(early_stop):
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, density_screen=False)
    r.eval()
    maps, sweep, _ = frame_call(r, batch, 64, five_lights())
    want = {k: v.clone() for k, v in sweep(early_stop=early_stop).items()}
    got = maps(maps=(), want_max=False, early_stop=early_stop)
    assert set(got) == set(want)
    for k in want:
        assert same_bits(got[k], want[k]), k
    # ... and with every map asked for the sweep's outputs keep those bits; without the colour the rest still does
    full = maps(early_stop=early_stop)
    for k in want:
        assert same_bits(full[k], want[k]), k
    bare = maps(want_color=False, early_stop=early_stop)
    assert "color" not in bare
    for k in ("albedo", "normal", "shading", "maps_max", "disp_map", "acc_map", "depth_map", "weights"):
        assert same_bits(bare[k], full[k]), k


# ------------------------------------------------------------------------------------------------------------------------
# 4. invariances
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 128])
def test_grouping_of_the_lights_does_not_change_a_bit(S):
    from dsnerf_amd import _lib
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, S=S, density_screen=False)
    r.eval()
    maps, _, ws = frame_call(r, batch, S, five_lights())
    whole = {k: v.clone() for k, v in maps().items()}
    n_shaded = int(ws.buf[:256].view(torch.int32)[_lib.CNT_POS])
    assert n_shaded > 0
    for G in (1, 2, 5):
        out = maps(scratch_bytes=G * 16 * n_shaded + 16)      # holds G lights' colours and factors, not one more
        for k in whole:
            assert same_bits(out[k], whole[k]), (G, k)
    singles = [maps(slice(k, k + 1)) for k in range(5)]
    for k in range(5):
        assert same_bits(singles[k]["shading"][0], whole["shading"][k]) and same_bits(singles[k]["color"][0], whole["color"][k]), k
        assert same_bits(singles[k]["albedo"], whole["albedo"]) and same_bits(singles[k]["normal"], whole["normal"]), k
    assert float(whole["maps_max"][1]) == max(float(s["maps_max"][1]) for s in singles)
    again = maps()
    for k in whole:
        assert same_bits(again[k], whole[k]), k
    with pytest.raises(RuntimeError, match="light_scratch is too small"):
        maps(scratch_bytes=16 * n_shaded - 256)


def test_chunked_equals_unchunked():
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces)
    r.early_stop = False      # (one pass: every ray's sums are its own, whatever else is in the call)
    r.eval()
    warm(r, batch)
    lights = five_lights()[:3]
    whole = r.render_view_maps(dict(batch), lights=lights, device_output=True)
    parts = r.render_view_maps(dict(batch), lights=lights, chunk=7000, device_output=True)
    assert_same(parts, whole, keys=KEYS + MAPS)
    one = r.render_view_maps(dict(batch), chunk=7000, device_output=True)
    assert_same([one], [r.render_view_maps(dict(batch), device_output=True)], keys=KEYS + MAPS)


@pytest.mark.parametrize("S", [64, 128])
def test_ragged_ray_counts(S):
    """R = 37 (two full workgroups of the compositor and a partial one) and R = 5 (fewer rays than one workgroup's 16): the five rays
    have the bits they have among the 37, colours and shared outputs equal the sweep's"""
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, S=S, density_screen=False)
    r.eval()
    lights = five_lights()
    maps_all, _, _ = frame_call(r, batch, S, lights)
    acc = maps_all(maps=(), want_max=False)["acc_map"].cpu()
    hit, miss = torch.nonzero(acc > 0.5)[:, 0], torch.nonzero(acc == 0)[:, 0]
    sel = torch.cat([hit[torch.from_numpy(np.linspace(0, len(hit) - 1, 36).astype(np.int64))], miss[:1]])
    sel = torch.cat([sel[:4], sel[-1:], sel[4:-1]])      # (the first five: four hits and the miss)
    m37, s37, _ = frame_call(r, batch, S, lights, sel)
    m5, _, _ = frame_call(r, batch, S, lights, sel[:5])
    a, b, c = m37(), m5(), s37()
    assert a["albedo"].shape == (37, 3) and a["shading"].shape == (5, 37) and b["shading"].shape == (5, 5)
    for k in ("color", "disp_map", "acc_map", "depth_map", "weights", "z_vals"):
        assert same_bits(a[k], c[k]), k
    assert same_bits(b["albedo"], a["albedo"][:5]) and same_bits(b["normal"], a["normal"][:5])
    assert same_bits(b["shading"], a["shading"][:, :5].contiguous()) and same_bits(b["color"], a["color"][:, :5].contiguous())
    assert float(a["albedo"][4].abs().max()) == 0.0 and float(a["normal"][4].abs().max()) == 0.0 and float(a["shading"][:, 4].abs().max()) == 0.0
    assert float(a["albedo"][:4].abs().min(0).values.max()) > 0.0


def test_empty_shading_list_gives_zero_maps():
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
    want = [{k: v.clone() for k, v in img.items()} for img in r.render_view_lights(dict(batch), lights, device_output=True)]
    got = r.render_view_maps(dict(batch), lights=lights, device_output=True)
    assert int(r._ws.buf[:256].view(torch.int32)[_lib.CNT_POS]) == 0
    assert_same(got, want)
    for g in got:
        for k in MAPS:
            assert float(g[k].abs().max()) == 0.0, k
        assert bool(torch.isnan(g["coarse_disp"]).all())
    maps, _, _ = frame_call(r, batch, 64, lights)
    assert maps()["maps_max"].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------------------------------
# 5. early stop
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname,hw", [("x_w4", 512), ("", 160)])
def test_sliced_maps_stay_within_the_reported_bound(wname, hw):
    canon, faces, batch = full_frame(hw=hw)
    r = renderer_with(state(wname or None), canon, faces, density_screen=False)
    r.early_stop = True
    r.eval()
    warm(r, batch)
    lights = five_lights()[:2]
    sliced = r.render_view_maps(dict(batch), lights=lights, device_output=True)
    info = r.last_frame_info
    assert info["early_stop"] and not info["rendered_again_in_one_pass"]
    bound = info["maps_bound"]
    S = 64
    assert bound["normal"] == (S + 1) * (info["early_stop_eps"] + 2.0 ** -22)
    assert bound["albedo"] == bound["normal"] * info["maps_max"]["essence"] and bound["shading"] == bound["normal"] * info["maps_max"]["light"]
    r.early_stop = False
    whole = r.render_view_maps(dict(batch), lights=lights, device_output=True)
    assert not r.last_frame_info["early_stop"] and "maps_bound" not in r.last_frame_info
    for a, b in zip(sliced, whole):
        for k in MAPS:
            err = float((a[k] - b[k]).abs().max())
            print(wname or "default", hw, k, "%.2e (bound %.2e)" % (err, bound[k]))
            assert err <= bound[k], (k, err, bound[k])
    # (early stop did leave something out, or the comparison says nothing)
    assert any(not torch.equal(a[k], b[k]) for a, b in zip(sliced, whole) for k in MAPS) or wname == ""


# ------------------------------------------------------------------------------------------------------------------------
# 6. the bench frame against the oracle
# ------------------------------------------------------------------------------------------------------------------------
def test_bench_frame_maps_match_the_oracle():
    """w4, 512 x 512 x 64, the 768 rays of test_bench_frame_vis_lighting_angles.  Oracle: O.render for z / weights, then O.warp ->
    O.field -> O.normal_world -> O.lighting(essence = 1) per sample, composited by the restatement.  Albedo and shading within
    1e-4 max(1, max|map|) on every ray; the normal map within 1e-4 on all but at most 2 % of the hit rays (acc > 1e-3), at least one
    allowed: a cap set beforehand from the real reference against this oracle on these rays (1 of 265 hit rays: an ill-conditioned
    normal), not from the code under test."""
    from dsnerf_amd import _lib
    canon, faces, batch = full_frame(hw=512)
    sd = state("x_w4")
    r = renderer_with(sd, canon, faces, density_screen=False)
    r.eval()
    S, sel = 64, np.linspace(0, 512 * 512 - 1, 768).astype(np.int64)
    lights = [{}, {"rot": torch.Tensor(angle2rot(108)), "rot_center": HEAD}]
    maps, _, _ = frame_call(r, batch, S, lights)
    out = maps()
    si = torch.from_numpy(sel).cuda()
    code = sd["nerf.embedding.weight"][5]
    e = _oracle_subset(batch, canon, faces, sd, S, sel, code)
    P = O.Params(sd)
    o, d = batch["ray_o"][0].numpy()[sel], batch["ray_d"][0].numpy()[sel]
    pts = (o[:, None, :] + d[:, None, :] * e["z_vals"][..., None]).astype(np.float32).reshape(-1, 3)
    dirs = np.repeat(d[:, None, :], S, 1).reshape(-1, 3)
    xyz = batch["xyz"][0].numpy()
    wr = O.warp(pts, dirs, xyz, canon, faces)
    sig, ess, gr = O.field(wr["x_c"], P, code, O.pose_feat(batch["poses"][0].numpy(), P)[1])
    _, nw = O.normal_world(wr["x_c"], gr, canon, xyz, faces)
    ones = np.ones_like(ess)
    L = np.stack([O.lighting(nw, pts, dirs, ones, P)[:, 0],
                  O.lighting(nw, pts, dirs, ones, P, rot=lights[1]["rot"].numpy(), rot_center=HEAD.numpy()[0, :2])[:, 0]])
    listed = MR.listed_samples(sig.reshape(-1, S), wr["transparent"].reshape(-1, S))
    want = MR.maps(e["weights"], ess, nw, L, listed)
    assert maxdiff(out["weights"][si].cpu().numpy(), e["weights"]) < 1e-4
    for k, got in (("albedo", out["albedo"][si]), ("shading", out["shading"][:, si])):
        err, bar = maxdiff(got.cpu().numpy(), want[k]), 1e-4 * big(want[k])
        print(k, "%.2e (bar %.2e)" % (err, bar))
        assert err < bar, (k, err, bar)
    nd = np.abs(out["normal"][si].cpu().numpy().astype(np.float64) - want["normal"]).max(-1)
    hit = e["acc_map"] > 1e-3
    over = np.nonzero(hit & (nd >= 1e-4))[0]
    cap = max(1, int(0.02 * int(hit.sum())))
    worst = int(nd.argmax())
    msg = "normal map: %d of %d hit rays at or above 1e-4 (cap %d); worst ray %d: %.2e" % (len(over), int(hit.sum()), cap, sel[worst], nd[worst])
    print(msg)
    assert int(hit.sum()) > 100 and float(nd[~hit].max(initial=0.0)) < 1e-4, msg
    assert len(over) <= cap, msg


# ------------------------------------------------------------------------------------------------------------------------
# 7. the render path is untouched
# ------------------------------------------------------------------------------------------------------------------------
def test_maps_call_leaves_the_renderer_as_it_was():
    canon, faces, batch = full_frame(hw=160)
    r = renderer_with(state(), canon, faces, density_screen=False)
    r.eval()
    lc = torch.tensor([0.1, 0.2, 1.1])
    r.net.set_light_center(lc)
    held = r.net.light_center
    warm(r, batch)
    lights = five_lights()
    before = r.render_view(dict(batch))
    sweep_before = r.render_view_lights(dict(batch), lights)
    got = r.render_view_maps(dict(batch))
    got_l = r.render_view_maps(dict(batch), lights=lights)
    assert r._frame_src is None
    assert r.net.light_center is held and torch.equal(held.cpu(), lc) and r.net.rot is None and r.net.rot_center is None
    after = r.render_view(dict(batch))
    sweep_after = r.render_view_lights(dict(batch), lights)
    assert_same([after], [before])
    assert_same(sweep_after, sweep_before)
    assert_same([got], [before])
    assert_same(got_l, sweep_before)
    assert set(got) == set(KEYS) | set(MAPS) and all(v.device.type == "cpu" for v in got.values())
    assert all(set(g) == set(KEYS) | set(MAPS) and g["albedo"] is got_l[0]["albedo"] for g in got_l)
    with pytest.raises(ValueError):
        r.render_view_maps(dict(batch), maps=("albedo", "depth"))
    with pytest.raises(ValueError):
        r.render_view_maps(dict(batch), maps=())
    r.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        r.render_view_maps(dict(batch))


def test_train_mode_render_after_a_maps_call_matches_its_golden():
    """the small_train case's Renderer: a maps call on its scene and workspace first (eval mode, the case's 64 rays as an 8 x 8 view
    at the 16-lane compositor's S = 64), then Renderer.render in train mode at the case's own S = 16 against the reference"""
    from cases import make_batch, make_renderer
    g = load("small_train")
    r = make_renderer(g, "small_train")
    S = int(g["S"])
    r.eval()
    view = make_batch(g)
    view["img"] = torch.zeros(1, 8, 8, 3, dtype=torch.float64)
    view["mask_at_box"] = torch.ones(1, 64, dtype=torch.bool)
    r.cfg.MODEL.COARSE_RAY_SAMPLING = 64
    m = r.render_view_maps(view, lights=five_lights()[:2])
    assert set(m[0]) == set(KEYS) | set(MAPS) and m[0]["albedo"].shape == (8, 8, 3) and float(m[0]["albedo"].abs().max()) > 0
    r.cfg.MODEL.COARSE_RAY_SAMPLING = S
    r.train()
    torch.manual_seed(233)
    out = {k: v.detach().cpu().numpy() for k, v in r.render(make_batch(g))["coarse"].items()}
    assert np.array_equal(out["z_vals"], g["render:z_vals"])
    for k, tol in (("color", 1e-4), ("acc_map", 1e-4), ("weights", 1e-4), ("depth_map", 3e-4)):
        assert maxdiff(out[k], g["render:" + k]) < tol, (k, maxdiff(out[k], g["render:" + k]), tol)
