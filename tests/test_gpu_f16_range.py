"""GPU tests of the split-fp16 range guard AT its edges (csrc/dsn_field16.hip header, DESIGN 4.1 "Range guard"): parameter sets
built so that values land next to each threshold rather than far beyond it, as tests/test_gpu_round2.py's overflowing_state does.
  * adjoint band: sigma-adjoints of the early trunk layers inside [2^15, 65 000) x 64 - the band where a reverse-pass split's
    lo = fp16((v - hi) 2^12) overflows while the value itself is below the forward guard - with small forward activations;
  * weight edge: one weight at 1023.5 (the largest the forward images hold) and at 1100 / 2000, in a trunk layer and the rgb head;
  * lighting band: hidden activations of the lighting MLP across 32 768 and 65 504.
Eval paths must give finite values, the exact-fp32 kernel's bits where they flag and the stage bars elsewhere; training counts."""
import numpy as np
import pytest
import torch

import train_oracle as TO
from helpers import load, state
from test_gpu_render import make_batch
from test_gpu_round2 import full_frame, renderer_with

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16_RANGE, F16_RANGE_SCALED = 65000.0, 32768.0
BAND = (F16_RANGE_SCALED * 64.0, F16_RANGE * 64.0)       # sigma-adjoints whose reverse-pass value g / 64 is in the scaled gap


def copy(sd):
    return {k: v.copy() for k, v in sd.items()}


def points(g, copies=9, seed=11):
    """the canonical points of full_eval plus seeded jitter: > 1e5 points"""
    rng = np.random.default_rng(seed)
    x = g["x_c"].astype(np.float32)
    xs = [x] + [x + rng.normal(0.0, 0.01, x.shape).astype(np.float32) for _ in range(copies - 1)]
    return np.concatenate(xs)


def trunk64(sd, g, x):
    """float64 restatement of the trunk (train_oracle's order): sigma, the 7 pre-activations (grad retained) and the activations"""
    p32 = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items() if k.startswith("pose_mlp")}
    pose = TO.linear(p32, "pose_mlp.4", torch.relu(TO.linear(p32, "pose_mlp.2", torch.relu(
        TO.linear(p32, "pose_mlp.0", TO.rod2quat(torch.from_numpy(g["poses"]), torch.float32))))))
    P = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV, torch.float64) for k, v in sd.items()}
    xc = torch.from_numpy(x).to(DEV, torch.float64)
    N = xc.shape[0]
    pe = TO.encode(xc)
    h = torch.cat([P["nerf.embedding.weight"][int(g["frame"])].expand(N, -1), pe, pose.detach().to(DEV, torch.float64).expand(N, -1)], -1)
    if torch.is_grad_enabled():
        h.requires_grad_(True)
    zs, hs = [], []
    for name in ["nerf.stage1.0", "nerf.stage1.2", "nerf.stage1.4", "nerf.stage1.6", "nerf.stage2.0", "nerf.stage2.2", "nerf.stage2.4"]:
        if name == "nerf.stage2.0":
            h = torch.cat([h, pe], -1)
        z = TO.linear(P, name, h)
        if z.requires_grad:
            z.retain_grad()
        zs.append(z)
        h = torch.relu(z)
        hs.append(h)
    sigma = TO.linear(P, "nerf.density_net.0", h)
    return sigma, zs, hs


def reverse_values(sd, g, x):
    """per layer: what k_field16's reverse pass splits - the relu-masked sigma-adjoints of stage1.0 .. stage2.2, times 2^-6 -
    and the per-sample forward maximum"""
    sigma, zs, hs = trunk64(sd, g, x)
    sigma.sum().backward()
    rev = [(z.grad * (z > 0)).abs() / 64.0 for z in zs[:6]]
    fmax = torch.stack([h.abs().amax(-1) for h in hs]).amax(0)
    return rev, fmax


def adjoint_band_state():
    """density head, stage2.4 and stage2.2 scaled up (biases with them: the relu patterns stay), weights <= 1023, so that the
    reverse-pass values of most samples peak inside the scaled gap [32 768, 65 000) while the forward activations stay small"""
    g = load("full_eval")
    x = points(g)
    sd0 = copy(state())
    wden = float(np.abs(sd0["nerf.density_net.0.weight"]).max())
    cd, c12 = 1000.0 / wden, 1.0

    def scaled():
        c = float(np.sqrt(c12))
        sd = copy(sd0)
        sd["nerf.density_net.0.weight"] *= np.float32(cd)
        sd["nerf.density_net.0.bias"] *= np.float32(cd * c12)
        sd["nerf.stage2.2.weight"] *= np.float32(c)
        sd["nerf.stage2.2.bias"] *= np.float32(c)
        sd["nerf.stage2.4.weight"] *= np.float32(c)
        sd["nerf.stage2.4.bias"] *= np.float32(c12)
        return sd

    for _ in range(2):      # (the top layer's adjoints scale with cd c, the ones below with cd c^2: two rounds settle the median)
        with torch.enable_grad():
            rev, _ = reverse_values(scaled(), g, x)
        amax = torch.stack([r.amax(-1) for r in rev]).amax(0)
        c12 *= 48000.0 / float(amax.median())
    return scaled(), g, x


def weight_edge_state(place, w):
    sd = copy(state())
    sd[{"trunk": "nerf.stage1.2.weight", "rgb": "nerf.rgb_net.1.weight", "light": "lighting_mlp.lights_encoding.2.weight"}[place]][3, 5] = \
        np.float32(w)
    return sd


def scene_for(sd, g):
    from dsnerf_amd import _lib
    packed = _lib.PackedParams(DEV).update({k: torch.from_numpy(v) for k, v in sd.items()})
    sc = _lib.Scene(torch.from_numpy(g["canonical_vertex"]), torch.from_numpy(g["faces"].astype(np.int64)), DEV)
    sc.set_frame(packed, torch.from_numpy(g["xyz"]), torch.from_numpy(g["poses"]), int(g["frame"]))
    return sc, packed


def check_field(sd, g, x_np):
    """_lib.field (single launch) and field_forward + field_reverse against the exact-fp32 kernel.  Returns the flagged fraction."""
    from dsnerf_amd import _lib
    sc, packed = scene_for(sd, g)
    x = torch.from_numpy(x_np).to(DEV)
    a = _lib.field(sc, packed, x, fp32=False)
    b = _lib.field(sc, packed, x, fp32=True)
    for t in a:
        assert bool(torch.isfinite(t).all()), "non-finite output of the split-fp16 field"
    same = (a[0] == b[0]) & (a[1] == b[1]).all(-1) & (a[2] == b[2]).all(-1)
    other = ~same
    if bool(other.any()):
        # the stage bars (tests/test_gpu_stages.py: sigma 1e-4 at O(10), essence 1e-4, d sigma/dx 1e-4 relative), relative to the
        # set's own scale; sigma against the float64 trunk too: where float32 itself is coarser than the bar (activations near
        # 65 000), the split's 22 bits may be 4x further from it than the exact kernel's 24
        ss = max(1.0, float(b[0].abs().max()) / 10.0)
        with torch.no_grad():
            s64 = trunk64(sd, g, x_np)[0].reshape(-1)
        e16, e32 = (a[0].double() - s64).abs(), (b[0].double() - s64).abs()
        assert float(e32.max()) < 1e-3 * ss          # (the restatement is the kernels' function)
        bar = 4.0 * float(e32.max()) + 1e-4 * ss
        assert float(e16[other].max()) <= bar, (float(e16[other].max()), float(e32.max()))
        assert float((a[1] - b[1])[other].abs().max()) < 1e-4 * max(1.0, float(b[1].abs().max()))
        gn = b[2].norm(dim=-1)
        rel = ((a[2] - b[2]).norm(dim=-1) / gn.clamp_min(1e-30 + 1e-6 * float(gn.max())))[other]
        assert float(rel.max()) < 1e-3, float(rel.max())
    sig, ess, rec, pos = _lib.field_forward(sc, packed, x)
    gr = _lib.field_reverse(sc, packed, x, rec, pos, sig, ess)
    assert bool(torch.isfinite(sig).all()) and bool(torch.isfinite(ess).all())
    # (samples with sigma <= 0 have no reverse pass in the two-launch form: the single launch may flag them on their adjoints)
    want = a[0] > 0
    assert torch.equal(sig[want], a[0][want]) and torch.equal(ess[want], a[1][want])
    assert bool((sig[~want] <= 0).all())
    assert bool(torch.isfinite(gr[want]).all())
    assert torch.equal(gr[want], a[2][want])
    return float(same.float().mean())


def check_frame(sd, hw=64, colour_scale=1.0):
    """render_rays with the density screen on and off against the exact-fp32 frame; the relighting sweep per light"""
    from dsnerf_amd import _lib
    canon, faces, batch = full_frame(hw=hw)
    r = renderer_with(sd, canon, faces)
    r.eval()
    r._set_frame(batch)
    S = 64
    o, d = r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0])
    pk = r.net.packed(r.device)
    pk.calibrate_screen(r.scene)          # (the screen's margin for these parameters, as Renderer does before its first frame)

    def run(**kw):
        n, f = r._dev(batch["near"][0]).clone(), r._dev(batch["far"][0]).clone()
        return _lib.render_rays(r.scene, pk, _lib.RenderWorkspace(r.device), o, d, n, f, S, r._t_vals(S), **kw)

    exact = run(fp32=True)
    scale = max(1.0, colour_scale, float(exact["color"].abs().max()))      # (colour_scale: the largest colour of a sample)
    # (with the density screen on, the frame also carries the screen's own drops - its calibration, not the range guard, bounds
    # them: 10x the parity bar there)
    for kw, bar in (({"screen": False}, 1e-4), ({"screen": True}, 1e-3)):
        out = run(**kw)
        assert bool(torch.isfinite(out["color"]).all()) and bool(torch.isfinite(out["weights"]).all()), kw
        assert float((out["color"] - exact["color"]).abs().max()) < bar * scale, kw
        assert float((out["weights"] - exact["weights"]).abs().max()) < bar, kw
    # relighting sweep (no exact twin): each light of the sweep is render_rays under that light, bit for bit
    plain = run()
    n, f = r._dev(batch["near"][0]).clone(), r._dev(batch["far"][0]).clone()
    sw = _lib.render_rays_lights(r.scene, pk, _lib.RenderWorkspace(r.device), o, d, n, f, S, r._t_vals(S),
                                 _lib.light_records([{}, {}], None, r.device))
    for k in range(2):
        assert torch.equal(sw["color"][k], plain["color"]), k
    # density grid (density-only kernel + its fallback) against the exact one
    axes, vol = r.density_grid(batch, resolution=24)
    _, vol32 = r.density_grid(batch, axes=axes, fp32=True)
    assert bool(torch.isfinite(vol).all())
    assert float((vol - vol32).abs().max()) < 1e-4 * max(1.0, float(vol32.abs().max()) / 10.0)


def training_count(sd):
    g = load("small_train")
    r = renderer_with(sd, g["canonical_vertex"], g["faces"], S=int(g["S"]))
    r.train()
    r.render(make_batch(g))
    return r.range_overflow_count()


# ------------------------------------------------------------------------------------------------------------------------
def test_adjoint_band():
    sd, g, x = adjoint_band_state()
    for k in ("nerf.density_net.0.weight", "nerf.stage2.2.weight", "nerf.stage2.4.weight"):
        assert float(np.abs(sd[k]).max()) <= 1023.0, k
    rev, fmax = reverse_values(sd, g, x)
    # precondition: tens of thousands of reverse-pass values in the scaled gap, the forward activations inside the forward range
    in_band = sum(int(((r >= BAND[0] / 64.0) & (r < BAND[1] / 64.0)).sum()) for r in rev)
    assert in_band >= 20000, in_band
    assert float(fmax.max()) < F16_RANGE_SCALED
    frac = check_field(sd, g, x)
    assert frac > 0.0          # some samples took the exact kernel
    check_frame(sd)


@pytest.mark.parametrize("place", ["trunk", "rgb"])
def test_weight_edge(place):
    g = load("full_eval")
    x = g["x_c"].astype(np.float32)
    # 1023.5: fp16(64 w) = 65504 still holds - the split path serves (almost) every sample
    frac = check_field(weight_edge_state(place, 1023.5), g, x)
    assert frac < 0.5, frac
    for w in (1100.0, 2000.0):
        sd = weight_edge_state(place, w)
        frac = check_field(sd, g, x)
        assert frac == 1.0, (w, frac)          # every sample is the exact kernel's
    check_frame(weight_edge_state(place, 2000.0))
    assert training_count(weight_edge_state(place, 1100.0)) > 0


def unit_dirs(g):
    d = np.repeat(g["ray_d"][:, None, :], int(g["S"]), 1).reshape(-1, 3).astype(np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def lighting_band_state(g, target):
    """lights_encoding.0 scaled up by c (bias with it), lights_encoding.2's bias up by c, and the output layer's weights (an fp32
    dot: no split) down by c: the median per-sample maximum of the first hidden layer at `target`, the output unchanged"""
    sd = copy(state())
    S = int(g["S"])
    li = np.concatenate([g["n_w"], g["pts"].reshape(-1, 3), unit_dirs(g)], -1)
    W, b = sd["lighting_mlp.lights_encoding.0.weight"].astype(np.float64), sd["lighting_mlp.lights_encoding.0.bias"].astype(np.float64)
    h = np.maximum(li.astype(np.float64) @ W.T + b, 0.0).max(-1)
    c = target / float(np.median(h))
    assert c * float(np.abs(W).max()) < 30000.0          # (the lighting images hold |w| < 32 768)
    sd["lighting_mlp.lights_encoding.0.weight"] *= np.float32(c)
    sd["lighting_mlp.lights_encoding.0.bias"] *= np.float32(c)
    sd["lighting_mlp.lights_encoding.2.bias"] *= np.float32(c)
    sd["lighting_mlp.lights_encoding.4.weight"] *= np.float32(1.0 / c)
    return sd, h * c


@pytest.mark.parametrize("edge,target", [(32768.0, 36000.0), (65504.0, 62000.0)])
def test_lighting_band(edge, target):
    from dsnerf_amd import _lib
    g = load("full_eval")
    sd, hs = lighting_band_state(g, target)
    assert int((hs > edge).sum()) > 100 and int((hs < edge).sum()) > 100
    sc, packed = scene_for(sd, g)
    S = int(g["S"])
    dirs = np.repeat(g["ray_d"][:, None, :], S, 1).reshape(-1, 3)
    args = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV) for a in (g["n_w"], g["pts"].reshape(-1, 3), dirs, g["essence"])]
    a = _lib.light(packed, *args)
    b = _lib.light(packed, *args, fp32=True)
    assert bool(torch.isfinite(a).all())
    same = (a == b).all(-1)
    flagged_expected = torch.from_numpy(hs >= F16_RANGE_SCALED * 1.0001).to(DEV)
    # every sample past the scaled threshold takes the exact kernel's bits; the others meet the bar
    assert bool(same[flagged_expected].all())
    other = ~same
    cmax = max(1.0, float(b.abs().max()))
    if bool(other.any()):
        assert float((a - b)[other].abs().max()) < 1e-4 * cmax
    assert training_count(sd) > 0


def test_lighting_weight_edge():
    """a lighting weight the images cannot hold (residual 16 -> lo = 65 536): exact lighting everywhere, training counts"""
    from dsnerf_amd import _lib
    g = load("full_eval")
    sd = weight_edge_state("light", 40016.0)
    sc, packed = scene_for(sd, g)
    S = int(g["S"])
    dirs = np.repeat(g["ray_d"][:, None, :], S, 1).reshape(-1, 3)
    args = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV) for a in (g["n_w"], g["pts"].reshape(-1, 3), dirs, g["essence"])]
    assert torch.equal(_lib.light(packed, *args), _lib.light(packed, *args, fp32=True))
    assert training_count(sd) > 0
