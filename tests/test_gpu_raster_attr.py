"""The mesh preview with per-vertex normals and colours on the device (dsn_raster_mesh_attr, _lib.raster_mesh(vertex_normals=...,
vertex_colors=..., smooth=, lit=)) against dsn_raster_mesh itself - face and depth are the same pass: the same bits - and against the
numpy restatement of include/dsnerf.h's shade rule (tests/raster_attr_restate.py): out_attr and out_normal within 10 x the float32
rule's own error on that input (tests/golden/raster_attr_spread.json, floor 2e-6), the colour equal but for one level on at most
0.5 % of the covered pixels.  The whole module runs with poisoned scratch."""
import json
import os

import numpy as np
import pytest
import torch

import raster_attr_restate as A
import raster_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE_KW = {"smooth_lit": dict(smooth=True, lit=True), "smooth_unlit": dict(smooth=True, lit=False), "flat_lit": dict(smooth=False, lit=True)}


@pytest.fixture(autouse=True)
def poisoned_scratch(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


@pytest.fixture(scope="module")
def inputs():
    """name -> (keyword arguments of the restatement, raster_restate.raster's result), computed once"""
    from dsnerf_amd import _lib
    out = {}
    for name, kw in A.gpu_inputs(_lib.mc_table()).items():
        out[name] = (kw, R.raster(kw["verts"], kw["faces"], kw["pose"], kw["fx"], kw["fy"], 0.05, None, kw["H"], kw["W"]))
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_attr_spread.json")) as fh:
        return json.load(fh)["cases"]


def T(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def gpu(kw, normals="own", colors="own", **more):
    from dsnerf_amd import _lib
    n = kw["normals"] if isinstance(normals, str) else normals
    c = kw["colors"] if isinstance(colors, str) else colors
    out = _lib.raster_mesh(T(kw["verts"], np.float32), T(kw["faces"], np.int32), camera_pose=kw["pose"], fx=kw["fx"], fy=kw["fy"],
                           height=kw["H"], width=kw["W"], vertex_normals=T(n, np.float32), vertex_colors=T(c, np.float32), **more)
    return {k: t.cpu().numpy() for k, t in out.items() if not k.startswith("_")}


def plain(kw, **more):
    from dsnerf_amd import _lib
    out = _lib.raster_mesh(T(kw["verts"], np.float32), T(kw["faces"], np.int32), camera_pose=kw["pose"], fx=kw["fx"], fy=kw["fy"],
                           height=kw["H"], width=kw["W"], **more)
    return {k: t.cpu().numpy() for k, t in out.items() if not k.startswith("_")}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def against_restatement(out, ref, bar_attr, bar_normal):
    """out_attr / out_normal within the bars and colour within the level bar wherever the device and the restatement chose the same
    fragment (they may differ where the restatement's two nearest fragments are within 4 float32 steps: tests/test_gpu_raster.py)"""
    hit = ref["face"] >= 0
    covered = max(int(hit.sum()), 1)
    near = R.ulp_gap(ref["depth"], ref["depth2"]) <= 4
    diff = (out["face"] != ref["face"]) | (out["depth"].view(np.uint32) != ref["depth"].view(np.uint32))
    assert not (diff & ~near).any() and int((near & hit).sum()) <= 0.001 * covered
    same = ~diff
    dn = np.abs(out["normal"].astype(np.float64) - ref["normal"])[same]
    print("covered %d, other winner on %d, out_normal differs by %.3g (bar %.3g)" % (covered, int(diff.sum()), dn.max(), bar_normal))
    assert dn.max() <= bar_normal
    if "attr" in ref:
        a, b = out["attr"][same], ref["attr"][same]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        da = np.abs(np.nan_to_num(a).astype(np.float64) - np.nan_to_num(b))
        print("out_attr differs by %.3g (bar %.3g)" % (da.max(), bar_attr))
        assert da.max() <= bar_attr
        assert (out["attr"][~hit & same] == 0).all()
    dc = np.abs(out["color"].astype(np.int64) - ref["color"].astype(np.int64)).max(axis=-1)
    dc[diff] = 0
    print("colour differs by one level on %d" % int((dc > 0).sum()))
    assert dc.max() <= 1 and int((dc > 0).sum()) <= 0.005 * covered
    assert (out["color"][~hit & same] == 255).all() and (out["normal"][~hit & same] == 0).all()


def own_spread(ref, mode, base, kw):
    """the float32 rule's own error on an input the fixture has no record of (the same figures, by the same function)"""
    s = A.spread(ref, A.raster_attr(mode=mode, dtype=np.float64, base=base, **kw))
    assert s["level_max"] <= 1 and s["level_share"] <= 0.005, s
    return s


@pytest.mark.parametrize("mode", list(A.MODES))
@pytest.mark.parametrize("name", ["quad", "spheres34_64x64", "spheres40_80x96", "spheres28_53x37"])
def test_against_the_plain_rasteriser_and_the_restatement(inputs, recorded, name, mode):
    kw, base = inputs[name]
    out = gpu(kw, **MODE_KW[mode])
    flat = plain(kw)
    # visibility is dsn_raster_mesh's own pass: GPU against GPU, bit for bit
    assert np.array_equal(out["face"], flat["face"]) and np.array_equal(bits(out["depth"]), bits(flat["depth"]))
    assert out["normal"].shape == (kw["H"], kw["W"], 3) and out["attr"].shape == (kw["H"], kw["W"], 3) and out["color"].dtype == np.uint8
    ref = A.raster_attr(mode=A.MODES[mode], base=base, **kw)
    rec = recorded[name + ":" + mode]
    assert (ref["face"] >= 0).sum() == rec["covered"]
    against_restatement(out, ref, max(10 * rec["attr"], 2e-6), max(10 * rec["normal"], 2e-6))
    if mode != "flat_lit":
        assert not np.array_equal(out["color"], flat["color"])
    # two calls: the same bits
    again = gpu(kw, **MODE_KW[mode])
    for k in out:
        assert np.array_equal(bits(out[k]), bits(again[k])), k


def test_quad_reproduces_the_affine_colour(inputs):
    """perspective-correct: out_attr is the affine colour at the fragment's world point"""
    kw, base = inputs["quad"]
    out = gpu(kw, smooth=True)
    hit = np.flatnonzero(out["face"].reshape(-1) >= 0)
    assert hit.size == 36
    y, x = hit // 8, hit % 8
    z = out["depth"].reshape(-1)[hit].astype(np.float64)
    world = np.stack([((2 * x + 1) / 8 - 1) * z / A.QUAD_F, (1 - (2 * y + 1) / 8) * z / A.QUAD_F, -z], axis=1)
    assert np.abs(out["attr"].reshape(-1, 3)[hit] - A.affine_colour(world)).max() < 2e-6


@pytest.mark.parametrize("big", [1, 1 << 30])
def test_every_triangle_through_each_raster_form(inputs, recorded, big):
    """big_pixels = 1: every triangle whose box holds two pixels or more takes the wave form; 2^30: none does.  The same bits as the
    default threshold, in every output"""
    name = "spheres34_64x64"
    kw, base = inputs[name]
    boxes = R.box_pixels(kw["verts"], kw["faces"], kw["pose"], kw["fx"], kw["fy"], 0.05, kw["H"], kw["W"])
    assert (boxes > 1).sum() > 100 and (boxes == 1).sum() > 100
    want = gpu(kw, smooth=True)
    out = gpu(kw, smooth=True, big_pixels=big)
    for k in want:
        assert np.array_equal(bits(out[k]), bits(want[k])), k
    ref = A.raster_attr(mode=A.SMOOTH, base=base, **kw)
    rec = recorded[name + ":smooth_lit"]
    against_restatement(out, ref, max(10 * rec["attr"], 2e-6), max(10 * rec["normal"], 2e-6))
    # big triangles with attributes: the mesh of the plain rasteriser's wave-form test
    v, f, pose = R.big_triangle_mesh()
    rng = np.random.default_rng(4)
    nrm = rng.standard_normal(v.shape).astype(np.float32)
    kb = dict(verts=v, faces=f, pose=pose, fx=1.0, fy=1.0, H=256, W=256, normals=nrm, colors=A.position_colour(v))
    want = gpu(kb, smooth=True, lit=False)
    out = gpu(kb, smooth=True, lit=False, big_pixels=big)
    for k in want:
        assert np.array_equal(bits(out[k]), bits(want[k])), k
    ref = A.raster_attr(mode=A.SMOOTH | A.UNLIT, **kb)
    s = own_spread(ref, A.SMOOTH | A.UNLIT, ref, kb)
    against_restatement(out, ref, max(10 * s["attr"], 2e-6), max(10 * s["normal"], 2e-6))


def test_bad_normals_fall_back_to_the_flat_normal(inputs, recorded):
    name = "spheres28_53x37"
    kw, base = inputs[name]
    V = kw["verts"].shape[0]
    nrm = kw["normals"].copy()
    rng = np.random.default_rng(9)
    bad = rng.choice(V, V // 10, replace=False)
    nrm[bad[0::3]] = np.nan
    nrm[bad[1::3]] = 0.0
    nrm[bad[2::3], 1] = np.inf
    out = gpu(kw, normals=nrm, smooth=True)
    flat = gpu(kw, smooth=False)
    good = gpu(kw, smooth=True)
    isbad = np.zeros(V, bool)
    isbad[bad] = True
    fb = np.zeros(out["face"].shape, bool)
    hit = out["face"] >= 0
    fb[hit] = isbad[kw["faces"][out["face"][hit]]].any(axis=1)
    assert fb.sum() > 20 and (hit & ~fb).sum() > 20
    for k in ("normal", "color", "attr", "face", "depth"):      # GPU against GPU: flat where a vertex normal is bad, untouched elsewhere
        assert np.array_equal(bits(out[k][fb]), bits(flat[k][fb])), k
        assert np.array_equal(bits(out[k][~fb]), bits(good[k][~fb])), k
    assert np.isfinite(out["normal"]).all()
    ref = A.raster_attr(mode=A.SMOOTH, base=base, **{**kw, "normals": nrm})
    s = own_spread(ref, A.SMOOTH, base, {**kw, "normals": nrm})
    against_restatement(out, ref, max(10 * s["attr"], 2e-6), max(10 * s["normal"], 2e-6))


def test_nan_colours_are_black_and_out_of_range_colours_clamped(inputs, recorded):
    name = "spheres28_53x37"
    kw, base = inputs[name]
    col = kw["colors"].copy()
    rng = np.random.default_rng(10)
    V = col.shape[0]
    sel = rng.choice(V, V // 8, replace=False)
    col[sel[0::2], 0] = np.nan
    col[sel[1::2]] = [3.0, -2.0, 0.5]
    for mode in ("smooth_lit", "smooth_unlit"):
        out = gpu(kw, colors=col, **MODE_KW[mode])
        ref = A.raster_attr(mode=A.MODES[mode], base=base, **{**kw, "colors": col})
        s = own_spread(ref, A.MODES[mode], base, {**kw, "colors": col})
        against_restatement(out, ref, max(10 * s["attr"], 2e-6), max(10 * s["normal"], 2e-6))
        nan = np.isnan(out["attr"][..., 0])
        assert nan.sum() > 10 and (out["color"][nan][:, 0] == 0).all()
    over = out["attr"][..., 0] > 1.0
    assert over.sum() > 3 and (out["color"][over][:, 0] == 255).all() and (out["color"][out["attr"][..., 1] < 0][:, 1] == 0).all()


def test_out_of_range_faces_are_dropped_and_not_gathered(inputs):
    kw, base = inputs["spheres34_64x64"]
    good = gpu(kw, smooth=True)
    V = kw["verts"].shape[0]
    bad_v = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 2.47], [0, 0, 5.0], [0.1, 0, 0], [0, 0.1, 0]], np.float32)
    bad_f = np.array([[0, 1, V + 6], [0, -1, 2], [2 ** 31 - 1, 1, 2], [-2 ** 31, 1, 2], [V, V + 4, V + 5], [V + 1, V + 4, V + 5],
                      [V + 2, V + 4, V + 5], [V + 3, V + 4, V + 5], [5, 5, 9], [V + 4, V + 4, V + 5]], np.int32)
    k2 = dict(kw, verts=np.concatenate([kw["verts"], bad_v]), faces=np.concatenate([kw["faces"], bad_f]),
              normals=np.concatenate([kw["normals"], np.ones((6, 3), np.float32)]), colors=np.concatenate([kw["colors"], np.ones((6, 3), np.float32)]))
    out = gpu(k2, smooth=True)
    for k in good:
        assert np.array_equal(bits(out[k]), bits(good[k])), k
    # no faces / no vertices: the empty image; every face refers to a missing vertex
    from dsnerf_amd import _lib
    e = np.zeros((0, 3), np.float32)
    for vv, ff in ((kw["verts"][:3], np.zeros((0, 3), np.int32)), (e, np.zeros((0, 3), np.int32)), (e, kw["faces"])):
        o = _lib.raster_mesh(T(vv, np.float32), T(ff, np.int32), height=5, width=7, vertex_normals=T(np.ones_like(vv), np.float32),
                             vertex_colors=T(np.ones_like(vv), np.float32), smooth=True)
        assert (o["color"] == 255).all() and (o["face"] == -1).all() and (o["normal"] == 0).all() and (o["attr"] == 0).all()
    with pytest.raises(ValueError):
        _lib.raster_mesh(T(kw["verts"], np.float32), T(kw["faces"], np.int32), height=8, vertex_colors=T(kw["colors"][:-1], np.float32))
    with pytest.raises(ValueError):
        _lib.raster_mesh(T(kw["verts"], np.float32), T(kw["faces"], np.int32), height=8, smooth=True)


def test_without_attributes_it_is_the_plain_image(inputs):
    """the entry point with no attributes and the new outputs null: dsn_raster_mesh's image; flat mode with the normal image asked for
    (the new shade kernel): the same colour, and the flat normal of every pixel"""
    from dsnerf_amd import _lib
    kw, base = inputs["spheres40_80x96"]
    H, W = kw["H"], kw["W"]
    want = plain(kw)
    tv, tf = T(kw["verts"], np.float32), T(kw["faces"], np.int32)
    pose, _, _ = _lib.raster_camera(kw["pose"], np.pi / 3, H, W)
    light = R.light_values()
    V, F = kw["verts"].shape[0], kw["faces"].shape[0]
    nbytes = _lib.lib().dsn_raster_workspace_bytes(V, F, H, W)
    ws = _lib._scratch(nbytes, torch.device(DEV))
    face = torch.full((H, W), 7, dtype=torch.int32, device=DEV)
    depth = torch.full((H, W), 7.0, device=DEV)
    color = torch.full((H, W, 3), 7, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().dsn_raster_mesh_attr(_lib._ptr(tv), V, _lib._ptr(tf), F, pose.ctypes.data, kw["fx"], kw["fy"], 0.05, light.ctypes.data, H, W,
                                         _lib._ptr(face), _lib._ptr(depth), _lib._ptr(color), _lib._ptr(ws), nbytes, 0, 0, None, None, 0, None,
                                         None, _lib._stream())
    assert rc == 0, _lib.lib().dsn_last_error()
    for k, t in (("face", face), ("depth", depth), ("color", color)):
        assert np.array_equal(bits(t.cpu().numpy()), bits(want[k])), k
    # only the normal image
    normal = torch.full((H, W, 3), 7.0, device=DEV)
    rc = _lib.lib().dsn_raster_mesh_attr(_lib._ptr(tv), V, _lib._ptr(tf), F, pose.ctypes.data, kw["fx"], kw["fy"], 0.05, light.ctypes.data, H, W,
                                         None, None, None, _lib._ptr(ws), nbytes, 0, 0, None, None, 0, _lib._ptr(normal), None, _lib._stream())
    assert rc == 0, _lib.lib().dsn_last_error()
    o = _lib.raster_mesh(tv, tf, camera_pose=kw["pose"], fx=kw["fx"], fy=kw["fy"], height=H, width=W, vertex_normals=T(kw["normals"], np.float32))
    assert set(o) == {"color", "depth", "face", "normal"}
    assert np.array_equal(o["color"].cpu().numpy(), want["color"]) and torch.equal(o["normal"], normal)
    ref = A.raster_attr(mode=0, base=base, **{**kw, "colors": None})
    assert np.abs(o["normal"].cpu().numpy().astype(np.float64) - ref["normal"]).max() < 2e-4
    assert set(_lib.raster_mesh(tv, tf, height=8)) == {"color", "depth", "face"}
