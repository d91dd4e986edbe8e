"""The mesh preview on the device (dsn_raster_mesh, _lib.raster_mesh, Visualizer3D.render_mesh) against the numpy restatement of
include/dsnerf.h's rule (tests/raster_restate.py): face and depth bit for bit - a pixel may differ only where the restatement's two
nearest fragments are within 4 float32 steps of each other, at most 0.1 % of the covered pixels - and colour equal but for one level
on at most 0.5 % of them (a one-ulp difference can cross a rounding boundary; tests/test_raster_host.py checks that the float32 and
float64 restatements differ less than that on these inputs).  The whole module runs with poisoned scratch."""
import ctypes as C

import numpy as np
import pytest
import torch

import raster_restate as R
from helpers import load
from test_gpu_render import make_batch, make_renderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def poisoned_scratch(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


@pytest.fixture(scope="module")
def table():
    from dsnerf_amd import _lib
    return _lib.mc_table()


@pytest.fixture(scope="module")
def spheres(table):
    """the two-spheres meshes and their restated images, computed once: {(n, H, W): (verts, faces, restatement)}"""
    out = {}
    for n, H, W in R.SPHERE_CASES:
        v, f = R.two_spheres(n, table)
        out[(n, H, W)] = (v, f, R.raster(v, f, H=H, W=W))
    return out


def gpu(verts, faces, **kw):
    from dsnerf_amd import _lib
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(DEV)
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(DEV)
    return {k: t.cpu().numpy() for k, t in _lib.raster_mesh(v, f, **kw).items() if not k.startswith("_")}


def same_as_restatement(out, ref):
    hit = ref["face"] >= 0
    covered = max(int(hit.sum()), 1)
    near = R.ulp_gap(ref["depth"], ref["depth2"]) <= 4
    assert int((near & hit).sum()) <= 0.001 * covered                    # (the input: checked on the restatement alone)
    diff = (out["face"] != ref["face"]) | (out["depth"].view(np.uint32) != ref["depth"].view(np.uint32))
    print("covered %d, near-ties %d, face/depth differ on %d" % (covered, int((near & hit).sum()), int(diff.sum())))
    assert not (diff & ~near).any(), int((diff & ~near).sum())
    assert out["color"].shape == ref["color"].shape and out["color"].dtype == np.uint8
    dc = np.abs(out["color"].astype(np.int64) - ref["color"].astype(np.int64)).max(axis=-1)
    dc[diff] = 0                                                         # (another winner: another triangle's shade)
    print("colour differs by one level on %d" % int((dc > 0).sum()))
    assert dc.max() <= 1 and int((dc > 0).sum()) <= 0.005 * covered
    assert (out["color"][~hit & ~diff] == 255).all() and (out["depth"][~hit & ~diff] == 0).all()


def test_exact_centre_quad():
    v, f, pose = R.exact_quad(4.0)
    out = gpu(v, f, camera_pose=pose, fx=1.0, fy=1.0, height=8)
    same_as_restatement(out, R.raster(v, f, pose, 1.0, 1.0, 0.05, H=8))
    want = np.zeros((8, 8), bool)
    want[1:5, 1:5] = True
    assert np.array_equal(out["face"] >= 0, want) and (out["depth"][want] == 4).all()


@pytest.mark.parametrize("case", R.SPHERE_CASES, ids=lambda c: "grid%d_%dx%d" % c)
def test_two_spheres(spheres, case):
    n, H, W = case
    v, f, ref = spheres[case]
    out = gpu(v, f, height=H, width=W)
    assert out["face"].shape == (H, W) and out["depth"].shape == (H, W) and out["color"].shape == (H, W, 3)
    assert (ref["face"] >= 0).sum() > 0.1 * H * W
    same_as_restatement(out, ref)


def test_one_pixel_image(spheres):
    v, f, _ = spheres[R.SPHERE_CASES[2]]
    out = gpu(v, f, height=1)
    ref = R.raster(v, f, H=1)
    assert ref["face"][0, 0] >= 0
    same_as_restatement(out, ref)


def test_w4_body_mesh():
    """extract_mesh of the w4 body at resolution 64 into 256 x 256, the camera 2.5 in front of its bounding-box centre"""
    g = load("full_eval_w4")
    r = make_renderer(g, "full_eval_w4")
    r.eval()
    m = r.extract_mesh(make_batch(g), 64, level=0.5, gradient_direction="ascent")
    v, f = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    assert f.shape[0] > 1000
    pose = np.eye(4)
    pose[:3, 3] = 0.5 * (v.min(axis=0) + v.max(axis=0)).astype(np.float64) + np.array([0.0, 0.0, 2.5])
    from dsnerf_amd import _lib
    out = {k: t.cpu().numpy() for k, t in _lib.raster_mesh(m["verts"], m["faces"], camera_pose=pose, height=256).items()}
    fx, fy = R.default_scales()
    ref = R.raster(v, f, pose, fx, fy, 0.05, H=256)
    assert (ref["face"] >= 0).sum() > 2000 and (ref["face"] < 0).sum() > 2000
    same_as_restatement(out, ref)
    # the shading of the inputs: float32 and float64 agree to a level (as tests/test_raster_host.py checks for the spheres)
    _, l32 = R.shade_levels(v, f, pose, fx, fy, R.light_values(), 256, 256, ref["face"], ref["depth"])
    _, l64 = R.shade_levels(v, f, pose, fx, fy, R.light_values(), 256, 256, ref["face"], ref["depth"], dtype=np.float64)
    d = np.abs(l32.astype(np.float64) - l64)
    assert d.max() <= 1 and (d > 0).sum() < 0.005 * (ref["face"] >= 0).sum()
    del r


def test_big_triangles_take_the_wave_form_and_change_nothing(spheres):
    """boxes below, at, one above and far above DSN_RM_BIG_PIXELS and a triangle filling the image; the same mesh with every
    triangle in the wave form and with none; micro-triangles and big ones in one call"""
    v, f, pose = R.big_triangle_mesh()
    ref = R.raster(v, f, pose, 1.0, 1.0, 0.05, H=256)
    assert sorted(R.box_pixels(v, f, pose, 1.0, 1.0, 0.05, 256, 256).tolist()) == [15, 16, 17, 10000, 65536]
    for big in (0, 1, 15, 16, 17, 1 << 30):
        out = gpu(v, f, camera_pose=pose, fx=1.0, fy=1.0, height=256, big_pixels=big)
        same_as_restatement(out, ref)
    # the small triangles scaled by two about the image's corner: every box above the threshold
    v2, f2, _ = R.screen_mesh([[[2 * x, 2 * y] for x, y in t] for t in
                               [R.box_tri(3, 5, 3, 5), R.box_tri(20, 5, 4, 4), R.box_tri(40, 5, 1, 17)]], 2.0, 256, 256)
    same_as_restatement(gpu(v2, f2, camera_pose=pose, fx=1.0, fy=1.0, height=256), R.raster(v2, f2, pose, 1.0, 1.0, 0.05, H=256))
    # a backdrop behind the spheres and a pane in front of part of them, in one call with the micro-triangles
    case = R.SPHERE_CASES[0]
    sv, sf, _ = spheres[case]
    extra = np.array([[-6, -6, -1.5], [6, -6, -1.5], [0, 8, -1.5], [-0.9, -0.2, 1.0], [0.1, -0.3, 1.0], [-0.4, 0.5, 1.2]], np.float32)
    mv = np.concatenate([sv, extra])
    mf = np.concatenate([sf, np.array([[0, 1, 2], [3, 4, 5]], np.int32) + sv.shape[0]])
    ref = R.raster(mv, mf, H=case[1], W=case[2])
    boxes = R.box_pixels(mv, mf, R.DEFAULT_POSE, *R.default_scales(), 0.05, case[1], case[2])
    assert (boxes[-2:] > 16).all() and np.median(boxes[:-2]) <= 4 and (ref["face"] >= 0).all()
    assert {int(mf.shape[0]) - 1, int(mf.shape[0]) - 2} <= set(np.unique(ref["face"]).tolist()) and len(np.unique(ref["face"])) > 100
    same_as_restatement(gpu(mv, mf, height=case[1], width=case[2]), ref)


def test_determinism_and_face_order(spheres):
    v, f, ref = spheres[R.SPHERE_CASES[1]]
    n, H, W = R.SPHERE_CASES[1]
    a, b = gpu(v, f, height=H, width=W), gpu(v, f, height=H, width=W)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    # the faces in reverse order: the same image up to the renumbering, except where two fragments tie exactly in depth
    rev = gpu(v, f[::-1], height=H, width=W)
    back = np.where(rev["face"] >= 0, f.shape[0] - 1 - rev["face"], -1)
    tie = (ref["depth"] == ref["depth2"]) & (ref["face"] >= 0)
    assert np.array_equal(rev["depth"].view(np.uint32), a["depth"].view(np.uint32))
    assert np.array_equal(back[~tie], a["face"][~tie]) and np.array_equal(rev["color"][~tie], a["color"][~tie])
    # an exact tie goes to the lowest face index, whatever the order of arrival: the same triangle three times
    q, qf, pose = R.exact_quad(2.0)
    out = gpu(q, np.concatenate([qf[:1], qf[:1], qf[:1], qf]), camera_pose=pose, fx=1.0, fy=1.0, height=8)
    assert set(np.unique(out["face"]).tolist()) <= {-1, 0, 4} and (out["face"] == 0).sum() >= 6


def test_invalid_input_among_good_triangles(spheres):
    v, f, ref = spheres[R.SPHERE_CASES[0]]
    n, H, W = R.SPHERE_CASES[0]
    good = gpu(v, f, height=H, width=W)
    V = v.shape[0]
    bad_v = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 2.47], [0, 0, 5.0], [0.1, 0, 0], [0, 0.1, 0]], np.float32)
    bad_f = np.array([[0, 1, V + 6], [0, -1, 2], [2 ** 31 - 1, 1, 2], [-2 ** 31, 1, 2],              # indices out of range
                      [V, V + 4, V + 5], [V + 1, V + 4, V + 5], [V + 2, V + 4, V + 5], [V + 3, V + 4, V + 5],      # NaN, inf, znear, behind
                      [5, 5, 9], [V + 4, V + 4, V + 5]], np.int32)                                    # zero area
    out = gpu(np.concatenate([v, bad_v]), np.concatenate([f, bad_f]), height=H, width=W)
    for k in good:
        assert np.array_equal(out[k].view(np.uint8), good[k].view(np.uint8)), k
    same_as_restatement(out, ref)
    # no faces / no vertices: the empty image
    for vv, ff in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        e = gpu(vv, ff, height=5, width=7)
        assert (e["color"] == 255).all() and (e["depth"] == 0).all() and (e["face"] == -1).all() and e["color"].shape == (5, 7, 3)
    # every face refers to a missing vertex
    e = gpu(np.zeros((0, 3), np.float32), f, height=9)
    assert (e["face"] == -1).all() and (e["color"] == 255).all()


def test_each_output_may_be_null(spheres):
    from dsnerf_amd import _lib
    v, f, ref = spheres[R.SPHERE_CASES[2]]
    n, H, W = R.SPHERE_CASES[2]
    full = gpu(v, f, height=H, width=W)
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    pose, fx, fy = _lib.raster_camera(None, np.pi / 3, H, W)
    light = R.light_values()
    nbytes = _lib.lib().dsn_raster_workspace_bytes(v.shape[0], f.shape[0], H, W)
    outs = {"face": torch.full((H, W), 7, dtype=torch.int32, device=DEV), "depth": torch.full((H, W), 7.0, device=DEV),
            "color": torch.full((H, W, 3), 7, dtype=torch.uint8, device=DEV)}
    for only in ("face", "depth", "color"):
        ws = _lib._scratch(nbytes, torch.device(DEV))
        ptr = {k: (_lib._ptr(outs[k]) if k == only else None) for k in outs}
        rc = _lib.lib().dsn_raster_mesh(_lib._ptr(tv), v.shape[0], _lib._ptr(tf), f.shape[0], pose.ctypes.data, fx, fy, 0.05,
                                        light.ctypes.data, H, W, ptr["face"], ptr["depth"], ptr["color"], _lib._ptr(ws), nbytes,
                                        _lib._stream())
        assert rc == 0, _lib.lib().dsn_last_error()
        assert np.array_equal(outs[only].cpu().numpy().view(np.uint8), full[only].view(np.uint8)), only
    # a workspace one byte short is refused, and height / width are checked by the binding
    ws = _lib._scratch(nbytes, torch.device(DEV))
    assert _lib.lib().dsn_raster_mesh(_lib._ptr(tv), v.shape[0], _lib._ptr(tf), f.shape[0], pose.ctypes.data, fx, fy, 0.05, light.ctypes.data,
                                      H, W, None, _lib._ptr(outs["depth"]), None, _lib._ptr(ws), nbytes - 1, _lib._stream()) != 0
    with pytest.raises(RuntimeError):
        _lib.raster_mesh(tv, tf, height=0)
    with pytest.raises(RuntimeError):
        _lib.raster_mesh(tv, tf, height=8, znear=0.0)


def test_visualizer_render_mesh(spheres):
    from dsnerf_amd import _lib
    from dsnerf_amd.visualizer import Visualizer3D
    v, f, _ = spheres[R.SPHERE_CASES[0]]
    vis = Visualizer3D(64, 96, 0.5, "ascent")
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    want = _lib.raster_mesh(tv, tf, camera_pose=R.DEFAULT_POSE, yfov=np.pi / 3, height=96, width=96, znear=0.05, intensity=30.0,
                            inner=np.pi / 16, outer=np.pi / 6, base=0.3)["color"].cpu().numpy()
    img = vis.render_mesh((v, f))
    assert isinstance(img, np.ndarray) and img.shape == (96, 96, 3) and img.dtype == np.uint8
    assert (img[0, 0] == 255).all() and (img[-1, -1] == 255).all() and (img < 255).any() and np.array_equal(img, want)
    ref = R.raster(v, f, H=96)
    assert ((img[:, :, 0] == 255) | (ref["face"] >= 0)).all() and (img[ref["face"] < 0] == 255).all()
    for mesh in ({"verts": v, "faces": f}, (tv, tf), {"verts": tv, "faces": tf}, (v, f.astype(np.int64)), (v.astype(np.float64), f)):
        assert np.array_equal(vis.render_mesh(mesh), want)
    # a camera of the caller's: from the other side the image changes, and equals the binding's with that pose
    pose = np.array([[-1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1.0, -2.5], [0, 0, 0, 1]])
    other = vis.render_mesh((v, f), camera_pose=pose)
    assert not np.array_equal(other, want)
    assert np.array_equal(other, _lib.raster_mesh(tv, tf, camera_pose=pose, height=96)["color"].cpu().numpy())
    assert np.array_equal(vis.render_mesh((v, f), camera_pose=torch.from_numpy(pose)), other)
    with pytest.raises(ValueError):
        vis.render_mesh(None)


def test_render_view_is_untouched_by_render_mesh(spheres):
    from dsnerf_amd.visualizer import Visualizer3D
    g = load("small_view")
    r = make_renderer(g)
    r.eval()
    H, W = int(g["H"]), int(g["W"])

    def frame():
        b = make_batch(g)
        b["img"] = torch.zeros(1, H, W, 3, dtype=torch.float64)
        b["mask_at_box"] = torch.from_numpy(g["mask_at_box"])[None]
        return {k: v.clone() for k, v in r.render_view(b).items() if torch.is_tensor(v)}
    frame()          # (the first eval frame of a parameter version is early stop's probe frame)
    before = frame()
    v, f, _ = spheres[R.SPHERE_CASES[0]]
    img = Visualizer3D(64, 128, 0.5, "ascent").render_mesh((v, f))
    assert (img < 255).any()
    after = frame()
    assert set(before) == set(after) and len(before) >= 3
    for k in before:      # bit patterns (NaN-safe)
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
    del r
