"""The body model on the device (dsn_body_shape, dsn_body_pose; body.BodyModel, Renderer.pose_body, Renderer.view_batch): every output
bit for bit against the numpy restatement of include/dsnerf.h's rule (tests/body_pose_restate.py, itself pinned to the reference's
outputs by tests/test_body_pose_host.py), and the line from SMPL parameters to rendered frames end to end.  The joint chain goes
through the device's float64 sin / cos / sqrt, which may differ from numpy's by a float64 ulp before the one rounding: A, Rh_mat and
the pose features are allowed one float32 ulp with at least 99 % of a call's elements bit-equal, and everything downstream is compared
bit for bit with the restatement fed with the device's own A, Rh_mat and pose features.  The module runs with poisoned scratch: every
output and workspace is filled with 0xFF before the call."""
import json
import os

import numpy as np
import pytest
import torch

import body_pose_restate as BP
from helpers import GOLDEN, load
from test_gpu_render import make_batch, make_renderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("xyz", "xyz_smpl", "A", "bounds", "Rh_mat")
TABLES = {"smpl": BP.SMPL_PARENTS, "chain": BP.CHAIN_PARENTS, "star": BP.STAR_PARENTS}
BLOCK = 8          # poses per block of the vertex kernel (csrc/dsn_body.hip); its workgroups own 256 vertices


@pytest.fixture(autouse=True)
def poisoned_scratch(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


def L():
    import dsnerf_amd
    return dsnerf_amd._lib


def synth():
    from dsnerf_amd import synth as s
    return s


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


_models = {}


def model(V):
    """the synthetic body model of V vertices: numpy arrays, the restatement's shape outputs, device copies - made once"""
    if V not in _models:
        base = {162: lambda: synth().make_small_body()[0], 6890: lambda: load("full_eval")["canonical_vertex"]}.get(V, lambda: V)()
        vt, w, Jr, sd, pd = BP.make_model(base)
        betas = (synth().hash_normal(10, 77) * np.float32(0.8)).astype(np.float32)
        vs, jn = BP.shape(vt, sd, betas, Jr)
        m = dict(V=V, vt=vt, w=w, Jr=Jr, sd=sd, pd=pd, betas=betas, vs=vs, jn=jn)
        m.update({k + "_d": dev(m[k]) for k in ("vt", "w", "Jr", "sd", "pd", "betas", "vs", "jn")})
        _models[V] = m
    return _models[V]


def clip(P, seed=100):
    s = synth()
    poses = np.stack([s.make_poses(seed + i) for i in range(P)]) if P else np.zeros((0, 24, 3), np.float32)
    Rh = (s.hash_normal(3 * P, seed + 1000) * np.float32(0.7)).reshape(P, 3).astype(np.float32)
    Th = (s.hash_normal(3 * P, seed + 2000) * np.float32(0.9)).reshape(P, 3).astype(np.float32)
    return poses, Rh, Th


def run(m, poses, Rh=None, Th=None, pad=None, want=ALL, posedirs=True, parents=BP.SMPL_PARENTS):
    """one library call on 0xFF-filled outputs and workspace -> (outputs as numpy, the pose features the call left in its workspace)"""
    P = len(poses)
    ws = L()._scratch(max(L().lib().dsn_body_pose_workspace_bytes(m["V"], max(P, 1)), 256), DEV)
    out = L().body_pose(m["vs_d"], m["jn_d"], parents, m["w_d"], m["pd_d"] if posedirs else None, dev(poses), dev(Rh), dev(Th), pad, want,
                        workspace=ws)
    torch.cuda.synchronize()
    pf = ws[:P * 208 * 4].view(torch.float32).reshape(P, 208).cpu().numpy()
    return {k: v.cpu().numpy() for k, v in out.items()}, pf


def ulps(a, b):
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return np.where((a == 0) & (b == 0), 0, d)


def same_bits(got, want, what):
    """NaN where the restatement has NaN (no fill pattern left behind), the same bits everywhere else"""
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


def check(m, got, pf, poses, Rh=None, Th=None, pad=None, posedirs=True, parents=BP.SMPL_PARENTS):
    """a full-output call against the restatement (module docstring); returns the restatement's outputs"""
    P = len(poses)
    own = BP.pose(m["vs"], m["jn"], parents, m["w"], m["pd"] if posedirs else None, poses, Rh, Th, BP.PADS[pad])
    assert pf.shape == (P, 208) and not pf[:, 207].any()
    differing = total = 0
    for name, a, b in (("A", got["A"], own["A"]), ("Rh_mat", got["Rh_mat"], own["Rh_mat"]), ("pose feature", pf[:, :207], own["pf"])):
        assert a.shape == b.shape, name
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan), name
        u = ulps(a, b)[~nan]
        assert u.size == 0 or int(u.max()) <= 1, (name, int(u.max()))
        differing, total = differing + int((u != 0).sum()), total + u.size
    assert total == 0 or differing <= 0.01 * total, (differing, total)
    e = BP.pose(m["vs"], m["jn"], parents, m["w"], m["pd"] if posedirs else None, poses, Rh, Th, BP.PADS[pad], A=got["A"], Rh32=got["Rh_mat"],
                pf=pf[:, :207])
    for k in ("xyz", "xyz_smpl", "bounds"):
        same_bits(got[k], e[k], k)
    return e


# ---- dsn_body_shape ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 65, 162, 6890])
def test_shape_is_the_restatement(V):
    m = model(V)
    vs, jn = L().body_shape(m["vt_d"], m["sd_d"], m["betas_d"], m["Jr_d"])
    same_bits(vs.cpu().numpy(), m["vs"], "v_shaped")
    same_bits(jn.cpu().numpy(), m["jn"], "joints")
    assert float(np.abs(m["vs"] - m["vt"]).max()) > 1e-3 or V == 1
    vs3, jn3 = L().body_shape(m["vt_d"], m["sd_d"][:, :, :3].contiguous(), m["betas_d"][:3].contiguous(), None)      # fewer betas, no regressor
    assert jn3 is None
    same_bits(vs3.cpu().numpy(), BP.shape(m["vt"], m["sd"][:, :, :3], m["betas"][:3])[0], "v_shaped, B = 3")
    vs0, jn0 = L().body_shape(m["vt_d"], None, None, m["Jr_d"])                                                      # no shape blend shapes
    same_bits(vs0.cpu().numpy(), m["vt"], "v_shaped = v_template")
    same_bits(jn0.cpu().numpy(), BP.shape(m["vt"], None, None, m["Jr"])[1], "joints of the template")
    with pytest.raises(ValueError):
        L().body_shape(m["vt_d"], m["sd_d"], None, None)


# ---- dsn_body_pose against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 63, 64, 65, 162, 255, 256, 257, 6890])
def test_vertex_counts(V):
    """one vertex, around a wave, the small body, around the 256-vertex tile, the body: a pose block and one pose more"""
    m = model(V)
    poses, Rh, Th = clip(BLOCK + 1)
    got, pf = run(m, poses, Rh, Th, "h36m")
    e = check(m, got, pf, poses, Rh, Th, "h36m")
    if V >= 63:
        assert float(np.abs(e["v_posed"] - m["vs"][None]).max()) > 1e-3          # the pose blend shapes take part: centimetres


@pytest.mark.parametrize("V,P", [(65, 0), (65, 1), (65, 2), (65, 3), (65, BLOCK - 1), (65, BLOCK), (65, 33), (6890, 33)])
def test_pose_counts(V, P):
    m = model(V)
    poses, Rh, Th = clip(P, seed=300)
    got, pf = run(m, poses, Rh, Th, "zju_eval")
    assert {k: v.shape for k, v in got.items()} == {"xyz": (P, V, 3), "xyz_smpl": (P, V, 3), "A": (P, 24, 4, 4), "bounds": (P, 2, 3),
                                                     "Rh_mat": (P, 3, 3)}
    if P:
        check(m, got, pf, poses, Rh, Th, "zju_eval")


def test_optional_inputs_and_outputs():
    m = model(162)
    poses, Rh, Th = clip(3, seed=500)
    full = None
    for posedirs in (True, False):
        for rh in (Rh, None):
            for th in (Th, None):
                got, pf = run(m, poses, rh, th, "zju_train", posedirs=posedirs)
                check(m, got, pf, poses, rh, th, "zju_train", posedirs=posedirs)
                full = got if full is None else full
    # any subset of the outputs: the same bits as the call that asked for all of them
    for want in (("xyz",), ("xyz", "bounds"), ("xyz", "xyz_smpl"), ("xyz", "A"), ("xyz", "Rh_mat"), ("xyz", "A", "bounds")):
        got, _ = run(m, poses, Rh, Th, "zju_train", want=want)
        assert set(got) == set(want)
        for k in want:
            same_bits(got[k], full[k], (want, k))


@pytest.mark.parametrize("table", sorted(TABLES))
def test_parent_tables_and_pad_modes(table):
    m = model(64)
    poses, Rh, Th = clip(2, seed=700)
    none = None
    for pad in (None, "zju_train", "zju_eval", "h36m"):
        got, pf = run(m, poses, Rh, Th, pad, parents=TABLES[table])
        check(m, got, pf, poses, Rh, Th, pad, parents=TABLES[table])
        none = got if none is None else none
        same_bits(got["xyz"], none["xyz"], "xyz does not know about the padding")
    assert np.array_equal(none["bounds"][:, 0], none["xyz"].min(axis=1)) and np.array_equal(none["bounds"][:, 1], none["xyz"].max(axis=1))


def test_the_fixtures_poses_give_the_references_transforms():
    """the joint transforms of the fixture's pose sets (ordinary, zero, beyond pi, 1e-9) against the reference's own, on the device"""
    g = np.load(os.path.join(GOLDEN, "body_pose.npz"))
    m = dict(model(64))
    m["jn"], m["jn_d"] = g["joints"], dev(g["joints"])
    differing = total = 0
    for tn, parents in TABLES.items():
        for pn in ("poses", "zero", "beyond_pi", "tiny"):
            got, pf = run(m, g[f"poses:{pn}"], parents=parents)
            check(m, got, pf, g[f"poses:{pn}"], parents=parents)
            u = ulps(got["A"], g[f"A:{tn}:{pn}"])
            assert int(u.max()) <= 1, (tn, pn)
            differing, total = differing + int((u != 0).sum()), total + u.size
    assert differing <= 0.01 * total, (differing, total)


# ---- independence ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [162, 257])
def test_a_pose_does_not_know_its_neighbours(V):
    from dsnerf_amd.body import BodyModel
    m = model(V)
    P = BLOCK + 3
    poses, Rh, Th = clip(P, seed=900)
    whole, _ = run(m, poses, Rh, Th, "h36m")
    again, _ = run(m, poses, Rh, Th, "h36m")
    order = np.arange(P)[::-1].copy()
    order[[0, 5]] = order[[5, 0]]
    moved, _ = run(m, poses[order], Rh[order], Th[order], "h36m")
    for k in ALL:
        same_bits(again[k], whole[k], ("repeated", k))
        same_bits(moved[k], whole[k][order], ("another position, other neighbours", k))
    for i in range(P):
        one, _ = run(m, poses[i:i + 1], Rh[i:i + 1], Th[i:i + 1], "h36m")
        for k in ALL:
            same_bits(one[k], whole[k][i:i + 1], ("one pose per call", i, k))
    bm = BodyModel(m["vt"], m["w"], BP.SMPL_PARENTS, J_regressor=m["Jr"], shapedirs=m["sd"], posedirs=m["pd"], device=DEV).set_shape(m["betas"])
    same_bits(bm.v_shaped.cpu().numpy(), m["vs"], "BodyModel.set_shape")
    same_bits(bm.joints.cpu().numpy(), m["jn"], "BodyModel.set_shape joints")
    assert bm.slab_poses() >= 1 and bm.slab_poses(1) == 1
    for slab in (None, 1, 4, BLOCK, P):
        out = bm.pose(poses.reshape(P, 72), Rh, Th, pad="h36m", want=ALL, slab=slab)
        for k in ALL:
            same_bits(out[k].cpu().numpy(), whole[k], ("slab", slab, k))
    assert set(bm.pose(poses)) == {"xyz", "A", "bounds"}


# ---- NaN ------------------------------------------------------------------------------------------------------------------------------------
def test_nan_stays_in_its_pose_and_bounds_follow_the_rule():
    m = model(257)
    P = BLOCK + 2
    poses, Rh, Th = clip(P, seed=1100)
    clean, _ = run(m, poses, Rh, Th, "zju_train")
    poses, Th = poses.copy(), Th.copy()
    poses[3, 5, 1] = np.nan            # one joint of pose 3: its whole body (every vertex has weight on every joint)
    Th[6, 1] = np.nan                  # pose 6: the y coordinate of every world vertex, nothing else
    got, pf = run(m, poses, Rh, Th, "zju_train")
    e = check(m, got, pf, poses, Rh, Th, "zju_train")
    assert np.isnan(got["xyz"][3]).all() and np.isnan(got["bounds"][3]).all()
    assert np.isnan(got["xyz"][6, :, 1]).all() and not np.isnan(got["xyz"][6][:, [0, 2]]).any() and not np.isnan(got["xyz_smpl"][6]).any()
    assert np.isnan(got["bounds"][6, :, 1]).all() and not np.isnan(got["bounds"][6][:, [0, 2]]).any()      # a NaN on an axis: both of its bounds
    assert np.isnan(e["bounds"][6, :, 1]).all()
    ok = [i for i in range(P) if i not in (3, 6)]
    for k in ALL:
        same_bits(got[k][ok], clean[k][ok], ("the other poses", k))
    same_bits(got["A"][6], clean["A"][6], "pose 6's transforms")
    same_bits(got["xyz_smpl"][6], clean["xyz_smpl"][6], "pose 6 before Th")


def test_bad_arguments_are_errors():
    m = model(64)
    poses, Rh, Th = clip(2)
    with pytest.raises(ValueError):
        L().body_pose(m["vs_d"], m["jn_d"], BP.SMPL_PARENTS, m["w_d"], None, dev(poses), pad="padded")
    with pytest.raises(ValueError):
        L().body_pose(m["vs_d"], m["jn_d"], BP.SMPL_PARENTS, m["w_d"], None, dev(poses), want=("xyz", "normals"))
    with pytest.raises(ValueError):
        L().body_pose(m["vs_d"], m["jn_d"], BP.SMPL_PARENTS, m["w_d"], None, dev(poses), Rh=dev(Rh[:1]))
    # shapes and dtypes are checked before a pointer reaches the library
    for bad in (dict(weights=m["w_d"][:-1].contiguous()), dict(weights=m["w_d"][:, :23].contiguous()), dict(joints=m["jn_d"][:23].contiguous()),
                dict(posedirs=m["pd_d"][:, :-3].contiguous()), dict(posedirs=m["pd_d"].double()), dict(weights=m["w_d"].cpu()),
                dict(v_shaped=m["vs_d"].reshape(-1)), dict(posedirs=m["pd_d"].t()), dict(poses=dev(poses).reshape(-1)[:100])):
        kw = dict(v_shaped=m["vs_d"], joints=m["jn_d"], parents=BP.SMPL_PARENTS, weights=m["w_d"], posedirs=m["pd_d"], poses=dev(poses))
        kw.update(bad)
        with pytest.raises(ValueError):
            L().body_pose(**kw)
    with pytest.raises(RuntimeError, match="parents"):
        L().body_pose(m["vs_d"], m["jn_d"], np.r_[-1, np.arange(1, 24)], m["w_d"], None, dev(poses))


# ---- dsn_lbs_warp takes the transforms as they are -----------------------------------------------------------------------------------------
def test_lbs_warp_inverts_the_skinning_with_the_returned_transforms():
    """the posed vertices (pose space) through dsn_lbs_warp with the call's own A, handed over as the device tensor it is: the unposed
    points are v_posed within the bar of the host round trip (twice the reference's own float32 - float64 distance, recorded with the
    fixture).  One-hot weights per vertex, by five bands of the body's height on five joints of the spine: every band has its own
    transform, and "rigid_center" (the mean of the nearest face's three vertex weights) gives a vertex exactly its own weights wherever
    that face lies inside the vertex's band - the vertices that are checked, a quarter of the body at least and some of every band."""
    with open(os.path.join(GOLDEN, "body_pose_errors.json")) as f:
        bar = 2 * json.load(f)["ppts_to_pts_f32_vs_f64"]
    s = synth()
    canon, faces = s.make_small_body()
    m = dict(model(162))
    y = m["vt"][:, 1]
    band = np.clip(((y - y.min()) / (np.ptp(y) + 1e-6) * 5).astype(int), 0, 4)
    part = np.array([0, 3, 6, 9, 12])[band]
    m["w"] = np.zeros((162, 24), np.float32)
    m["w"][np.arange(162), part] = 1.0
    m["w_d"] = dev(m["w"])
    poses, _, _ = clip(3, seed=41)
    got, pf = run(m, poses)
    e = check(m, got, pf, poses)
    out = L().body_pose(m["vs_d"], m["jn_d"], BP.SMPL_PARENTS, m["w_d"], m["pd_d"], dev(poses), want=("xyz", "A"))
    packed = L().PackedParams(DEV).update({k: torch.from_numpy(v) for k, v in s.make_state_dict().items()})
    sc = L().Scene(torch.from_numpy(canon), torch.from_numpy(faces), DEV)
    for p in range(3):
        sc.set_frame(packed, out["xyz"][p], torch.from_numpy(poses[p]), 5)
        assert out["A"][p].is_cuda
        o = L().lbs_warp(sc, out["xyz"][p], m["w_d"], out["A"][p], "rigid_center")
        z, idx = o["pts_zero"].cpu().numpy(), o["face_idx"].cpu().numpy()
        inside = (part[faces[idx]] == part[:, None]).all(axis=1)
        assert inside.mean() >= 0.25 and len(set(part[inside])) == 5, (p, inside.mean())
        assert np.array_equal(o["weights"].cpu().numpy()[inside], m["w"][inside])
        err = float(np.abs(z.astype(np.float64) - e["v_posed"][p])[inside].max())
        print(f"pose {p}: |lbs_warp(xyz) - v_posed| = {err:.3e} on {int(inside.sum())} vertices, bar {bar:.3e}")
        assert err <= bar, (p, err, bar)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def camera(centre, H, W, dist=2.4, ang=0.25):
    c, s = np.cos(ang), np.sin(ang)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    T = np.array([0.0, 0.0, dist]) - R @ np.asarray(centre, np.float64)
    f = 0.9 * min(H, W) * dist / 1.9
    K = np.array([[f, 0.0, W / 2 - 0.5], [0.0, f, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    return K, R, T


@pytest.fixture(scope="module")
def line():
    """(name, H, W) -> (case, renderer, body model, the posed 5-pose clip, camera, image size) of a golden case's body, made once;
    the renderers go with the module (later modules count the live ones)"""
    cache = {}
    yield lambda name, H, W: _line(cache, name, H, W)
    cache.clear()
    _models.clear()
    import gc
    gc.collect()


def _line(_lines, name, H, W):
    from dsnerf_amd.body import BodyModel
    if name not in _lines:
        g = load(name)
        r = make_renderer(g)
        r.eval()
        m = model(int(g["canonical_vertex"].shape[0]))
        bm = BodyModel(g["canonical_vertex"], m["w"], BP.SMPL_PARENTS, J_regressor=m["Jr"], shapedirs=m["sd"], posedirs=m["pd"], device=DEV)
        bm.set_shape(m["betas"] * np.float32(0.3))
        poses, Rh, Th = clip(5, seed=1300)
        Th = Th * np.float32(0.2) + np.array([0.1, -0.1, 1.0], np.float32)
        posed = r.pose_body(bm, poses, Rh * np.float32(0.3), Th)
        K, R, T = camera(posed["xyz"][0].mean(dim=0).cpu().numpy(), H, W)
        r.render_view(r.view_batch(posed, 0, K, R, T, H, W, frame=int(g["frame"])))      # (the parameter version's first eval frame is early stop's probe)
        _lines[name] = (g, r, bm, posed, (K, R, T), (H, W))
    return _lines[name]


def host_batch(posed, k, cam, H, W, frame):
    """the batch of pose k assembled on the host from the same vertices and bounds, as a data set would hand it over"""
    K, R, T = cam
    bounds = posed["bounds"][k].cpu().numpy()
    ro, rd, near, far, mask = (t.cpu() for t in L().camera_rays(K, R, T, bounds, H, W))
    return {"ray_o": ro[mask][None], "ray_d": rd[mask][None], "near": near[mask][None], "far": far[mask][None],
            "xyz": posed["xyz"][k].cpu()[None], "poses": posed["poses"][k].cpu()[None], "Th": posed["Th"][k].cpu().reshape(1, 1, 3),
            "frame": torch.tensor([frame]), "img": torch.zeros(1, H, W, 3, dtype=torch.float64), "mask_at_box": mask[None]}


def bits_equal(a, b):
    assert set(a) == set(b) and len(a) >= 4
    for k in a:
        x, y = a[k].contiguous().cpu(), b[k].contiguous().cpu()
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k


@pytest.mark.parametrize("name,H,W", [("small_view", 37, 53), ("full_eval", 64, 64)])
def test_view_batch_renders_what_the_host_batch_renders(line, name, H, W):
    g, r, bm, posed, cam, _ = line(name, H, W)
    frame = int(g["frame"])
    assert posed["xyz"].is_cuda and tuple(posed["xyz"].shape) == (5, bm.V, 3) and tuple(posed["bounds"].shape) == (5, 2, 3)
    for k in (1, 4):
        b = r.view_batch(posed, k, *cam, H, W, frame=frame, save_name="frame%04d" % k)
        assert all(b[key].is_cuda for key in ("xyz", "poses", "Th", "Rh", "bounds", "ray_o", "ray_d", "near", "far", "mask_at_box", "img"))
        assert b["save_name"] == "frame%04d" % k and tuple(b["img"].shape) == (1, H, W, 3) and tuple(b["Rh"].shape) == (1, 3, 3)
        n = int(b["mask_at_box"].sum())
        assert 0 < n <= H * W and tuple(b["ray_o"].shape) == (1, n, 3) and tuple(b["near"].shape) == (1, n)
        dev_img = r.render_view(b)
        host_img = r.render_view(host_batch(posed, k, cam, H, W, frame))
        bits_equal(dev_img, host_img)
        assert float(dev_img["coarse_acc"].abs().sum()) > 0.0
    # the pose the pose MLP sees is the caller's: handing over other poses changes the batch's poses and nothing else
    other = posed["poses"].clone()
    other[:, 1, 2] -= 0.6
    other[:, 2, 2] += 0.6
    b = r.view_batch(posed, 1, *cam, H, W, poses=other, frame=frame)
    assert torch.equal(b["poses"][0], other[1]) and torch.equal(b["xyz"][0], posed["xyz"][1])
    assert torch.equal(r.view_batch(posed, 1, *cam, H, W, poses=other[1], frame=frame)["poses"], b["poses"])
    with pytest.raises(IndexError):
        r.view_batch(posed, 5, *cam, H, W)


def test_render_views_over_the_clip_equals_single_renders(line):
    g, r, bm, posed, cam, (H, W) = line("small_view", 37, 53)
    batches = [r.view_batch(posed, k, *cam, H, W, frame=int(g["frame"])) for k in range(5)]
    single = [{k: v.clone() for k, v in r.render_view(b, device_output=True).items()} for b in batches]
    clip_out = r.render_views(batches, frames_in_flight=3, device_output=True)
    assert len(clip_out) == 5
    for a, b in zip(clip_out, single):
        bits_equal(a, b)
    assert not torch.equal(single[0]["coarse_color"], single[3]["coarse_color"])


def test_pose_mesh_takes_the_posed_bodies_and_render_view_is_untouched(line):
    g, r, bm, posed, cam, (H, W) = line("small_view", 37, 53)

    def frame():
        bt = make_batch(g)
        bt["img"] = torch.zeros(1, int(g["H"]), int(g["W"]), 3, dtype=torch.float64)
        bt["mask_at_box"] = torch.from_numpy(g["mask_at_box"])[None]
        return {k: v.clone() for k, v in r.render_view(bt).items() if torch.is_tensor(v)}
    frame()
    before = frame()
    again = r.pose_body(bm, posed["poses"], None, posed["Th"], pad="zju_train")
    assert torch.equal(again["A"], posed["A"]) and not torch.equal(again["bounds"], posed["bounds"])
    after = frame()
    bits_equal(before, after)
    batch = r.view_batch(posed, 0, *cam, H, W, frame=int(g["frame"]))
    mesh = r.extract_mesh(batch, 24, normals=True)
    assert mesh is not None
    b = r.bind_mesh(batch, mesh)
    on_device = r.pose_mesh(b, posed["xyz"], stretch=True)
    uploaded = r.pose_mesh(b, posed["xyz"].cpu().numpy(), stretch=True)
    assert on_device["verts"].shape[0] == 5
    for k in ("verts", "normals", "stretch"):
        assert torch.equal(on_device[k].view(torch.int32), uploaded[k].view(torch.int32)), k
    # pose 0 is the pose the mesh was bound in: it comes back where it was
    assert float((on_device["verts"][0] - b["verts"]).abs().max()) < 1e-5
    with pytest.raises(ValueError):
        r.pose_body(type("OtherBody", (), {"V": 64})(), posed["poses"])      # a body model of another vertex count
