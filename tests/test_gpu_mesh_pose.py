"""A mesh bound to the body and carried to other poses on the device (dsn_mesh_bind_normals, dsn_mesh_pose, dsn_mesh_stretch; Renderer.bind_mesh,
Renderer.pose_mesh, visualizer.cull_stretched, Visualizer3D.render_mesh_sequence): the three kernels bit for bit against the numpy
restatement of include/dsnerf.h's rule (tests/mesh_pose_restate.py, itself pinned to the reference's float32 outputs by
tests/test_mesh_pose_host.py), the binding against dsn_warp composed by hand, and the whole line end to end.  The module runs with
poisoned scratch, and the raw calls hand the kernels output buffers filled with 0xFF."""
import numpy as np
import pytest
import torch

import mesh_pose_restate as MP
from helpers import load
from test_gpu_render import make_batch, make_renderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def poisoned_scratch(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


def synth():
    from dsnerf_amd import synth as s
    return s


@pytest.fixture(scope="module")
def bodies():
    """name -> (faces [Fb,3] int32, targets [3,Vb,3] float32: the case's posed body, its canonical body, the canonical body under
    synth.pose_body(seed=7))"""
    cache = {}

    def get(name):
        if name not in cache:
            g = load(name)
            canon = g["canonical_vertex"].astype(np.float32)
            cache[name] = (g["faces"].astype(np.int32), np.stack([g["xyz"].astype(np.float32), canon,
                                                                  synth().pose_body(canon, seed=7, trans=(-0.3, 0.25, 0.6))]))
        return cache[name]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def scene():
    """name -> (case, eval-mode Renderer, batch, extract_mesh(batch, 48, normals=True, attributes=("albedo",)), its binding), once"""
    cache = {}

    def get(name):
        if name not in cache:
            g = load(name)
            r = make_renderer(g, name)
            r.eval()
            batch = make_batch(g)
            mesh = r.extract_mesh(batch, 48, normals=True, attributes=("albedo",))
            assert mesh is not None, name
            cache[name] = (g, r, batch, mesh, r.bind_mesh(batch, mesh))
        return cache[name]
    yield get
    cache.clear()


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def filled(*shape):
    return torch.full(shape, -1, dtype=torch.int32, device=DEV).view(torch.float32)      # every byte 0xFF


def words(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def same_as_restatement(got, want, what):
    """got: a float32 device tensor the kernel filled; want: the restatement's float32 array.  NaN where the restatement has NaN (no
    fill pattern left behind), the same bits everywhere else"""
    w = words(got).reshape(-1)
    want = np.ascontiguousarray(want, np.float32).reshape(-1)
    assert w.shape == want.shape, what
    assert not (w == FILL).any(), f"{what}: words the kernel did not write"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(w.view(np.float32)), nan), what
    assert np.array_equal(w[~nan], want.view(np.uint32)[~nan]), what


def random_binding(N, Fb, seed):
    s = synth()
    fi = ((s.hash_uniform(N, seed) * Fb).astype(np.int64) % max(Fb, 1)).astype(np.int32)
    uv = (s.hash_uniform(2 * N, seed + 1).reshape(N, 2) * 2.0 - 0.5).astype(np.float32)
    h = ((s.hash_uniform(N, seed + 2) - 0.5) * 0.1).astype(np.float32)
    n = s.hash_normal(3 * N, seed + 3).reshape(N, 3).astype(np.float64)
    n = (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    return fi, uv, h, n


def raw_bind_normals(body, faces, fi, normals):
    from dsnerf_amd import _lib
    N = fi.shape[0]
    cov = filled(N, 3)
    args = [dev(body), dev(faces), dev(fi), dev(normals)]
    p = _lib._ptr
    _lib._check(_lib.lib().dsn_mesh_bind_normals(p(args[0]), body.shape[0], p(args[1]), faces.shape[0], p(args[2]) if N else None,
                                                 p(args[3]) if N else None, N, p(cov) if N else None, _lib._stream()), "dsn_mesh_bind_normals")
    return cov


def raw_pose(targets, faces, fi, uv, h, cov, want_normals=True, null_status=False):
    """dsn_mesh_pose itself on 0xFF-filled outputs and a poisoned workspace; (verts, normals or None, status word or None)"""
    from dsnerf_amd import _lib
    P, Vb = targets.shape[:2]
    N = fi.shape[0]
    nbytes = _lib.lib().dsn_mesh_pose_workspace_bytes(P, faces.shape[0])
    assert nbytes == P * faces.shape[0] * 64
    ws = _lib._scratch(nbytes, torch.device(DEV))
    out_v, out_n = filled(P, N, 3), (filled(P, N, 3) if want_normals else None)
    status = None if null_status else torch.zeros(1, dtype=torch.int32, device=DEV)
    keep = [dev(targets), dev(faces), dev(fi), dev(uv), dev(h), None if cov is None else (cov if torch.is_tensor(cov) else dev(cov))]
    p = _lib._ptr
    opt = lambda t: p(t) if N and t is not None else None
    _lib._check(_lib.lib().dsn_mesh_pose(p(keep[0]), P, Vb, p(keep[1]), faces.shape[0], opt(keep[2]), opt(keep[3]), opt(keep[4]), opt(keep[5]),
                                         N, opt(out_v), opt(out_n), p(status), p(ws), _lib._stream()), "dsn_mesh_pose")
    return out_v, out_n, None if status is None else int(status.cpu()[0])


def raw_stretch(bind, posed, faces):
    from dsnerf_amd import _lib
    P, N, T = posed.shape[0], bind.shape[0], faces.shape[0]
    out = filled(P, T)
    keep = [dev(bind), posed if torch.is_tensor(posed) else dev(posed), dev(faces)]
    p = _lib._ptr
    _lib._check(_lib.lib().dsn_mesh_stretch(p(keep[0]) if N else None, p(keep[1]) if N else None, P, N, p(keep[2]) if T else None, T,
                                            p(out) if T else None, _lib._stream()), "dsn_mesh_stretch")
    return out


@pytest.mark.parametrize("name", ["small_eval", "full_eval", "full_eval_nu"])
def test_kernels_have_the_restatement_bits(bodies, name):
    faces, targets = bodies(name)
    Fb = faces.shape[0]
    assert Fb == (320 if name == "small_eval" else 13776)
    for k, N in enumerate((0, 1, 63, 64, 65, 257)):
        fi, uv, h, nrm = random_binding(N, Fb, 500 + 10 * k)
        cov = raw_bind_normals(targets[0], faces, fi, nrm)
        want_cov = MP.bind_normals(targets[0], faces, fi, nrm)
        if N:
            same_as_restatement(cov, want_cov, (name, N, "cov"))
        for P in (1, 2, 3):
            wv, wn, _ = MP.pose(targets[:P], faces, fi, uv, h, want_cov)
            for with_normals in (True, False):
                v, n, status = raw_pose(targets[:P], faces, fi, uv, h, cov if with_normals else None, with_normals)
                assert status == 0 and v.shape == (P, N, 3)
                if N:
                    same_as_restatement(v, wv, (name, N, P, "verts"))
                    if with_normals:
                        same_as_restatement(n, wn, (name, N, P, "normals"))
            # the stretch of these points as a mesh of the test's own: consecutive triples, one degenerate face and two bad ones
            tri = np.array([[i, (i + 1) % max(N, 1), (i + 2) % max(N, 1)] for i in range(N)] + [[0, 0, 0], [0, 1, N], [-1, 0, 1]], np.int32)
            posed, _, _ = raw_pose(targets[:P], faces, fi, uv, h, None, False)
            bind = wv[0] if N else np.zeros((0, 3), np.float32)
            st = raw_stretch(bind, posed, tri)
            want = MP.stretch(bind, wv, tri)
            same_as_restatement(st, want, (name, N, P, "stretch"))
            assert np.isposinf(want[:, -2:]).all() and (N < 3 or np.isfinite(want[:, :N]).all())
            if N >= 3:
                assert (want[:, N] == 1.0).all() and (want[0, :N] == 1.0).all()       # a point face; pose 0 is the bind pose


@pytest.mark.parametrize("name", ["small_eval", "full_eval"])
def test_extracted_mesh_in_three_poses(scene, bodies, name):
    from dsnerf_amd import _lib
    g, r, batch, mesh, b = scene(name)
    faces, targets = bodies(name)
    N, T = mesh["verts"].shape[0], mesh["faces"].shape[0]
    assert N > 257 and b["face_idx"].shape == (N,) and b["uv"].shape == (N, 2) and b["h"].shape == (N,) and b["cov"].shape == (N, 3)
    fi, uv, h = (b[k].cpu().numpy() for k in ("face_idx", "uv", "h"))
    want_cov = MP.bind_normals(targets[0], faces, fi, mesh["normals"].cpu().numpy())
    same_as_restatement(b["cov"], want_cov, "cov")
    out = r.pose_mesh(b, dev(targets), stretch=True)
    assert out["verts"].shape == (3, N, 3) and out["normals"].shape == (3, N, 3) and out["stretch"].shape == (3, T)
    assert out["faces"] is b["faces"] and set(out) == {"verts", "normals", "stretch", "faces"}
    wv, wn, _ = MP.pose(targets, faces, fi, uv, h, want_cov)
    same_as_restatement(out["verts"], wv, "verts")
    same_as_restatement(out["normals"], wn, "normals")
    same_as_restatement(out["stretch"], MP.stretch(mesh["verts"].cpu().numpy(), wv, mesh["faces"].cpu().numpy()), "stretch")
    # three poses in one call: the bits of three calls, with or without normals
    for p in range(3):
        one = r.pose_mesh(b, targets[p], stretch=True)
        assert one["verts"].shape == (N, 3) and one["normals"].shape == (N, 3) and one["stretch"].shape == (T,)
        for k in ("verts", "normals", "stretch"):
            assert np.array_equal(words(one[k]), words(out[k][p])), (p, k)
        bare = r.pose_mesh(b, targets[p][None], normals=False)
        assert bare["normals"] is None and bare["stretch"] is None and np.array_equal(words(bare["verts"][0]), words(out["verts"][p]))
    # a list of batches is the stack of their bodies
    b2 = dict(batch, xyz=torch.from_numpy(targets[2])[None])
    lst = r.pose_mesh(b, [batch, b2])
    assert np.array_equal(words(lst["verts"]), words(out["verts"][[0, 2]])) and np.array_equal(words(lst["normals"]), words(out["normals"][[0, 2]]))
    # the canonical body: dsn_warp's own x_c, bit for bit (no restatement involved)
    can = r.pose_mesh(b, "canonical")
    assert can["verts"].shape == (N, 3) and np.array_equal(words(can["verts"]), words(b["x_c"]))
    assert np.array_equal(words(can["verts"]), words(out["verts"][1]))
    # round trip: back onto the body it was bound with every vertex returns, transparent ones included, within the parity bar
    err = float((out["verts"][0] - mesh["verts"]).abs().max())
    print(name, "round trip %.3g m over %d vertices, %d of them transparent" % (err, N, int((~b["valid"]).sum())))
    assert err < 1e-4
    ln = out["normals"][0].norm(dim=1)
    ok = mesh["normals"].norm(dim=1) > 0
    assert float((out["normals"][0] - mesh["normals"])[ok].abs().max()) < 1e-4 and float((ln[ok] - 1).abs().max()) < 1e-5
    with pytest.raises(ValueError):
        r.pose_mesh(b, targets[0][:-1])
    with pytest.raises(ValueError):
        r.pose_mesh(b, "zero")


def test_binding_is_the_warp_by_hand(scene):
    from dsnerf_amd import _lib
    g, r, batch, mesh, b = scene("full_eval")
    N = mesh["verts"].shape[0]
    sc = _lib.Scene(torch.from_numpy(g["canonical_vertex"]), torch.from_numpy(g["faces"].astype(np.int64)), DEV)
    sc.set_frame(r.net.packed(r.device), torch.from_numpy(g["xyz"]), torch.from_numpy(g["poses"]), int(g["frame"]),
                 zero_code=r.net.nerf.w is not None)
    w = _lib.warp(sc, mesh["verts"], None, 1, want_dir=False, want_uvh=True)
    for slab in (1000, N, 1 << 22):
        bb = r.bind_mesh(batch, mesh, slab=slab)
        for k in ("face_idx", "uv", "h", "x_c"):
            assert np.array_equal(words(bb[k]), words(w[k])), (slab, k)
        assert torch.equal(bb["valid"], w["transparent"] == 0) and np.array_equal(words(bb["cov"]), words(b["cov"]))
    # verts and faces by reference, every other entry of the mesh passed through untouched
    assert b["albedo"] is mesh["albedo"] and b["normals"] is mesh["normals"]
    assert b["verts"].data_ptr() == mesh["verts"].data_ptr() and b["faces"].data_ptr() == mesh["faces"].data_ptr()
    # a plain pair binds without normals and poses without them
    pair = r.bind_mesh(batch, (mesh["verts"].cpu().numpy(), mesh["faces"].cpu().numpy()))
    assert pair["cov"] is None and np.array_equal(words(pair["uv"]), words(b["uv"]))
    assert r.pose_mesh(pair, "canonical")["normals"] is None
    with pytest.raises(ValueError):
        r.bind_mesh(batch, (mesh["verts"], mesh["faces"], mesh["normals"][:-1]))


def test_bad_bindings(bodies):
    faces, targets = bodies("small_eval")
    Fb = faces.shape[0]
    fi, uv, h, nrm = random_binding(130, Fb, 77)
    good_cov = MP.bind_normals(targets[0], faces, fi, nrm)
    gv, gn, _ = MP.pose(targets[:2], faces, fi, uv, h, good_cov)
    # face_idx of -1 and Fb: NaN rows in every pose, status bit 0, the neighbouring rows untouched
    bad = fi.copy()
    bad[5], bad[64] = -1, Fb
    cov = raw_bind_normals(targets[0], faces, bad, nrm)
    same_as_restatement(cov, MP.bind_normals(targets[0], faces, bad, nrm), "cov")
    v, n, status = raw_pose(targets[:2], faces, bad, uv, h, cov)
    assert status == 1
    wv, wn, wstatus = MP.pose(targets[:2], faces, bad, uv, h, MP.bind_normals(targets[0], faces, bad, nrm))
    assert wstatus == 1
    same_as_restatement(v, wv, "verts")
    same_as_restatement(n, wn, "normals")
    vv, nn = v.cpu().numpy(), n.cpu().numpy()
    rows = np.ones(130, bool)
    rows[[5, 64]] = False
    assert np.isnan(vv[:, ~rows]).all() and np.isnan(nn[:, ~rows]).all()
    assert np.array_equal(vv[:, rows].view(np.uint32), gv[:, rows].view(np.uint32)) and np.array_equal(nn[:, rows].view(np.uint32), gn[:, rows].view(np.uint32))
    # NaN uv propagates into that vertex alone; the status stays clear
    uv2 = uv.copy()
    uv2[9, 1] = np.nan
    v, n, status = raw_pose(targets[:2], faces, fi, uv2, h, dev(good_cov))
    assert status == 0
    vv = v.cpu().numpy()
    rows = np.arange(130) != 9
    assert np.isnan(vv[:, 9]).all() and np.array_equal(vv[:, rows].view(np.uint32), gv[:, rows].view(np.uint32))
    same_as_restatement(n, gn, "normals")                 # (the covector does not depend on uv)
    # null optional pointers: no covector, no normals, no status word - bad rows included
    v, n, status = raw_pose(targets[:2], faces, bad, uv, h, None, want_normals=False, null_status=True)
    assert n is None and status is None
    same_as_restatement(v, wv, "verts")
    # the wrapper reports the status without reading it back, and refuses a body of another size
    from dsnerf_amd import _lib
    o = _lib.mesh_pose({"face_idx": dev(bad), "uv": dev(uv), "h": dev(h)}, dev(faces), dev(targets[:1]))
    assert o["normals"] is None and o["status"].is_cuda and int(o["status"].cpu()[0]) == _lib.MESH_POSE_BAD_BINDING
    with pytest.raises(ValueError):
        _lib.mesh_pose({"face_idx": dev(fi), "uv": dev(uv[:-1]), "h": dev(h)}, dev(faces), dev(targets[:1]))


@pytest.mark.parametrize("name", ["small_eval", "full_eval"])
def test_end_to_end(scene, bodies, name):
    from dsnerf_amd.visualizer import Visualizer3D, cull_stretched
    g, r, batch, mesh, b = scene(name)
    faces, targets = bodies(name)
    N, T = mesh["verts"].shape[0], mesh["faces"].shape[0]
    assert set(mesh) == {"verts", "faces", "normals", "albedo"}
    target = synth().pose_body(g["canonical_vertex"].astype(np.float32), seed=7)
    out = r.pose_mesh(b, target, stretch=True)
    assert out["verts"].shape == (N, 3) and out["normals"].shape == (N, 3) and out["stretch"].shape == (T,) and out["faces"].shape == (T, 3)
    valid = b["valid"]
    assert valid.dtype == torch.bool and 0.5 < float(valid.float().mean()) <= 1.0
    assert bool(torch.isfinite(out["verts"][valid]).all()) and bool(torch.isfinite(out["normals"][valid]).all())
    assert b["albedo"] is mesh["albedo"]
    st = out["stretch"]
    assert bool(torch.isfinite(st).all()) and float(st.min()) > 0
    ratio = float(st.median()) * 1.05
    posed = dict(b, verts=out["verts"], normals=out["normals"])
    culled = cull_stretched(posed, st, ratio)
    keep = st <= ratio
    assert 0 < int(keep.sum()) < T and torch.equal(culled["faces"], mesh["faces"][keep])
    assert culled["verts"] is out["verts"] and culled["albedo"] is mesh["albedo"]
    assert cull_stretched(posed, st)["faces"].shape[0] == int((st <= 2.0).sum())
    with pytest.raises(ValueError):
        cull_stretched(posed, st[:-1])
    # two poses as a sequence, the camera in front of the first one's bounding box
    v0 = mesh["verts"].cpu().numpy()
    pose = np.eye(4)
    pose[:3, 3] = 0.5 * (v0.min(axis=0) + v0.max(axis=0)).astype(np.float64) + np.array([0.0, 0.0, 2.5])
    vis = Visualizer3D(48, 96, 0.5, "ascent")
    seq_targets = np.stack([targets[0], synth().pose_body(g["canonical_vertex"].astype(np.float32), seed=7, trans=tuple(g["Th"].reshape(-1)[:3]))])
    seq = vis.render_mesh_sequence(r, b, seq_targets, camera_pose=pose, chunk=1, colors="albedo")
    assert isinstance(seq, np.ndarray) and seq.shape == (2, 96, 96, 3) and seq.dtype == np.uint8
    assert (seq[0] != 255).any() and (seq[1] != 255).any() and (seq[0] != seq[1]).any()
    again = vis.render_mesh_sequence(r, b, seq_targets, camera_pose=pose, chunk=8, colors="albedo")
    assert np.array_equal(seq, again)                                  # the same bits, whatever the chunk
    # frame 0 is the bound pose: render_mesh of the mesh posed by hand
    first = r.pose_mesh(b, targets[0])
    by_hand = vis.render_mesh(dict(mesh, verts=first["verts"], normals=first["normals"]), camera_pose=pose, colors="albedo")
    assert np.array_equal(seq[0], by_hand)
    thin = vis.render_mesh_sequence(r, b, seq_targets, camera_pose=pose, max_stretch=ratio)
    assert thin.shape == seq.shape and (thin[1] != 255).any()


def test_render_view_is_untouched_by_the_sequence():
    from dsnerf_amd.visualizer import Visualizer3D
    g = load("small_view")
    r = make_renderer(g)
    r.eval()
    H, W = int(g["H"]), int(g["W"])

    def frame():
        bt = make_batch(g)
        bt["img"] = torch.zeros(1, H, W, 3, dtype=torch.float64)
        bt["mask_at_box"] = torch.from_numpy(g["mask_at_box"])[None]
        return {k: v.clone() for k, v in r.render_view(bt).items() if torch.is_tensor(v)}
    frame()          # (the first eval frame of a parameter version is early stop's probe frame)
    before = frame()
    batch = make_batch(g)
    mesh = r.extract_mesh(batch, 24, normals=True)
    assert mesh is not None
    b = r.bind_mesh(batch, mesh, slab=500)
    canon = g["canonical_vertex"].astype(np.float32)
    out = r.pose_mesh(b, np.stack([g["xyz"], synth().pose_body(canon, seed=7)]), stretch=True)
    assert out["verts"].shape[0] == 2
    Visualizer3D(24, 32, 0.5, "ascent").render_mesh_sequence(r, b, [batch, batch], max_stretch=2.0)
    after = frame()
    assert set(before) == set(after) and len(before) >= 3
    for k in before:      # bit patterns (NaN-safe)
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
    del r
