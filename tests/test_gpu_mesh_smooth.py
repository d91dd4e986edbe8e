"""Mesh smoothing and face normals on the device (dsn_mesh_smooth / dsn_mesh_vertex_normals, _lib.mesh_smooth / mesh_vertex_normals,
visualizer.smooth_mesh / vertex_normals, Renderer.extract_mesh(smooth=...)): the moved vertices (as uint32 words), the four counts and the
normals bit for bit against the numpy restatement of include/dsnerf.h's rules (tests/mesh_smooth_restate.py).  The whole module runs with
poisoned scratch: the workspace's earlier contents are 0xFF bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_cc_restate as CC
import mesh_smooth_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
NOF = np.zeros((0, 3), np.int32)
TAUBIN3 = [0.5, -0.53, 0.5]


@pytest.fixture(autouse=True)
def poisoned_scratch(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


def gpu(verts, faces):
    return (torch.from_numpy(np.ascontiguousarray(verts, F32).reshape(-1, 3)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)).to(DEV))


def bits(a):
    return a.detach().cpu().numpy().view(np.uint32) if torch.is_tensor(a) else np.ascontiguousarray(a).view(np.uint32)


def check(verts, faces, factors, origin=None, k=None, normals=True):
    """the device calls against the restatement, bit for bit: the moved vertices, the counts, the normals of the mesh given and of the
    smoothed one; returns the restatement's dict"""
    from dsnerf_amd import _lib
    verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    want = R.smooth(verts, faces, factors, origin, k)
    info = {}
    dv, df = gpu(verts, faces)
    out = _lib.mesh_smooth(dv, df, factors, origin=origin, scale_exp=k, info=info)
    got = [info[n] for n in _lib.MESH_SMOOTH_COUNTS]
    print("V", verts.shape[0], "T", faces.shape[0], "steps", len(factors), "counts", got, "k", info["scale_exp"])
    assert got == want["counts"].tolist(), (got, want["counts"].tolist())
    assert info["scale_exp"] == want["k"] and np.array_equal(bits(info["origin"]), bits(want["origin"]))
    assert out.dtype == torch.float32 and tuple(out.shape) == verts.shape
    diff = bits(out) != bits(want["verts"])
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())
    assert np.array_equal(bits(dv), bits(verts))                                 # the input is not written
    if normals:
        for vv, dd in ((verts, dv), (want["verts"], out)):
            n = _lib.mesh_vertex_normals(dd, df)
            ref = R.vertex_normals(vv, faces)
            diff = bits(n) != bits(ref)
            assert n.dtype == torch.float32 and not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())
    return want


@pytest.fixture(scope="module")
def mc_meshes():
    """name -> (verts, faces) numpy, from the library's own marching cubes on the volumes of the component tests"""
    from dsnerf_amd import _lib

    def mc(vol, n, level, direction):
        v, f = _lib.marching_cubes(torch.from_numpy(vol).to(DEV), CC.axes_of(n), level, direction)
        return v.cpu().numpy(), f.cpu().numpy()
    return {"spheres": mc(CC.spheres_volume(), 32, 0.0, "ascent"), "noise": mc(CC.noise_volume(), 24, 0.5, "descent")}


@pytest.mark.parametrize("name", ["spheres", "noise"])
@pytest.mark.parametrize("steps", [0, 1, 2, 3, 20])
def test_marching_cubes_meshes(mc_meshes, name, steps):
    v, f = mc_meshes[name]
    want = check(v, f, R.taubin(10)[:steps], normals=steps in (0, 20))
    assert want["counts"][0] == f.shape[0] and want["counts"][2] == v.shape[0] and 6 <= want["counts"][3] < R.HEAVY


@pytest.mark.parametrize("factors", [[1.0], [0.0, 0.0], [-0.53], [0.25, -1.0, 1.0, 0.0, 0.75]])
def test_factors(mc_meshes, factors):
    v, f = mc_meshes["noise"]
    want = check(v, f, factors, normals=False)
    if not any(factors):
        assert np.array_equal(bits(want["verts"]), bits(v))


@pytest.mark.parametrize("V", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025])
def test_strip_sizes(V):
    """wave and scan-tile edges; strips are open meshes: boundary vertices at both ends and along both sides"""
    if V < 3:
        v = np.arange(3 * V, dtype=F32).reshape(V, 3)
        f = np.array([[0, 1, 2], [0, 0, 0], [1, 0, 1]], np.int32)
        for ff in (f, NOF):
            want = check(v, ff, TAUBIN3)
            assert want["counts"].tolist() == [0, ff.shape[0], 0, 0] and np.array_equal(bits(want["verts"]), bits(v))
        return
    v, f = CC.strip(V - 2)
    v = v + np.array([1.5, -2.25, 0.125], F32)
    want = check(v, f, TAUBIN3)
    assert want["counts"].tolist() == [V - 2, 0, V, min(3, V - 2)]
    check(*CC.strip(V - 2, reverse=True), TAUBIN3)


@pytest.mark.parametrize("centre_last", [False, True])
@pytest.mark.parametrize("n", [R.HEAVY - 1, R.HEAVY, R.HEAVY + 1])
def test_fans_at_the_heavy_threshold(n, centre_last):
    """the centre's row has n entries: summed by its own lane up to DSN_MESH_SMOOTH_HEAVY, by the whole wave beyond"""
    v, f = CC.fan(n, centre_last)
    rng = np.random.default_rng(n)
    v = (v + rng.normal(0, 0.05, v.shape)).astype(F32)
    want = check(v, f, TAUBIN3 + [-0.53])
    assert want["counts"].tolist() == [n, 0, n + 2, n]
    # two heavy rows and a light one in one wave, the heavy ones not at lane 0
    v2 = np.concatenate([v, v + F32(3.0)])
    f2 = np.concatenate([f, f[::-1] + v.shape[0]])
    check(np.concatenate([np.full((5, 3), 7.0, F32), v2]), f2 + 5, TAUBIN3)


def test_fan_of_200000_faces():
    v, f = CC.fan(200_000)
    v = (v + np.random.default_rng(1).normal(0, 0.01, v.shape)).astype(F32)
    want = check(v, f, TAUBIN3)
    assert want["counts"].tolist() == [200_000, 0, 200_002, 200_000]
    check(*CC.fan(200_000, centre_last=True), [0.5])


def test_interleaved_strips():
    v, f = CC.interleaved_strips(1000, 200)
    want = check(v, f, [0.5, -0.53])
    assert want["counts"].tolist() == [200_000, 0, 202_000, 3]


def test_edges_of_the_rule():
    nan, inf = np.nan, np.inf
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [nan, 0, 0], [0, inf, 0], [5, 5, 5], [2, 2, 2], [0.5, 0.5, -1],
                  [-3, -2, -1], [-0.0, -0.0, -0.0], [0, 0, -inf], [-1.5, 0.25, -4]], F32)
    V = v.shape[0]
    f = np.array([[0, 1, 2], [1, 3, 2], [0, 0, 1], [2, 1, 2], [0, 1, V], [-1, 0, 1], [0, 1, 4], [5, 1, 2], [2 ** 31 - 1, 0, 1],
                  [-2 ** 31, 1, 2], [0, 8, 1], [3, 3, 3], [9, 10, 12], [12, 10, 9], [9, 11, 12], [10, 12, 0]], np.int32)
    want = check(v, f, TAUBIN3 + [1.0, 0.0])
    assert want["counts"].tolist() == [6, 10, 8, 3]
    for i in (4, 5, 6, 7, 11):
        assert np.array_equal(bits(want["verts"][i]), bits(v[i]))
    # unused vertices among many, negative coordinates, NaN and infinite rows sprinkled over a real mesh
    rng = np.random.default_rng(13)
    sv, sf = R.icosphere(3, centre=(-2.0, 0.5, -7.0), noise=0.02)
    sv = np.concatenate([sv, (rng.random((300, 3)) * 4 - 3).astype(F32)])
    sv[[7, 100, 400]] = [[nan, 0, 0], [0, -inf, 0], [inf, inf, inf]]
    want = check(sv, sf, R.taubin(4))
    assert want["counts"][1] == 5 + 6 + 6 and want["counts"][2] == 642 - 3
    # divergence into the clamp of q (eight extents away) stays deterministic: factors far outside what smooths
    want = check(R.icosphere(3, centre=(-2.0, 0.5, -7.0), noise=0.02)[0], sf, [-40.0] * 30)
    assert np.isfinite(want["verts"]).all() and np.abs(want["verts"]).max() > 1e3


def test_shuffled_and_reversed_faces(mc_meshes):
    v, f = mc_meshes["spheres"]
    rng = np.random.default_rng(5)
    base = check(v, f, R.taubin(3))
    rot = f.copy()
    rot[1::3] = rot[1::3][:, [1, 2, 0]]
    rot[2::3] = rot[2::3][:, [2, 0, 1]]
    for ff in (f[rng.permutation(f.shape[0])], f[::-1], rot):
        want = check(v, ff, R.taubin(3))
        assert np.array_equal(bits(want["verts"]), bits(base["verts"])) and want["counts"].tolist() == base["counts"].tolist()


def test_planar_coordinate_keeps_its_bits():
    v, f = R.grid_plane(9)
    want = check(v, f, [0.5] * 10)
    assert np.array_equal(bits(want["verts"][:, 2]), bits(v[:, 2]))
    one = check(v, f, [0.5])["verts"]
    i, j = np.divmod(np.arange(81), 9)
    inner = (i > 0) & (i < 8) & (j > 0) & (j < 8)
    assert np.array_equal(bits(one[inner]), bits(v[inner]))


def test_callers_scale_is_honoured(mc_meshes):
    v, f = mc_meshes["noise"]
    o, k = R.scale_of(v)
    base = check(v, f, TAUBIN3, normals=False)
    coarse = check(v, f, TAUBIN3, origin=np.array([-3.5, 1.25, 0.0], F32), k=k - 14, normals=False)
    assert not np.array_equal(bits(coarse["verts"]), bits(base["verts"]))
    same = check(v, f, TAUBIN3, origin=o, k=k, normals=False)
    assert np.array_equal(bits(same["verts"]), bits(base["verts"]))
    # three steps through one call = three calls at one scale
    x = v
    for fac in TAUBIN3:
        x = check(x, f, [fac], origin=o, k=k, normals=False)["verts"]
    assert np.array_equal(bits(x), bits(base["verts"]))


def test_determinism_null_counts_and_a_dirty_workspace(mc_meshes):
    """two calls give the same bits; out_counts4 may be null; the workspace's contents do not matter (0xFF, zeros, the last call's, 0x5A);
    the phases one by one through the _ex entry give the same result"""
    from dsnerf_amd import _lib
    lib = _lib.lib()
    v, f = mc_meshes["spheres"]
    want = R.smooth(v, f, R.taubin(2))
    wn = R.vertex_normals(v, f)
    dv, df = gpu(v, f)
    a, b = _lib.mesh_smooth(dv, df, R.taubin(2)), _lib.mesh_smooth(dv, df, R.taubin(2))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(_lib.mesh_vertex_normals(dv, df).view(torch.int32), _lib.mesh_vertex_normals(dv, df).view(torch.int32))
    V, T = v.shape[0], f.shape[0]
    nbytes = lib.dsn_mesh_smooth_workspace_bytes(V, T)
    P = _lib._ptr
    fac = np.asarray(R.taubin(2), F32)
    o, k = R.scale_of(v)
    shift = R.area_shift(v, T)
    for fill in (255, 0, None, 0x5A):
        if fill is not None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        counts = torch.full((4,), -7, dtype=torch.int64, device=DEV) if fill != 0 else None
        out = torch.full((V, 3), 7.0, device=DEV)
        assert lib.dsn_mesh_smooth(P(dv), P(df), V, T, o.ctypes.data, k, fac.ctypes.data, 4, P(ws), nbytes, P(out), P(counts),
                                   _lib._stream()) == 0, lib.dsn_last_error()
        assert np.array_equal(bits(out), bits(want["verts"]))
        if counts is not None:
            assert counts.cpu().tolist() == want["counts"].tolist()
        nrm = torch.full((V, 3), 7.0, device=DEV)
        assert lib.dsn_mesh_vertex_normals(P(dv), P(df), V, T, shift, P(ws), nbytes, P(nrm), _lib._stream()) == 0, lib.dsn_last_error()
        assert np.array_equal(bits(nrm), bits(wn))
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
    out = torch.full((V, 3), 7.0, device=DEV)
    counts = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    for ph in (_lib.SM_COUNT, _lib.SM_SCAN, _lib.SM_FILL, _lib.SM_STEP):
        assert lib.dsn_mesh_smooth_ex(P(dv), P(df), V, T, o.ctypes.data, k, fac.ctypes.data, 4, P(ws), nbytes, P(out), P(counts), ph,
                                      _lib._stream()) == 0, lib.dsn_last_error()
    assert np.array_equal(bits(out), bits(want["verts"])) and counts.cpu().tolist() == want["counts"].tolist()
    nrm = torch.full((V, 3), 7.0, device=DEV)
    assert lib.dsn_mesh_vertex_normals_ex(P(dv), P(df), V, T, shift, P(ws), nbytes, P(nrm), _lib.SM_NORMALS, _lib._stream()) == 0      # the lists are there
    assert np.array_equal(bits(nrm), bits(wn))
    # error paths leave the outputs alone
    out.fill_(7.0)
    assert lib.dsn_mesh_smooth(P(dv), P(df), V, T, o.ctypes.data, k, fac.ctypes.data, 4, P(ws), nbytes, P(dv), None, _lib._stream()) != 0
    assert b"overlap" in lib.dsn_last_error()
    assert lib.dsn_mesh_smooth(P(dv), P(df), V, T, o.ctypes.data, k, fac.ctypes.data, 4, P(ws), nbytes - 16, P(out), None, _lib._stream()) != 0
    assert (out == 7.0).all() and np.array_equal(bits(dv), bits(v))
    with pytest.raises(ValueError):
        _lib.mesh_smooth(dv, df, [0.5, float("nan")])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_smooth_mesh_forms(mc_meshes):
    """visualizer.smooth_mesh / vertex_normals: tuples and dicts, numpy and device, against the restatement's dict handling"""
    from dsnerf_amd import visualizer
    v, f = mc_meshes["noise"]
    V = v.shape[0]
    rng = np.random.default_rng(4)
    want = R.smooth(v, f, R.taubin(2))
    wn = R.vertex_normals(want["verts"], f)
    out = visualizer.smooth_mesh((v, f), iterations=2)
    assert len(out) == 2 and all(isinstance(a, np.ndarray) for a in out) and np.array_equal(bits(out[0]), bits(want["verts"])) and out[1] is f
    out = visualizer.smooth_mesh((v, f, np.zeros_like(v)), iterations=2)
    assert len(out) == 3 and np.array_equal(bits(out[2]), bits(wn))
    assert len(visualizer.smooth_mesh((v, f), iterations=2, normals=True)) == 3 and len(visualizer.smooth_mesh((v, f, v), 2, normals=False)) == 2
    dv, df = gpu(v, f)
    out = visualizer.smooth_mesh((dv, df), iterations=2, normals=True)
    assert all(torch.is_tensor(a) and a.is_cuda for a in out) and np.array_equal(bits(out[0]), bits(want["verts"])) and np.array_equal(bits(out[2]), bits(wn))
    lap = visualizer.smooth_mesh((v, f), iterations=3, lamb=0.25, mu=None)
    assert np.array_equal(bits(lap[0]), bits(R.smooth(v, f, [0.25] * 3)["verts"]))
    assert np.array_equal(bits(visualizer.smooth_mesh((v, f), iterations=0)[0]), bits(v))
    mesh = {"verts": v, "faces": f, "normals": v.copy(), "albedo": rng.random((V, 3)).astype(F32), "colour": rng.random((2, V, 3)).astype(F32),
            "source_vertex": np.arange(V, dtype=np.int32), "face_idx": np.zeros(V, np.int32), "uv": np.zeros((V, 2), F32),
            "h": np.zeros(V, F32), "cov": None, "x_c": np.zeros((V, 3), F32), "name": "body", "n_components": 3}
    got, ref = visualizer.smooth_mesh(mesh, iterations=2), R.smooth_dict(mesh, iterations=2)
    assert set(got) == set(ref) and not set(got) & set(visualizer.BINDING_KEYS)
    for key in ref:
        if key == "smooth_info":
            assert set(got[key]) == set(ref[key])
            for kk in ref[key]:
                assert np.array_equal(np.asarray(got[key][kk]), np.asarray(ref[key][kk])), kk
        elif isinstance(ref[key], np.ndarray):
            assert isinstance(got[key], np.ndarray) and np.array_equal(bits(got[key].astype(F32)), bits(ref[key].astype(F32))), key
        else:
            assert got[key] == ref[key]
    assert got["albedo"] is mesh["albedo"]
    assert np.array_equal(bits(visualizer.vertex_normals(mesh)), bits(R.vertex_normals(v, f)))
    assert same_bits(visualizer.vertex_normals({"verts": dv, "faces": df}).cpu(), torch.from_numpy(R.vertex_normals(v, f)))
    # the normals agree with marching cubes' in direction (both follow the winding's side)
    from dsnerf_amd import _lib
    sv, sf, sn = _lib.marching_cubes(torch.from_numpy(CC.spheres_volume()).to(DEV), CC.axes_of(32), 0.0, "descent", want_normals=True)
    fn = _lib.mesh_vertex_normals(sv, sf)
    cos = (fn * sn).sum(dim=1)
    print("face normals against marching cubes' normals: smallest cosine", float(cos.min()))
    assert float(cos.min()) > 0.7


def test_extract_mesh_end_to_end(tmp_path):
    from dsnerf_amd import synth, visualizer
    from helpers import load
    from test_gpu_render import make_batch, make_renderer
    g = load("full_eval_w4")
    r = make_renderer(g, "full_eval_w4")
    r.eval()
    batch = make_batch(g)
    plain = r.extract_mesh(batch, 48, normals=True, largest_component=True)
    got = r.extract_mesh(batch, 48, smooth=3, normals=True, largest_component=True, target_vertices=600, attributes=("albedo", "colour", "valid"))
    again = r.extract_mesh(batch, 48, normals=True, largest_component=True)
    assert set(plain) == set(again) and all(same_bits(plain[k], again[k]) if torch.is_tensor(plain[k]) else plain[k] == again[k] for k in plain)
    assert "smooth_info" not in plain and set(got) >= set(plain) | {"smooth_info", "simplify_info", "cluster_source", "albedo", "colour", "valid"}
    # = the restatement on the unsmoothed mesh, then simplify_mesh, then the attributes at the final vertices
    pv, pf = plain["verts"].cpu().numpy(), plain["faces"].cpu().numpy()
    ref = R.smooth(pv, pf, R.taubin(3))
    info = got["smooth_info"]
    print("end to end: V", pv.shape[0], "T", pf.shape[0], "counts", ref["counts"].tolist(), "k", ref["k"])
    assert [info[k] for k in ("contributing_faces", "skipped_faces", "vertices_moved")] == ref["counts"][:3].tolist() and info["scale_exp"] == ref["k"]
    assert ref["counts"][0] == pf.shape[0] and ref["counts"][2] == pv.shape[0]
    smoothed = visualizer.smooth_mesh(plain, iterations=3)
    assert np.array_equal(bits(smoothed["verts"]), bits(ref["verts"])) and same_bits(smoothed["faces"], plain["faces"])
    assert np.array_equal(bits(smoothed["normals"]), bits(R.vertex_normals(ref["verts"], pf)))
    assert same_bits(smoothed["source_vertex"], plain["source_vertex"])
    thin = visualizer.simplify_mesh(smoothed, target_vertices=600)
    for k in ("verts", "faces", "normals", "source_vertex", "cluster_source"):
        assert same_bits(got[k], thin[k]), k
    assert 100 < got["verts"].shape[0] <= 600
    direct = r.mesh_attributes(batch, got["verts"])
    for k in ("albedo", "colour", "valid"):
        assert same_bits(got[k], direct[k]), k
    # smooth as a dict of keywords: plain Laplacian steps shrink
    lap = r.extract_mesh(batch, 48, smooth={"iterations": 5, "mu": None, "lamb": 0.5}, largest_component=True)
    assert np.array_equal(bits(lap["verts"]), bits(R.smooth(pv, pf, [0.5] * 5)["verts"])) and "normals" not in lap
    assert abs(R.volume(lap["verts"].cpu().numpy(), pf)) < abs(R.volume(pv, pf))
    with pytest.raises(ValueError):
        r.extract_mesh(batch, 48, smooth=2.5)
    # smooth -> bind -> pose: a smoothed mesh binds and poses like any other; a binding loses its record when it is smoothed
    binding = r.bind_mesh(batch, smoothed)
    canon = g["canonical_vertex"].astype(F32)
    targets = np.stack([canon, synth.pose_body(canon, seed=7, trans=(-0.3, 0.25, 0.6))])
    posed = r.pose_mesh(binding, targets)
    assert posed["verts"].shape == (2,) + tuple(smoothed["verts"].shape) and posed["normals"] is not None
    assert torch.isfinite(posed["verts"][:, binding["valid"]]).all()
    resmoothed = visualizer.smooth_mesh(binding, iterations=1)
    assert not set(resmoothed) & set(visualizer.BINDING_KEYS) and "valid" in resmoothed
    # render_mesh(smooth=True) with normals from vertex_normals: the posed mesh has none of its own from the faces
    vis = visualizer.Visualizer3D(48, 64, 0.5, "ascent")
    pose = np.eye(4)
    pose[:3, 3] = ref["verts"].mean(axis=0) + np.array([0, 0, 2.5])
    mesh = {"verts": smoothed["verts"], "faces": smoothed["faces"]}
    with pytest.raises(ValueError):
        vis.render_mesh(mesh, camera_pose=pose, smooth=True)
    mesh["normals"] = visualizer.vertex_normals(mesh)
    assert same_bits(mesh["normals"], smoothed["normals"])
    img = vis.render_mesh(mesh, camera_pose=pose, smooth=True)
    flat = vis.render_mesh(mesh, camera_pose=pose, smooth=False)
    assert img.shape == (64, 64, 3) and img.dtype == np.uint8 and (img != 255).any() and (img != flat).any()
    assert ((img != 255).any(axis=2) == (flat != 255).any(axis=2)).all()
    # save_ply reads back
    path = str(tmp_path / "smooth.ply")
    visualizer.save_ply(path, smoothed)
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    K, T = pv.shape[0], pf.shape[0]
    assert f"element vertex {K}".encode() in head and f"element face {T}".encode() in head and len(body) == K * 24 + T * 13
    vrec = np.frombuffer(body, dtype=[("p", "<f4", (3,)), ("n", "<f4", (3,))], count=K)
    assert np.array_equal(bits(vrec["p"]), bits(ref["verts"])) and np.array_equal(bits(vrec["n"]), bits(smoothed["normals"]))
    # Visualizer3D.get_mesh_from_grid(smooth=3) = smooth_mesh of its plain output
    axes, vol = r.density_grid(batch, resolution=48)
    pts = np.stack(np.meshgrid(*[np.asarray(a, F32) for a in axes], indexing="ij"), -1)
    pred = vol.cpu().numpy()[..., None]
    base = vis.get_mesh_from_grid(pts, pred, return_normals=True, largest_component=True)
    sm = vis.get_mesh_from_grid(pts, pred, return_normals=True, largest_component=True, smooth=3)
    ws = visualizer.smooth_mesh(base, iterations=3)
    assert len(sm) == len(ws) == 3 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(sm, ws))
    assert np.array_equal(bits(sm[0]), bits(ref["verts"])) and not np.array_equal(bits(sm[2]), bits(base[2]))
    del r


def test_render_view_is_untouched_by_the_smoothing():
    from helpers import load
    from test_gpu_render import make_batch, make_renderer
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
    mesh = r.extract_mesh(make_batch(g), 24, normals=True, attributes=("colour",), smooth=2)
    assert mesh is not None and mesh["colour"].shape[0] == mesh["verts"].shape[0] and "smooth_info" in mesh
    assert r.extract_mesh(make_batch(g), 16, level=1e9, smooth=2) is None
    after = frame()
    assert set(before) == set(after) and len(before) >= 3
    for k in before:      # bit patterns (NaN-safe)
        assert same_bits(before[k], after[k]), k
    del r
