"""Mesh simplification on the device (dsn_mesh_simplify_count / dsn_mesh_simplify_emit / dsn_mesh_simplify_cells, _lib.mesh_simplify /
mesh_cell_count / mesh_target_search, visualizer.simplify_mesh, Renderer.extract_mesh(target_vertices=...)): the simplified vertices
(as uint32 words), faces, cluster_source, vertex_cluster and the seven counts bit for bit against the numpy restatement of
include/dsnerf.h's rule (tests/mesh_simplify_restate.py).  The whole module runs with poisoned scratch: the workspace's earlier contents
are 0xFF bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_cc_restate as CC
import mesh_simplify_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
NOF = np.zeros((0, 3), np.int32)


@pytest.fixture(autouse=True)
def poisoned_scratch(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


def gpu(verts, faces):
    return (torch.from_numpy(np.ascontiguousarray(verts, F32).reshape(-1, 3)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)).to(DEV))


def bits(a):
    return a.detach().cpu().numpy().view(np.uint32) if torch.is_tensor(a) else np.ascontiguousarray(a).view(np.uint32)


def check(verts, faces, cell, origin=None, g=None, want=None):
    """the device call against the restatement, bit for bit (every output and all counts); returns the restatement's dict"""
    from dsnerf_amd import _lib
    verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    ro, rg = R.default_grid(verts, cell, origin, g)
    if want is None:
        want = R.simplify(verts, faces, cell, ro, rg)
    info = {}
    dv, df = gpu(verts, faces)
    v, f, src, vc = _lib.mesh_simplify(dv, df, cell, origin=origin, g=g, info=info)
    got = [info[k] for k in _lib.MESH_SIMPLIFY_COUNTS]
    print("counts", got, "grid", info["g"])
    assert got == want["counts"].tolist(), (got, want["counts"].tolist())
    assert info["g"] == rg and np.array_equal(bits(info["origin"]), bits(ro)) and F32(info["cell"]) == F32(cell)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and src.dtype == torch.int32 and vc.dtype == torch.int32
    assert tuple(v.shape) == want["verts"].shape and tuple(f.shape) == want["faces"].shape
    assert np.array_equal(vc.cpu().numpy(), want["vertex_cluster"])
    assert np.array_equal(src.cpu().numpy(), want["cluster_source"])
    assert np.array_equal(bits(v), bits(want["verts"]))
    assert np.array_equal(f.cpu().numpy(), want["faces"])
    assert _lib.mesh_cell_count(dv, cell, origin=origin, g=g) == want["counts"][0]
    return want


@pytest.fixture(scope="module")
def mc_meshes():
    """name -> (verts, faces) numpy, from the library's own marching cubes on the volumes of the component tests"""
    from dsnerf_amd import _lib

    def mc(vol, n, level, direction):
        v, f = _lib.marching_cubes(torch.from_numpy(vol).to(DEV), CC.axes_of(n), level, direction)
        return v.cpu().numpy(), f.cpu().numpy()
    return {"spheres": mc(CC.spheres_volume(), 32, 0.0, "ascent"), "noise": mc(CC.noise_volume(), 24, 0.5, "descent")}


@pytest.mark.parametrize("name,size", [("spheres", 32), ("noise", 24)])
@pytest.mark.parametrize("n", [4, 8, 16, 32])
def test_marching_cubes_meshes(mc_meshes, name, size, n):
    v, f = mc_meshes[name]
    want = check(v, f, F32(size / n))
    K, kept = int(want["counts"][0]), int(want["counts"][1])
    assert 8 <= K < v.shape[0] and 0 < kept < f.shape[0]
    # a grid of the caller's that cuts part of the mesh off
    check(v, f, F32(size / n), origin=np.array([3.25, 2.5, 4.0], F32), g=[max(n // 2, 1), n, max(n - 1, 1)])


SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049]


@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    """wave and scan-tile edges in V and in T; random vertices in a box of 9 x 7 x 5 cells, random faces (many not live, many duplicates)"""
    rng = np.random.default_rng(100 + n)
    for V, T in ((n, n), (n, 2049), (2049, n)):
        v = (rng.random((V, 3)) * np.array([9, 7, 5])).astype(F32)
        f = rng.integers(0, max(V, 1), (T, 3)).astype(np.int32)
        want = check(v, f, F32(1.0), origin=np.zeros(3, F32), g=[9, 7, 5])
        assert want["counts"][0] == min(V, np.unique(np.floor(v).astype(int), axis=0).shape[0])
        if V == 0:
            assert want["counts"].tolist() == [0, 0, 0, 0, 0, T, 0]


STRESS = 200_000


def test_contention_one_cell():
    rng = np.random.default_rng(7)
    v = (rng.random((STRESS, 3)) * 0.999).astype(F32)
    f = rng.integers(0, STRESS, (1000, 3)).astype(np.int32)
    want = check(v, f, F32(1.0), origin=np.zeros(3, F32), g=[1, 1, 1])
    assert want["counts"].tolist() == [1, 0, 0, 0, 0, 0, 0] and (want["vertex_cluster"] == 0).all()
    # all coincident: the smallest index
    want = check(np.full((STRESS, 3), 0.5, F32), f, F32(1.0), origin=np.zeros(3, F32), g=[1, 1, 1])
    assert want["cluster_source"].tolist() == [0]


def test_contention_distinct_cells_and_triples():
    v, o, cell, g, perm = R.distinct_cells(STRESS)
    _, f = CC.strip(STRESS - 2)                              # 200 000 - 2 faces, every cluster triple distinct
    want = check(v, f, cell, origin=o, g=g)
    assert want["counts"].tolist() == [STRESS, STRESS - 2, STRESS - 2, 0, 0, 0, 0]
    assert np.array_equal(want["cluster_source"], np.argsort(perm)) and np.array_equal(want["vertex_cluster"], perm)
    assert np.array_equal(want["faces"], perm[f])
    # the face array shuffled, and reversed
    rng = np.random.default_rng(19)
    check(v, f[rng.permutation(f.shape[0])], cell, origin=o, g=g)
    check(v, f[::-1], cell, origin=o, g=g)


def test_contention_one_triple():
    """200 000 faces on one cluster triple, every rotation and winding, from 30 vertices in three cells: exactly face 0 stays"""
    rng = np.random.default_rng(11)
    v = (rng.random((30, 3)) * 0.9 + 0.05).astype(F32)
    v[:, 0] += np.arange(30) % 3
    pick = rng.integers(0, 10, (STRESS, 3)) * 3 + np.arange(3)[None, :]
    order = np.argsort(rng.random((STRESS, 3)), axis=1)
    f = np.take_along_axis(pick, order, axis=1).astype(np.int32)
    want = check(v, f, F32(1.0), origin=np.zeros(3, F32), g=[3, 1, 1])
    assert want["counts"].tolist() == [3, 1, STRESS, STRESS - 1, 0, 0, 0] and want["keep"][0] and want["faces"].tolist() == [(f[0] % 3).tolist()]
    # reversed: the same triple, now the other end's face
    want = check(v, f[::-1], F32(1.0), origin=np.zeros(3, F32), g=[3, 1, 1])
    assert want["faces"].tolist() == [(f[-1] % 3).tolist()]


def test_shuffled_and_reversed_faces(mc_meshes):
    v, f = mc_meshes["spheres"]
    rng = np.random.default_rng(5)
    base = check(v, f, F32(2.0))
    for ff in (f[rng.permutation(f.shape[0])], f[::-1], f[:, [1, 2, 0]]):
        want = check(v, ff, F32(2.0))
        assert want["counts"].tolist() == base["counts"].tolist()
        assert np.array_equal(want["cluster_source"], base["cluster_source"])          # the vertices do not depend on the faces
        assert np.array_equal(np.unique(np.sort(want["faces"], 1), axis=0), np.unique(np.sort(base["faces"], 1), axis=0))


def test_edges_of_the_rule():
    nan, inf = np.nan, np.inf
    o, g = np.array([-1, -1, -1], F32), [2, 2, 2]
    v = np.array([[-1, -1, -1], [0, 0, 0], [1, 0, 0], [0.999999, 0.5, 0.5], [-1.0001, 0, 0], [nan, 0, 0], [0, inf, 0], [0, 0, -inf],
                  [-0.5, -0.5, -0.5], [0, 1, 0], [0, 0, 1], [-1, 0, -1], [0.5, -0.25, 0.75], [-0.0, -0.0, -0.0], [0.25, 0.25, nan],
                  [-inf, -inf, -inf], [0.75, -0.75, 0.75]], F32)
    V = v.shape[0]
    f = np.array([[0, 1, 3], [-1, 0, 1], [0, 1, V], [0, 1, 2], [0, 8, 1], [1, 1, 0], [0, 11, 12], [12, 11, 0], [0, 12, 16], [5, 0, 11],
                  [2 ** 31 - 1, 0, 1], [-2 ** 31, 0, 1], [11, 0, 12], [3, 11, 12]], np.int32)
    want = check(v, f, F32(1.0), origin=o, g=g)
    assert want["vertex_cluster"][:9].tolist() == [0, 3, -1, 3, -1, -1, -1, -1, 0] and want["counts"][4] == 9 and want["counts"][5] == 4
    # negative coordinates with the default grid (every finite vertex inside), vertices used by no face
    rng = np.random.default_rng(13)
    v2 = np.concatenate([v, (rng.random((500, 3)) * 4 - 3).astype(F32)])
    want = check(v2, f, F32(0.3))
    assert want["counts"][4] == 5                            # the NaN and infinite ones
    # a vertex exactly on every cell boundary
    j, i, k = np.meshgrid(np.arange(5), np.arange(5), np.arange(5))
    v3 = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(F32) * F32(0.5)
    want = check(v3, NOF, F32(0.5), origin=np.zeros(3, F32), g=[4, 4, 4])
    assert want["counts"][0] == 64 and want["counts"][4] == 125 - 64


def test_cap():
    """K = 2^21 is accepted; 2^21 + 1 vertices in distinct cells set the status bit: ValueError, and the counts say why"""
    from dsnerf_amd import _lib
    n = R.CAP
    v, o, cell, g, perm = R.distinct_cells(n + 1)
    assert g == [129, 128, 128]
    f = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    keep = perm[: n + 1] < n                                 # drop the vertex of the last cell: 2^21 cells, all occupied
    want = check(v[keep], f, cell, origin=o, g=[128, 128, 128])
    assert want["counts"].tolist() == [n, 2, 2, 0, 0, 0, 0]
    want = R.simplify(v, f, cell, o, g)
    assert want["counts"].tolist() == [n + 1, 0, 0, 0, 0, 0, R.TOO_MANY]
    dv, df = gpu(v, f)
    info = {}
    with pytest.raises(ValueError, match="larger cell"):
        _lib.mesh_simplify(dv, df, cell, origin=o, g=g, info=info)
    assert [info[k] for k in _lib.MESH_SIMPLIFY_COUNTS] == want["counts"].tolist()
    assert _lib.mesh_cell_count(dv, cell, origin=o, g=g) == n + 1
    # emit on that workspace writes nothing
    lib = _lib.lib()
    g3 = (C.c_int * 3)(*g)
    nbytes = lib.dsn_mesh_simplify_workspace_bytes(n + 1, 2, g3)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
    counts = torch.empty(7, dtype=torch.int64, device=DEV)
    vc = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    oo = np.ascontiguousarray(o, F32)
    assert lib.dsn_mesh_simplify_count(_lib._ptr(dv), _lib._ptr(df), n + 1, 2, oo.ctypes.data, float(cell), g3, _lib._ptr(ws), nbytes,
                                       _lib._ptr(vc), _lib._ptr(counts), _lib._stream()) == 0, lib.dsn_last_error()
    assert counts.cpu().tolist() == want["counts"].tolist() and np.array_equal(vc.cpu().numpy(), want["vertex_cluster"])
    ov = torch.full((16, 3), 7.0, device=DEV)
    of = torch.full((2, 3), -7, dtype=torch.int32, device=DEV)
    assert lib.dsn_mesh_simplify_emit(_lib._ptr(dv), _lib._ptr(df), n + 1, 2, g3, _lib._ptr(ws), nbytes, 16, 2, _lib._ptr(ov), _lib._ptr(of),
                                      None, _lib._stream()) == 0, lib.dsn_last_error()
    assert (ov == 7.0).all() and (of == -7).all()


def test_determinism_null_outputs_and_a_dirty_workspace(mc_meshes):
    """two calls give the same bits; vertex_cluster and cluster_source may be null; the workspace's contents do not matter (0xFF, zeros,
    the last call's, 0x5A); emit twice; counts above what was reported write no row beyond K and T'"""
    from dsnerf_amd import _lib
    lib = _lib.lib()
    v, f = mc_meshes["spheres"]
    cell = F32(1.5)
    o, g = R.default_grid(v, cell)
    want = R.simplify(v, f, cell, o, g)
    dv, df = gpu(v, f)
    a, b = _lib.mesh_simplify(dv, df, cell), _lib.mesh_simplify(dv, df, cell)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))
    V, T = v.shape[0], f.shape[0]
    g3 = (C.c_int * 3)(*g)
    nbytes = lib.dsn_mesh_simplify_workspace_bytes(V, T, g3)
    K, nf = int(want["counts"][0]), int(want["counts"][1])
    assert K + 5 <= min(V, g[0] * g[1] * g[2]) and nf + 5 <= T
    P = _lib._ptr
    for fill in (255, 0, None, 0x5A):
        if fill is not None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        counts = torch.full((7,), -7, dtype=torch.int64, device=DEV)
        vc = torch.full((V,), -9, dtype=torch.int32, device=DEV) if fill == 0 else None
        assert lib.dsn_mesh_simplify_count(P(dv), P(df), V, T, o.ctypes.data, float(cell), g3, P(ws), nbytes, P(vc), P(counts),
                                           _lib._stream()) == 0, lib.dsn_last_error()
        assert counts.cpu().tolist() == want["counts"].tolist()
        if vc is not None:
            assert np.array_equal(vc.cpu().numpy(), want["vertex_cluster"])
        for with_src, extra in ((False, 0), (True, 0), (False, 5)):
            ov = torch.full((K + extra, 3), 7.0, device=DEV)
            of = torch.full((nf + extra, 3), -7, dtype=torch.int32, device=DEV)
            src = torch.full((K,), -7, dtype=torch.int32, device=DEV) if with_src else None
            assert lib.dsn_mesh_simplify_emit(P(dv), P(df), V, T, g3, P(ws), nbytes, K + extra, nf + extra, P(ov), P(of), P(src),
                                              _lib._stream()) == 0, lib.dsn_last_error()
            assert np.array_equal(bits(ov[:K]), bits(want["verts"])) and np.array_equal(of[:nf].cpu().numpy(), want["faces"])
            assert (ov[K:] == 7.0).all() and (of[nf:] == -7).all()
            if with_src:
                assert np.array_equal(src.cpu().numpy(), want["cluster_source"])
    # the counting-only call on a dirty workspace of its own size
    nb0 = lib.dsn_mesh_simplify_workspace_bytes(V, 0, g3)
    assert 0 < nb0 <= nbytes
    outK = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    assert lib.dsn_mesh_simplify_cells(P(dv), V, o.ctypes.data, float(cell), g3, P(ws), nb0, P(outK), _lib._stream()) == 0
    assert int(outK.cpu()) == K


def test_target_search(mc_meshes):
    from dsnerf_amd import _lib, visualizer
    v, f = mc_meshes["spheres"]
    dv, df = gpu(v, f)
    for N in (1, 50, 700, 10 ** 6):
        n, cell, o, g, probes = R.target_search(v, N)
        info = {}
        got = _lib.mesh_target_search(dv, N, info=info)
        print("target", N, "n", info["n"], "probes", info["probes"])
        assert info["n"] == n and info["probes"] == probes and len(probes) <= 12 and F32(got) == cell
        want = R.simplify(v, f, cell, o, g)
        assert want["counts"][0] <= N
        out = visualizer.simplify_mesh((v, f), target_vertices=N)
        assert all(isinstance(a, np.ndarray) for a in out) and len(out) == 2
        assert np.array_equal(bits(out[0]), bits(want["verts"])) and np.array_equal(out[1], want["faces"])
    # a mesh without a finite vertex, and an empty one
    for vv in (np.full((4, 3), np.nan, F32), np.zeros((0, 3), F32)):
        out = visualizer.simplify_mesh((vv, np.array([[0, 1, 2]], np.int32)), target_vertices=10)
        assert out[0].shape == (0, 3) and out[1].shape == (0, 3)
    with pytest.raises(ValueError):
        visualizer.simplify_mesh((v, f), target_vertices=0)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_extract_mesh_end_to_end(tmp_path):
    from dsnerf_amd import visualizer
    from dsnerf_amd import synth
    from helpers import load
    from test_gpu_render import make_batch, make_renderer
    g = load("full_eval_w4")
    r = make_renderer(g, "full_eval_w4")
    r.eval()
    batch = make_batch(g)
    kw = dict(normals=True, attributes=("albedo", "colour", "sigma", "valid"))
    N = 600
    full = r.extract_mesh(batch, 48, **kw)
    got = r.extract_mesh(batch, 48, target_vertices=N, **kw)
    again = r.extract_mesh(batch, 48, **kw)
    assert set(full) == set(again) and all(same_bits(full[k], again[k]) for k in full)          # the keywords off: what it returned before
    assert set(got) == set(full) | {"cluster_source", "vertex_cluster", "simplify_info"}
    # = simplify_mesh(extract_mesh(...)), and the restatement's mesh at the restatement's n
    want = visualizer.simplify_mesh(full, target_vertices=N)
    assert set(want) == set(got)
    for k in got:
        if k != "simplify_info":
            assert same_bits(got[k], want[k]), k
    fv, ff = full["verts"].cpu().numpy(), full["faces"].cpu().numpy()
    n, cell, o, gg, probes = R.target_search(fv, N)
    ref = R.simplify(fv, ff, cell, o, gg)
    info = got["simplify_info"]
    print("end to end: V", fv.shape[0], "->", ref["counts"].tolist(), "n", n)
    assert info["n"] == n and info["probes"] == probes and info["g"] == gg and [info[k] for k in ("n_clusters", "n_faces")] == ref["counts"][:2].tolist()
    assert 100 < ref["counts"][0] <= N
    assert np.array_equal(bits(got["verts"]), bits(ref["verts"])) and np.array_equal(got["faces"].cpu().numpy(), ref["faces"])
    assert np.array_equal(got["cluster_source"].cpu().numpy(), ref["cluster_source"])
    assert np.array_equal(got["vertex_cluster"].cpu().numpy(), ref["vertex_cluster"])
    # attributes evaluated at the few vertices = the full mesh's, gathered (the dict gather of the restatement)
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in full.items()}
    rd = R.gather_dict(host, ref)
    for k in ("normals", "albedo", "colour", "sigma", "valid"):
        assert np.array_equal(bits(got[k].to(torch.float32)), bits(rd[k].astype(F32))), k
    direct = r.mesh_attributes(batch, got["verts"])
    idx = got["cluster_source"].long()
    full_attr = r.mesh_attributes(batch, full["verts"])
    for k in direct:
        assert same_bits(direct[k], full_attr[k][idx]), k
    # with the component filter in front: source_vertex is gathered too
    both = r.extract_mesh(batch, 48, largest_component=True, simplify_cell=float(cell), normals=True)
    lc = r.extract_mesh(batch, 48, largest_component=True, normals=True)
    assert same_bits(both["source_vertex"], lc["source_vertex"][both["cluster_source"].long()])
    assert same_bits(both["verts"], full["verts"][both["source_vertex"].long()]) and same_bits(both["normals"], full["normals"][both["source_vertex"].long()])
    with pytest.raises(ValueError):
        r.extract_mesh(batch, 48, simplify_cell=0.1, target_vertices=5)
    # a simplified binding poses as the full binding, gathered: two poses, with normals
    binding = r.bind_mesh(batch, full)
    small = visualizer.simplify_mesh(binding, target_vertices=N)
    assert same_bits(small["cluster_source"], got["cluster_source"]) and small["face_idx"].shape[0] == got["verts"].shape[0]
    canon = g["canonical_vertex"].astype(F32)
    targets = np.stack([canon, synth.pose_body(canon, seed=7, trans=(-0.3, 0.25, 0.6))])
    pf, ps = r.pose_mesh(binding, targets), r.pose_mesh(small, targets)
    assert ps["normals"] is not None and same_bits(ps["verts"], pf["verts"][:, idx]) and same_bits(ps["normals"], pf["normals"][:, idx])
    assert same_bits(ps["faces"], got["faces"])
    # save_ply reads back; render_mesh takes it as it is
    path = str(tmp_path / "small.ply")
    visualizer.save_ply(path, got, colors="colour")
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    K, T = got["verts"].shape[0], got["faces"].shape[0]
    assert f"element vertex {K}".encode() in head and f"element face {T}".encode() in head
    vrec = np.frombuffer(body, dtype=[("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))], count=K)
    frec = np.frombuffer(body, dtype=[("k", "u1"), ("v", "<i4", (3,))], count=T, offset=K * 27)
    assert len(body) == K * 27 + T * 13 and np.array_equal(bits(vrec["p"]), bits(ref["verts"])) and np.array_equal(frec["v"], ref["faces"])
    vis = visualizer.Visualizer3D(48, 64, 0.5, "ascent")
    pose = np.eye(4)
    pose[:3, 3] = ref["verts"].mean(axis=0) + np.array([0, 0, 2.5])
    img = vis.render_mesh(got, camera_pose=pose, colors="albedo")
    assert img.shape == (64, 64, 3) and img.dtype == np.uint8 and (img != 255).any()
    # Visualizer3D.get_mesh_from_grid(target_vertices=N) = simplify_mesh of its plain output
    axes, vol = r.density_grid(batch, resolution=48)
    pts = np.stack(np.meshgrid(*[np.asarray(a, F32) for a in axes], indexing="ij"), -1)
    pred = vol.cpu().numpy()[..., None]
    plain = vis.get_mesh_from_grid(pts, pred, return_normals=True)
    thin = vis.get_mesh_from_grid(pts, pred, return_normals=True, target_vertices=N)
    ws = visualizer.simplify_mesh(plain, target_vertices=N)
    assert len(thin) == len(ws) == 3 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(thin, ws))
    assert np.array_equal(bits(thin[0]), bits(ref["verts"]))
    del r


def test_render_view_is_untouched_by_the_simplification():
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
    mesh = r.extract_mesh(make_batch(g), 24, normals=True, attributes=("colour",), target_vertices=200)
    assert mesh is not None and 0 < mesh["verts"].shape[0] <= 200 and mesh["colour"].shape[0] == mesh["verts"].shape[0]
    assert r.extract_mesh(make_batch(g), 16, level=1e9, target_vertices=200) is None
    after = frame()
    assert set(before) == set(after) and len(before) >= 3
    for k in before:      # bit patterns (NaN-safe)
        assert same_bits(before[k], after[k]), k
    del r
