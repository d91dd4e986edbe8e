"""Mesh components on the device (dsn_mesh_cc_label / dsn_mesh_cc_emit, _lib.mesh_components / largest_component,
Renderer.extract_mesh(largest_component=True), dsnerf_amd.visualizer): labels, the six counts, the filtered mesh and source_vertex bit
for bit against the numpy restatement of include/dsnerf.h's rule (tests/mesh_cc_restate.py).  The whole module runs with poisoned
scratch: the workspace's earlier contents are 0xFF bytes."""
import numpy as np
import pytest
import torch

import mesh_cc_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


@pytest.fixture(autouse=True)
def poisoned_scratch(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


@pytest.fixture(scope="module")
def mc_meshes():
    """name -> (verts, faces) numpy, from the library's own marching cubes on the volumes of the host tests"""
    from dsnerf_amd import _lib

    def mc(vol, n, level, direction):
        v, f = _lib.marching_cubes(torch.from_numpy(vol).to(DEV), R.axes_of(n), level, direction)
        return v.cpu().numpy(), f.cpu().numpy()
    one = R.spheres_volume(32, R.SPHERES[:1])
    return {"spheres": mc(R.spheres_volume(), 32, 0.0, "ascent"), "noise": mc(R.noise_volume(), 24, 0.5, "descent"),
            "one": mc(one, 32, 0.0, "ascent")}


def gpu(verts, faces):
    return torch.from_numpy(np.ascontiguousarray(verts, F32)).to(DEV), torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(DEV)


def check(verts, faces, want_labels=None):
    """both device calls against the restatement, bit for bit; returns the restatement's dict and the labels the device gave"""
    from dsnerf_amd import _lib
    verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    rv, rf, rsrc, c = R.largest_component(verts, faces)
    dv, df = gpu(verts, faces)
    m = _lib.mesh_components(dv, df)
    lab = m["labels"].cpu().numpy()
    assert lab.dtype == np.int32 and np.array_equal(lab, c["labels"] if want_labels is None else want_labels)
    got = [m["n_components"], m["winner"], m["n_verts"], m["n_faces"], m["area_sum"], m["faces_in_winner"]]
    assert got == c["counts"].tolist(), (got, c["counts"].tolist())
    assert m["area_shift"] == c["area_shift"] and m["area"] == c["area"]
    info = {}
    v, f, src = _lib.largest_component(dv, df, info=info)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and src.dtype == torch.int32
    assert v.shape == rv.shape and f.shape == rf.shape and src.shape == rsrc.shape
    assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32))          # (bits: NaN vertices come back as they are)
    assert np.array_equal(f.cpu().numpy(), rf) and np.array_equal(src.cpu().numpy(), rsrc)
    assert info["n_components"] == c["counts"][0] and info["winner"] == c["counts"][1]
    return c, lab


def test_marching_cubes_meshes(mc_meshes):
    v, f = mc_meshes["spheres"]
    c, _ = check(v, f)
    assert c["counts"][0] == 3 and 0 < c["counts"][2] < v.shape[0]
    v, f = mc_meshes["noise"]
    c, _ = check(v, f)
    assert c["counts"][0] > 100
    # a single sphere comes back bit for bit
    from dsnerf_amd import _lib
    v, f = mc_meshes["one"]
    c, _ = check(v, f)
    assert c["counts"].tolist()[:4] == [1, 0, v.shape[0], f.shape[0]]
    dv, df = gpu(v, f)
    ov, of, src = _lib.largest_component(dv, df)
    assert torch.equal(ov, dv) and torch.equal(of, df) and torch.equal(src, torch.arange(v.shape[0], dtype=torch.int32, device=DEV))


STRESS = 200_000


def stress_meshes():
    rng = np.random.default_rng(17)
    v, f = R.strip(STRESS)
    yield "strip", v, f, True
    vr, fr = R.strip(STRESS, reverse=True)
    yield "strip reversed numbers", vr, fr, True
    yield "strip shuffled", v, f[rng.permutation(STRESS)], True
    yield "strip backwards", v, f[::-1], True
    yield "strip reversed numbers shuffled", vr, fr[rng.permutation(STRESS)], True
    yield "fan first", *R.fan(STRESS // 2), True
    yield "fan last", *R.fan(STRESS // 2, centre_last=True), True
    yield "interleaved strips", *R.interleaved_strips(1000, STRESS // 1000), False


@pytest.mark.parametrize("case", range(8))
def test_union_find_under_stress(case):
    """grids that span every XCD; every mesh but the last is one component with label 0"""
    from dsnerf_amd import _lib
    name, v, f, single = list(stress_meshes())[case]
    V = v.shape[0]
    want = R.labels(V, f)
    if single:
        assert (want == 0).all()
    else:
        assert len(np.unique(want)) == 1000
    c, lab = check(v, f, want)
    dv, df = gpu(v, f)
    for _ in range(2):                                      # (check ran it once: three calls, the same labels)
        assert np.array_equal(_lib.mesh_components(dv, df)["labels"].cpu().numpy(), lab), name
    if not single:                                          # another face order of the same mesh: the same labels and sums
        perm = np.random.default_rng(23).permutation(f.shape[0])
        m0, m1 = _lib.mesh_components(dv, df), _lib.mesh_components(dv, torch.from_numpy(np.ascontiguousarray(f[perm])).to(DEV))
        assert torch.equal(m0["labels"], m1["labels"]) and m0["area_sum"] == m1["area_sum"] and m0["winner"] == m1["winner"] == 999 * (V // 1000)


def test_exact_tie_goes_to_the_smaller_label(mc_meshes):
    v, f = mc_meshes["one"]
    n = v.shape[0]
    vv = np.concatenate([v, v])
    for ff in (np.concatenate([f, f + n]), np.concatenate([f + n, f])):
        c, _ = check(vv, ff)
        (l0, (s0, _)), (l1, (s1, _)) = sorted(c["sums"].items())
        assert (l0, l1) == (0, n) and s0 == s1 and c["counts"][1] == 0


T_ = R.TILE


@pytest.mark.parametrize("nv,nf", [(0, 0), (1, 1), (1, T_ + 1), (3, 1), (T_ - 1, T_ - 3), (T_, T_ - 2), (T_ + 1, T_ - 1), (3 * T_ + 77, 3 * T_ + 75),
                                   (100, T_), (100, T_ + 1), (100, 3 * T_ + 77)])
def test_edges_of_the_scans(nv, nf):
    v, f = R.mesh_with_counts(nv, nf)
    c, _ = check(v, f)
    assert c["counts"][2] == nv and c["counts"][3] == nf
    if nv >= 3:                                             # the same winner alone: it comes back as it is
        v1, f1 = R.mesh_with_counts(nv, nf, extra=False)
        c, _ = check(v1, f1)
        assert c["counts"].tolist()[:4] == [1, 0, nv, nf]


def test_empty_meshes():
    from dsnerf_amd import _lib
    v = np.arange(15, dtype=F32).reshape(5, 3)
    for vv, ff in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), F32), np.array([[0, 1, 2]], np.int32)),
                   (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32))):
        c, lab = check(vv, ff)
        assert c["counts"].tolist() == [0, -1, 0, 0, 0, 0] and (lab == -1).all()
        ov, of, src = _lib.largest_component(*gpu(vv, ff))
        assert ov.shape == (0, 3) and of.shape == (0, 3) and src.shape == (0,)


def test_bad_input():
    nan, inf = np.nan, np.inf
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [nan, 0, 0], [inf, 1, 1], [5, 5, 5], [0, 0, 2], [0.5, 0, 2], [0, 0.5, 2], [9, 9, 9]], F32)
    f = np.array([[0, 1, 2], [2, 3, 4], [6, 7, 8], [6, 7, 10], [-1, 0, 1], [0, 0, 1], [2 ** 31 - 1, 1, 2], [-2 ** 31, 6, 7], [8, 8, 8]], np.int32)
    c, lab = check(v, f)
    assert lab.tolist() == [0, 0, 0, 0, 0, -1, 6, 6, 6, -1]
    # the component with the NaN and inf vertices wins (area 1 against 0.25) and they are emitted as they are
    assert c["counts"].tolist()[:4] == [2, 0, 5, 3] and c["counts"][5] == 3
    k = c["area_shift"]
    assert c["sums"][0][0] == int(np.ldexp(1.0, k)) and c["sums"][6] == (int(np.ldexp(0.25, k)), 2)
    # all of a wave's faces invalid, and invalid faces between valid ones across a tile
    rng = np.random.default_rng(29)
    v, f = R.strip(3000)
    f = f.copy()
    f[64:128] = -5
    f[rng.choice(3000, 300, replace=False), rng.integers(0, 3, 300)] = v.shape[0] + 7
    c, _ = check(v, f)
    assert c["counts"][0] > 1


def test_null_optional_outputs_and_a_dirty_workspace(mc_meshes):
    """labels_v and source_vertex may be null; the workspace's contents do not matter (0xFF, zeros, the last call's); emit twice"""
    import ctypes as C
    from dsnerf_amd import _lib
    lib = _lib.lib()
    v, f = mc_meshes["spheres"]
    rv, rf, rsrc, c = R.largest_component(v, f)
    dv, df = gpu(v, f)
    V, T = v.shape[0], f.shape[0]
    nbytes = lib.dsn_mesh_cc_workspace_bytes(V, T)
    nv, nf = int(c["counts"][2]), int(c["counts"][3])
    for fill in (255, 0, None, 0x5A):
        if fill is not None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        counts = torch.full((6,), -7, dtype=torch.int64, device=DEV)
        labels = torch.full((V,), -9, dtype=torch.int32, device=DEV) if fill == 0 else None
        assert lib.dsn_mesh_cc_label(_lib._ptr(dv), _lib._ptr(df), V, T, c["area_shift"], _lib._ptr(ws), nbytes, _lib._ptr(labels),
                                     _lib._ptr(counts), _lib._stream()) == 0, lib.dsn_last_error()
        assert counts.cpu().tolist() == c["counts"].tolist()
        if labels is not None:
            assert np.array_equal(labels.cpu().numpy(), c["labels"])
        for with_src in (False, True, False):
            ov = torch.full((nv, 3), 7.0, device=DEV)
            of = torch.full((nf, 3), -7, dtype=torch.int32, device=DEV)
            src = torch.full((nv,), -7, dtype=torch.int32, device=DEV) if with_src else None
            assert lib.dsn_mesh_cc_emit(_lib._ptr(dv), _lib._ptr(df), V, T, _lib._ptr(ws), nbytes, nv, nf, _lib._ptr(ov), _lib._ptr(of),
                                        _lib._ptr(src), _lib._stream()) == 0, lib.dsn_last_error()
            assert np.array_equal(ov.cpu().numpy(), rv) and np.array_equal(of.cpu().numpy(), rf)
            if with_src:
                assert np.array_equal(src.cpu().numpy(), rsrc)
    v2, f2, none = _lib.largest_component(dv, df, want_source=False)
    assert none is None and np.array_equal(v2.cpu().numpy(), rv) and np.array_equal(f2.cpu().numpy(), rf)
    # a shift of the caller's (here: coarser by 20 bits) is the restatement's with that shift
    k = c["area_shift"] - 20
    c2 = R.components(v, f, k)
    counts = torch.empty(6, dtype=torch.int64, device=DEV)
    assert lib.dsn_mesh_cc_label(_lib._ptr(dv), _lib._ptr(df), V, T, k, _lib._ptr(ws), nbytes, None, _lib._ptr(counts), _lib._stream()) == 0
    assert counts.cpu().tolist() == c2["counts"].tolist() and c2["counts"][4] != c["counts"][4]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_extract_mesh_end_to_end(tmp_path):
    from dsnerf_amd import visualizer
    from helpers import load
    from test_gpu_render import make_batch, make_renderer
    g = load("full_eval_w4")
    r = make_renderer(g, "full_eval_w4")
    r.eval()
    batch = make_batch(g)
    kw = dict(normals=True, attributes=("albedo", "colour"))
    plain = r.extract_mesh(batch, 40, **kw)
    before = r.extract_mesh(batch, 40)
    got = r.extract_mesh(batch, 40, largest_component=True, **kw)
    after = r.extract_mesh(batch, 40)
    assert set(before) == set(after) == {"verts", "faces"} and all(same_bits(before[k], after[k]) for k in before)
    assert same_bits(plain["verts"], before["verts"]) and same_bits(plain["faces"], before["faces"])
    assert set(got) == set(plain) | {"source_vertex", "n_components"}
    pv, pf = plain["verts"].cpu().numpy(), plain["faces"].cpu().numpy()
    rv, rf, rsrc, c = R.largest_component(pv, pf)
    assert got["n_components"] == c["counts"][0] >= 1 and 1000 < rv.shape[0] <= pv.shape[0]
    assert np.array_equal(got["verts"].cpu().numpy(), rv) and np.array_equal(got["faces"].cpu().numpy(), rf)
    assert np.array_equal(got["source_vertex"].cpu().numpy(), rsrc)
    idx = torch.from_numpy(rsrc.astype(np.int64)).to(DEV)
    for k in ("normals", "albedo", "colour"):
        assert same_bits(got[k], plain[k][idx]), k
    # the module-level filter on the unfiltered dict: the same mesh, every per-vertex array gathered; numpy in, numpy out
    again = visualizer.largest_component(plain)
    assert set(again) == set(got) and all(same_bits(again[k], got[k]) for k in got if k != "n_components")
    host = visualizer.largest_component((pv, pf, plain["normals"].cpu().numpy()))
    assert all(isinstance(a, np.ndarray) for a in host) and len(host) == 3
    assert np.array_equal(host[0], rv) and np.array_equal(host[1], rf) and np.array_equal(host[2], got["normals"].cpu().numpy())
    # render_mesh and save_ply take it as it is
    vis = visualizer.Visualizer3D(40, 64, 0.5, "ascent")
    pose = np.eye(4)
    pose[:3, 3] = rv.mean(axis=0) + np.array([0, 0, 2.5])
    img = vis.render_mesh(got, camera_pose=pose, colors="albedo")
    assert img.shape == (64, 64, 3) and img.dtype == np.uint8 and (img != 255).any()
    visualizer.save_ply(str(tmp_path / "body.ply"), got, colors="colour")
    head = open(tmp_path / "body.ply", "rb").read(600)          # (the header: 13 lines)
    assert f"element vertex {rv.shape[0]}".encode() in head and f"element face {rf.shape[0]}".encode() in head
    # Visualizer3D.get_mesh_from_grid(largest_component=True) = the module-level filter of its unfiltered output
    axes, vol = r.density_grid(batch, resolution=40)
    pts = np.stack(np.meshgrid(*[np.asarray(a, F32) for a in axes], indexing="ij"), -1)
    pred = vol.cpu().numpy()[..., None]
    full = vis.get_mesh_from_grid(pts, pred, return_normals=True)
    kept = vis.get_mesh_from_grid(pts, pred, return_normals=True, largest_component=True)
    want = visualizer.largest_component(full)
    assert len(kept) == len(want) == 3 and all(np.array_equal(a, b) for a, b in zip(kept, want))
    two = vis.get_mesh_from_grid(pts, pred, largest_component=True)
    assert len(two) == 2 and np.array_equal(two[0], kept[0]) and np.array_equal(two[1], kept[1])
    del r


def test_render_view_is_untouched_by_the_filter():
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
    mesh = r.extract_mesh(make_batch(g), 24, normals=True, attributes=("colour",), largest_component=True)
    assert mesh is not None and mesh["n_components"] >= 1 and mesh["verts"].shape[0] == mesh["source_vertex"].shape[0] > 0
    assert r.extract_mesh(make_batch(g), 16, level=1e9, largest_component=True) is None
    after = frame()
    assert set(before) == set(after) and len(before) >= 3
    for k in before:      # bit patterns (NaN-safe)
        assert same_bits(before[k], after[k]), k
    del r
