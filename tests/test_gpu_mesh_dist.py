"""The distance between meshes on the device (dsn_mesh_dist_build / _query / _reduce, dsn_mesh_sample_surface, _lib.mesh_dist_* /
mesh_sample_surface, visualizer.closest_point / sample_surface / mesh_distance, Renderer.extract_mesh(report_distance=True)): squared
distance (as uint32 words), face index and closest point bit for bit against the brute-force numpy restatement of include/dsnerf.h's rule
(tests/mesh_dist_restate.py), which knows no grid; the reduction and the sampler bit for bit against theirs.  The whole module runs with
poisoned scratch: workspaces and outputs start as 0xFF bytes."""
import numpy as np
import pytest
import torch

import mesh_cc_restate as CC
import mesh_dist_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


@pytest.fixture(autouse=True)
def poisoned_scratch(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


def gpu(verts, faces):
    return (torch.from_numpy(np.ascontiguousarray(verts, F32).reshape(-1, 3)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)).to(DEV))


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def query(verts, faces, points, box=None, **kw):
    from dsnerf_amd import _lib
    dv, df = gpu(verts, faces)
    index = _lib.mesh_dist_build(dv, df, box=box)
    out = _lib.mesh_dist_query(index, torch.from_numpy(np.ascontiguousarray(points, F32).reshape(-1, 3)).to(DEV), **kw)
    return out, index


def check(verts, faces, points, want=None, box=None):
    """the device call against brute force, bit for bit; returns (brute force's triple, the index's info)"""
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    if want is None:
        want = R.brute_force(verts, faces, points)
    out, index = query(verts, faces, points, box=box)
    n = points.shape[0]
    assert out["dist2"].dtype == torch.float32 and out["face"].dtype == torch.int32 and out["point"].dtype == torch.float32
    assert tuple(out["dist2"].shape) == (n,) and tuple(out["face"].shape) == (n,) and tuple(out["point"].shape) == (n, 3)
    face = out["face"].cpu().numpy()
    bad = np.nonzero(face != want[1])[0]
    assert bad.size == 0, (bad[:5], face[bad[:5]], want[1][bad[:5]], out["dist2"].cpu().numpy()[bad[:5]], want[0][bad[:5]])
    assert np.array_equal(bits(out["dist2"]), bits(want[0]))
    assert np.array_equal(bits(out["point"]), bits(want[2]))
    return want, index["info"]


def torus(nu=24, nv=12, R0=1.0, r0=0.35, centre=(0.0, 0.0, 0.0)):
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    p = np.stack([(R0 + r0 * np.cos(v)) * np.cos(u), (R0 + r0 * np.cos(v)) * np.sin(u), r0 * np.sin(v)], -1).reshape(-1, 3) + np.array(centre)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx, np.roll(idx, -1, 0), np.roll(np.roll(idx, -1, 0), -1, 1), np.roll(idx, -1, 1)
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return p.astype(F32), f.astype(np.int32)


def tiny_soup(n, lo, hi, size, seed):
    """n small triangles with corners in the box [lo, hi]"""
    rng = np.random.default_rng(seed)
    c = lo + rng.random((n, 1, 3)) * (np.asarray(hi, np.float64) - lo - size)
    v = (c + rng.random((n, 3, 3)) * size).reshape(-1, 3).astype(F32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


@pytest.fixture(scope="module")
def targets():
    """name -> (verts, faces) numpy"""
    from dsnerf_amd import _lib

    def mc(vol, n, level, direction):
        v, f = _lib.marching_cubes(torch.from_numpy(vol).to(DEV), CC.axes_of(n), level, direction)
        return v.cpu().numpy(), f.cpu().numpy()
    t = {"triangle": (np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], F32), np.array([[0, 1, 2]], np.int32)),
         "two": (np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.25]], F32), np.array([[0, 1, 2], [0, 3, 1]], np.int32)),
         "cube": R.cube_mesh(),
         "sphere16": mc(CC.spheres_volume(16, (((7.3, 7.9, 8.2), 5.1),)), 16, 0.0, "ascent"),
         "sphere32": mc(CC.spheres_volume(32), 32, 0.0, "ascent"),
         "torus": torus(),
         "noise": mc(CC.noise_volume(14), 14, 0.5, "descent")}
    # every triangle in one cell of a box that two far corners stretch
    v, f = tiny_soup(400, (4.0, 4.0, 4.0), (4.2, 4.2, 4.2), 0.05, 1)
    cv, cf = tiny_soup(2, (0.0, 0.0, 0.0), (0.01, 0.01, 0.01), 0.005, 2)
    cv[3:] += F32(10.0)
    t["one_cell"] = (np.concatenate([v, cv]), np.concatenate([f, cf + v.shape[0]]))
    # every triangle spans the box: the pair count pushes the level up to a single cell
    rng = np.random.default_rng(3)
    big = (rng.random((300, 3, 3)) * 0.05 + np.array([[0, 0, 0], [1, 0.1, 0.9], [0.1, 1, 0.95]])[None]).reshape(-1, 3).astype(F32)
    t["all_span"] = (big, np.arange(900, dtype=np.int32).reshape(300, 3))
    # one triangle spanning the whole box among many tiny ones
    v, f = tiny_soup(600, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.02, 4)
    v[:3] = np.array([[0, 0, 0], [1, 0.05, 1], [0.05, 1, 1]], F32)
    t["one_spans"] = (v, f)
    for k, (v, f) in t.items():
        print(k, "V", v.shape[0], "T", f.shape[0])
    return t


def query_points(v, f, other, seed):
    """the query sets of one target: the other mesh's vertices moved into its box, points on its surface, points far outside (ten
    extents), points exactly on cell planes, and noise around the box"""
    from dsnerf_amd import _lib
    rng = np.random.default_rng(seed)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    ext = max(float((hi - lo).max()), 1e-3)
    ov = other.astype(np.float64)
    ov = lo + (ov - ov.min(axis=0)) / max(float((ov.max(axis=0) - ov.min(axis=0)).max()), 1e-9) * ext
    surf = R.sample_surface(v, f, 300, seed=seed)[0]
    far = (lo + hi) / 2 + (rng.random((40, 3)) - 0.5) * 2 * 10 * ext
    g, cell = _lib.mesh_dist_grid(f.shape[0], (v.min(axis=0), v.max(axis=0)))
    o = v.min(axis=0)
    planes = []
    for _ in range(120):
        k = [rng.integers(0, int(g[a]) + 1) for a in range(3)]
        p = np.array([F32(o[a] + F32(F32(k[a]) * cell)) for a in range(3)], F32)
        free = rng.random(3) < 0.4                          # some coordinates off the planes
        planes.append(np.where(free, (lo + rng.random(3) * (hi - lo)).astype(F32), p))
    around = lo - 0.3 * ext + rng.random((300, 3)) * (hi - lo + 0.6 * ext)
    return np.concatenate([ov[:: max(1, ov.shape[0] // 300)][:300], surf, far, np.array(planes), around, v[:: max(1, v.shape[0] // 100)][:100]]).astype(F32)


NAMES = ["triangle", "two", "cube", "sphere16", "sphere32", "torus", "noise", "one_cell", "all_span", "one_spans"]


@pytest.fixture(scope="module")
def references(targets):
    """name -> (points, brute force's triple): computed once, shared, never changed"""
    out = {}
    for k, name in enumerate(NAMES):
        v, f = targets[name]
        pts = query_points(v, f, targets["torus" if name != "torus" else "sphere16"][0], 10 + k)
        out[name] = (pts, R.brute_force(v, f, pts))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_against_brute_force(targets, references, name):
    v, f = targets[name]
    pts, want = references[name]
    _, info = check(v, f, pts, want)
    print(name, "queries", pts.shape[0], info, "mean list", info["listed_pairs"] / max(info["cells"], 1))
    assert info["valid_faces"] == f.shape[0] and info["listed_pairs"] >= f.shape[0]
    assert info["listed_pairs"] <= R.entries_cap(f.shape[0]) and info["cells"] <= R.cells_cap(f.shape[0])
    m = R.GridModel(v, f) if f.shape[0] <= 1000 else None
    if m is not None:
        assert (info["level"], info["cells"], info["listed_pairs"]) == (m.level, int(np.prod(m.g)), m.pairs[m.level])
    if name == "all_span":
        assert info["level"] > 0
    if name == "one_cell":
        assert info["cells"] > 100                           # a real grid, with all but two faces in one of its cells


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 3000])
def test_query_counts(targets, references, n):
    v, f = targets["sphere16"]
    pts, want = references["sphere16"]
    reps = (n + pts.shape[0] - 1) // pts.shape[0] if n else 0
    idx = np.tile(np.arange(pts.shape[0]), max(reps, 1))[:n]
    got, _ = check(v, f, pts[idx], tuple(w[idx] for w in want))
    if n == 0:
        assert got[0].shape == (0,)


def test_ties_duplicates_and_face_order(targets, references):
    """duplicated faces, a reversed and a shuffled face list: distance and point keep their bits, the face index follows the rule"""
    v, f = targets["torus"]
    pts, want = references["torus"]
    pts, want = pts[:600], tuple(w[:600] for w in want)
    T = f.shape[0]
    rng = np.random.default_rng(8)
    for perm in (np.arange(T)[::-1], rng.permutation(T), np.concatenate([np.arange(T), np.arange(T)]), np.concatenate([rng.permutation(T), np.arange(T)])):
        first = np.full(T, 2 * T, np.int64)
        np.minimum.at(first, perm, np.arange(perm.shape[0]))          # the lowest new index of every old face
        # the new index the rule must report: the lowest among the faces that tie for the minimum - recomputed by brute force
        got, _ = check(v, f[perm], pts)
        assert np.array_equal(bits(got[0]), bits(want[0]))   # the distance keeps its bits under any order
        same_face = perm[got[1]] == want[1]
        print("queries whose winner is the same old face", int(same_face.sum()), "of", same_face.size)
        # the point keeps its bits wherever the same face wins.  Where ANOTHER face wins now, the two tie in the distance bit for bit (a
        # query on a shared edge or vertex, or so far away that neighbouring faces round to one distance) and the rule reports the lower
        # index's own closest point - check() has compared it with brute force on this very list
        assert np.array_equal(bits(got[2])[same_face], bits(want[2])[same_face])
        assert (got[1] <= first[want[1]]).all()              # never a higher index than the old winner's first copy
        if np.array_equal(perm[:T], np.arange(T)):           # duplicates appended: nothing changes at all
            assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
        else:
            assert same_face.any() and not same_face.all()   # the list has both: queries with one nearest face and queries with a tie
    # rotating the corners of every face is another triangle for the rule's arithmetic: only the restatement of that list binds
    check(v, np.roll(f, 1, axis=1), pts)
    # exact ties by construction: coplanar faces sharing an edge, queries on the perpendicular through it
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0]], F32)
    f2 = np.array([[0, 1, 2], [0, 3, 1]], np.int32)
    q2 = np.array([(0.5, 0, 1), (0.25, 0, 2), (0.75, 0, -0.5)], F32)
    for faces in (f2, f2[::-1], np.concatenate([f2[::-1], f2, f2])):
        got, _ = check(v2, faces, q2)
        assert got[1].tolist() == [0, 0, 0] and got[0].tolist() == [1.0, 4.0, 0.25]


def test_the_margin_case():
    """a face just inside a farther shell that is nearer by a few float32 steps than the nearest candidate of the nearer shell: brute force
    picks it (tests/test_mesh_dist_host.py shows that a search stopping on the bare bound does not), and so must the kernel"""
    mc = R.margin_case()
    p = mc["point"]
    want = R.brute_force(mc["verts"], mc["faces"], p[None])
    assert want[1][0] == mc["far_face"]
    assert mc["model"].query(p, margin=False)[1] == mc["near_face"]
    got, info = check(mc["verts"], mc["faces"], np.stack([p, p, mc["verts"][0]]))
    assert got[1][0] == mc["far_face"] and info["level"] == 0 and info["cells"] == int(np.prod(mc["model"].g))


def test_invalid_faces_and_points(targets):
    v, f = targets["sphere16"]
    rng = np.random.default_rng(12)
    V, T = v.shape[0], f.shape[0]
    v = np.concatenate([v, np.array([[np.nan, 1, 1], [np.inf, 2, 2], [3, -np.inf, 3]], F32)])
    f = f.copy()
    bad = rng.choice(T, 60, replace=False)
    f[bad[:15], 0] = -1
    f[bad[15:30], 1] = V + 3
    f[bad[30:40], 2] = 2 ** 31 - 1
    f[bad[40:60], rng.integers(0, 3, 20)] = V + rng.integers(0, 3, 20)          # a vertex that is not finite
    assert int(R.valid_faces(v, f).sum()) == T - 60
    pts = np.concatenate([v[:V:7], (rng.random((300, 3)) * 16).astype(F32)])
    pts[5] = [np.nan, 1, 1]
    pts[70] = [1, np.inf, 1]
    pts[71] = [1, 1, -np.inf]
    box = (v[:V].min(axis=0), v[:V].max(axis=0))
    want, info = check(v, f, pts)
    assert info["valid_faces"] == T - 60
    assert np.isnan(want[0][[5, 70, 71]]).all() and (want[1][[5, 70, 71]] == -1).all() and np.isfinite(want[0][[4, 6, 69, 72]]).all()
    # = the restatement with those faces removed
    keep = np.setdiff1d(np.arange(T), bad)
    less = R.brute_force(v, f[keep], pts)
    assert np.array_equal(bits(less[0]), bits(want[0])) and np.array_equal(bits(less[2]), bits(want[2]))
    assert np.array_equal(np.where(less[1] >= 0, keep[np.maximum(less[1], 0)], -1), want[1])
    # null optional outputs: each output alone carries the same bits; outputs start as 0xFF bytes (poisoned) and are written everywhere
    from dsnerf_amd import _lib
    for only in ("dist2", "face", "point"):
        out, _ = query(v, f, pts, want_distance=only == "dist2", want_face=only == "face", want_point=only == "point")
        assert [k for k in out if out[k] is not None] == [only]
        assert np.array_equal(bits(out[only]), bits(want[{"dist2": 0, "face": 1, "point": 2}[only]]))
    # a dirty workspace and repeated calls: the same bits; a caller's box that is larger than the mesh
    dv, df = gpu(v, f)
    dp = torch.from_numpy(pts).to(DEV)
    index = _lib.mesh_dist_build(dv, df)
    first = _lib.mesh_dist_query(index, dp)
    index["ws"].fill_(0xFF)
    unbuilt = _lib.mesh_dist_query(index, dp)               # a workspace no build has filled: NaN, -1, NaN - no fault
    assert torch.isnan(unbuilt["dist2"]).all() and (unbuilt["face"] == -1).all() and torch.isnan(unbuilt["point"]).all()
    state = {"ws": index["ws"], "counts": index["counts"]}
    for _ in range(2):
        index = _lib.mesh_dist_build(dv, df, state=state)
        again = _lib.mesh_dist_query(index, dp)
        assert all(np.array_equal(bits(first[k]), bits(again[k])) for k in first)
    check(v, f, pts, want, box=(box[0] - F32(3.0), box[1] + F32(5.0)))
    # a target without a valid face, an empty target
    with pytest.raises(ValueError):
        _lib.mesh_dist_build(dv, torch.full((4, 3), -1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        _lib.mesh_dist_build(dv, df[:0])
    with pytest.raises(ValueError):
        _lib.mesh_dist_build(dv[:0], df)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1024, 1025, 70001])
def test_reduction(n):
    from dsnerf_amd import _lib
    rng = np.random.default_rng(40 + n)
    cases = [(rng.random(n) ** 2 * 3).astype(F32)]
    if n > 10:
        x = cases[0].copy()
        x[rng.integers(0, n, 7)] = np.nan
        top = F32(np.nanmax(x) + 1)
        x[[n // 2, n - 1, n // 3]] = top                    # the maximum three times: the lowest index
        cases += [x, np.full(n, np.nan, F32), np.zeros(n, F32)]
    for x in cases:
        got = _lib.mesh_dist_reduce(torch.from_numpy(x).to(DEV)).cpu().numpy()
        want = R.reduce_stats(x)
        print(n, got.tolist())
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    if n > 10:
        assert R.reduce_stats(cases[1])[5] == n // 3 and R.reduce_stats(cases[1])[1] >= 1


@pytest.mark.parametrize("n", [0, 1, 64, 1000])
def test_sampler(n):
    from dsnerf_amd import _lib
    v, f = R.icosphere(3)
    f = f.copy()
    f[5] = [0, 0, 1]
    f[40] = [0, 1, 10 ** 6]
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [10, 0, 0], [11.5, 0, 0], [10, 0, 4]], F32)
    f2 = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    for (verts, faces), seed in (((v, f), 9), ((v2, f2), 0), ((v, f), 2 ** 63 + 12345)):
        dv, df = gpu(verts, faces)
        pts, face = _lib.mesh_sample_surface(dv, df, n, seed)
        wp, wf = R.sample_surface(verts, faces, n, seed)
        assert tuple(pts.shape) == (n, 3) and tuple(face.shape) == (n,)
        assert np.array_equal(face.cpu().numpy(), wf) and np.array_equal(bits(pts), bits(wp))
        if n == 1000:
            p64, f64 = _lib.mesh_sample_surface(dv, df, 64, seed)
            assert np.array_equal(bits(p64), bits(pts[:64])) and torch.equal(f64, face[:64])
            only = _lib.mesh_sample_surface(dv, df, n, seed, want_face=False)
            assert only[1] is None and np.array_equal(bits(only[0]), bits(pts))
    if n == 64:                                               # a mesh without area: NaN, -1
        pts, face = _lib.mesh_sample_surface(*gpu(v2, np.array([[0, 0, 1]], np.int32)), n, 0)
        assert torch.isnan(pts).all() and (face == -1).all()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_mesh_distance_forms(targets):
    """visualizer.closest_point / sample_surface / mesh_distance on small meshes: numpy and device forms, dicts and tuples, the figures
    against the restatement"""
    from dsnerf_amd import visualizer
    v, f = targets["sphere16"]
    tv, tf = targets["torus"]
    tv = (tv * 4 + np.array([8, 8, 8])).astype(F32)
    cp = visualizer.closest_point((v, f), tv)
    want = R.brute_force(v, f, tv)
    assert cp["distance"].is_cuda and np.array_equal(bits(cp["distance"]), bits(np.sqrt(want[0])))
    assert np.array_equal(cp["face"].cpu().numpy(), want[1]) and np.array_equal(bits(cp["point"]), bits(want[2]))
    s = visualizer.sample_surface({"verts": torch.from_numpy(v).to(DEV), "faces": torch.from_numpy(f).to(DEV)}, 500, seed=3)
    ws = R.sample_surface(v, f, 500, 3)
    assert np.array_equal(bits(s["points"]), bits(ws[0])) and np.array_equal(s["face"].cpu().numpy(), ws[1])
    d = visualizer.mesh_distance((v, f), {"verts": tv, "faces": tf}, return_distances=True)
    ab, ba = R.reduce_stats(want[0]), R.reduce_stats(R.brute_force(tv, tf, v)[0])
    for name, w in (("a_to_b", ba), ("b_to_a", ab)):
        got = d[name]
        assert all(isinstance(got[k], float) for k in ("mean", "rms", "max", "argmax", "count"))
        assert got["count"] == w[0] and got["mean"] == w[2] / w[0] and got["rms"] == (w[3] / w[0]) ** 0.5 and got["max"] == w[4] and got["argmax"] == w[5]
        assert got["distance"].is_cuda and got["distance"].shape[0] == w[0]
    assert d["chamfer"] == (d["a_to_b"]["mean"] + d["b_to_a"]["mean"]) / 2 and d["hausdorff"] == max(d["a_to_b"]["max"], d["b_to_a"]["max"])
    one = visualizer.mesh_distance((v, f), (tv, tf), symmetric=False)
    assert "b_to_a" not in one and one["a_to_b"] == {k: d["a_to_b"][k] for k in one["a_to_b"]} and one["chamfer"] == one["a_to_b"]["mean"]
    sampled = visualizer.mesh_distance((v, f), (tv, tf), samples=700, seed=5)
    pa = R.sample_surface(v, f, 700, 5)[0]
    wa = R.reduce_stats(R.brute_force(tv, tf, pa)[0])
    assert sampled["a_to_b"]["count"] == 700 and sampled["a_to_b"]["mean"] == wa[2] / 700 and sampled["a_to_b"]["max"] == wa[4]
    again = visualizer.mesh_distance((v, f), (tv, tf), samples=700, seed=5)
    assert again == sampled
    with pytest.raises(ValueError):
        visualizer.mesh_distance((v, f), (tv, np.full((3, 3), -1, np.int32)))
    with pytest.raises(ValueError):
        visualizer.mesh_distance((v, f), (tv, tf), samples="faces")


def test_extract_mesh_end_to_end():
    """the small body: what simplification and smoothing do to the surface, in numbers"""
    from dsnerf_amd import visualizer
    from helpers import load
    from test_gpu_render import make_batch, make_renderer
    g = load("full_eval_w4")
    r = make_renderer(g, "full_eval_w4")
    r.eval()
    batch = make_batch(g)
    dense = r.extract_mesh(batch, 48, largest_component=True)
    same = visualizer.mesh_distance(dense, dense)
    print("mesh against itself", same)
    for name in ("a_to_b", "b_to_a"):
        assert same[name]["mean"] == 0.0 and same[name]["rms"] == 0.0 and same[name]["max"] == 0.0 and same[name]["count"] == dense["verts"].shape[0]
    assert same["chamfer"] == 0.0 and same["hausdorff"] == 0.0
    thin = visualizer.simplify_mesh(dense, target_vertices=600)
    d = visualizer.mesh_distance(thin, dense, samples="vertices")
    cell = float(thin["simplify_info"]["cell"])
    print("simplified against dense", d, "cell", cell, "diagonal", cell * 3 ** 0.5)
    assert d["a_to_b"]["max"] == 0.0                       # the simplified vertices are a subset of the dense ones
    assert 0.0 < d["b_to_a"]["max"] <= cell * 3 ** 0.5 and d["hausdorff"] == d["b_to_a"]["max"] and d["chamfer"] == d["b_to_a"]["mean"] / 2
    ds = visualizer.mesh_distance(thin, dense, samples=4000, seed=1)
    print("simplified against dense, surface samples", ds)
    assert ds["a_to_b"]["max"] > 0.0 and ds["a_to_b"]["count"] == 4000
    smooth = visualizer.smooth_mesh(dense, iterations=3)
    dm = visualizer.mesh_distance(smooth, dense)
    print("smoothed against dense", dm)
    assert dm["a_to_b"]["max"] > 0.0 and dm["b_to_a"]["max"] > 0.0 and dm["chamfer"] > 0.0
    # extract_mesh(report_distance=True): the same figures as the direct call; without the option nothing changes
    plain = r.extract_mesh(batch, 48, largest_component=True, target_vertices=600)
    rep = r.extract_mesh(batch, 48, largest_component=True, target_vertices=600, report_distance=True)
    assert "distance" not in plain and set(rep) == set(plain) | {"distance"}
    for k in plain:
        if torch.is_tensor(plain[k]):
            assert same_bits(plain[k], rep[k]) and same_bits(plain[k], thin[k]), k
    assert rep["distance"] == d
    with pytest.raises(ValueError):
        r.extract_mesh(batch, 48, report_distance=True)
    # Visualizer3D.get_mesh_from_grid: one more element
    vis = visualizer.Visualizer3D(48, 64, 0.5, "ascent")
    axes, vol = r.density_grid(batch, resolution=48)
    pts = np.stack(np.meshgrid(*[np.asarray(a, F32) for a in axes], indexing="ij"), -1)
    pred = vol.cpu().numpy()[..., None]
    base = vis.get_mesh_from_grid(pts, pred, largest_component=True, target_vertices=600)
    with_report = vis.get_mesh_from_grid(pts, pred, largest_component=True, target_vertices=600, report_distance=True)
    assert len(base) == 2 and len(with_report) == 3 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(base, with_report))
    assert with_report[2] == d
    del r


def test_render_view_is_untouched_by_the_distances():
    from dsnerf_amd import visualizer
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
    mesh = r.extract_mesh(make_batch(g), 24, target_vertices=150, report_distance=True)
    assert mesh is not None and mesh["distance"]["a_to_b"]["max"] == 0.0 and mesh["distance"]["hausdorff"] > 0.0
    full = r.extract_mesh(make_batch(g), 24)
    assert visualizer.mesh_distance(mesh, full, samples=500)["a_to_b"]["count"] == 500
    after = frame()
    assert set(before) == set(after) and len(before) >= 3
    for k in before:      # bit patterns (NaN-safe)
        assert same_bits(before[k], after[k]), k
    del r
