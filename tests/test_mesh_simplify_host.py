"""Mesh simplification without a GPU: the numpy restatement of include/dsnerf.h's rule (tests/mesh_simplify_restate.py) on meshes whose
result is known, the properties the rule promises, and the argument checks of dsn_mesh_simplify_* through the loaded library."""
import ctypes as C

import numpy as np
import pytest

import mesh_simplify_restate as R

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


@pytest.fixture(scope="module")
def sphere():
    v, f = R.icosphere(4)
    assert v.shape == (2562, 3) and f.shape == (5120, 3) and R.euler(2562, f) == 2 and R.closed(f)
    return v, f


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_planar_grid_halves(n):
    """a 2n x 2n grid of vertices, cells of 2 x 2 vertices: the n x n grid, and of each cell's four vertices (all equally far from their
    mean) the one with the smallest index"""
    m = 2 * n
    v, f = R.planar_grid(m)
    out = R.simplify(v, f, 2.0, np.zeros(3, F32), [n, n, 1])
    assert out["verts"].shape == (n * n, 3) and out["faces"].shape == (2 * (n - 1) ** 2, 3)
    ci, cj = np.divmod(np.arange(n * n), n)
    assert np.array_equal(out["cluster_source"], 2 * ci * m + 2 * cj)
    assert np.array_equal(out["verts"], v[out["cluster_source"]])
    assert out["counts"].tolist()[:1] + out["counts"].tolist()[4:] == [n * n, 0, 0, 0]
    if n > 1:      # the result is the n x n grid mesh: the same edges as planar_grid(n)'s
        want, _ = R.edge_counts(R.planar_grid(n)[1])
        got, cnt = R.edge_counts(out["faces"])
        assert np.array_equal(got, want) and R.euler(n * n, out["faces"]) == 1 and cnt.max() == 2


@pytest.mark.parametrize("n,K,T", [(4, 56, 108), (8, 248, 492), (16, 800, 1596)])
def test_icosphere_stays_closed(sphere, n, K, T):
    v, f = sphere
    o, c, g = R.cube_grid(n)
    out = R.simplify(v, f, c, o, g)
    assert out["counts"].tolist() == [K, T, T, 0, 0, 0, 0]
    assert R.euler(K, out["faces"]) == 2 and R.closed(out["faces"])


def test_duplicates_are_part_of_the_rule():
    """the 40 962-vertex icosphere at 32 cells per axis: closed only because duplicate triangles go"""
    v, f = R.icosphere(6)
    o, c, g = R.cube_grid(32)
    out = R.simplify(v, f, c, o, g)
    K, kept, live, dup = out["counts"].tolist()[:4]
    assert dup > 0 and kept + dup == live and R.euler(K, out["faces"]) == 2
    tri = np.sort(out["faces"], axis=1)
    assert np.unique(tri, axis=0).shape[0] == kept


def test_subset_property(sphere):
    rng = np.random.default_rng(3)
    v, f = sphere
    v = (v * F32(0.37) + rng.normal(0, 0.002, v.shape).astype(F32)).astype(F32)
    cell = F32(0.09)
    o, g = R.default_grid(v, cell)
    out = R.simplify(v, f, cell, o, g)
    src, vc = out["cluster_source"], out["vertex_cluster"]
    assert (vc >= 0).all() and out["counts"][4] == 0
    assert np.array_equal(out["verts"].view(np.uint32), v[src].view(np.uint32))
    assert np.array_equal(vc[src], np.arange(src.size))                      # a representative is a member of its cluster
    dist = np.linalg.norm(v.astype(np.float64) - out["verts"][vc].astype(np.float64), axis=1)
    assert dist.max() <= np.sqrt(3.0) * float(cell) * (1 + 1e-6)
    assert out["faces"].min() >= 0 and out["faces"].max() < src.size
    assert np.array_equal(out["faces"], vc[f[out["keep"]]])                  # input order and winding


def test_ties_go_to_the_smaller_index():
    o, g = np.zeros(3, F32), [2, 1, 1]
    # coincident vertices; two vertices symmetric about the mean (the third sits on it in the first cell)
    v = np.array([[1.5, 0.5, 0.5], [0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [1.5, 0.5, 0.5], [1.5, 0.5, 0.5]], F32)
    out = R.simplify(v, np.zeros((0, 3), np.int32), 1.0, o, g)
    assert out["cluster_source"].tolist() == [1, 0] and out["vertex_cluster"].tolist() == [1, 0, 0, 1, 1]
    out = R.simplify(v[::-1], np.zeros((0, 3), np.int32), 1.0, o, g)
    assert out["cluster_source"].tolist() == [2, 0]
    # ... and a vertex on the mean wins whatever its index
    v = np.array([[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [0.5, 0.5, 0.5]], F32)
    assert R.simplify(v, np.zeros((0, 3), np.int32), 1.0, o, g)["cluster_source"].tolist() == [2]


def test_sums_stay_below_2_to_the_63():
    n, q = 2 ** 31 - 1, 2 ** 32 - 1          # the most members a cluster can have, the largest q (t < 4096: q < 2^32)
    assert n * q < 2 ** 63
    assert int(np.floor(float(np.nextafter(F32(4096), F32(0))) * 2.0 ** 20)) <= q
    # q is exact in double: a float32 times 2^20
    t = np.nextafter(F32(4096), F32(0))
    assert float(t) * 2.0 ** 20 == np.ldexp(float(t), 20)


def test_face_order_decides_which_duplicate_stays():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.4, 0.5], [1.6, 0.4, 0.5], [0.4, 1.6, 0.5]], F32)
    f = np.array([[0, 1, 2], [4, 5, 3], [5, 4, 3], [0, 1, 3], [0, 0, 1], [2, 1, 0]], np.int32)
    o, g = np.zeros(3, F32), [2, 2, 1]
    out = R.simplify(v, f, 1.0, o, g)
    assert out["keep"].tolist() == [True, False, False, False, False, False] and out["counts"].tolist()[:4] == [3, 1, 4, 3]
    assert out["faces"].tolist() == [[0, 2, 1]]                             # face 0's winding, clusters in cell order
    rev = R.simplify(v, f[::-1], 1.0, o, g)
    assert rev["keep"].tolist() == [True, False, False, False, False, False]
    assert rev["faces"].tolist() == [[1, 2, 0]]                             # now face (2, 1, 0) is the first of its triple


def test_edges_of_the_rule():
    nan, inf = np.nan, np.inf
    o, g = np.array([-1, -1, -1], F32), [2, 2, 2]
    v = np.array([[-1, -1, -1], [0, 0, 0], [1, 0, 0], [0.999999, 0.5, 0.5], [-1.0001, 0, 0], [nan, 0, 0], [0, inf, 0], [0, 0, -inf],
                  [-0.5, -0.5, -0.5]], F32)
    f = np.array([[0, 1, 3], [-1, 0, 1], [0, 1, 9], [0, 1, 2], [0, 8, 1], [1, 1, 0]], np.int32)
    out = R.simplify(v, f, 1.0, o, g)
    assert out["vertex_cluster"].tolist() == [0, 1, -1, 1, -1, -1, -1, -1, 0]      # t = g is outside, the origin and a boundary inside
    assert out["counts"].tolist() == [2, 0, 0, 0, 5, 2, 0]


def test_target_search_and_defaults(sphere):
    v, _ = sphere
    n, cell, o, g, probes = R.target_search(v, 500)
    assert len(probes) == 12 and probes[0] == 2049 and g == [n, n, n]
    assert R.cell_count(v, cell, o, g) <= 500
    o2, g2 = R.default_grid(v, R.target_cell(v, n + 1))
    assert R.cell_count(v, R.target_cell(v, n + 1), o2, g2) > 500
    inside, _, _ = R.locate(v, o, cell, g)
    assert inside.all()
    # no finite vertex, one vertex, a flat mesh
    n0, c0, o0, g0, _ = R.target_search(np.full((3, 3), np.nan, F32), 5)
    assert (n0, c0, o0.tolist(), g0) == (4096, F32(1.0), [0.0, 0.0, 0.0], [1, 1, 1])
    assert R.cell_count(np.full((3, 3), np.nan, F32), 1.0, np.zeros(3, F32), [1, 1, 1]) == 0
    one = np.array([[3, 4, 5]], F32)
    assert R.target_cell(one, 7) == F32(1.0) and R.default_grid(one, 1.0)[1] == [1, 1, 1]


def test_gather_dict(sphere):
    v, f = sphere
    rng = np.random.default_rng(2)
    V = v.shape[0]
    mesh = {"verts": v, "faces": f, "normals": v.copy(), "colour": rng.random((2, V, 3)).astype(F32), "sigma": rng.random(V).astype(F32),
            "face_idx": rng.integers(0, 99, V).astype(np.int32), "uv": rng.random((V, 2)).astype(F32), "cov": None, "name": "body"}
    o, c, g = R.cube_grid(8)
    out = R.simplify(v, f, c, o, g)
    got = R.gather_dict(mesh, out)
    src = out["cluster_source"]
    assert got["name"] == "body" and got["cov"] is None and got["colour"].shape == (2, src.size, 3)
    assert np.array_equal(got["colour"][1], mesh["colour"][1][src]) and np.array_equal(got["uv"], mesh["uv"][src])
    assert np.array_equal(got["normals"], got["verts"])


def test_abi_symbols_and_argument_checks(lib):
    import dsnerf_amd
    L = dsnerf_amd._lib
    names = ("dsn_mesh_simplify_workspace_bytes", "dsn_mesh_simplify_count", "dsn_mesh_simplify_emit", "dsn_mesh_simplify_cells",
             "dsn_mesh_simplify_count_ex", "dsn_mesh_simplify_emit_ex")
    for n in names:
        assert hasattr(lib, n) and n in L.EXPORTS
    assert (L.MESH_SIMPLIFY_MAX_G, L.MESH_SIMPLIFY_MAX_CLUSTERS) == (R.MAX_G, R.CAP)
    z, one, al = None, C.c_void_p(1), C.c_void_p(4096)
    G = lambda *g: (C.c_int * 3)(*g)
    org = (C.c_float * 3)(0.0, 0.0, 0.0)
    wb = lib.dsn_mesh_simplify_workspace_bytes
    # sizes
    assert wb(100, 200, G(4096, 1, 1)) > 0 and wb(100, 200, G(4097, 1, 1)) == 0 and wb(100, 200, G(0, 1, 1)) == 0
    assert wb(100, 200, G(2048, 1024, 1024)) > 0 and wb(100, 200, G(2048, 1024, 1025)) == 0          # 2^31 cells, and more
    assert wb(-1, 0, G(1, 1, 1)) == 0 and wb(0, 1 << 31, G(1, 1, 1)) == 0 and wb(1 << 31, 0, G(1, 1, 1)) == 0 and wb(1, 1, None) == 0
    assert wb(0, 0, G(1, 1, 1)) > 0
    small, big = wb(1000, 2000, G(8, 8, 8)), wb(1000, 2000, G(256, 256, 256))
    assert big - small >= 2 * (256 ** 3 - 8 ** 3) // 8 and small >= 1000 * 8 + 2 * 2000 * 12          # bit grid + prefix; table at load 1/2
    n = wb(10, 10, G(4, 4, 4))

    def count(v=one, f=one, V=10, T=10, o=org, cell=1.0, g=G(4, 4, 4), ws=al, nb=n, vc=z, cnt=one):
        return lib.dsn_mesh_simplify_count(v, f, V, T, o, cell, g, ws, nb, vc, cnt, z)

    def emit(v=one, f=one, V=10, T=10, g=G(4, 4, 4), ws=al, nb=n, nv=5, nf=5, ov=one, of=one, src=z):
        return lib.dsn_mesh_simplify_emit(v, f, V, T, g, ws, nb, nv, nf, ov, of, src, z)

    def cells(v=one, V=10, o=org, cell=1.0, g=G(4, 4, 4), ws=al, nb=n, out=one):
        return lib.dsn_mesh_simplify_cells(v, V, o, cell, g, ws, nb, out, z)
    bad_count = [(dict(v=z), b"null mesh"), (dict(f=z), b"null mesh"), (dict(o=z), b"null argument"), (dict(g=None), b"null argument"),
                 (dict(ws=z), b"null argument"), (dict(cnt=z), b"null argument"), (dict(V=-1), b"negative"), (dict(T=1 << 31), b"2^31"),
                 (dict(g=G(4097, 1, 1)), b"4096"), (dict(g=G(4, 0, 4)), b"4096"), (dict(g=G(2048, 1024, 1025)), b"2^31"),
                 (dict(cell=0.0), b"cell"), (dict(cell=-1.0), b"cell"), (dict(cell=float("nan")), b"cell"), (dict(cell=float("inf")), b"cell"),
                 (dict(cell=1e-45), b"cell"), (dict(o=(C.c_float * 3)(0.0, float("nan"), 0.0)), b"origin"),
                 (dict(ws=C.c_void_p(4100)), b"16-byte"), (dict(nb=n - 1), b"too small"), (dict(nb=0), b"too small")]
    for kw, msg in bad_count:
        assert count(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_mesh_simplify_count" in err and msg in err, (kw, err)
    assert lib.dsn_mesh_simplify_count_ex(one, one, 10, 10, org, 1.0, G(4, 4, 4), al, n, z, one, 128, z) != 0 and b"phases" in lib.dsn_last_error()
    bad_emit = [(dict(v=z), b"null mesh"), (dict(g=None), b"null argument"), (dict(ws=z), b"null argument"), (dict(nv=11), b"more clusters"),
                (dict(nf=11), b"more clusters"), (dict(nv=9, g=G(2, 2, 2)), b"more clusters"), (dict(nv=-1), b"negative"),
                (dict(ov=z), b"null output"), (dict(of=z), b"null output"), (dict(ws=C.c_void_p(4104)), b"16-byte"), (dict(nb=n - 16), b"too small"),
                (dict(g=G(4097, 1, 1)), b"4096")]
    for kw, msg in bad_emit:
        assert emit(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_mesh_simplify_emit" in err and msg in err, (kw, err)
    assert lib.dsn_mesh_simplify_emit_ex(one, one, 10, 10, G(4, 4, 4), al, n, 5, 5, one, one, z, 64, z) != 0 and b"phases" in lib.dsn_last_error()
    assert emit(nv=0, nf=0, ov=z, of=z) == 0                                 # nothing to write: no device work
    for kw, msg in [(dict(v=z), b"null mesh"), (dict(out=z), b"null argument"), (dict(g=G(1, 1, 4097)), b"4096"), (dict(cell=0.0), b"cell"),
                    (dict(ws=C.c_void_p(4097)), b"16-byte"), (dict(nb=16), b"too small"), (dict(V=1 << 31), b"2^31")]:
        assert cells(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_mesh_simplify_cells" in err and msg in err, (kw, err)


def test_python_argument_checks():
    from dsnerf_amd import _lib, visualizer
    box = (np.zeros(3, F32), np.array([1, 2, 0.5], F32))
    o, g = _lib.mesh_simplify_grid(box, 0.25)
    assert o.tolist() == [0, 0, 0] and g == [5, 9, 3]
    assert _lib.mesh_simplify_grid(None, 0.25) [1] == [1, 1, 1]
    for cell in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            _lib._mesh_simplify_check_grid(cell, o, g)
    with pytest.raises(ValueError):
        _lib._mesh_simplify_check_grid(1.0, o, [4097, 1, 1])
    _lib._mesh_simplify_check_grid(1.0, o, [4096, 1, 1])
    v, f = R.planar_grid(4)
    for kw in (dict(), dict(cell=1.0, target_vertices=5)):
        with pytest.raises(ValueError):
            visualizer.simplify_mesh((v, f), **kw)
    for n in (1, 7, 100, 4096):
        assert F32(_lib.mesh_target_cell(box, n)) == R.target_cell(np.stack(box), n)
