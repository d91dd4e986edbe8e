"""Mesh components without a GPU: the numpy restatement of include/dsnerf.h's rule (tests/mesh_cc_restate.py) against
scipy.sparse.csgraph under the vertex rule and, on marching-cubes outputs, under trimesh's edge rule; the winner, the shift's bound, order
independence, ties, the reported area; and the argument checks of the entry points."""
import ctypes as C

import numpy as np
import pytest

import mc_restate as M
import mesh_cc_restate as R

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


@pytest.fixture(scope="module")
def meshes():
    """name -> (verts, faces) of the marching-cubes outputs the GPU tests use too, by the numpy marching cubes"""
    import dsnerf_amd
    table = dsnerf_amd._lib.mc_table()
    return {
        "noise": M.marching_cubes(R.noise_volume(), R.axes_of(24), 0.5, "descent", table),
        "smooth": M.marching_cubes(R.smooth_volume(), R.axes_of(24), 0.5, "descent", table),
        "spheres": M.marching_cubes(R.spheres_volume(), R.axes_of(32), 0.0, "ascent", table),
    }


def test_partition_is_scipys_and_on_marching_cubes_the_edge_rule_too(meshes):
    seen = {}
    for name, (v, f) in meshes.items():
        V = v.shape[0]
        lab = R.labels(V, f)
        comp, used = R.partition_by_vertices(V, f)
        assert used.all() and (lab >= 0).all()                      # marching cubes leaves no vertex unused
        assert R.same_partition(lab, comp), name
        # labels are minimum indices
        for l in np.unique(lab):
            assert np.flatnonzero(lab == l)[0] == l
        assert (lab <= np.arange(V)).all()
        # trimesh's rule (faces joined through shared edges) gives the same classes of faces here
        assert R.same_partition(lab[f[:, 0]], R.partition_by_edges(V, f)), name
        seen[name] = len(np.unique(lab))
    assert seen["noise"] > 100 and 2 <= seen["smooth"] < 40 and seen["spheres"] == 3, seen


def test_the_rules_differ_at_a_pinch_vertex():
    """two triangles that touch in one vertex: one component here, two under the edge rule; coincident positions under different
    indices do not connect"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 0]], F32)
    f = np.array([[0, 1, 2], [0, 3, 4]])
    assert R.labels(6, f).tolist() == [0, 0, 0, 0, 0, -1]
    assert len(np.unique(R.partition_by_edges(6, f))) == 2
    assert R.labels(6, np.array([[0, 1, 2], [5, 3, 4]])).tolist() == [0, 0, 0, 3, 3, 3]
    # invalid faces connect nothing, repeated indices do
    assert R.labels(6, np.array([[0, 1, 2], [2, 3, 6], [2, -1, 3], [4, 4, 5], [5, 5, 3]])).tolist() == [0, 0, 0, 3, 3, 3]


def test_the_big_sphere_wins(meshes):
    v, f = meshes["spheres"]
    c = R.components(v, f)
    sums = sorted((s for s, _ in c["sums"].values()), reverse=True)
    assert len(sums) == 3 and 0.25 < sums[1] / sums[0] < 0.37             # (4.1 / 7.3)^2 = 0.315: no rounding decides the winner
    w = int(c["counts"][1])
    centre = v[c["labels"] == w].mean(axis=0)
    assert np.abs(centre - np.array(R.SPHERES[0][0])).max() < 0.2
    nv, nf, src, _ = R.largest_component(v, f)
    assert nv.shape[0] == c["counts"][2] and nf.shape[0] == c["counts"][3] == c["counts"][5]
    assert np.array_equal(nv, v[src]) and np.array_equal(src[nf], f[c["keep_f"]])       # order, winding and the vertex map
    assert M.euler_characteristic(nv, nf) == 2
    # the reported area: within 1e-6 of the float64 area of the winner, and near the sphere's 4 pi r^2
    assert abs(c["area"] - M.area(nv, nf)) <= 1e-6 * M.area(nv, nf)
    assert abs(c["area"] / (4 * np.pi * 7.3 ** 2) - 1) < 0.05


def test_the_shift_keeps_the_sum_below_2_61_at_the_bound():
    """T copies of the largest triangle of a box (two face diagonals at a corner... the doubled area of any triangle is below D2)"""
    for box, T in (((1.0, 1.0, 1.0), 1), ((2.0, 0.5, 3.0), 10_200_000), ((1e-3, 2e-3, 1e-3), 1 << 20), ((3e4, 1e4, 2e4), (1 << 31) - 1),
                   ((1.9999, 1.9999, 1.9999), 255), ((1e19, 1e19, 1e19), 7), ((1e-12, 1e-12, 1e-12), 3)):
        bx, by, bz = box
        v = np.array([[0, 0, 0], [bx, by, 0], [0, by, bz], [bx, 0, bz], [bx, by, bz]], F32)
        k = R.area_shift(v, T)
        assert -60 <= k <= 60
        best = 0
        for tri in ([0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 4, 1], [0, 2, 3]):
            best = max(best, int(R.face_q(v, np.array([tri]), k)[0]))
        assert best * T < 2 ** 61, (box, T, k)
        if abs(k) < 60:
            assert best * T >= 2 ** 56, (box, T, k)                       # ... and not far below: the bits are used
    # no finite vertex, no vertex at all, extents that overflow
    assert R.area_shift(np.full((3, 3), np.nan, F32), 5) == 61 - 3
    assert R.area_shift(np.zeros((0, 3), F32), 0) == 60
    assert R.area_shift(np.array([[3e38, 0, 0], [-3e38, 0, 0]], F32), 1) == -60


def test_shift_of_the_binding_is_the_restatements():
    from dsnerf_amd import _lib
    rng = np.random.default_rng(3)
    for scale, T in ((1.0, 1), (1e-3, 1000), (50.0, 10_200_000), (1e20, 3)):
        v = (rng.standard_normal((50, 3)) * scale).astype(F32)
        v[7] = np.nan
        fin = np.isfinite(v).all(axis=1)
        assert _lib.mesh_area_shift(v[fin].min(axis=0), v[fin].max(axis=0), T) == R.area_shift(v, T)
    assert _lib.mesh_area_shift(None, None, 5) == R.area_shift(np.full((3, 3), np.inf, F32), 5)
    assert _lib.MESH_CC_TILE == R.TILE


def test_sums_do_not_depend_on_the_face_order(meshes):
    v, f = meshes["noise"]
    a = R.components(v, f)
    rng = np.random.default_rng(11)
    for _ in range(3):
        b = R.components(v, f[rng.permutation(f.shape[0])])
        assert a["sums"] == b["sums"] and np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["labels"], b["labels"])


def test_ties_go_to_the_smaller_label(meshes):
    v, f = meshes["spheres"]
    _, _, src, c = R.largest_component(v, f)
    one_v, one_f = v[src], np.searchsorted(src, f[c["keep_f"]])
    n = one_v.shape[0]
    vv = np.concatenate([one_v, one_v])
    for ff in (np.concatenate([one_f, one_f + n]), np.concatenate([one_f + n, one_f])):
        cc = R.components(vv, ff)
        (l0, (s0, n0)), (l1, (s1, n1)) = sorted(cc["sums"].items())
        assert s0 == s1 and n0 == n1 and (l0, l1) == (0, n) and cc["counts"][1] == 0
        assert R.largest_component(vv, ff)[2].tolist() == list(range(n))


def test_bad_input_rules():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.inf, 1, 1], [5, 5, 5], [0, 0, 2], [3, 0, 2], [0, 3, 2]], F32)
    f = np.array([[0, 1, 2], [2, 3, 4], [6, 7, 8], [6, 7, 9], [-1, 0, 1], [0, 0, 1]])
    c = R.components(v, f)
    assert c["labels"].tolist() == [0, 0, 0, 0, 0, -1, 6, 6, 6]
    assert c["counts"][0] == 2 and c["sums"][0][1] == 3 and c["sums"][6][1] == 1
    k = c["area_shift"]
    assert c["sums"][0][0] == int(np.ldexp(1.0, k)) and c["sums"][6][0] == int(np.ldexp(9.0, k))      # NaN / inf faces add 0
    nv, nf, src, _ = R.largest_component(v, f)
    assert src.tolist() == [6, 7, 8] and nf.tolist() == [[0, 1, 2]]
    # no valid face at all, no faces, no vertices
    for vv, ff in ((v, np.array([[0, 1, 9]])), (v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), F32), np.array([[0, 1, 2]]))):
        c = R.components(vv, ff)
        assert c["counts"].tolist() == [0, -1, 0, 0, 0, 0] and (c["labels"] == -1).all()
    # the constructed meshes of the GPU test have the counts they are built for
    T = R.TILE
    for nvk, nfk in ((0, 0), (1, 1), (1, T + 1), (3, 1), (T - 1, T - 3), (T, T - 2), (T + 1, T - 1), (100, T), (100, 3 * T + 77)):
        cc = R.components(*R.mesh_with_counts(nvk, nfk))
        assert cc["counts"][2] == nvk and cc["counts"][3] == nfk, (nvk, nfk, cc["counts"])


def test_abi_argument_errors(lib):
    import dsnerf_amd
    z, one = None, C.c_void_p(64)
    names = ("dsn_mesh_cc_workspace_bytes", "dsn_mesh_cc_label", "dsn_mesh_cc_emit", "dsn_mesh_cc_label_ex", "dsn_mesh_cc_emit_ex")
    for name in names:
        assert hasattr(lib, name) and name in dsnerf_amd._lib.EXPORTS
    assert lib.dsn_abi_version() == 8
    wb = lib.dsn_mesh_cc_workspace_bytes
    assert wb(0, 0) >= 64 and wb(0, 0) % 16 == 0 and wb(100, 200) >= 100 * 25
    assert wb(5_100_000, 10_200_000) < 140e6                                  # the resolution-512 body: 25 bytes a vertex + the tiles
    for bad in ((-1, 0), (0, -1), (1 << 31, 0), (0, 1 << 31)):
        assert wb(*bad) == 0, bad
    prev = 0
    for V, T in ((0, 0), (1, 0), (1, 5000), (1023, 5000), (1025, 5000), (100000, 5000), (100000, 500000)):
        assert wb(V, T) >= prev and wb(V, T) % 16 == 0
        prev = wb(V, T)
    ws = wb(3, 1)

    def label(verts=one, faces=one, nv=3, nf=1, shift=10, w=one, nbytes=ws, lab=one, counts=one):
        return lib.dsn_mesh_cc_label(verts, faces, nv, nf, shift, w, nbytes, lab, counts, z)

    def emit(verts=one, faces=one, nv=3, nf=1, w=one, nbytes=ws, ov=3, of=1, outv=one, outf=one, src=one):
        return lib.dsn_mesh_cc_emit(verts, faces, nv, nf, w, nbytes, ov, of, outv, outf, src, z)

    common = [(dict(verts=z), b"null"), (dict(faces=z), b"null"), (dict(w=z), b"null"), (dict(nv=-1), b"negative"), (dict(nf=-1), b"negative"),
              (dict(nv=1 << 31), b"2^31"), (dict(nf=1 << 31), b"2^31"), (dict(nbytes=ws - 1), b"workspace"), (dict(nbytes=0), b"workspace"),
              (dict(w=C.c_void_p(72)), b"aligned")]
    for kw, msg in common + [(dict(counts=z), b"null"), (dict(shift=61), b"area_shift"), (dict(shift=-61), b"area_shift")]:
        assert label(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_mesh_cc_label" in err and msg in err, (kw, err)
    for kw, msg in common + [(dict(outv=z), b"null output"), (dict(outf=z), b"null output"), (dict(ov=-1), b"negative"), (dict(of=-1), b"negative"),
                             (dict(ov=4), b"more kept"), (dict(of=2), b"more kept")]:
        assert emit(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_mesh_cc_emit" in err and msg in err, (kw, err)
    assert lib.dsn_mesh_cc_label_ex(one, one, 3, 1, 10, one, ws, one, one, 256, z) != 0 and b"phases" in lib.dsn_last_error()
    assert lib.dsn_mesh_cc_emit_ex(one, one, 3, 1, one, ws, 3, 1, one, one, one, -1, z) != 0 and b"phases" in lib.dsn_last_error()
    # nothing to emit: a valid call that touches nothing
    assert emit(ov=0, of=0, outv=z, outf=z, src=z) == 0


def test_connected_switch_still_raises_and_says_where_to_go():
    from dsnerf_amd import visualizer
    vis = visualizer.Visualizer3D(16, 16, 0.5, "ascent", connected=True)
    with pytest.raises(NotImplementedError, match="largest_component"):
        vis.get_mesh_from_grid(np.zeros((4, 4, 4, 3), F32), np.zeros((4, 4, 4, 1), F32))
    assert "largest_component" in visualizer.__doc__ and callable(visualizer.largest_component)
    import inspect
    from dsnerf_amd import Renderer
    assert inspect.signature(Renderer.extract_mesh).parameters["largest_component"].default is False
    assert inspect.signature(visualizer.Visualizer3D.get_mesh_from_grid).parameters["largest_component"].default is False
