"""Marching cubes without a GPU: the case table of dsn_mc_table_host (edges, fans, no cracks, winding), the numpy restatement of the
whole extraction (tests/mc_restate.py) against closed forms, and the argument checks of the mesh entry points."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mc_restate as M


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


@pytest.fixture(scope="module")
def table():
    import dsnerf_amd
    return dsnerf_amd._lib.mc_table()


def tris(table, cs):
    n = table[cs, 0]
    return table[cs, 1:1 + 3 * n].reshape(n, 3)


def crossing_edges(cs):
    out = set()
    for e in range(12):
        a, b = M.edge_corners(e)
        if ((cs >> a) & 1) != ((cs >> b) & 1):
            out.add(e)
    return out


def test_table_shape(table):
    assert table.shape == (256, 16)
    assert table[0, 0] == 0 and table[255, 0] == 0
    assert (table[:, 0] <= 5).all()
    for cs in range(256):
        n = table[cs, 0]
        assert (table[cs, 1 + 3 * n:] == -1).all()


def test_every_case_uses_exactly_its_crossing_edges(table):
    for cs in range(256):
        used = set(tris(table, cs).reshape(-1).tolist())
        assert used == crossing_edges(cs), cs


def test_fans_boundary_once_diagonals_twice(table):
    """within a cell each boundary edge of a fan (two consecutive loop vertices) is used once, each fan diagonal twice - in opposite
    directions - and no directed edge twice"""
    for cs in range(256):
        t = tris(table, cs)
        if t.size == 0:
            continue
        directed = [(int(a), int(b)) for tri in t for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))]
        assert len(set(directed)) == len(directed), cs
        und = {}
        for a, b in directed:
            und.setdefault(frozenset((a, b)), []).append((a, b))
        for key, uses in und.items():
            assert len(uses) in (1, 2), (cs, key)
            if len(uses) == 2:
                assert uses[0] == uses[1][::-1], (cs, key)
        # boundary edges (used once) form the loops: every crossing edge has one boundary edge in and one out
        bnd = [u[0] for u in und.values() if len(u) == 1]
        outs = sorted(a for a, _ in bnd)
        ins = sorted(b for _, b in bnd)
        assert outs == sorted(crossing_edges(cs)) == ins, cs


def face_segments(table, cs, axis, side):
    """the undirected boundary segments of the case's loops that lie on cube face (axis, side)"""
    t = tris(table, cs)
    directed = [(int(a), int(b)) for tri in t for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))]
    und = {}
    for a, b in directed:
        und[frozenset((a, b))] = und.get(frozenset((a, b)), 0) + 1
    on_face = lambda e: all(((c >> axis) & 1) == side for c in M.edge_corners(e))
    return {k for k, v in und.items() if v == 1 and all(on_face(e) for e in k)}


def test_no_cracks_between_cells(table):
    """two cases that agree on a face's four corners cut the same segments on it - so the two cells sharing the face do too (the
    neighbour sees the face as its opposite side: the segments must map onto each other's edges)"""
    for axis in range(3):
        face_c = [c for c in range(8) if not (c >> axis) & 1]
        opp = lambda c: c | (1 << axis)

        def mapped_edge(e):        # edge of face (axis, 1) of this cell -> the same grid edge on face (axis, 0) of the neighbour cell
            a, b = M.edge_corners(e)
            a2, b2 = a & ~(1 << axis), b & ~(1 << axis)
            return next(f for f in range(12) if set(M.edge_corners(f)) == {a2, b2})

        for bits in range(16):
            ref = None
            for rest in range(16):
                # this cell's face (axis, 1) has the corner values `bits`; the neighbour's face (axis, 0) the same values
                cs_hi = 0
                cs_lo = 0
                others = [c for c in range(8) if not (c >> axis) & 1]
                for m, c in enumerate(face_c):
                    if (bits >> m) & 1:
                        cs_hi |= 1 << opp(c)
                        cs_lo |= 1 << c
                for m, c in enumerate(others):
                    if (rest >> m) & 1:
                        cs_hi |= 1 << c
                        cs_lo |= 1 << opp(c)
                seg_hi = {frozenset(mapped_edge(e) for e in s) for s in face_segments(table, cs_hi, axis, 1)}
                seg_lo = face_segments(table, cs_lo, axis, 0)
                assert seg_hi == seg_lo, (axis, bits, rest)
                if ref is None:
                    ref = seg_lo
                assert seg_lo == ref, (axis, bits, rest)


def test_descent_normals_point_out_of_the_object(table):
    """with midpoint vertices, each loop's normal (its fan's summed (v1 - v0) x (v2 - v0): the loop's vector area, whatever the fan)
    points from inside to outside: along the sum of (outside corner - inside corner) over the loop's edges.  (A single fan triangle of
    a non-planar loop can lean the other way; the loop cannot.)  Loops are the runs of triangles with one apex: each loop is fanned
    from its lowest edge and loops have different lowest edges."""
    mid = lambda e: sum(M.corner_xyz(c) for c in M.edge_corners(e)) / 2.0
    for cs in range(1, 255):
        t = tris(table, cs)
        for apex in np.unique(t[:, 0]):
            loop = t[t[:, 0] == apex]
            A = sum(np.cross(mid(b) - mid(a), mid(c) - mid(a)) for a, b, c in loop)
            G = 0
            for e in set(loop.reshape(-1).tolist()):
                a, b = M.edge_corners(e)
                cin, cout = (a, b) if (cs >> a) & 1 else (b, a)
                G = G + (M.corner_xyz(cout) - M.corner_xyz(cin))
            assert np.dot(A, G) > 0, (cs, loop)


def axes_for(n, lo=-1.0, hi=1.0):
    a = np.linspace(lo, hi, n).astype(np.float32)
    return a, a, a


def sdf_grid(axes, fn):
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in axes], indexing="ij")
    return fn(X, Y, Z).astype(np.float32)


def check_closed(verts, faces):
    n, dup, unpaired = M.directed_edge_counts(faces)
    assert n > 0 and dup == 0 and unpaired == 0        # every directed edge once, and its reverse present: closed, oriented
    assert np.unique(faces).size == verts.shape[0]      # every vertex is used


def test_sphere_is_a_closed_manifold(table):
    ax = axes_for(40)
    vol = sdf_grid(ax, lambda x, y, z: 0.7 - np.sqrt(x * x + y * y + z * z))
    v, f = M.marching_cubes(vol, ax, 0.0, "descent", table)
    check_closed(v, f)
    assert M.euler_characteristic(v, f) == 2
    # descent: normals point out of the object (values above the level) = away from the centre
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3) > 0).mean() > 0.99


def test_torus_and_two_spheres(table):
    ax = axes_for(48)
    torus = sdf_grid(ax, lambda x, y, z: 0.25 - np.sqrt((np.sqrt(x * x + y * y) - 0.6) ** 2 + z * z))
    v, f = M.marching_cubes(torus, ax, 0.0, "ascent", table)
    check_closed(v, f)
    assert M.euler_characteristic(v, f) == 0
    two = sdf_grid(ax, lambda x, y, z: np.maximum(0.3 - np.sqrt((x - 0.5) ** 2 + y * y + z * z), 0.3 - np.sqrt((x + 0.5) ** 2 + y * y + z * z)))
    v, f = M.marching_cubes(two, ax, 0.0, "descent", table)
    check_closed(v, f)
    assert M.euler_characteristic(v, f) == 4


def test_sphere_area_converges(table):
    r = 0.6
    errs = []
    for n in (24, 48, 96):
        ax = axes_for(n)
        v, f = M.marching_cubes(sdf_grid(ax, lambda x, y, z: r - np.sqrt(x * x + y * y + z * z)), ax, 0.0, "descent", table)
        errs.append(abs(M.area(v, f) / (4 * np.pi * r * r) - 1))
    assert errs[2] < errs[1] < errs[0] and errs[2] < 0.01, errs


def test_noise_volume_is_closed_away_from_the_border(table):
    """seeded noise (many ambiguous faces) inside a border of outside values: no boundary - every directed edge has its reverse.
    (Not a 2-manifold: where two cells fan a loop across the same ambiguous face, their fan diagonals lie in that face and touch.)"""
    rng = np.random.default_rng(5)
    vol = rng.standard_normal((12, 13, 11)).astype(np.float32)
    vol[[0, -1]] = -1
    vol[:, [0, -1]] = -1
    vol[:, :, [0, -1]] = -1
    ax = [np.arange(s, dtype=np.float32) for s in vol.shape]
    v, f = M.marching_cubes(vol, ax, 0.0, "descent", table)
    n, dup, unpaired = M.directed_edge_counts(f)
    assert n > 3000 and unpaired == 0
    assert np.unique(f).size == v.shape[0]


def test_abi_argument_errors(lib):
    z, i64 = None, C.c_int64
    one = C.c_void_p(1)
    calls = {
        "dsn_density_grid": lambda: lib.dsn_density_grid(z, 1, 1, z, z, 2, z, 2, z, 2, 0, z, 8, z, 0, z),
        "dsn_mc_count": lambda: lib.dsn_mc_count(z, 2, 2, 2, 0.0, z, z, z),
        "dsn_mc_emit": lambda: lib.dsn_mc_emit(z, 2, 2, 2, z, z, z, 0.0, 0, z, 0, 0, z, z, z),
        "dsn_mc_table_host": lambda: lib.dsn_mc_table_host(z, 0),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert name.encode() in lib.dsn_last_error(), (name, lib.dsn_last_error())
    # bad sizes and arguments, before any device work
    assert lib.dsn_mc_workspace_bytes(1, 2, 2) == 0 and lib.dsn_mc_workspace_bytes(2, 2, 2) > 0
    assert lib.dsn_density_grid_workspace_bytes(0) == 0 and lib.dsn_density_grid_workspace_bytes(1 << 20) >= 28 * (1 << 20)
    for nx, ny, nz in ((2, 2, 2), (17, 33, 65), (1251, 1395, 512)):
        assert lib.dsn_mc_workspace_bytes(nx, ny, nz) <= 8 * nx * ny * nz
    assert lib.dsn_mc_workspace_bytes(2048, 1024, 1024) == 0                     # 2^31 points
    assert lib.dsn_mc_count(one, 1, 2, 2, 0.0, one, one, z) != 0 and b"grid size" in lib.dsn_last_error()
    assert lib.dsn_mc_count(one, 2, 2, 2, float("nan"), one, one, z) != 0 and b"NaN" in lib.dsn_last_error()
    assert lib.dsn_mc_emit(one, 2, 2, 2, one, one, one, 0.0, 2, one, 1, 1, one, one, z) != 0 and b"gradient_direction" in lib.dsn_last_error()
    assert lib.dsn_mc_emit(one, 2, 2, 2, one, one, one, 0.0, 0, one, 1 << 31, 1, one, one, z) != 0 and b"2^31" in lib.dsn_last_error()
    assert lib.dsn_mc_emit(one, 2, 2, 2, one, one, one, 0.0, 0, one, 3, 1, z, one, z) != 0 and b"null output" in lib.dsn_last_error()
    ws = lib.dsn_density_grid_workspace_bytes(i64(64))
    assert lib.dsn_density_grid(one, 1, 1, one, one, 4, one, 4, one, 8, 0, one, 16, one, ws, z) != 0 and b"x-plane" in lib.dsn_last_error()
    assert lib.dsn_density_grid(one, 1, 1, one, one, 4, one, 4, one, 4, 0, one, 64, one, 16, z) != 0 and b"workspace" in lib.dsn_last_error()
    assert lib.dsn_density_grid(one, 1, 1, one, one, 4, one, 4, one, 4, 1, one, 64, one, ws, z) != 0 and b"flags" in lib.dsn_last_error()
    assert lib.dsn_density_grid(one, 1, 1, one, one, 2048, one, 1024, one, 1024, 0, one, 1 << 30, one, ws, z) != 0
    assert b"2^31" in lib.dsn_last_error()
    assert lib.dsn_density_grid(one, 1, 1, one, one, 0, one, 4, one, 4, 0, one, 64, one, ws, z) != 0 and b"empty" in lib.dsn_last_error()
    buf = np.zeros(16, dtype=np.int32)
    assert lib.dsn_mc_table_host(buf.ctypes.data, buf.size) != 0 and b"fewer than" in lib.dsn_last_error()


def test_all_cases_restated_on_2x2x2(table):
    """each of the 256 cases alone on a 2 x 2 x 2 grid: vertices on exactly its crossing edges, faces = its table row"""
    ax = (np.array([0, 1], np.float32),) * 3
    for cs in range(256):
        vol = np.array([1.0 if (cs >> c) & 1 else -1.0 for c in range(8)], np.float32)
        vol = vol.reshape(2, 2, 2, order="F")          # corner c = dx + 2 dy + 4 dz -> vol[dx, dy, dz]
        v, f = M.marching_cubes(vol, ax, 0.0, "descent", table)
        assert v.shape[0] == len(crossing_edges(cs)) and f.shape[0] == table[cs, 0]
        assert np.allclose(np.sort(v, axis=0), np.sort(v, axis=0))        # (finite)
        assert np.isfinite(v).all() and (v >= 0).all() and (v <= 1).all()
