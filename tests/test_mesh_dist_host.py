"""The numpy restatement of the mesh-distance rules (tests/mesh_dist_restate.py) against float64 closed forms, on the CPU, and the
argument checks of the new entry points through the library (they return before any device work).

The bound between the float32 rule and a float64 closed form, used throughout (BOUND below).  With eps = 2^-24, S = the largest absolute
coordinate of the triangle and d the distance: the inputs are float32 numbers, so both sides start from the same values.  The rule's
closest point is a + v ab + w ac with weights in [0, 1]: differences (1 rounding, values up to 2 S), two products (up to 2 S) and two sums
(up to 5 S) per axis - under 7 eps S per axis, 12.2 eps S over three axes - plus what the roundings of the weights move it: the weights come
from dot products whose relative error is a few eps each, and the point moves by (error of the weight) x (edge length) - another few eps S
for a well-shaped triangle and a point within a few S.  p - q and the dot product add 4 eps d.  BOUND = 32 eps max(S, |p|, d) on the
DISTANCE covers this about twice; the tests use triangles with angles of 30 degrees and more and points within 10 S."""
import ctypes as C

import numpy as np
import pytest

import mesh_dist_restate as R

F32 = np.float32
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


def bound(verts, points, d):
    return 32.0 * EPS * max(float(np.abs(verts).max()), float(np.abs(points).max()), float(np.max(d)))


def seg_dist(p, a, b):
    ab = b - a
    L = float(ab @ ab)
    t = 0.0 if L == 0.0 else min(1.0, max(0.0, float((p - a) @ ab) / L))
    return float(np.linalg.norm(p - (a + t * ab)))


def tri_dist(p, a, b, c):
    """float64 closed form, written differently from the rule: the foot of the perpendicular if it lies inside, else the nearest edge"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    n = np.cross(b - a, c - a)
    nn = float(n @ n)
    best = min(seg_dist(p, a, b), seg_dist(p, b, c), seg_dist(p, c, a))
    if nn > 0.0:
        foot = p - n * (float((p - a) @ n) / nn)
        inside = all(float(np.cross(v - u, foot - u) @ n) >= 0.0 for u, v in ((a, b), (b, c), (c, a)))
        if inside:
            best = min(best, abs(float((p - a) @ n)) / nn ** 0.5)
    return best


def mesh_dist(points, verts, faces):
    return np.array([min(tri_dist(p, *verts[f].astype(np.float64)) for f in faces) for p in np.asarray(points, np.float64)])


def test_one_triangle_seven_regions():
    a, b, c = np.array([[0, 0, 0]], F32), np.array([[2, 0, 0]], F32), np.array([[0, 2, 0]], F32)
    cases = [((-1, -1, 0.5), 1, (0, 0, 0)), ((3, -0.5, 0), 2, (2, 0, 0)), ((1, -1, 0), 3, (1, 0, 0)), ((-0.5, 3, 0), 4, (0, 2, 0)),
             ((-1, 1, 0), 5, (0, 1, 0)), ((2, 2, 0), 6, (1, 1, 0)), ((0.5, 0.5, 3), 7, (0.5, 0.5, 0)),
             ((1, 0, 0), None, (1, 0, 0)), ((2, 0, 0), None, (2, 0, 0)), ((0.25, 0.25, 0), None, (0.25, 0.25, 0)), ((1, 1, 0), None, (1, 1, 0))]
    pts = np.array([k[0] for k in cases], F32)
    d2, q, region = R.closest_on_triangles(pts, a, b, c)
    assert d2.dtype == F32 and q.dtype == F32
    for k, (p, reg, want) in enumerate(cases):
        if reg is not None:
            assert region[k, 0] == reg, (p, region[k, 0], reg)
        exact = tri_dist(p, a[0], b[0], c[0])
        assert abs(np.sqrt(float(d2[k, 0])) - exact) <= bound(np.stack([a, b, c]), pts, exact), (p, d2[k, 0], exact)
        assert np.abs(q[k, 0].astype(np.float64) - np.array(want)).max() <= bound(np.stack([a, b, c]), pts, exact), (p, q[k, 0])
    assert (d2[7:, 0] == 0).all()                          # on an edge, on a vertex, in the plane inside, on the long edge: exactly 0


def test_random_triangles_against_float64():
    rng = np.random.default_rng(3)
    worst = 0.0
    for trial in range(40):
        scale = 10.0 ** rng.integers(-2, 3)
        while True:
            tri = ((rng.random((3, 3)) - 0.5) * 2 * scale).astype(F32)
            e = [tri[(k + 1) % 3] - tri[k] for k in range(3)]
            cosines = [abs(float(e[k] @ e[(k + 1) % 3]) / (np.linalg.norm(e[k]) * np.linalg.norm(e[(k + 1) % 3]))) for k in range(3)]
            if max(cosines) < np.cos(np.pi / 6):           # every angle between 30 and 150 degrees
                break
        pts = ((rng.random((200, 3)) - 0.5) * 6 * scale).astype(F32)
        d2, _, region = R.closest_on_triangles(pts, tri[None, 0], tri[None, 1], tri[None, 2])
        exact = np.array([tri_dist(p, *tri) for p in pts])
        err = np.abs(np.sqrt(d2[:, 0].astype(np.float64)) - exact)
        b = bound(tri, pts, exact)
        worst = max(worst, float(err.max() / b))
        assert (err <= b).all(), (trial, err.max(), b)
        assert len(set(region[:, 0].tolist())) >= 5        # the points reach most regions
    print("worst error / bound", worst)


def test_zero_area_triangles():
    pts = np.array([(-1, 0.5, 0), (0.5, 1, 0), (1, 0, 0), (1.5, -2, 1), (3, 1, 0), (2, 0, 0), (0, 0, 0), (1.25, 0, 0.5)], F32)
    seg = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F32)
    import itertools
    for order in itertools.product(range(3), repeat=3):    # every way three corners land on the points of a segment (27: segments and points)
        tri = seg[list(order)]
        d2, q, region = R.closest_on_triangles(pts, tri[None, 0], tri[None, 1], tri[None, 2])
        lo, hi = tri[:, 0].min(), tri[:, 0].max()
        want = np.array([seg_dist(p.astype(np.float64), np.array([lo, 0, 0.0]), np.array([hi, 0, 0.0])) for p in pts])
        assert np.isfinite(d2).all() and (region[:, 0] <= 6).all(), (order, region[:, 0])
        assert (np.abs(np.sqrt(d2[:, 0].astype(np.float64)) - want) <= bound(tri, pts, want)).all(), (order, d2[:, 0], want)
    # the same through brute_force: zero-area faces are valid faces
    faces = np.array([[0, 0, 0], [0, 1, 1], [2, 1, 0]], np.int32)
    d2, face, _ = R.brute_force(seg, faces, np.array([(-1, 0, 0), (1.5, 1, 0)], F32))
    assert face.tolist() == [0, 2] and d2.tolist() == [1.0, 1.0]       # (-1, 0, 0) is 1 from all three: the lowest index


def test_unit_cube():
    v, f = R.cube_mesh()
    pts = np.array([(0.5, 0.5, 0.5), (2, 0.5, 0.5), (2, 2, 2), (0.5, 0.5, -3), (0.25, 0.5, 0.75), (-1, -1, 0.5), (0.5, 0.5, 1.0)], F32)
    want = np.array([0.5, 1.0, 3 ** 0.5, 3.0, 0.25, 2 ** 0.5, 0.0])
    d2, face, q = R.brute_force(v, f, pts)
    assert (np.abs(np.sqrt(d2.astype(np.float64)) - want) <= bound(v, pts, want)).all(), (d2, want)
    assert (np.abs(mesh_dist(pts, v, f) - want) < 1e-12).all()
    assert face[0] == 0                                    # the centre is 0.5 from all six sides: the lowest face index
    assert np.array_equal(q[2], np.array([1, 1, 1], F32)) and face[3] in (8, 9)      # the z = 0 side


def test_icosphere_against_the_sphere():
    v, f = R.icosphere(1)
    assert f.shape[0] == 80
    tri = v[f].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    inradius = float(np.min(np.abs((tri[:, 0] * n).sum(axis=1)) / np.linalg.norm(n, axis=1)))
    assert 0.8 < inradius < 1.0
    rng = np.random.default_rng(11)
    for r in (0.25, 0.9, 1.0, 1.5, 3.0):
        d = rng.normal(size=(40, 3))
        pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * r).astype(F32)
        rr = np.linalg.norm(pts.astype(np.float64), axis=1)
        d2, face, _ = R.brute_force(v, f, pts)
        dist = np.sqrt(d2.astype(np.float64))
        tol = bound(v, pts, dist)
        if r > 1.0:
            assert (dist >= rr - 1.0 - tol).all() and (dist <= rr - inradius + tol).all()
        elif r < inradius:
            assert (dist >= inradius - rr - tol).all() and (dist <= 1.0 - rr + tol).all()
        else:
            assert (dist <= 1.0 - inradius + tol).all()
        assert (np.abs(dist - mesh_dist(pts, v, f)) <= tol).all() and (face >= 0).all()


def test_tie_goes_to_the_lowest_face_index():
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0]], F32)
    f = np.array([[0, 1, 2], [0, 3, 1]], np.int32)         # coplanar, sharing the edge on the x axis
    pts = np.array([(0.5, 0, 1), (0.25, 0, 2), (0.75, 0, -0.5)], F32)      # on the perpendicular through the shared edge
    for faces in (f, f[::-1]):
        d2, face, q = R.brute_force(v, faces, pts)
        assert d2.tolist() == [1.0, 4.0, 0.25] and face.tolist() == [0, 0, 0]
        assert np.array_equal(q, pts * np.array([1, 1, 0], F32))
    # duplicated faces: the first copy
    d2, face, _ = R.brute_force(v, np.concatenate([f[1:], f, f]), np.array([(0.5, 0.5, 1), (0.5, -0.5, 1)], F32))
    assert face.tolist() == [1, 0]
    # invalid faces take no part; a point that is not finite; a mesh without a valid face
    vb = np.concatenate([v, np.array([[np.nan, 0, 0], [np.inf, 0, 0]], F32)])
    fb = np.array([[0, 1, 4], [0, 1, 9], [-1, 0, 1], [5, 0, 1], [0, 1, 2]], np.int32)
    d2, face, q = R.brute_force(vb, fb, np.array([(0.5, 0.5, 1), (np.nan, 0, 0), (0, np.inf, 0)], F32))
    assert face.tolist() == [4, -1, -1] and d2[0] == 1.0 and np.isnan(d2[1:]).all() and np.isnan(q[1:]).all()
    d2, face, q = R.brute_force(vb, fb[:4], np.zeros((1, 3), F32))
    assert np.isposinf(d2[0]) and face[0] == -1 and np.isnan(q).all()


def test_grid_model_returns_the_brute_force_answer():
    """the search the header describes, with its margin, against the rule - on the CPU, before any kernel is involved"""
    rng = np.random.default_rng(21)
    for T, spread in ((1, 1.0), (40, 1.0), (300, 0.02)):
        v = (rng.random((3 * T, 3)) * np.array([1.0, 0.6, 0.3])).astype(F32)
        v = (v.reshape(T, 3, 3)[:, :1] + (v.reshape(T, 3, 3) - 0.5) * spread).reshape(-1, 3).astype(F32)
        f = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
        if T == 300:
            v[:3] = np.array([[-0.1, -0.1, -0.1], [1.2, 0.0, 0.5], [0.0, 0.8, 0.5]], F32)        # one face across the whole box
        m = R.GridModel(v, f)
        pts = np.concatenate([(rng.random((12, 3)) * 1.4 - 0.2), rng.random((3, 3)) * 20 - 10, v[::max(1, 3 * T // 4)][:4]]).astype(F32)
        d2, face, q = R.brute_force(v, f, pts)
        for k, p in enumerate(pts):
            gd, gf, gq, _ = m.query(p)
            assert F32(gd).view(np.uint32) == d2[k].view(np.uint32) and gf == face[k] and np.array_equal(gq.view(np.uint32), q[k].view(np.uint32))
        assert m.pairs[m.level] <= R.entries_cap(T) and int(np.prod(m.g)) <= R.cells_cap(T)


def test_the_margin_case_needs_the_margin():
    mc = R.margin_case()
    m, p = mc["model"], mc["point"]
    d2, face, q = R.brute_force(mc["verts"], mc["faces"], p[None])
    assert face[0] == mc["far_face"]                       # the rule picks the face in the farther shell ...
    tri = mc["verts"][mc["faces"][mc["near_face"]]]
    dn, _, _ = R.closest_on_triangles(p[None], tri[None, 0], tri[None, 1], tri[None, 2])
    steps = int(dn[0, 0].view(np.uint32)) - int(d2[0].view(np.uint32))
    assert 1 <= steps <= 16, steps                         # ... by a few float32 steps of the squared distance
    gd, gf, _, shells = m.query(p, margin=True)
    assert gf == mc["far_face"] and shells == 2 and F32(gd).view(np.uint32) == d2[0].view(np.uint32)
    nd, nf, _, nshells = m.query(p, margin=False)
    assert nf == mc["near_face"] and nshells == 1          # the bare bound stops one shell early and returns the wrong face


def test_grid_rule_matches_the_library(lib):
    lib.dsn_mesh_dist_grid_host.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(2)
    boxes = [((0, 0, 0), (1, 1, 1)), ((0, 0, 0), (0, 0, 0)), ((-1, 2, 3), (5, 2, 3.5)), ((0.1, 0.1, 0.1), (1.3, 1.3, 1.3)), ((0, 0, 0), (1, 1e-30, 0))]
    boxes += [tuple(np.sort(rng.normal(size=(2, 3)) * 10.0 ** rng.integers(-3, 4), axis=0)) for _ in range(20)]
    for lo, hi in boxes:
        for T in (1, 12, 200, 5000, 10 ** 7, 2 ** 31 - 1):
            b = np.concatenate([np.asarray(lo, F32), np.asarray(hi, F32)])
            g, cell = np.zeros(3, np.int32), np.zeros(1, F32)
            assert lib.dsn_mesh_dist_grid_host(T, b.ctypes.data, g.ctypes.data, cell.ctypes.data) == 0
            rg, rc = R.grid_rule(T, (b[:3], b[3:]))
            assert g.tolist() == rg.tolist() and cell[0].view(np.uint32) == F32(rc).view(np.uint32), (lo, hi, T, g, rg, cell, rc)
            assert int(np.prod(rg)) <= R.cells_cap(T) and rg.max() <= R.MAX_G


def test_reduction_restatement():
    rng = np.random.default_rng(4)
    for n in (0, 1, 255, 256, 257, 1023, 1025, 70001):
        x = (rng.random(n) ** 2).astype(F32)
        if n > 10:
            x[rng.integers(0, n, 5)] = np.nan
            x[[3, 7]] = x[np.nanargmax(x)] = F32(2.0)      # the maximum three times: the lowest index
        s = R.reduce_stats(x)
        ok = ~np.isnan(x)
        assert s[0] == ok.sum() and s[1] == (~ok).sum()
        d = np.sqrt(x[ok].astype(np.float64))
        # float64 sums of n positive terms: any order agrees within n eps64 relative
        assert abs(s[2] - d.sum()) <= n * 2.0 ** -52 * max(d.sum(), 1.0) and abs(s[3] - (d * d).sum()) <= n * 2.0 ** -52 * max((d * d).sum(), 1.0)
        if ok.any():
            assert s[4] == d.max() and s[5] == np.nonzero(ok & (x == x[ok].max()))[0][0]
            if n > 10:
                assert s[5] == min(3, int(np.nonzero(x == F32(2.0))[0][0]))
        else:
            assert s[4] == 0.0 and s[5] == -1.0


def test_sampler_restatement():
    # the prefix: monotone, close to a plain cumulative sum, the last entry is the total; two groups of tiles
    v, f = R.icosphere(3)
    assert f.shape[0] == 1280
    f = f.copy()
    f[5] = [0, 0, 1]                                       # a zero-area face and an invalid one: never drawn
    f[40] = [0, 1, 10 ** 6]
    area = R.face_areas(v, f)
    cum = R.surface_cum(v, f)
    assert area[5] == 0.0 and area[40] == 0.0 and (np.diff(cum) >= 0).all()
    assert np.abs(cum - np.cumsum(area)).max() <= 1280 * 2.0 ** -52 * cum[-1]
    pts, face = R.sample_surface(v, f, 3000, seed=9)
    assert pts.dtype == F32 and face.dtype == np.int32 and (face >= 0).all() and (face < 1280).all()
    assert 5 not in face and 40 not in face and len(set(face.tolist())) > 1000
    # a sample lies in its face: in the plane and inside, within float32 error.  The point is a + u ab + v ac in float32: under 7 eps S per
    # axis as in the module docstring (no weights to round: u and v are exact), so 16 eps S bounds the distance to the triangle.
    tri = v[f[face]].astype(np.float64)
    dist = np.array([tri_dist(p, *t) for p, t in zip(pts[:400].astype(np.float64), tri[:400])])
    assert dist.max() <= 16 * EPS * 1.0, dist.max()
    # sample i depends on (seed, i) only; another seed gives other points
    p64, f64 = R.sample_surface(v, f, 64, seed=9)
    assert np.array_equal(p64.view(np.uint32), pts[:64].view(np.uint32)) and np.array_equal(f64, face[:64])
    assert not np.array_equal(R.sample_surface(v, f, 64, seed=10)[1], f64)
    # two triangles with areas 1 : 3.  n = 4000 draws, p = 1/4: the count of the small face is binomial with mean 1000 and standard
    # deviation sqrt(4000 x 1/4 x 3/4) = 27.4; five standard deviations (137) are passed with probability 6e-7 per seed.
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [10, 0, 0], [11.5, 0, 0], [10, 0, 4]], F32)      # areas 1 and 1/2 x 1.5 x 4 = 3
    f2 = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    assert R.face_areas(v2, f2).tolist() == [1.0, 3.0]
    for seed in (0, 1, 2):
        _, face = R.sample_surface(v2, f2, 4000, seed=seed)
        assert abs(int((face == 0).sum()) - 1000) <= 137, (seed, int((face == 0).sum()))
    # a mesh without area
    pts, face = R.sample_surface(v2, np.array([[0, 0, 1]], np.int32), 5)
    assert np.isnan(pts).all() and (face == -1).all()


def test_argument_checks(lib):
    """null pointers, negative counts, sizes of 2^31, an empty target, a bad box: every entry point returns non-zero with its name in the
    message, before any device work (no GPU needed); the workspace sizes are functions of the counts alone"""
    i64, sz, vp = C.c_int64, C.c_size_t, C.c_void_p
    lib.dsn_mesh_dist_workspace_bytes.restype = lib.dsn_mesh_dist_reduce_workspace_bytes.restype = lib.dsn_mesh_sample_workspace_bytes.restype = sz
    lib.dsn_mesh_dist_workspace_bytes.argtypes = [i64, i64]
    lib.dsn_mesh_dist_reduce_workspace_bytes.argtypes = [i64]
    lib.dsn_mesh_sample_workspace_bytes.argtypes = [i64]
    lib.dsn_mesh_dist_build.argtypes = [vp, vp, i64, i64, vp, vp, sz, vp, vp]
    lib.dsn_mesh_dist_query.argtypes = [vp, vp, i64, i64, vp, sz, vp, i64, vp, vp, vp, vp]
    lib.dsn_mesh_dist_reduce.argtypes = [vp, i64, vp, sz, vp, vp]
    lib.dsn_mesh_sample_surface.argtypes = [vp, vp, i64, i64, C.c_uint64, i64, vp, sz, vp, vp, vp]
    lib.dsn_mesh_dist_grid_host.argtypes = [i64, vp, vp, vp]
    W = lib.dsn_mesh_dist_workspace_bytes
    assert W(8, 12) > 0 and W(8, 12) == W(10 ** 6, 12) and W(8, 12) % 16 == 0 and W(8, 13) >= W(8, 12)
    assert W(8, 0) == 0 and W(-1, 12) == 0 and W(8, -1) == 0 and W(2 ** 31, 12) == 0 and W(8, 2 ** 31) == 0
    assert W(8, 10 ** 7) < 1 << 30                         # 10 M faces: under 1 GiB
    assert lib.dsn_mesh_dist_reduce_workspace_bytes(0) > 0 and lib.dsn_mesh_dist_reduce_workspace_bytes(-1) == 0
    assert lib.dsn_mesh_dist_reduce_workspace_bytes(2 ** 31) == 0 and lib.dsn_mesh_sample_workspace_bytes(0) == 0
    assert lib.dsn_mesh_sample_workspace_bytes(100) >= 800 and lib.dsn_mesh_sample_workspace_bytes(2 ** 31) == 0

    def fails(rc, name, word):
        msg = lib.dsn_last_error().decode()
        assert rc != 0 and name in msg and word in msg, (rc, msg)
    buf = np.zeros(64, np.float64)                         # stands in for device pointers: every call below is rejected before it is read
    p, box, bad_box = buf.ctypes.data, np.array([0, 0, 0, 1, 1, 1], F32), np.array([0, 0, 0, 1, np.nan, 1], F32)
    big = 1 << 20
    fails(lib.dsn_mesh_dist_build(None, None, 0, 0, None, None, 0, None, None), "dsn_mesh_dist_build", "empty")
    fails(lib.dsn_mesh_dist_build(p, p, 8, 0, box.ctypes.data, p, big, None, None), "dsn_mesh_dist_build", "empty")
    fails(lib.dsn_mesh_dist_build(p, p, -1, 12, box.ctypes.data, p, big, None, None), "dsn_mesh_dist_build", "negative")
    fails(lib.dsn_mesh_dist_build(p, p, 2 ** 31, 12, box.ctypes.data, p, big, None, None), "dsn_mesh_dist_build", "2^31")
    fails(lib.dsn_mesh_dist_build(None, p, 8, 12, box.ctypes.data, p, big, None, None), "dsn_mesh_dist_build", "null")
    fails(lib.dsn_mesh_dist_build(p, None, 8, 12, box.ctypes.data, p, big, None, None), "dsn_mesh_dist_build", "null")
    fails(lib.dsn_mesh_dist_build(p, p, 8, 12, None, p, big, None, None), "dsn_mesh_dist_build", "null")
    fails(lib.dsn_mesh_dist_build(p, p, 8, 12, box.ctypes.data, None, big, None, None), "dsn_mesh_dist_build", "null")
    fails(lib.dsn_mesh_dist_build(p, p, 8, 12, bad_box.ctypes.data, p, big, None, None), "dsn_mesh_dist_build", "box")
    fails(lib.dsn_mesh_dist_build(p, p, 8, 12, box[[3, 1, 2, 0, 4, 5]].copy().ctypes.data, p, big, None, None), "dsn_mesh_dist_build", "box")
    fails(lib.dsn_mesh_dist_build(p, p, 8, 12, box.ctypes.data, p, W(8, 12) - 1, None, None), "dsn_mesh_dist_build", "too small")
    fails(lib.dsn_mesh_dist_build(p, p, 8, 12, box.ctypes.data, p + 4, big, None, None), "dsn_mesh_dist_build", "aligned")
    fails(lib.dsn_mesh_dist_query(None, None, 0, 0, None, 0, None, 0, None, None, None, None), "dsn_mesh_dist_query", "empty")
    fails(lib.dsn_mesh_dist_query(p, p, 8, 12, p, big, p, -1, None, None, None, None), "dsn_mesh_dist_query", "negative")
    fails(lib.dsn_mesh_dist_query(p, p, 8, 12, p, big, p, 2 ** 31, None, None, None, None), "dsn_mesh_dist_query", "2^31")
    fails(lib.dsn_mesh_dist_query(p, p, 8, 12, None, big, p, 4, None, None, None, None), "dsn_mesh_dist_query", "null")
    fails(lib.dsn_mesh_dist_query(p, p, 8, 12, p, big, None, 4, None, None, None, None), "dsn_mesh_dist_query", "null points")
    fails(lib.dsn_mesh_dist_query(p, p, 8, 12, p, 16, p, 4, None, None, None, None), "dsn_mesh_dist_query", "too small")
    fails(lib.dsn_mesh_dist_reduce(None, 4, p, big, p, None), "dsn_mesh_dist_reduce", "null")
    fails(lib.dsn_mesh_dist_reduce(p, 4, None, big, p, None), "dsn_mesh_dist_reduce", "null")
    fails(lib.dsn_mesh_dist_reduce(p, 4, p, big, None, None), "dsn_mesh_dist_reduce", "null")
    fails(lib.dsn_mesh_dist_reduce(p, -4, p, big, p, None), "dsn_mesh_dist_reduce", "negative")
    fails(lib.dsn_mesh_dist_reduce(p, 2 ** 31, p, big, p, None), "dsn_mesh_dist_reduce", "2^31")
    fails(lib.dsn_mesh_dist_reduce(p, 5000, p, 16, p, None), "dsn_mesh_dist_reduce", "too small")
    fails(lib.dsn_mesh_sample_surface(None, None, 0, 0, 0, 0, None, 0, None, None, None), "dsn_mesh_sample_surface", "empty")
    fails(lib.dsn_mesh_sample_surface(p, p, 8, 12, 0, -1, p, big, None, None, None), "dsn_mesh_sample_surface", "negative")
    fails(lib.dsn_mesh_sample_surface(p, p, 8, 12, 0, 2 ** 31, p, big, None, None, None), "dsn_mesh_sample_surface", "2^31")
    fails(lib.dsn_mesh_sample_surface(None, p, 8, 12, 0, 4, p, big, None, None, None), "dsn_mesh_sample_surface", "null")
    fails(lib.dsn_mesh_sample_surface(p, p, 8, 12, 0, 4, None, big, None, None, None), "dsn_mesh_sample_surface", "null")
    fails(lib.dsn_mesh_sample_surface(p, p, 8, 12, 0, 4, p, 8, None, None, None), "dsn_mesh_sample_surface", "too small")
    g, cell = np.zeros(3, np.int32), np.zeros(1, F32)
    fails(lib.dsn_mesh_dist_grid_host(12, None, g.ctypes.data, cell.ctypes.data), "dsn_mesh_dist_grid_host", "null")
    fails(lib.dsn_mesh_dist_grid_host(0, box.ctypes.data, g.ctypes.data, cell.ctypes.data), "dsn_mesh_dist_grid_host", "n_faces")
    fails(lib.dsn_mesh_dist_grid_host(12, bad_box.ctypes.data, g.ctypes.data, cell.ctypes.data), "dsn_mesh_dist_grid_host", "box")


def test_wrappers_exist_and_check_their_arguments():
    """the bindings and the visualizer functions import on any machine; the host grid rule and the argument checks need no device"""
    from dsnerf_amd import _lib, visualizer
    for name in ("mesh_dist_build", "mesh_dist_query", "mesh_dist_reduce", "mesh_sample_surface", "mesh_dist_grid"):
        assert callable(getattr(_lib, name))
    for name in ("closest_point", "sample_surface", "mesh_distance"):
        assert callable(getattr(visualizer, name))
    g, cell = _lib.mesh_dist_grid(200, ((0.1, 0.1, 0.1), (1.3, 1.3, 1.3)))
    rg, rc = R.grid_rule(200, (np.full(3, 0.1, F32), np.full(3, 1.3, F32)))
    assert g.tolist() == rg.tolist() and cell == rc
    with pytest.raises(ValueError):
        visualizer.mesh_distance((np.zeros((3, 3), F32), np.array([[0, 1, 2]])), (np.zeros((3, 3), F32), np.array([[0, 1, 2]])), samples=2.5)
