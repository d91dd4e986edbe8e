"""Mesh smoothing and face normals without a GPU: the numpy restatement of include/dsnerf.h's rules (tests/mesh_smooth_restate.py) against
closed forms and a float64 scipy.sparse umbrella step, the properties the rules promise, and the argument checks of dsn_mesh_smooth* /
dsn_mesh_vertex_normals* through the loaded library."""
import ctypes as C

import numpy as np
import pytest

import mesh_smooth_restate as R

F32 = np.float32
CENTRE = (2.2, -2.6, 3.1)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


@pytest.fixture(scope="module")
def noisy():
    v, f = R.icosphere(3, centre=CENTRE, noise=0.02, seed=3)
    assert v.shape == (642, 3) and f.shape == (1280, 3)
    return v, f


def radial_rms(v):
    r = np.linalg.norm(np.asarray(v, np.float64) - np.array(CENTRE), axis=1)
    return float(np.sqrt(np.mean((r - r.mean()) ** 2)))


@pytest.mark.parametrize("level", [2, 3, 4])
def test_one_step_against_float64(level):
    """|x' - float64 umbrella step| <= |f| 2^-k (every q is floored: a difference of two is off by less than one unit, and so is their
    mean) + half an ulp of the largest |x'| (the one rounding to float32)"""
    v, f = R.icosphere(level, centre=CENTRE, noise=0.02, seed=level)
    for fac in (0.5, -0.53, 1.0):
        out = R.smooth(v, f, [fac])
        ref = R.umbrella_float64(v, f, float(F32(fac)))
        k = out["k"]
        err = np.abs(out["verts"].astype(np.float64) - ref).max(axis=0)
        bound = abs(fac) * 2.0 ** -k + 0.5 * np.spacing(np.abs(out["verts"]).max(axis=0).astype(F32)).astype(np.float64)
        print("level", level, "factor", fac, "k", k, "err", err, "bound", bound)
        assert k == 25 and (err <= bound).all()
        assert out["counts"].tolist() == [f.shape[0], 0, v.shape[0], 6]


def test_taubin_keeps_the_volume_and_laplacian_shrinks(noisy):
    v, f = noisy
    vol0, rms0 = R.volume(v, f), radial_rms(v)
    t = R.smooth(v, f, R.taubin(10))["verts"]
    lap = R.smooth(v, f, R.taubin(20, 0.5, None))["verts"]
    print("volume", vol0, "taubin", R.volume(t, f) / vol0, "laplacian", R.volume(lap, f) / vol0, "rms", rms0, radial_rms(t))
    assert abs(R.volume(t, f) / vol0 - 1.0) < 0.02
    assert R.volume(lap, f) / vol0 < 0.8
    assert radial_rms(t) < 0.5 * rms0


def test_planar_grid():
    v, f = R.grid_plane(9)
    x = v
    for _ in range(10):
        x = R.smooth(x, f, [0.5])["verts"]
        assert np.array_equal(bits(x[:, 2]), bits(v[:, 2]))                      # the plane's coordinate keeps its bits
    one = R.smooth(v, f, [0.5])["verts"]
    i, j = np.divmod(np.arange(81), 9)
    inner = (i > 0) & (i < 8) & (j > 0) & (j < 8)
    assert np.array_equal(bits(one[inner]), bits(v[inner]))                      # a symmetric umbrella: the sum is exactly 0
    assert not np.array_equal(bits(one[~inner]), bits(v[~inner]))                # the boundary leans inward
    # ten steps through one call = ten calls with the same origin and k
    o, k = R.scale_of(v)
    many = R.smooth(v, f, [0.5] * 10, o, k)["verts"]
    y = v
    for _ in range(10):
        y = R.smooth(y, f, [0.5], o, k)["verts"]
    assert np.array_equal(bits(many), bits(y))


def test_face_order_and_rotation(noisy):
    v, f = noisy
    rng = np.random.default_rng(2)
    base = R.smooth(v, f, R.taubin(3))
    nb = R.vertex_normals(v, f)
    rot = f.copy()
    for t in range(f.shape[0]):
        rot[t] = np.roll(f[t], t % 3)
    for ff in (f[rng.permutation(f.shape[0])], f[::-1], rot):
        out = R.smooth(v, ff, R.taubin(3))
        assert np.array_equal(bits(out["verts"]), bits(base["verts"])) and out["counts"].tolist() == base["counts"].tolist()
    for ff in (f[rng.permutation(f.shape[0])], f[::-1]):                         # (a rotation changes the float32 cross product's roundings)
        assert np.array_equal(bits(R.vertex_normals(v, ff)), bits(nb))


def test_skipped_faces_and_unused_vertices():
    nan, inf = np.nan, np.inf
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [nan, 0, 0], [0, inf, 0], [5, 5, 5], [2, 2, 2], [0.5, 0.5, -1]], F32)
    V = v.shape[0]
    f = np.array([[0, 1, 2], [1, 3, 2], [0, 0, 1], [2, 1, 2], [0, 1, V], [-1, 0, 1], [0, 1, 4], [5, 1, 2], [2 ** 31 - 1, 0, 1],
                  [-2 ** 31, 1, 2], [0, 8, 1], [3, 3, 3]], np.int32)
    out = R.smooth(v, f, [0.5, -0.53, 0.25])
    assert R.contributing(v, f).tolist() == [True, True] + [False] * 8 + [True, False]
    assert out["counts"].tolist() == [3, 9, 5, 3] and out["n"].tolist() == [4, 6, 4, 2, 0, 0, 0, 0, 2]
    for i in (4, 5, 6, 7):                                                       # not finite, or used by no contributing face: the bits
        assert np.array_equal(bits(out["verts"][i]), bits(v[i]))
    only = R.smooth(v, f[[0, 1, 10]], [0.5, -0.53, 0.25])
    assert np.array_equal(bits(only["verts"]), bits(out["verts"]))               # the skipped faces change nothing
    # one step by hand at vertex 3 (neighbours 1 and 2 through one face): x + f (mean - x), exactly representable here
    one = R.smooth(v, f, [0.5])["verts"]
    assert one[3].tolist() == [0.75, 0.75, 0.25]
    # factor 0 moves nothing, factor 1 lands on the (quantised) neighbours' mean
    assert np.array_equal(bits(R.smooth(v, f, [0.0, 0.0])["verts"]), bits(v))
    assert R.smooth(v, f, [1.0])["verts"][3].tolist() == [0.5, 0.5, 0.0]
    # no finite vertex, no vertex, no face
    allnan = np.full((3, 3), nan, F32)
    out = R.smooth(allnan, [[0, 1, 2]], [0.5])
    assert np.array_equal(bits(out["verts"]), bits(allnan)) and out["counts"].tolist() == [0, 1, 0, 0] and out["k"] == 27
    assert R.smooth(np.zeros((0, 3), F32), [[0, 1, 2]], [0.5])["counts"].tolist() == [0, 1, 0, 0]
    assert R.smooth(v, np.zeros((0, 3), np.int32), [0.5])["counts"].tolist() == [0, 0, 0, 0]


def test_no_steps_returns_the_input(noisy):
    v, f = noisy
    w = v.copy()
    w[5] = [np.nan, -np.inf, -0.0]
    out = R.smooth(w, f, [])
    assert np.array_equal(bits(out["verts"]), bits(w)) and out["counts"][0] == f.shape[0] - 5          # (vertex 5 is one of the twelve with five faces)


def test_sum_bounds():
    """|S| <= 2 T (2^31 - 1) < 2^63 at T = 2^31 - 1: q in [-2^30, 2^30 - 1], so a difference is at most 2^31 - 1 in magnitude, a face adds
    two of them, at most T faces meet in a vertex.  The normals: |n_c| <= D2 < 2^e, so a term is below 2^(e + shift) = 2^(61 - bit_length(T))
    and T < 2^bit_length(T) of them stay below 2^61."""
    T = 2 ** 31 - 1
    qlo, qhi = int(R.QLO), int(R.QHI)
    assert (qlo, qhi) == (-2 ** 30, 2 ** 30 - 1) and qhi - qlo == 2 ** 31 - 1
    assert 2 * T * (qhi - qlo) < 2 ** 63
    q = R.quantise(np.array([[1e30, -1e30, np.inf], [np.nan, 0.0, -np.inf]], F32), np.zeros(3, F32), 27)
    assert q.tolist() == [[qhi, qlo, 0], [0, 0, 0]]
    for T in (1, 2, 1000, 2 ** 20, 2 ** 31 - 1):
        for ext in (1e-3, 1.0, 300.0):
            box = np.array([[0, 0, 0], [ext, ext / 2, ext / 3]], F32)
            s = R.area_shift(box, T)
            d = box[1] - box[0]
            d2 = float(F32(F32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
            assert T * int(np.floor(np.ldexp(d2, s))) < 2 ** 61


def test_caller_scale():
    assert R.scale_of(np.array([[1, 2, 3], [1.5, 2.25, 3.99]], F32))[1] == 27
    assert R.scale_of(np.array([[1, 2, 3], [2, 2.25, 3.99]], F32))[1] == 26          # D = 1: frexp exponent 1
    assert R.scale_of(np.array([[1, 2, 3], [1, 2, 3]], F32))[1] == 27                # D = 0
    o, k = R.scale_of(np.array([[-4, 0, 0], [4, 1, np.nan], [0.5, 0.5, 0.5]], F32))
    assert o.tolist() == [-4, 0, 0]
    assert k == 27 - 3                                                               # D = 4.5 over the two finite vertices
    from dsnerf_amd import _lib
    for pts in ([[1, 2, 3], [1.5, 2.25, 3.99]], [[1, 2, 3], [2, 2.25, 3.99]], [[1, 2, 3], [1, 2, 3]], [[-300, 2, 3], [1, 700.5, 3e-3]]):
        v = np.array(pts, F32)
        o, k = _lib.mesh_smooth_scale((v.min(axis=0), v.max(axis=0)))
        ro, rk = R.scale_of(v)
        assert k == rk and np.array_equal(bits(o), bits(ro))
    o, k = _lib.mesh_smooth_scale(None)
    assert o.tolist() == [0, 0, 0] and k == 27
    # the box maps to [0, 2^27)
    v = (np.random.default_rng(1).random((100, 3)) * 37.5 - 20).astype(F32)
    o, k = R.scale_of(v)
    q = R.quantise(v, o, k)
    assert q.min() == 0 and 2 ** 26 <= q.max() < 2 ** 27


@pytest.mark.parametrize("level,limit", [(3, 1.0), (4, 1.0)])
def test_normals_of_a_sphere(level, limit):
    v, f = R.icosphere(level, centre=CENTRE)
    n = R.vertex_normals(v, f).astype(np.float64)
    radial = v.astype(np.float64) - np.array(CENTRE)
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip((n * radial).sum(axis=1), -1, 1)))
    print("level", level, "largest angle to the radial direction", ang.max())
    assert ang.max() < limit and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    flipped = R.vertex_normals(v, f[:, ::-1]).astype(np.float64)                 # the other winding: the other side
    assert ((flipped * radial).sum(axis=1) < -0.99).all()


def test_normals_skip_what_adds_nothing():
    nan = np.nan
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 2, 0], [3, 3, 0], [nan, 0, 0], [9, 9, 9]], F32)
    f = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    base = R.vertex_normals(v, f, shift=40)
    assert base[:4].tolist() == [[0, 0, 1]] * 4 and base[4:].tolist() == [[0, 0, 0]] * 4
    more = np.concatenate([f, np.array([[0, 3, 4], [3, 4, 5], [0, 0, 1], [1, 2, 2], [3, 0, 3], [0, 1, 6], [0, 1, 8], [-1, 0, 1]], np.int32)])
    got = R.vertex_normals(v, more, shift=40)                                    # collinear, repeated, NaN, out of range
    assert np.array_equal(bits(got), bits(base))
    assert np.array_equal(R.normal_sums(v, more, 40), R.normal_sums(v, f, 40))
    # a repeated index gives exactly zero whatever the third corner (also where the edge overflows: not finite, counts as 0)
    w = np.array([[3e38, 1, 2], [-3e38, 5, 6], [0.3, 0.7, 0.9]], F32)
    assert not R.normal_sums(w, np.array([[0, 0, 1], [0, 1, 1], [1, 0, 1], [2, 2, 0], [0, 2, 0]], np.int32), 0).any()
    # area weighting: the larger face decides
    v2 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 10]], F32)
    n = R.vertex_normals(v2, np.array([[0, 1, 2], [0, 3, 1]], np.int32))
    assert n[0, 1] > 0.99 and 0 < n[0, 2] < 0.11 and n[2].tolist() == [0, 0, 1] and n[3].tolist() == [0, 1, 0]


def test_smooth_dict(noisy):
    v, f = noisy
    rng = np.random.default_rng(4)
    V = v.shape[0]
    mesh = {"verts": v, "faces": f, "normals": v.copy(), "albedo": rng.random((V, 3)).astype(F32), "colour": rng.random((2, V, 3)).astype(F32),
            "source_vertex": np.arange(V, dtype=np.int32), "face_idx": np.zeros(V, np.int32), "uv": np.zeros((V, 2), F32),
            "h": np.zeros(V, F32), "cov": None, "x_c": np.zeros((V, 3), F32), "name": "body", "n_components": 3}
    out = R.smooth_dict(mesh, iterations=2)
    assert set(out) == {"verts", "faces", "normals", "albedo", "colour", "source_vertex", "name", "n_components", "smooth_info"}
    assert out["albedo"] is mesh["albedo"] and out["faces"] is f and out["name"] == "body"
    assert np.array_equal(bits(out["verts"]), bits(R.smooth(v, f, [0.5, -0.53, 0.5, -0.53])["verts"]))
    assert np.array_equal(bits(out["normals"]), bits(R.vertex_normals(out["verts"], f)))
    assert out["smooth_info"]["factors"].tolist() == [F32(0.5), F32(-0.53)] * 2 and out["smooth_info"]["scale_exp"] == 25
    assert "normals" not in R.smooth_dict(mesh, 1, normals=False)
    plain = {"verts": v, "faces": f}
    assert "normals" not in R.smooth_dict(plain, 1) and "normals" in R.smooth_dict(plain, 1, normals=True)
    lap = R.smooth_dict(plain, 3, lamb=0.25, mu=None)
    assert np.array_equal(bits(lap["verts"]), bits(R.smooth(v, f, [0.25] * 3)["verts"]))


def test_python_argument_checks(noisy):
    from dsnerf_amd import _lib, visualizer
    v, f = noisy
    assert visualizer.smooth_keywords(3) == {"iterations": 3} and visualizer.smooth_keywords({"iterations": 2, "mu": None}) == {"iterations": 2, "mu": None}
    for bad in (True, 2.5, "3", None):
        with pytest.raises(ValueError):
            visualizer.smooth_keywords(bad)
    with pytest.raises(ValueError):
        visualizer.smooth_mesh((v, f), iterations=-1)
    with pytest.raises(ValueError):
        visualizer.smooth_mesh((v, f), iterations=2049)                          # 4098 steps
    with pytest.raises(ValueError):
        visualizer.smooth_mesh((v, f), iterations=4097, mu=None)
    for kw in (dict(factors=[0.5, np.nan]), dict(factors=[np.inf]), dict(origin=[0, np.nan, 0]), dict(scale_exp=901), dict(factors=[0.5] * 4097)):
        args = dict(factors=[0.5], origin=np.zeros(3, F32), scale_exp=27)
        args.update(kw)
        with pytest.raises(ValueError):
            _lib._mesh_smooth_check(args["factors"], args["origin"], args["scale_exp"])
    assert (_lib.MESH_SMOOTH_HEAVY, _lib.MESH_SMOOTH_MAX_STEPS) == (R.HEAVY, R.MAX_STEPS)
    assert set(visualizer.BINDING_KEYS) == set(R.BINDING_KEYS)
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dsnerf.h")).read()
    defs = dict(re.findall(r"#define (DSN_(?:SM|MESH_SMOOTH)_\w+) (\d+)", header))
    assert {k: int(x) for k, x in defs.items()} == {
        "DSN_MESH_SMOOTH_HEAVY": _lib.MESH_SMOOTH_HEAVY, "DSN_MESH_SMOOTH_MAX_STEPS": _lib.MESH_SMOOTH_MAX_STEPS,
        "DSN_MESH_SMOOTH_MAX_EXP": _lib.MESH_SMOOTH_MAX_EXP, "DSN_SM_COUNT": _lib.SM_COUNT, "DSN_SM_SCAN": _lib.SM_SCAN, "DSN_SM_FILL": _lib.SM_FILL,
        "DSN_SM_STEP": _lib.SM_STEP, "DSN_SM_NORMALS": _lib.SM_NORMALS}


def test_abi_symbols_and_argument_checks(lib):
    import dsnerf_amd
    L = dsnerf_amd._lib
    for n in ("dsn_mesh_smooth_workspace_bytes", "dsn_mesh_smooth", "dsn_mesh_smooth_ex", "dsn_mesh_vertex_normals", "dsn_mesh_vertex_normals_ex"):
        assert hasattr(lib, n) and n in L.EXPORTS
    z, one, far, al = None, C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(4096)
    org = (C.c_float * 3)(0.0, 0.0, 0.0)
    fac = (C.c_float * 2)(0.5, -0.53)
    wb = lib.dsn_mesh_smooth_workspace_bytes
    assert wb(-1, 0) == 0 and wb(0, -1) == 0 and wb(1 << 31, 0) == 0 and wb(0, 1 << 31) == 0 and wb(0, 0) > 0
    # row lengths, cursors, prefixes (16 V), entries (24 T), two position buffers (24 V)
    assert wb(1000, 2000) >= 40 * 1000 + 24 * 2000 and wb(1000, 2000) % 16 == 0 and wb((1 << 31) - 1, (1 << 31) - 1) > 3 * 8 * ((1 << 31) - 1)
    n = wb(10, 10)

    def smooth(v=one, f=one, V=10, T=10, o=org, k=27, fc=fac, ns=2, ws=al, nb=n, out=far, cnt=z):
        return lib.dsn_mesh_smooth(v, f, V, T, o, k, fc, ns, ws, nb, out, cnt, z)

    def normals(v=one, f=one, V=10, T=10, shift=30, ws=al, nb=n, out=far):
        return lib.dsn_mesh_vertex_normals(v, f, V, T, shift, ws, nb, out, z)
    nanf, inff = (C.c_float * 2)(0.5, float("nan")), (C.c_float * 2)(float("inf"), 0.5)
    bad = [(dict(v=z), b"null mesh"), (dict(f=z), b"null mesh"), (dict(out=z), b"null output"), (dict(ws=z), b"null argument"),
           (dict(o=z), b"null argument"), (dict(fc=z), b"null factors"), (dict(V=-1), b"negative"), (dict(T=-1), b"negative"),
           (dict(V=1 << 31), b"2^31"), (dict(T=1 << 31), b"2^31"), (dict(ns=-1), b"n_steps"), (dict(ns=4097), b"n_steps"),
           (dict(k=901), b"scale_exp"), (dict(k=-901), b"scale_exp"), (dict(fc=nanf), b"factor"), (dict(fc=inff), b"factor"),
           (dict(o=(C.c_float * 3)(0.0, float("nan"), 0.0)), b"origin"), (dict(o=(C.c_float * 3)(float("-inf"), 0.0, 0.0)), b"origin"),
           (dict(ws=C.c_void_p(4104)), b"16-byte"), (dict(nb=n - 1), b"too small"), (dict(nb=0), b"too small"),
           (dict(out=one), b"overlap"), (dict(out=C.c_void_p((1 << 20) + 116)), b"overlap"), (dict(out=C.c_void_p((1 << 20) - 116)), b"overlap")]
    for kw, msg in bad:
        assert smooth(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_mesh_smooth" in err and msg in err, (kw, err)
    for ph in (16, 32, -1):
        assert lib.dsn_mesh_smooth_ex(one, one, 10, 10, org, 27, fac, 2, al, n, far, z, ph, z) != 0 and b"phases" in lib.dsn_last_error()
    bad = [(dict(v=z), b"null mesh"), (dict(f=z), b"null mesh"), (dict(out=z), b"null output"), (dict(ws=z), b"null argument"),
           (dict(V=-1), b"negative"), (dict(T=1 << 31), b"2^31"), (dict(shift=61), b"shift"), (dict(shift=-61), b"shift"),
           (dict(ws=C.c_void_p(4097)), b"16-byte"), (dict(nb=n - 16), b"too small"), (dict(out=one), b"overlap")]
    for kw, msg in bad:
        assert normals(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_mesh_vertex_normals" in err and msg in err, (kw, err)
    for ph in (8, 32, -1):
        assert lib.dsn_mesh_vertex_normals_ex(one, one, 10, 10, 30, al, n, far, ph, z) != 0 and b"phases" in lib.dsn_last_error()
