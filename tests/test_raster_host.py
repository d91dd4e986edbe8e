"""The mesh rasteriser without a GPU: closed forms for the numpy restatement of include/dsnerf.h's rule (tests/raster_restate.py) -
exact coverage and depth, orientation, dropped triangles, the spotlight - the properties of the inputs the GPU tests use (few
near-ties, float32 and float64 shading agree), and the argument checks of the entry points."""
import ctypes as C

import numpy as np
import pytest

import raster_restate as R

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


@pytest.fixture(scope="module")
def table():
    import dsnerf_amd
    return dsnerf_amd._lib.mc_table()


def test_exact_quad_covers_every_pixel_once():
    """corners and the shared diagonal on pixel centres: top and left edges in, bottom and right out, each pixel in one triangle, and
    the flat depth is w"""
    for w in (4.0, 0.5, 64.0):
        v, f, pose = R.exact_quad(w)
        out = R.raster(v, f, pose, 1.0, 1.0, 0.05, H=8)
        want = np.zeros((8, 8), np.int64)
        want[1:5, 1:5] = 1
        assert np.array_equal(out["count"], want)
        assert np.array_equal(out["face"] >= 0, want == 1)
        assert (out["depth"][1:5, 1:5] == F32(w)).all() and (out["depth"][want == 0] == 0).all()
        assert (out["color"][want == 0] == 255).all()
        # the diagonal's pixels (x = y) belong to one triangle, the others split by side
        fc = out["face"][1:5, 1:5]
        assert (fc[np.triu_indices(4, 1)] == 0).all() and (fc[np.tril_indices(4, -1)] == 1).all()
        assert len(set(np.diag(fc).tolist())) == 1
        # either winding and either diagonal orientation: the same coverage
        out2 = R.raster(v, f[:, ::-1], pose, 1.0, 1.0, 0.05, H=8)
        assert np.array_equal(out2["count"], want) and np.array_equal(out2["depth"], out["depth"])


def test_orientation_row0_is_top_and_x_is_right():
    # a small triangle up and to the right of the axis of the default camera (at z = 2.5, looking down -z, y up)
    v = np.array([[0.5, 0.5, 0.0], [0.7, 0.5, 0.0], [0.5, 0.7, 0.0]], F32)
    out = R.raster(v, np.array([[0, 1, 2]]), H=64)
    ys, xs = np.nonzero(out["face"] >= 0)
    assert ys.size > 0 and ys.max() < 32 and xs.min() >= 32
    # its projection: x = 0.5 at distance 2.5 with fx = cot(30 deg) -> px = (0.5 fx / 2.5 + 1) 32
    fx, fy = R.default_scales()
    assert abs(xs.min() - (0.5 * fx / 2.5 + 1) * 32) <= 1 and abs(ys.max() - (1 - 0.5 * fy / 2.5) * 32) <= 1
    # nearer is smaller depth, and depth is the distance along -z
    assert np.allclose(out["depth"][out["face"] >= 0], 2.5, rtol=1e-6)
    # a rotated camera: from +x looking at the origin, world +y stays up, world -z is to the right
    pose = np.array([[0.0, 0.0, 1.0, 2.5], [0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    v = np.array([[0.0, 0.5, -0.5], [0.0, 0.5, -0.7], [0.0, 0.7, -0.5]], F32)
    ys, xs = np.nonzero(R.raster(v, np.array([[0, 1, 2]]), pose, H=64)["face"] >= 0)
    assert ys.size > 0 and ys.max() < 32 and xs.min() >= 32


def test_dropped_triangles_leave_the_good_one_alone():
    good = np.array([[-0.5, -0.5, 0.0], [0.6, -0.4, 0.1], [0.0, 0.7, -0.2]], F32)
    ref = R.raster(good, np.array([[0, 1, 2]]), H=48)
    assert (ref["face"] == 0).sum() > 100
    nan, inf = np.nan, np.inf
    bad = {
        "behind znear": [[0.0, 0.0, 1.0], [0.2, 0.0, 1.0], [0.0, 0.2, 2.46]],           # w = 0.04 <= znear on one vertex
        "behind the camera": [[0.0, 0.0, 1.0], [0.2, 0.0, 1.0], [0.0, 0.2, 3.0]],
        "nan": [[0.0, 0.0, 1.0], [nan, 0.0, 1.0], [0.0, 0.2, 1.0]],
        "inf": [[0.0, 0.0, 1.0], [0.2, inf, 1.0], [0.0, 0.2, 1.0]],
        "zero area": [[0.0, 0.0, 1.0], [0.2, 0.2, 1.0], [0.4, 0.4, 1.0]],
        "guard band": [[0.0, 0.0, 1.0], [1.0e5, 0.0, 2.4], [0.0, 0.2, 1.0]],            # |X| > 2^24 sub-pixels
    }
    for name, tri in bad.items():
        v = np.concatenate([good, np.array(tri, F32)])
        out = R.raster(v, np.array([[0, 1, 2], [3, 4, 5]]), H=48)
        for k in ("face", "depth", "color", "count"):
            assert np.array_equal(out[k], ref[k]), (name, k)
        # without the flaw the same triangle is drawn (in front of the good one: z = 1 is nearer the camera)
    ok = np.concatenate([good, np.array([[0.0, 0.0, 1.0], [0.2, 0.0, 1.0], [0.0, 0.2, 1.0]], F32)])
    assert (R.raster(ok, np.array([[0, 1, 2], [3, 4, 5]]), H=48)["face"] == 1).sum() > 10
    # indices out of range, either side
    for idx in ([0, 1, 3], [0, -1, 2], [2 ** 31 - 1, 1, 2]):
        out = R.raster(good, np.array([[0, 1, 2], idx]), H=48)
        assert np.array_equal(out["face"], ref["face"]) and np.array_equal(out["count"], ref["count"])
    # the guard band itself: |X| = 2^24 is valid, one sub-pixel beyond is not (fx = fy = 1, w = 1, W = 2: X = (x + 1) 256)
    X, _, _, valid = R.project(np.array([[65535.0, 0, -1], [65535.00390625 + 0.00390625, 0, -1], [-65537.0, 0, -1]], F32), np.eye(4), 1.0, 1.0,
                               0.05, 2, 2)
    assert valid.tolist() == [True, False, True] and X[0] == 2 ** 24 and X[2] == -2 ** 24
    # no faces at all
    out = R.raster(good, np.zeros((0, 3), np.int32), H=5, W=7)
    assert (out["face"] == -1).all() and (out["depth"] == 0).all() and (out["color"] == 255).all() and out["color"].shape == (5, 7, 3)


def test_nearest_fragment_wins_and_ties_go_to_the_lowest_face():
    # (legs of 8 pixels: the area is a power of two, the barycentrics and the flat depth exact)
    near = R.screen_mesh([[[2, 2], [10, 2], [2, 10]]], 2.0, 16, 16)
    far = R.screen_mesh([[[2, 2], [10, 2], [2, 10]]], 4.0, 16, 16)
    v = np.concatenate([far[0], near[0], near[0]])
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    out = R.raster(v, f, np.eye(4), 1.0, 1.0, 0.05, H=16)
    hit = out["face"] >= 0
    assert hit.sum() > 20 and (out["face"][hit] == 1).all() and (out["count"][hit] == 3).all()
    assert (out["depth"][hit] == 2).all() and (out["depth2"][hit] == 2).all() and (R.ulp_gap(out["depth"], out["depth2"])[hit] == 0).all()
    out = R.raster(v[:6], f[:2], np.eye(4), 1.0, 1.0, 0.05, H=16)
    assert (out["depth2"][hit] == 4).all() and np.isinf(out["depth2"][~hit]).all() and (R.ulp_gap(out["depth"], out["depth2"]) > 4).all()


def level64(x, y, H, W, dist, fx, fy, intensity=30.0, inner=np.pi / 16, outer=np.pi / 6, base=0.3):
    """a plane facing the camera at distance `dist`, in float64 from the physics: Lambert, inverse square, glTF's cone falloff"""
    xn, yn = (2 * x + 1) / W - 1, 1 - (2 * y + 1) / H
    p = np.array([xn * dist / fx, yn * dist / fy, -dist])
    r = np.linalg.norm(p)
    cos = dist / r                                   # both the angle off the axis and the angle to the plane's normal
    s = np.clip((cos - np.cos(outer)) / (np.cos(inner) - np.cos(outer)), 0, 1) ** 2
    return base / np.pi * intensity * s * cos / (r * r)


def test_spotlight_on_a_facing_plane():
    v = np.array([[-4, -4, 0], [4, -4, 0], [4, 4, 0], [-4, 4, 0]], F32)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    H = W = 64
    fx, fy = R.default_scales()
    out = R.raster(v, f, H=H)
    assert (out["face"] >= 0).all() and np.allclose(out["depth"], 2.5, rtol=1e-6)
    lv = out["color"][:, :, 0].astype(np.int64)
    assert np.array_equal(out["color"][:, :, 1], out["color"][:, :, 0]) and np.array_equal(out["color"][:, :, 2], out["color"][:, :, 0])
    ys, xs = np.mgrid[0:H, 0:W]
    want = np.vectorize(lambda x, y: level64(x, y, H, W, 2.5, fx, fy))(xs, ys)
    assert np.abs(lv - np.floor(np.minimum(want, 1) * 255 + 0.5)).max() <= 1
    assert (np.abs(lv - np.floor(np.minimum(want, 1) * 255 + 0.5)) == 1).mean() < 0.005
    # on the axis: 0.3 * 30 / pi / 2.5^2 = 0.458 -> level 117
    assert lv[31, 31] == lv[32, 32] == 117
    # full inside the inner cone (no falloff: Lambert and inverse square only), zero outside the outer cone
    cos = 2.5 / np.sqrt((((2 * xs + 1) / W - 1) * 2.5 / fx) ** 2 + ((1 - (2 * ys + 1) / H) * 2.5 / fy) ** 2 + 2.5 ** 2)
    inner, outer = cos > np.cos(np.pi / 16) + 1e-6, cos < np.cos(np.pi / 6) - 1e-6
    assert inner.sum() > 100 and outer.sum() > 100
    plain = 0.3 * 30 / np.pi * cos ** 3 / 2.5 ** 2
    assert np.abs(lv[inner] - np.floor(plain[inner] * 255 + 0.5)).max() <= 1
    assert (lv[outer] == 0).all() and (lv[~outer & (cos < np.cos(np.pi / 6) + 0.02)] <= 2).all()
    # a plane seen edge-on gets no light; the back of a triangle is lit like its front
    edge = np.array([[0, -1, -1], [0, 1, -1], [0, 0, 1]], F32)
    assert (R.raster(edge, np.array([[0, 1, 2]]), H=32)["face"] == -1).all()
    a = R.raster(v, f, H=H)["color"]
    b = R.raster(v, f[:, ::-1], H=H)["color"]
    assert np.array_equal(a, b)
    # a saturating light clamps at 255, base 0 is black
    assert R.raster(v, f, H=8, light=R.light_values(intensity=3000.0))["color"][4, 4, 0] == 255
    assert (R.raster(v, f, H=8, light=R.light_values(base=0.0))["color"] == 0).all()


def test_inputs_of_the_gpu_tests_have_no_near_ties_and_shade_alike(table):
    """what tests/test_gpu_raster.py relies on: on the two-spheres meshes at most 0.1 % of the covered pixels have their two nearest
    fragments within 4 float32 steps, and the float32 and float64 evaluations of the shade differ by at most one level on less than
    0.5 % of them (nowhere by more)"""
    for n, H, W in R.SPHERE_CASES:
        v, f = R.two_spheres(n, table)
        out = R.raster(v, f, H=H, W=W)
        hit = out["face"] >= 0
        assert hit.sum() > 0.1 * H * W and (out["count"][hit] >= 2).mean() > 0.9          # closed surfaces: front and back
        assert len(np.unique(out["face"][hit])) > 0.2 * hit.sum()                           # micro-triangles
        near = (R.ulp_gap(out["depth"], out["depth2"]) <= 4) & hit
        assert near.sum() <= 0.001 * hit.sum(), (n, int(near.sum()), int(hit.sum()))
        fx, fy = R.default_scales(height=H, width=W)
        _, l32 = R.shade_levels(v, f, R.DEFAULT_POSE, fx, fy, R.light_values(), H, W, out["face"], out["depth"])
        _, l64 = R.shade_levels(v, f, R.DEFAULT_POSE, fx, fy, R.light_values(), H, W, out["face"], out["depth"], dtype=np.float64)
        d = np.abs(l32.astype(np.float64) - l64)
        assert d.max() <= 1 and (d > 0).sum() < 0.005 * hit.sum(), (n, float(d.max()), int((d > 0).sum()))
        # occlusion: both spheres are seen, and where they overlap on screen the nearer one wins
        assert 0 < out["depth"][hit].min() < 2.0 and out["depth"][hit].max() > 2.5


def test_box_sizes_of_the_big_triangle_mesh():
    """the mesh of the GPU test of the wave form: bounding boxes of 15, 16 (the threshold), 17 and 10 000 pixels, one triangle over the
    whole 256 x 256 image"""
    import dsnerf_amd
    assert dsnerf_amd._lib.RM_BIG_PIXELS == 16
    v, f, pose = R.big_triangle_mesh()
    assert R.box_pixels(v, f, pose, 1.0, 1.0, 0.05, 256, 256).tolist() == [15, 16, 17, 10000, 65536]
    out = R.raster(v, f, pose, 1.0, 1.0, 0.05, H=256)
    assert (out["face"] >= 0).all() and set(np.unique(out["face"]).tolist()) == {0, 1, 2, 3, 4}
    assert np.allclose(out["depth"][out["face"] == 4], 8, rtol=1e-6) and np.allclose(out["depth"][out["face"] == 3], 4, rtol=1e-6)


def test_abi_argument_errors(lib):
    import dsnerf_amd
    z, one = None, C.c_void_p(64)
    for name in ("dsn_raster_workspace_bytes", "dsn_raster_mesh", "dsn_raster_mesh_ex"):
        assert hasattr(lib, name) and name in dsnerf_amd._lib.EXPORTS
    wb = lib.dsn_raster_workspace_bytes
    assert wb(0, 0, 1, 1) >= 8 and wb(100, 200, 64, 64) >= 12 * 100 + 4 * 200 + 8 * 64 * 64
    assert wb(5_100_000, 10_200_000, 1024, 1024) < 140e6
    for bad in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (0, 0, 16385, 8), (0, 0, 8, 16385), (1 << 31, 0, 8, 8), (0, 1 << 31, 8, 8)):
        assert wb(*bad) == 0, bad
    assert wb(0, 0, 16384, 16384) >= 8 * 16384 * 16384
    # monotone in every argument
    base = (1000, 2000, 100, 120)
    for k in range(4):
        prev = wb(*base)
        for step in (1, 7, 1000):
            a = list(base)
            a[k] += step
            assert wb(*a) >= prev
            prev = wb(*a)
    pose = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2.5)
    light = (C.c_float * 4)(30.0, 0.98, 0.87, 0.3)
    ws = wb(3, 1, 8, 8)

    def call(verts=one, nv=3, faces=one, nf=1, p=pose, fx=1.0, fy=1.0, znear=0.05, lt=light, H=8, W=8, of=one, od=one, oc=one, w=one,
             nbytes=ws):
        return lib.dsn_raster_mesh(verts, nv, faces, nf, p, fx, fy, znear, lt, H, W, of, od, oc, w, nbytes, z)

    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(verts=z), b"null"), (dict(faces=z), b"null"), (dict(p=z), b"null"), (dict(lt=z), b"null"), (dict(w=z), b"null"),
        (dict(of=z, od=z, oc=z), b"no output"),
        (dict(H=0), b"16384"), (dict(W=0), b"16384"), (dict(H=16385), b"16384"), (dict(W=-3), b"16384"),
        (dict(nv=-1), b"negative"), (dict(nf=-1), b"negative"), (dict(nv=1 << 31), b"2^31"),
        (dict(nbytes=ws - 1), b"workspace"), (dict(nbytes=0), b"workspace"), (dict(w=C.c_void_p(72)), b"aligned"),
        (dict(fx=nan), b"finite"), (dict(fy=inf), b"finite"), (dict(znear=nan), b"finite"), (dict(znear=-inf), b"finite"),
        (dict(znear=0.0), b"positive"), (dict(znear=-1.0), b"positive"),
        (dict(lt=(C.c_float * 4)(30.0, 0.5, 0.5, 0.3)), b"cos_inner"), (dict(lt=(C.c_float * 4)(nan, 0.9, 0.5, 0.3)), b"finite"),
        (dict(p=(C.c_float * 12)(*([nan] * 12))), b"finite"),
    ]
    for kw, msg in cases:
        assert call(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_raster_mesh" in err and msg in err, (kw, err)
    assert lib.dsn_raster_mesh_ex(one, 3, one, 1, pose, 1.0, 1.0, 0.05, light, 8, 8, one, one, one, one, ws, 32, 0, z) != 0
    assert b"phases" in lib.dsn_last_error()
    assert lib.dsn_raster_mesh_ex(one, 3, one, 1, pose, 1.0, 1.0, 0.05, light, 8, 8, one, one, one, one, ws, 0, -1, z) != 0
    assert b"big_pixels" in lib.dsn_last_error()


def test_visualizer_render_mesh_rejects_none():
    from dsnerf_amd.visualizer import Visualizer3D
    vis = Visualizer3D(64, 32, 0.5, "ascent")
    assert "pyrender) are not provided" not in __import__("dsnerf_amd.visualizer", fromlist=["x"]).__doc__
    with pytest.raises(ValueError):
        vis.render_mesh(None)
