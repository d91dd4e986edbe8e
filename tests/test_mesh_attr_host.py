"""Mesh normals, attributes and export without a GPU: the numpy restatements of include/dsnerf.h's rules for dsn_mc_normals
(tests/mc_normals_restate.py) and dsn_raster_mesh_attr (tests/raster_attr_restate.py) against closed forms, the float32 rule's own
error on the inputs of the GPU tests (tests/golden/raster_attr_spread.json), the argument checks of the new entry points, and
save_ply read back with numpy."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mc_normals_restate as N
import mc_restate as M
import raster_attr_restate as A
import raster_restate as R

F32 = np.float32
SPREAD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_attr_spread.json")


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


@pytest.fixture(scope="module")
def table():
    import dsnerf_amd
    return dsnerf_amd._lib.mc_table()


# ---- vertex normals -------------------------------------------------------------------------------------------------------------------
def sphere24():
    ax = tuple(np.arange(24, dtype=F32) for _ in range(3))
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in ax], indexing="ij")
    c = np.array([11.3, 11.7, 12.1])
    return (8.0 - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)).astype(F32), ax, c


def test_normals_of_a_sphere_are_radial(table):
    """8 - |p - c| on a 24^3 unit grid, centre off the lattice: within 1 degree of the radial direction (central differences at 8 cells
    radius: of order h^2 / 2 r^2, under half a degree), pointing out of the object for "descent" and into it for "ascent", and on the
    side of every triangle's geometric normal in both modes"""
    vol, ax, c = sphere24()
    for direction, sign in (("descent", 1.0), ("ascent", -1.0)):
        v, f = M.marching_cubes(vol, ax, 0.0, direction, table)
        n = N.normals(vol, ax, 0.0, direction)
        assert n.dtype == F32 and n.shape == v.shape and v.shape[0] > 1000
        radial = (v - c) / np.linalg.norm(v - c, axis=1, keepdims=True)
        ang = np.degrees(np.arccos(np.clip(sign * (n.astype(np.float64) * radial).sum(axis=1), -1, 1)))
        print(direction, "largest angle to the radial direction: %.3f degrees" % ang.max())
        assert ang.max() < 1.0
        assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
        g = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        assert ((g * n[f].sum(axis=1)).sum(axis=1) > 0).all()
        n64 = N.normals(vol, ax, 0.0, direction, dtype=np.float64)
        assert n64.dtype == np.float64 and np.abs(n64 - n).max() < 1e-5


def test_one_sided_forms_at_the_volume_faces(table):
    """a plane field v = a . p + b on non-uniform axes: every difference quotient - central over unequal intervals, one-sided on the
    outer faces - gives a, so every normal is -a / |a| (descent), also for the vertices on the faces the surface leaves through"""
    rng = np.random.default_rng(2)
    ax = tuple(np.cumsum(rng.uniform(0.5, 1.5, s)).astype(F32) for s in (9, 7, 6))
    a = np.array([0.5, -0.25, 1.0])
    X, Y, Z = np.meshgrid(*[x.astype(np.float64) for x in ax], indexing="ij")
    vol = (a[0] * X + a[1] * Y + a[2] * Z - 4.0).astype(F32)
    v, f = M.marching_cubes(vol, ax, 0.0, "descent", table)
    n = N.normals(vol, ax, 0.0, "descent")
    border = np.zeros(v.shape[0], bool)
    for d in range(3):
        border |= (v[:, d] == ax[d][0]) | (v[:, d] == ax[d][-1])
    assert border.sum() >= 8 and (~border).sum() >= 8
    assert np.abs(n + a / np.linalg.norm(a)).max() < 2e-5
    g = N.gradients(vol, ax)
    assert g.shape == vol.shape + (3,) and np.abs(g - a).max() < 2e-5
    # the forms themselves on one axis: v = x^2 at x = 0, 1, 3, 4
    sq = np.broadcast_to((np.array([0.0, 1.0, 3.0, 4.0]) ** 2)[:, None, None], (4, 2, 2)).astype(F32)
    gx = N.gradients(sq, (np.array([0, 1, 3, 4], F32), np.arange(2, dtype=F32), np.arange(2, dtype=F32)))[:, 0, 0, 0]
    assert gx.tolist() == [1.0, 3.0, 5.0, 7.0]          # (1 - 0) / 1, (9 - 0) / 3, (16 - 1) / 3, (16 - 9) / 1
    # a 2 x 2 x 2 grid: both points of every axis take the one interval there is
    cube = np.array([1, -1, -1, -1, -1, -1, -1, 2], F32).reshape(2, 2, 2)
    g = N.gradients(cube, tuple(np.array([0.0, 0.5], F32) for _ in range(3)))
    assert np.array_equal(g[0, ..., 0], g[1, ..., 0]) and np.array_equal(g[:, 0, :, 1], g[:, 1, :, 1]) and g[0, 0, 0, 0] == (cube[1, 0, 0] - cube[0, 0, 0]) / 0.5


def test_degenerate_inputs(table):
    rng = np.random.default_rng(7)
    noise = rng.standard_normal((11, 9, 8)).astype(F32)
    ax = tuple(np.arange(s, dtype=F32) for s in noise.shape)
    ref = N.normals(noise, ax, 0.5, "descent")
    assert np.isfinite(ref).all() and not (ref == 0).all(axis=1).any()
    nan = noise.copy()
    nan[4, 4, 4] = np.nan
    n = N.normals(nan, ax, 0.5, "descent")
    v, f = M.marching_cubes(nan, ax, 0.5, "descent", table)
    assert n.shape == v.shape and np.isfinite(n).all()
    zero = (n == 0).all(axis=1)
    # exactly the vertices whose edge has an end next to (or at) the NaN point along some axis
    nn_, d = N.crossing_edges(nan, 0.5)
    ijk = np.stack(np.unravel_index(nn_, nan.shape), axis=1)
    end_b = ijk.copy()
    end_b[np.arange(d.size), d] += 1
    near = lambda p: (np.abs(p - 4).sum(axis=1) <= 1)
    assert np.array_equal(zero, near(ijk) | near(end_b)) and zero.sum() > 0
    # a constant volume: a zero gradient everywhere; no vertices at a level it does not cross, zero normals for what lies on it
    const = np.full((4, 5, 6), 2.0, F32)
    axc = tuple(np.arange(s, dtype=F32) for s in const.shape)
    assert N.normals(const, axc, 0.5, "ascent").shape == (0, 3)
    assert (N.gradients(const, axc) == 0).all()
    flat = const.copy()
    flat[:2] = 1.0           # a step: the gradient across it is not zero, the normals are (+-1, 0, 0)
    n = N.normals(flat, axc, 1.5, "descent")
    assert n.shape[0] == 30 and (n[:, 0] == -1).all() and (n[:, 1:] == 0).all()
    with pytest.raises(ValueError):
        N.normals(const, axc, 0.5, "sideways")


# ---- interpolated attributes ----------------------------------------------------------------------------------------------------------
def test_weights_sum_to_one_and_reproduce_an_affine_colour(table):
    kw = A.quad_inputs()
    out = A.raster_attr(mode=A.SMOOTH, **kw)
    hit = out["hit"]
    assert hit.size == 36 and np.abs(out["weights"].sum(axis=1) - 1).max() <= 4 * np.finfo(F32).eps
    for n, H, W in R.SPHERE_CASES[:1]:
        k2 = A.gpu_inputs(table)["spheres%d_%dx%d" % (n, H, W)]
        assert np.abs(A.raster_attr(mode=0, **k2)["weights"].sum(axis=1) - 1).max() <= 4 * np.finfo(F32).eps
    # the fragment's world point: the pixel's ray at the winner's depth (identity camera at the origin)
    y, x = hit // 8, hit % 8
    z = out["depth"].reshape(-1)[hit].astype(np.float64)
    xn, yn = (2 * x + 1) / 8 - 1, 1 - (2 * y + 1) / 8
    world = np.stack([xn * z / A.QUAD_F, yn * z / A.QUAD_F, -z], axis=1)
    got = out["attr"].reshape(-1, 3)[hit]
    assert np.abs(got - A.affine_colour(world)).max() < 2e-6
    # the interpolated position is that point too
    pos = A.raster_attr(mode=0, **{**kw, "colors": kw["verts"]})["attr"].reshape(-1, 3)[hit]
    assert np.abs(pos - world).max() < 4e-6
    # screen-space weights (no 1 / w) do not reproduce it on this quad: the depth runs from 1.5 to 6
    X, Y, _, _ = R.project(kw["verts"], kw["pose"], A.QUAD_F, A.QUAD_F, 0.05, 8, 8)
    f = kw["faces"][out["face"].reshape(-1)[hit]]
    P = np.stack([X[f], Y[f]], axis=-1).astype(np.float64)
    cx, cy = 256.0 * x + 128, 256.0 * y + 128
    e = lambda a, b: (P[:, b, 0] - P[:, a, 0]) * (cy - P[:, a, 1]) - (P[:, b, 1] - P[:, a, 1]) * (cx - P[:, a, 0])
    lam = np.stack([e(1, 2), e(2, 0), e(0, 1)], axis=1)
    lam /= lam.sum(axis=1, keepdims=True)
    screen = (lam[:, :, None] * A.affine_colour(kw["verts"])[f]).sum(axis=1)
    assert np.abs(screen - A.affine_colour(world)).max() > 0.02


def test_flat_mode_without_attributes_is_the_plain_rasteriser(table):
    for n, H, W in R.SPHERE_CASES:
        v, f = R.two_spheres(n, table)
        base = R.raster(v, f, H=H, W=W)
        out = A.raster_attr(v, f, H=H, W=W, mode=0, base=base)
        for k in ("face", "depth", "color"):
            assert np.array_equal(out[k], base[k]), k
        assert "attr" not in out
        ln = np.linalg.norm(out["normal"].astype(np.float64), axis=-1)
        assert np.abs(ln[base["face"] >= 0] - 1).max() < 1e-5 and (ln[base["face"] < 0] == 0).all()
    v, f, pose = R.big_triangle_mesh()
    base = R.raster(v, f, pose, 1.0, 1.0, 0.05, H=256)
    assert np.array_equal(A.raster_attr(v, f, pose, 1.0, 1.0, H=256, mode=0, base=base)["color"], base["color"])


def test_modes_fallbacks_and_clamps():
    kw = A.quad_inputs()
    smooth = A.raster_attr(mode=A.SMOOTH, **kw)
    flat = A.raster_attr(mode=0, **kw)
    hit = smooth["hit"]
    assert not np.array_equal(smooth["normal"], flat["normal"])
    # unlit: the clamped colour itself, whatever the normals
    unlit = A.raster_attr(mode=A.UNLIT, **kw)
    want = np.floor(np.clip(unlit["attr"].reshape(-1, 3)[hit], 0, 1) * F32(255) + F32(0.5)).astype(np.uint8)
    assert np.array_equal(unlit["color"].reshape(-1, 3)[hit], want)
    assert np.array_equal(A.raster_attr(mode=A.UNLIT | A.SMOOTH, **kw)["color"], unlit["color"])
    # a NaN, an infinite or a zero vertex normal: every triangle that has it falls back to the flat normal (here: all pixels)
    for bad in ([np.nan, 0, 1], [0, 0, 0], [np.inf, 0, 0]):
        nrm = kw["normals"].copy()
        nrm[0] = bad                                        # vertex 0 is in both triangles
        fb = A.raster_attr(mode=A.SMOOTH, **{**kw, "normals": nrm})
        assert np.array_equal(fb["normal"], flat["normal"]) and np.array_equal(fb["color"], flat["color"])
    # vertex normals that cancel at the pixel: interpolated length 0 -> flat
    v, f, pose = R.screen_mesh([[[1, 1], [7, 1], [1, 7]]], 2.0, 8, 8)
    nrm = np.array([[1, 0, 0], [-1, 0, 0], [-1, 0, 0]], F32)
    o = A.raster_attr(v, f, pose, 1.0, 1.0, H=8, normals=nrm, mode=A.SMOOTH)
    f0 = A.raster_attr(v, f, pose, 1.0, 1.0, H=8, mode=0)
    w = o["weights"]
    cancel = (w[:, 0] == w[:, 1] + w[:, 2])
    assert cancel.any() and np.array_equal(o["normal"].reshape(-1, 3)[o["hit"]][cancel], f0["normal"].reshape(-1, 3)[o["hit"]][cancel])
    # colours: NaN is taken as 0, values beyond [0, 1] are clamped, out_attr keeps what was interpolated
    col = np.array([[np.nan, 2.0, -1.0]] * 4, F32)
    o = A.raster_attr(mode=A.UNLIT, **{**kw, "colors": col})
    px = o["color"].reshape(-1, 3)[hit]
    assert (px[:, 0] == 0).all() and (px[:, 1] == 255).all() and (px[:, 2] == 0).all()
    at = o["attr"].reshape(-1, 3)[hit]
    assert np.isnan(at[:, 0]).all() and np.abs(at[:, 1] - 2).max() < 1e-5 and np.abs(at[:, 2] + 1).max() < 1e-5
    lit = A.raster_attr(mode=0, **{**kw, "colors": col})["color"].reshape(-1, 3)[hit]
    assert (lit[:, 0] == 0).all() and (lit[:, 2] == 0).all()
    # a white colour under the light is 1 / base times the grey preview (before the clamp at 1)
    one = A.raster_attr(mode=0, **{**kw, "colors": np.ones((4, 3), F32)})
    grey = A.raster_attr(mode=0, **{**kw, "colors": None})
    assert np.array_equal(grey["color"], R.raster(kw["verts"], kw["faces"], kw["pose"], A.QUAD_F, A.QUAD_F, H=8)["color"])
    g = grey["level"].astype(np.float64)
    assert 0 < g.min() < 20 and g.max() > 255 * 0.3 and np.abs(np.minimum(g / 0.3, 255) - one["level"]).max() <= 2.5


def test_float32_and_float64_restatements_on_the_gpu_tests_inputs(table):
    """the float32 rule's own error: what tests/golden/raster_attr_spread.json records (the GPU tests' bars are 10 x its figures, floor
    2e-6), and the colour levels of the two restatements stay within the level bar of the GPU tests themselves"""
    with open(SPREAD) as fh:
        recorded = json.load(fh)["cases"]
    seen = set()
    for name, kw in A.gpu_inputs(table).items():
        base = R.raster(kw["verts"], kw["faces"], kw["pose"], kw["fx"], kw["fy"], 0.05, None, kw["H"], kw["W"])
        for mname, mode in A.MODES.items():
            a32 = A.raster_attr(mode=mode, base=base, **kw)
            a64 = A.raster_attr(mode=mode, base=base, dtype=np.float64, **kw)
            s = A.spread(a32, a64)
            key = name + ":" + mname
            seen.add(key)
            print(key, s)
            rec = recorded[key]
            assert s["covered"] == rec["covered"]
            for k in ("attr", "normal"):
                assert s[k] <= rec[k] * 1.001 + 1e-12, (key, k, s[k], rec[k])
            assert s["level_max"] <= 1 and s["level_share"] <= 0.005, (key, s)
            assert rec["level_max"] <= 1 and rec["level_share"] <= 0.005
    assert seen == set(recorded)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_argument_errors(lib):
    import dsnerf_amd
    z, one = None, C.c_void_p(64)
    for name in ("dsn_mc_normals", "dsn_raster_mesh_attr"):
        assert hasattr(lib, name) and name in dsnerf_amd._lib.EXPORTS
    assert lib.dsn_abi_version() == 8
    ws = lib.dsn_raster_workspace_bytes(3, 1, 8, 8)
    pose = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2.5)
    light = (C.c_float * 4)(30.0, 0.98, 0.87, 0.3)

    def rm(verts=one, nv=3, faces=one, nf=1, p=pose, znear=0.05, lt=light, H=8, W=8, of=one, od=one, oc=one, w=one, nbytes=ws, phases=0,
           big=0, vn=one, vc=one, mode=0, on=one, oa=one):
        return lib.dsn_raster_mesh_attr(verts, nv, faces, nf, p, 1.0, 1.0, znear, lt, H, W, of, od, oc, w, nbytes, phases, big, vn, vc, mode,
                                        on, oa, z)
    cases = [
        (dict(verts=z), b"null"), (dict(faces=z), b"null"), (dict(p=z), b"null"), (dict(lt=z), b"null"), (dict(w=z), b"null"),
        (dict(of=z, od=z, oc=z, on=z, oa=z), b"no output"),
        (dict(H=0), b"16384"), (dict(W=16385), b"16384"), (dict(nv=-1), b"negative"), (dict(nf=1 << 31), b"2^31"),
        (dict(nbytes=ws - 1), b"workspace"), (dict(w=C.c_void_p(72)), b"aligned"), (dict(znear=0.0), b"positive"),
        (dict(phases=32), b"phases"), (dict(big=-1), b"big_pixels"),
        (dict(mode=4), b"mode"), (dict(mode=-1), b"mode"),
        (dict(mode=1, vn=z), b"vertex_normals"), (dict(mode=3, vn=z), b"vertex_normals"), (dict(vc=z), b"vertex_colors"),
    ]
    for kw, msg in cases:
        assert rm(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_raster_mesh" in err and msg in err, (kw, err)

    def mc(vol=one, nx=4, ny=4, nz=4, x=one, y=one, zz=one, level=0.0, direction=0, w=one, nv=5, out=one):
        return lib.dsn_mc_normals(vol, nx, ny, nz, x, y, zz, C.c_float(level), direction, w, C.c_int64(nv), out, z)
    cases = [
        (dict(vol=z), b"null"), (dict(x=z), b"null"), (dict(y=z), b"null"), (dict(zz=z), b"null"), (dict(w=z), b"null"),
        (dict(out=z), b"null output"), (dict(nx=1), b"grid size"), (dict(nz=0), b"grid size"), (dict(nx=2048, ny=2048, nz=512), b"grid size"),
        (dict(level=float("nan")), b"NaN"), (dict(direction=2), b"gradient_direction"), (dict(direction=-1), b"gradient_direction"),
        (dict(nv=-1), b"negative"),
    ]
    for kw, msg in cases:
        assert mc(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_mc_normals" in err and msg in err, (kw, err)
    # no vertices: nothing to do, no buffer needed, the device is not touched
    assert mc(nv=0, out=z) == 0


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------
def read_ply(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:end].decode("ascii").split("\n")[:-1], data[end:]


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_save_ply(tmp_path, with_normals, with_colors):
    from dsnerf_amd.visualizer import save_ply
    rng = np.random.default_rng(3)
    V, T = 7, 5
    verts = rng.standard_normal((V, 3)).astype(F32)
    faces = rng.integers(0, V, (T, 3)).astype(np.int32)
    normals = rng.standard_normal((V, 3)).astype(F32)
    colors = rng.uniform(-0.2, 1.2, (V, 3)).astype(F32)
    colors[0] = [np.nan, 0.5, 1.0]
    mesh = {"verts": verts, "faces": faces.astype(np.int64)}
    if with_normals:
        mesh["normals"] = normals
    path = str(tmp_path / "m.ply")
    save_ply(path, mesh, colors=colors if with_colors else None)
    head, body = read_ply(path)
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + (["red", "green", "blue"] if with_colors else [])
    want = ["ply", "format binary_little_endian 1.0", "element vertex %d" % V]
    want += ["property %s %s" % ("uchar" if p in ("red", "green", "blue") else "float", p) for p in props]
    want += ["element face %d" % T, "property list uchar int vertex_indices", "end_header"]
    assert head == want
    vdt = np.dtype([(p, "u1" if p in ("red", "green", "blue") else "<f4") for p in props])
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert vdt.itemsize == 12 + 12 * with_normals + 3 * with_colors and fdt.itemsize == 13
    assert len(body) == V * vdt.itemsize + T * fdt.itemsize
    vr = np.frombuffer(body[:V * vdt.itemsize], dtype=vdt)
    fr = np.frombuffer(body[V * vdt.itemsize:], dtype=fdt)
    assert np.array_equal(np.stack([vr["x"], vr["y"], vr["z"]], 1).view(np.uint32), verts.view(np.uint32))
    if with_normals:
        assert np.array_equal(np.stack([vr["nx"], vr["ny"], vr["nz"]], 1).view(np.uint32), normals.view(np.uint32))
    if with_colors:
        c = np.where(np.isnan(colors), 0, np.clip(colors.astype(np.float64), 0, 1))
        assert np.array_equal(np.stack([vr["red"], vr["green"], vr["blue"]], 1), np.floor(c * 255 + 0.5).astype(np.uint8))
        assert vr["red"][0] == 0 and vr["green"][0] == 128 and vr["blue"][0] == 255
    assert (fr["n"] == 3).all() and np.array_equal(fr["v"], faces)
    # a tuple, a colour key of the dict, an empty mesh, and rows that do not match
    save_ply(path, (verts, faces, normals) if with_normals else (verts, faces), colors=colors if with_colors else None)
    assert read_ply(path) == (head, body)
    if with_colors:
        save_ply(path, dict(mesh, albedo=colors), colors="albedo")
        assert read_ply(path) == (head, body)
        with pytest.raises(ValueError):
            save_ply(path, mesh, colors="colour")
        with pytest.raises(ValueError):
            save_ply(path, mesh, colors=colors[:-1])
    save_ply(path, (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)))
    head0, body0 = read_ply(path)
    assert "element vertex 0" in head0 and "element face 0" in head0 and body0 == b""


def test_visualizer_docstring_mentions_attributes():
    doc = __import__("dsnerf_amd.visualizer", fromlist=["x"]).__doc__
    assert "geometry only" not in doc and "normals" in doc and "save_ply" in doc
