"""Marching-cubes vertex normals on the device (dsn_mc_normals, _lib.marching_cubes(want_normals=True), Renderer.extract_mesh(normals=True),
Visualizer3D.get_mesh_from_grid(return_normals=True)) bit for bit against the numpy restatement of include/dsnerf.h's rule
(tests/mc_normals_restate.py).  The whole module runs with poisoned scratch."""
import numpy as np
import pytest
import torch

import mc_normals_restate as N
import mc_restate as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def poisoned_scratch(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


@pytest.fixture(scope="module")
def table():
    from dsnerf_amd import _lib
    return _lib.mc_table()


def gpu(vol, axes, level, direction):
    from dsnerf_amd import _lib
    t = torch.from_numpy(np.ascontiguousarray(vol, np.float32)).to(DEV)
    plain = _lib.marching_cubes(t, axes, level, direction)
    out = _lib.marching_cubes(t, axes, level, direction, want_normals=True)
    assert len(plain) == 2 and len(out) == 3
    for a, b in zip(plain, out):      # asking for normals changes neither verts nor faces (bits: a vertex beside a NaN value is NaN)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    return tuple(a.cpu().numpy() for a in out)


def same_as_restatement(vol, axes, level, direction, table):
    v, f, n = gpu(vol, axes, level, direction)
    rv, rf = M.marching_cubes(vol, axes, level, direction, table)
    rn = N.normals(vol, axes, level, direction)
    assert np.array_equal(f, rf) and v.shape == rv.shape
    assert n.shape == rn.shape == v.shape and n.dtype == np.float32
    assert np.array_equal(n.view(np.uint32), rn.view(np.uint32)), int((n.view(np.uint32) != rn.view(np.uint32)).any(axis=1).sum())
    return v, f, n


def sphere24():
    ax = tuple(np.arange(24, dtype=np.float32) for _ in range(3))
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in ax], indexing="ij")
    c = np.array([11.3, 11.7, 12.1])
    return (8.0 - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)).astype(np.float32), ax, c


def test_all_256_cases_in_one_volume(table):
    """cube c of the batch volume [512, 2, 2] holds case c (x-planes 2 c and 2 c + 1), non-uniform axes"""
    rng = np.random.default_rng(1)
    vol = np.zeros((512, 2, 2), np.float32)
    for cs in range(256):
        mag = rng.uniform(0.1, 1.0, 8).astype(np.float32)
        vol[2 * cs:2 * cs + 2] = np.array([mag[c] if (cs >> c) & 1 else -mag[c] for c in range(8)], np.float32).reshape(2, 2, 2, order="F")
    ax = (np.cumsum(rng.uniform(0.5, 1.5, 512)).astype(np.float32), np.array([-1.0, 0.5], np.float32), np.array([2.0, 2.25], np.float32))
    for direction in ("descent", "ascent"):
        v, f, n = same_as_restatement(vol, ax, 0.0, direction, table)
        assert v.shape[0] > 1000 and f.shape[0] >= int(table[:, 0].sum())
        ln = np.linalg.norm(n.astype(np.float64), axis=1)
        assert np.abs(ln - 1).max() < 1e-6


def test_sphere_both_directions(table):
    vol, ax, c = sphere24()
    v, f, n = same_as_restatement(vol, ax, 0.0, "descent", table)
    va, fa, na = same_as_restatement(vol, ax, 0.0, "ascent", table)
    assert np.array_equal(na.view(np.uint32), (-n).view(np.uint32))
    radial = (v - c) / np.linalg.norm(v - c, axis=1, keepdims=True)
    assert np.degrees(np.arccos(np.clip((n * radial).sum(1), -1, 1))).max() < 1.0
    # the triangle orientation of either mode agrees with its normals
    for vv, ff, nn in ((v, f, n), (va, fa, na)):
        g = np.cross(vv[ff[:, 1]] - vv[ff[:, 0]], vv[ff[:, 2]] - vv[ff[:, 0]])
        assert ((g * nn[ff].sum(axis=1)).sum(axis=1) > 0).all()


def test_odd_grid_nonuniform_axes_nan_and_small_grids(table):
    rng = np.random.default_rng(7)
    ax = tuple(np.cumsum(rng.uniform(0.5, 1.5, s)).astype(np.float32) for s in (17, 9, 5))
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in ax], indexing="ij")
    vol = (np.sin(0.5 * X) + 0.3 * Y - 0.2 * Z * Z + 0.4).astype(np.float32)      # leaves through every face of the grid
    for direction in ("descent", "ascent"):
        v, f, n = same_as_restatement(vol, ax, 1.0, direction, table)
        assert v.shape[0] > 50
    border = np.zeros(v.shape[0], bool)
    for d in range(3):
        border |= (v[:, d] == ax[d][0]) | (v[:, d] == ax[d][-1])
    assert border.sum() > 10                                                       # the one-sided forms are in use
    # NaN among the values: outside for the surface, zero normals where a gradient reads one
    noise = rng.standard_normal((23, 17, 29)).astype(np.float32)
    noise[noise < -1.5] = np.nan
    axn = tuple(np.arange(s, dtype=np.float32) for s in noise.shape)
    v, f, n = same_as_restatement(noise, axn, 0.5, "descent", table)
    zero = (n == 0).all(axis=1)
    assert 0 < zero.sum() < n.shape[0] and np.isfinite(n).all()
    assert np.abs(np.linalg.norm(n[~zero].astype(np.float64), axis=1) - 1).max() < 1e-6
    # infinities
    inf = noise.copy()
    inf[np.isnan(inf)] = np.inf
    same_as_restatement(inf, axn, 0.5, "ascent", table)
    # a 2 x 2 x 2 grid: every gradient is one-sided
    cube = np.array([1, -1, -1, -1, -1, -1, -1, 2], np.float32).reshape(2, 2, 2)
    v, f, n = same_as_restatement(cube, tuple(np.array([0.0, 0.5], np.float32) for _ in range(3)), 0.0, "descent", table)
    assert v.shape[0] == 6
    # a level that is not crossed: no vertices, no launch, no fault
    for const in (1.0, -1.0):
        v, f, n = gpu(np.full((5, 6, 7), const, np.float32), tuple(np.arange(s, dtype=np.float32) for s in (5, 6, 7)), 0.0, "ascent")
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    # repeated calls: the same bits
    a = gpu(noise, axn, 0.0, "descent")
    b = gpu(noise, axn, 0.0, "descent")
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def test_several_tiles(table):
    """more grid points than one count tile (4096) and one block hold, sizes off every tile"""
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((37, 41, 19)).astype(np.float32)
    ax = tuple(np.cumsum(rng.uniform(0.5, 1.5, s)).astype(np.float32) for s in noise.shape)
    v, f, n = same_as_restatement(noise, ax, 0.1, "ascent", table)
    assert v.shape[0] > 20000


def test_visualizer_returns_normals(table):
    from dsnerf_amd.visualizer import Visualizer3D
    vol, ax, c = sphere24()
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    pts = np.stack([X, Y, Z], axis=-1)
    vis = Visualizer3D(24, 64, 0.0, "descent")
    pair = vis.get_mesh_from_grid(pts, vol[..., None])
    v, f, n = vis.get_mesh_from_grid(pts, vol[..., None], return_normals=True)
    assert len(pair) == 2 and np.array_equal(pair[0], v) and np.array_equal(pair[1], f)
    assert isinstance(n, np.ndarray) and np.array_equal(n.view(np.uint32), N.normals(vol, ax, 0.0, "descent").view(np.uint32))
    assert Visualizer3D(24, 64, 100.0, "descent").get_mesh_from_grid(pts, vol[..., None], return_normals=True) is None
