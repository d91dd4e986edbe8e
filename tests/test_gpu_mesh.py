"""Density grid and iso-surface on the device (dsn_density_grid, dsn_mc_count / dsn_mc_emit, Renderer.density_grid /
extract_mesh, dsnerf_amd.visualizer.Visualizer3D): the density-only split-fp16 kernel against the forward kernel and the exact one,
the grid against dsn_warp + the field kernels and against query_volume(w2l_without_lbs(points)), and the marching cubes bit for bit
against the numpy restatement of include/dsnerf.h's rule (tests/mc_restate.py).  Grids stay below ~5 M points."""
import numpy as np
import pytest
import torch

import mc_restate as M
import oracle as O
from helpers import load, state
from test_gpu_render import make_batch, make_renderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def table():
    from dsnerf_amd import _lib
    return _lib.mc_table()


@pytest.fixture(scope="module")
def body():
    """(case, eval-mode Renderer, batch) by case name, built once per module and dropped with it (a Renderer left alive would keep
    test_gpu_round5's host-pool test from running)"""
    cache = {}

    def get(name):
        if name not in cache:
            g = load(name)
            r = make_renderer(g, name)
            r.eval()
            cache[name] = (g, r, make_batch(g))
        return cache[name]
    yield get
    cache.clear()


def grid_points(axes):
    x, y, z = (np.asarray(a, np.float32) for a in axes)
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    return np.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], 1)


def split_vs_exact(r, x_act):
    """the forward kernel's sigma (NaN where it flags) and the exact kernel's sigma on the same canonical points"""
    from dsnerf_amd import _lib
    packed = r.net.packed(r.device)
    fwd = _lib.field_forward(r.scene, packed, x_act)[0]
    exact = _lib.field(r.scene, packed, x_act, want_essence=False, want_grad=False)[0]
    return fwd, exact


@pytest.mark.parametrize("name,res", [("full_eval_w4", 48), ("small_eval", 32)])
def test_density_grid_against_warp_and_field_kernels(body, name, res):
    from dsnerf_amd import _lib
    g, r, batch = body(name)
    axes, vol = r.density_grid(batch, resolution=res)
    assert vol.shape == tuple(len(a) for a in axes) and vol.numel() < 5_000_000
    pts = torch.from_numpy(grid_points(axes)).to(DEV)
    w = _lib.warp(r.scene, pts, None, 1, want_dir=False)
    tr = w["transparent"].bool()
    v = vol.reshape(-1)
    assert 0.05 < float((~tr).float().mean()) < 0.95
    assert bool((v[tr] == 0).all())
    x_act = w["x_c"][~tr].contiguous()
    fwd, exact = split_vs_exact(r, x_act)
    ok = ~torch.isnan(fwd)
    # the density-only kernel: the forward kernel's bits where that does not flag, the exact kernel's where it does
    assert torch.equal(v[~tr][ok], fwd[ok])
    assert torch.equal(v[~tr][~ok], exact[~ok])
    assert bool(torch.isfinite(v).all())
    # DSN_FIELD_FP32: query_volume(w2l_without_lbs(points)) bit for bit (the reference's chunk loop, one chunk)
    _, vol32 = r.density_grid(batch, axes=axes, fp32=True)
    frame = int(batch["frame"][0])
    pts_can, tmask = r.w2l_without_lbs(pts.reshape(1, -1, 1, 3), batch, r.canonical_model)
    q = r.query_volume(pts_can.reshape(1, -1, 3), torch.tensor([frame]).cuda(), tmask, batch).reshape(-1)
    assert torch.equal(vol32.reshape(-1), q)
    tol = max(1e-4, 4e-6 * float(vol32.abs().max()))
    assert float((vol - vol32).abs().max()) <= tol
    # the oracle (float32 C restatement of the reference's warp and network) on a subset
    sd = state(name)
    P = O.Params(sd)
    code = sd["nerf.embedding.weight"][frame] * (0 if r.net.nerf.w is not None else 1)
    idx = np.arange(0, pts.shape[0], 97)
    wp = O.warp(pts.cpu().numpy()[idx], None, g["xyz"], g["canonical_vertex"], g["faces"])
    osig = O.field(wp["x_c"], P, code, O.pose_feat(g["poses"], P)[1], want_grad=False, want_essence=False)[0]
    osig[wp["transparent"]] = 0
    assert np.array_equal(wp["transparent"], tr.cpu().numpy()[idx])
    assert float(np.abs(v.cpu().numpy()[idx] - osig).max()) < max(1e-4, 4e-6 * float(np.abs(osig).max()))
    # slab sizes: one x-plane, a non-divisor of nx, all planes -> the same bits
    plane = len(axes[1]) * len(axes[2])
    for slab in (plane, 5 * plane + 1, len(axes[0]) * plane):
        assert torch.equal(r.density_grid(batch, axes=axes, slab_points=slab)[1], vol)


def test_density_kernel_outside_the_fp16_range():
    """parameters whose activations leave the fp16 range (test_gpu_round2.overflowing_state): the density-only kernel flags those
    points and the exact kernel re-evaluates them - the grid equals the exact kernel there, the forward kernel elsewhere"""
    from dsnerf_amd import _lib
    from test_gpu_round2 import overflowing_state
    g = load("full_eval")
    sd = overflowing_state("nerf.stage1.4")
    packed = _lib.PackedParams(DEV).update({k: torch.from_numpy(v) for k, v in sd.items()})
    sc = _lib.Scene(torch.from_numpy(g["canonical_vertex"]), torch.from_numpy(g["faces"].astype(np.int64)), DEV)
    sc.set_frame(packed, torch.from_numpy(g["xyz"]), torch.from_numpy(g["poses"]), int(g["frame"]))
    from dsnerf_amd import Renderer
    axes = Renderer.grid_axes(torch.from_numpy(g["xyz"]), 24)
    vol = _lib.density_grid(sc, packed, axes).reshape(-1)
    w = _lib.warp(sc, torch.from_numpy(grid_points(axes)).to(DEV), None, 1, want_dir=False)
    act = ~w["transparent"].bool()
    x_act = w["x_c"][act].contiguous()
    fwd = _lib.field_forward(sc, packed, x_act)[0]
    exact = _lib.field(sc, packed, x_act, want_essence=False, want_grad=False)[0]
    flagged = torch.isnan(fwd)
    assert 0.0 < float(flagged.float().mean()) < 1.0
    assert torch.equal(vol[act][flagged], exact[flagged]) and torch.equal(vol[act][~flagged], fwd[~flagged])
    assert bool((vol[~act] == 0).all()) and bool(torch.isfinite(vol).all())


def gpu_mc(vol, axes, level, direction):
    from dsnerf_amd import _lib
    v, f = _lib.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, np.float32)).to(DEV), axes, level, direction)
    return v.cpu().numpy(), f.cpu().numpy()


def same_as_restatement(vol, axes, level, direction, table):
    v, f = gpu_mc(vol, axes, level, direction)
    rv, rf = M.marching_cubes(vol, axes, level, direction, table)
    assert v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(f, rf)
    return v, f


def test_all_256_cases(table):
    ax = (np.array([0.0, 1.0], np.float32), np.array([-1.0, 0.5], np.float32), np.array([2.0, 2.25], np.float32))
    rng = np.random.default_rng(1)
    for cs in range(256):
        mag = rng.uniform(0.1, 1.0, 8).astype(np.float32)
        vol = np.array([mag[c] if (cs >> c) & 1 else -mag[c] for c in range(8)], np.float32).reshape(2, 2, 2, order="F")
        v, f = same_as_restatement(vol, ax, 0.0, "descent", table)
        assert f.shape[0] == table[cs, 0]


def analytic(n, fn, lo=-1.0, hi=1.0):
    ax = tuple(np.linspace(lo, hi, n + k).astype(np.float32) for k in range(3))      # (three different lengths)
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in ax], indexing="ij")
    return fn(X, Y, Z).astype(np.float32), ax


def test_shapes_noise_levels_and_directions(table, monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")
    vol, ax = analytic(40, lambda x, y, z: 0.7 - np.sqrt(x * x + y * y + z * z))
    v, f = same_as_restatement(vol, ax, 0.0, "descent", table)
    assert M.euler_characteristic(v, f) == 2
    va, fa = same_as_restatement(vol, ax, 0.0, "ascent", table)
    assert np.array_equal(va, v) and np.array_equal(fa, f[:, ::-1])
    vol, ax = analytic(44, lambda x, y, z: 0.25 - np.sqrt((np.sqrt(x * x + y * y) - 0.6) ** 2 + z * z))
    v, f = same_as_restatement(vol, ax, 0.0, "ascent", table)
    assert M.euler_characteristic(v, f) == 0
    rng = np.random.default_rng(3)
    noise = rng.standard_normal((23, 17, 29)).astype(np.float32)
    ax = tuple(np.cumsum(rng.uniform(0.5, 1.5, s)).astype(np.float32) for s in noise.shape)
    same_as_restatement(noise, ax, 0.1, "descent", table)
    # a level equal to grid values (integers): equal counts as outside
    ints = rng.integers(0, 4, (15, 16, 17)).astype(np.float32)
    ax = tuple(np.arange(s, dtype=np.float32) for s in ints.shape)
    for level in (1.0, 2.0):
        same_as_restatement(ints, ax, level, "descent", table)
    # NaN is outside
    nan = noise.copy()
    nan[nan < -1.5] = np.nan
    rv, rf = M.marching_cubes(nan, tuple(np.arange(s, dtype=np.float32) for s in nan.shape), 0.5, "descent", table)
    v, f = gpu_mc(nan, tuple(np.arange(s, dtype=np.float32) for s in nan.shape), 0.5, "descent")
    assert np.array_equal(f, rf) and v.shape == rv.shape
    # all inside / all outside: nothing
    for const in (1.0, -1.0):
        v, f = gpu_mc(np.full((5, 6, 7), const, np.float32), tuple(np.arange(s, dtype=np.float32) for s in (5, 6, 7)), 0.0, "ascent")
        assert v.shape == (0, 3) and f.shape == (0, 3)
    # repeated calls: the same bits
    a = gpu_mc(noise, tuple(np.arange(s, dtype=np.float32) for s in noise.shape), 0.0, "descent")
    b = gpu_mc(noise, tuple(np.arange(s, dtype=np.float32) for s in noise.shape), 0.0, "descent")
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def test_extract_mesh_of_the_w4_body(body, table, monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")
    from dsnerf_amd import _lib
    g, r, batch = body("full_eval_w4")
    # (the first eval frame of a parameter version is early stop's probe frame, rendered in one pass; the frames after it follow
    #  the plan it made: compare two of those)
    r.render(batch)
    before = {k: v.clone() for k, v in r.render(batch)["coarse"].items() if torch.is_tensor(v)}
    axes, vol = r.density_grid(batch, resolution=64)
    m = r.extract_mesh(batch, 64, level=0.5, gradient_direction="ascent")
    after = {k: v for k, v in r.render(batch)["coarse"].items() if torch.is_tensor(v)}
    for k in before:      # the render path is untouched (bit patterns: disp is NaN where acc is 0)
        assert torch.equal(before[k].contiguous().view(torch.int32), after[k].contiguous().view(torch.int32)), k
    assert m is not None and m["faces"].dtype == torch.int32 and m["faces"].shape[0] > 1000
    v, f = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    rv, rf = M.marching_cubes(vol.cpu().numpy(), axes, 0.5, "ascent", table)
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)) and np.array_equal(f, rf)
    # boundary edges (a directed edge without its reverse) only where the surface meets the grid's outer faces
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key = set((de[:, 0] * (1 << 32) + de[:, 1]).tolist())
    open_e = [e for e in de if (e[1] * (1 << 32) + e[0]) not in key]
    ax32 = [np.asarray(a, np.float32) for a in axes]
    on_border = lambda p: any(p[d] in (ax32[d][0], ax32[d][-1]) for d in range(3))
    assert all(on_border(v[a]) and on_border(v[b]) for a, b in open_e)
    # a level above every density: None
    assert r.extract_mesh(batch, 16, level=float(vol.max()) + 1.0) is None


def test_visualizer_matches_the_reference_chunk_loop(body):
    from dsnerf_amd.visualizer import Visualizer3D
    g, r, batch = body("full_eval_w4")
    vis = Visualizer3D(40, 256, 0.5, "ascent")
    torch.manual_seed(11)
    grid_pts, grid_pred = vis.get_grid_pred_batch(r, batch["xyz"], batch)
    # the reference's loop (utils/visualizer.py:35-110) on the same renderer
    torch.manual_seed(11)
    grid = vis.get_grid(batch["xyz"][0])
    code_idx = torch.randperm(300)[:1]
    pts = grid["grid_pts"][None]
    pts_smpl_can, tmask = r.w2l_without_lbs(pts.unsqueeze(-2).cuda(), batch, r.canonical_model)
    pts_smpl_can = pts_smpl_can.unsqueeze(0)
    both = torch.cat([pts.cuda(), pts_smpl_can], dim=-1)
    pred = np.concatenate([r.query_volume(both[:, i:i + 100000], code_idx.cuda(), tmask[:, i:i + 100000], batch).cpu().numpy()
                           for i in range(0, pts.shape[1], 100000)], axis=1)
    X, Y, Z = (len(a) for a in grid["xyz"])
    assert grid_pts.shape == (1, X, Y, Z, 3) and grid_pred.shape == (1, X, Y, Z, 1)
    assert np.array_equal(grid_pts, pts.reshape(1, X, Y, Z, 3).numpy())
    ref = pred.reshape(1, X, Y, Z, 1)
    assert np.array_equal(ref == 0, grid_pred == 0)
    assert float(np.abs(ref - grid_pred).max()) <= max(1e-4, 4e-6 * float(np.abs(ref).max()))
    mesh = vis.get_mesh_from_grid(grid_pts[0], grid_pred[0])
    assert mesh is not None and mesh[1].shape[1] == 3
    with pytest.raises(NotImplementedError):
        Visualizer3D(40, 256, 0.5, "ascent", connected=True).get_mesh_from_grid(grid_pts, grid_pred)
