"""GPU: clear cells - fine cells every sample of which is transparent whichever face is nearest (csrc/dsn_nn.hip).

The lazy list build of a fused eval frame flags a visited cell when every member of its candidate list puts the whole guarded box
outside |h| <= 0.1, u in [-4, 5] or v in [-4, 5] (dsn_face_clears_box); such a cell gets an empty list and k_nns_search<true> writes
transparent = 1, x_c = 0 for its samples without a scan.  Nothing a frame computes may change: every test compares with
DSN_NN_NO_CLEAR_CELLS=1 (no flags) and with DSN_NN_EXHAUSTIVE bit for bit, and reads the flags back from the scene blob."""
import warnings

import numpy as np
import pytest
import torch

import nn_cases as N
from helpers import state
from test_gpu_nns_block import a256, geometry, read_fine_lists, read_geometry, same_geometry
from test_gpu_round2 import full_frame, renderer_with

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FINE_MAXCELL = 65536           # = DSN_NN_FINE_MAXCELL (csrc/dsn_nn.h)
SUPER_CAP = 4096               # = DSN_SUPER_CAP
OUT_KEYS = ("color", "disp_map", "acc_map", "depth_map", "weights", "z_vals")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fine_arrays(scene):
    """(header, U(B)^2 per cell, clear flag per cell) of the posed mesh's fine level (layout of dsn_grid_view, csrc/dsn_nn.h)"""
    M = FINE_MAXCELL
    o = scene._nn_off[N.LEVELS.index("world_fine")]
    h = N.read_header(scene, "world_fine")
    cap = min(max(2000 * scene.F, 1 << 20), 0x7fffff00)          # = dsn_nn_fine_cap(F): the array's size, whatever the logical capacity
    o_u2 = o + 256 + a256(4 * (M + 1))
    o_clear = o_u2 + a256(4 * M) + a256(16 * cap) + a256(4 * M) + a256(16 * (M // 32) * SUPER_CAP) + a256(8 * (SUPER_CAP // 64) * M)
    u2 = scene.buf[o_u2:o_u2 + 4 * h["ncell"]].view(torch.float32).cpu().numpy().copy()
    clear = scene.buf[o_clear:o_clear + h["ncell"]].cpu().numpy().copy()
    return h, u2, clear


def _cell_boxes(h, cells):
    """the guarded boxes of the given cells, float32 step for step as dsn_cell_box"""
    n = h["n"].astype(np.int64)
    cells = np.asarray(cells, np.int64)
    idx = np.stack([cells // (n[2] * n[1]), (cells // n[2]) % n[1], cells % n[2]], 1)
    lo = (h["lo"][None, :] + idx.astype(np.float32) * h["cell"]).astype(np.float32) - N.GRID_GUARD
    hi = (h["lo"][None, :] + (idx + 1).astype(np.float32) * h["cell"]).astype(np.float32) + N.GRID_GUARD
    return idx, lo.astype(np.float32), hi.astype(np.float32)


def _box_points(lo, hi, rng, n_inner=8):
    """per box: its 8 corners, its 6 face centres and n_inner seeded interior points -> [boxes, 14 + n_inner, 3] float32"""
    c = (0.5 * (lo.astype(np.float64) + hi)).astype(np.float32)
    pts = []
    for bits in range(8):
        pts.append(np.where([(bits >> a) & 1 for a in range(3)], hi, lo))
    for a in range(3):
        for side in (lo, hi):
            p = c.copy()
            p[:, a] = side[:, a]
            pts.append(p)
    for _ in range(n_inner):
        t = rng.uniform(0.0, 1.0, lo.shape)
        pts.append((lo + t * (hi.astype(np.float64) - lo)).astype(np.float32))
    out = np.stack(pts, 1).astype(np.float32)
    return np.minimum(np.maximum(out, lo[:, None, :]), hi[:, None, :])


def _frame(kind, hw=256):
    """(renderer, batch, case or None) of one of the three bodies: the uniform lattice, the SMPL-like one, the twinned lattice"""
    nonuniform = kind == "smpl"
    canon, faces, batch = full_frame(hw=hw, nonuniform=nonuniform)
    case = None
    if kind == "twin":
        case = N.twin_case(False, "orig")
        batch["xyz"] = torch.from_numpy(case["xyz"])[None]
        canon, faces = case["canon"], case["faces"]
    r = renderer_with(state("x_w4"), canon, faces, density_screen=False)
    r.eval()
    return r, batch, case


def _inputs(r, batch):
    return r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0]), r._dev(batch["near"][0]), r._dev(batch["far"][0])


def _same_outputs(a, b, what):
    for k in OUT_KEYS:
        assert torch.equal(torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0)), (what, k)


def _three_forms(r, batch, S, monkeypatch, what):
    """one lazily set eval frame with the flags, with DSN_NN_NO_CLEAR_CELLS=1 and through the exhaustive sweep: geometry (transparent,
    x_c, the active list as a set) and every rendered output bit for bit.  Returns (flags, samples per cell, header, the flagged run's
    geometry, the points, the lists of the run without flags)"""
    from dsnerf_amd import _lib
    o, d, near, far = _inputs(r, batch)
    pk = r.net.packed(r.device)
    R = o.shape[0]

    def run(lazy, **kw):
        r._set_frame(batch, lazy=lazy)
        ws, z = geometry(r.scene, pk, o, d, near, far, S, **kw)
        geo = read_geometry(ws, R, S)
        hdr, u2, clear = _fine_arrays(r.scene)
        lists = read_fine_lists(r.scene) if lazy else None
        r._set_frame(batch, lazy=lazy)
        out = _lib.render_rays(r.scene, pk, _lib.RenderWorkspace(r.device), o, d, near.clone(), far.clone(), S, r._t_vals(S), screen=False, **kw)
        torch.cuda.synchronize()
        assert r.scene.nn_overflow == {}
        return geo, z, out, hdr, u2, clear, lists

    on = run(True)
    assert on[3]["lazy"] == 2 and on[3]["total"] <= on[3]["cap"], on[3]
    monkeypatch.setenv("DSN_NN_NO_CLEAR_CELLS", "1")
    off = run(True)
    monkeypatch.delenv("DSN_NN_NO_CLEAR_CELLS")
    ref = run(False, exhaustive=True)
    assert ref[0]["active"].size > 100000
    for name, got in (("flags", on), ("no flags", off)):
        same_geometry(got[0], ref[0], (what, name))
        _same_outputs(got[2], ref[2], (what, name))
    assert torch.equal(on[1], ref[1])
    pts = (o[:, None, :] + d[:, None, :] * ref[1][..., None]).reshape(-1, 3).cpu().numpy()
    hdr, u2, clear = on[3], on[4], on[5]
    cell = N.cell_of(hdr, pts)
    per_cell = np.bincount(cell[cell >= 0], minlength=hdr["ncell"])
    visited = per_cell > 0
    flagged = (clear == 1) & visited
    n_in = int(per_cell[flagged].sum())
    tr_all = int(ref[0]["transparent"].sum())
    print(f"{what}: {int(flagged.sum())} of {int(visited.sum())} visited cells flagged, {n_in} of {pts.shape[0]} samples "
          f"({n_in / pts.shape[0]:.3f}) in them ({tr_all / pts.shape[0]:.3f} of the samples are transparent); list entries "
          f"{off[3]['total']} -> {on[3]['total']}; smallest U(B)^2 of a flagged cell {u2[flagged].min() if flagged.any() else float('nan'):.5f}")
    assert n_in > 0, "no flagged cell holds a sample: the comparison proves nothing"
    assert set(np.unique(clear[visited]).tolist()) <= {0, 1}
    assert (clear[~visited] == 0).all()          # (a clear build writes every cell's byte, from 0xFF-filled memory too: pins _fine_arrays' offset)
    # every sample of a flagged cell is transparent, a flagged cell has no list, every other visited cell the list it has without flags
    assert ref[0]["transparent"][np.isin(cell, np.nonzero(flagged)[0])].all()
    len_on, len_off = np.diff(on[6][1]), np.diff(off[6][1])
    assert (len_on[flagged] == 0).all() and np.array_equal(len_on[~flagged], len_off[~flagged])
    keep = np.repeat(~flagged, len_off)
    assert np.array_equal(on[6][2], off[6][2][keep])
    return flagged, per_cell, hdr, on[0], pts, off[6]


# ---------------------------------------------------------------------------------------------------------------------------
# whole frames
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "smpl", "twin"])
def test_frames_with_clear_cells_equal_the_frames_without_and_the_sweep(kind, monkeypatch):
    """256 x 256 x 64 lazily set eval frames of the lattice body (from scene and workspace memory filled with 0xFF), the SMPL-like body
    and the twinned lattice body: transparent, x_c, the active set and every rendered output with the flags == without == exhaustive"""
    if kind == "lattice":
        monkeypatch.setenv("DSN_POISON_SCRATCH", "1")
    r, batch, _ = _frame(kind)
    _three_forms(r, batch, 64, monkeypatch, kind)


# ---------------------------------------------------------------------------------------------------------------------------
# the flags themselves: the boxes of flagged cells, and the cells next to them
# ---------------------------------------------------------------------------------------------------------------------------
def _flags_of_a_frame():
    """the flags a 256 x 256 x 64 lazily set eval frame of the lattice body leaves, and the renderer that holds the frame (not kept
    between tests: a Renderer that stays alive changes what later tests of the suite see)"""
    r, batch, _ = _frame("lattice")
    o, d, near, far = _inputs(r, batch)
    pk = r.net.packed(r.device)
    r._set_frame(batch, lazy=True)
    ws, z = geometry(r.scene, pk, o, d, near, far, 64)
    hdr, u2, clear = _fine_arrays(r.scene)
    assert hdr["lazy"] == 2
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).cpu().numpy()
    cell = N.cell_of(hdr, pts)
    visited = np.bincount(cell[cell >= 0], minlength=hdr["ncell"]) > 0
    return r, batch, pk, hdr, (clear == 1) & visited, visited


def test_every_point_of_a_flagged_box_is_transparent_through_the_sweep():
    """at least 256 flagged cells spread over the grid: the 8 corners of the guarded box, its 6 face centres and 8 seeded interior
    points go through dsn_warp on a fully built scene with the exhaustive sweep - every one comes back transparent"""
    from dsnerf_amd import _lib
    r, batch, pk, hdr, flagged, visited = _flags_of_a_frame()
    cells = np.nonzero(flagged)[0]
    assert cells.size >= 256, cells.size
    cells = cells[np.unique(np.linspace(0, cells.size - 1, 600).astype(np.int64))]
    idx, lo, hi = _cell_boxes(hdr, cells)
    assert (np.ptp(idx, 0) >= np.array(hdr["n"]) // 2).all(), (np.ptp(idx, 0), hdr["n"])          # spread over the grid
    pts = _box_points(lo, hi, np.random.default_rng(5)).reshape(-1, 3)
    r._set_frame(batch, lazy=False)
    w = _lib.warp(r.scene, T(pts), None, 1, want_dir=False, want_uvh=True, exhaustive=True)
    tr = w["transparent"].cpu().numpy().astype(bool)
    bad = np.nonzero(~tr)[0]
    print(f"{cells.size} flagged cells, {pts.shape[0]} points on and in their guarded boxes, {bad.size} not transparent")
    assert bad.size == 0, (cells[bad[:8] // 22], pts[bad[:8]], [w[k].cpu().numpy()[bad[:8]] for k in ("u", "v", "h") if k in w])


def test_cells_next_to_flagged_ones_take_the_scan_and_equal_the_sweep(monkeypatch):
    """unflagged visited cells that share a face with a flagged one, and the flagged ones beside them: the same corner / face-centre /
    interior points as samples of a small lazily set batch (DSN_CELLMAJOR_MIN=1: the fused search) against the exhaustive sweep bit for
    bit.  The neighbours' points need not be transparent, those inside flagged cells are."""
    r, batch, pk, hdr, flagged, visited = _flags_of_a_frame()
    n = [int(x) for x in hdr["n"]]
    f3 = flagged.reshape(n)
    near_flag = np.zeros_like(f3)
    for a in range(3):
        sl_lo, sl_hi = [slice(None)] * 3, [slice(None)] * 3
        sl_lo[a], sl_hi[a] = slice(0, -1), slice(1, None)
        near_flag[tuple(sl_lo)] |= f3[tuple(sl_hi)]
        near_flag[tuple(sl_hi)] |= f3[tuple(sl_lo)]
    nb = np.nonzero(near_flag.reshape(-1) & visited & ~flagged)[0]
    assert nb.size >= 256, nb.size
    nb = nb[np.unique(np.linspace(0, nb.size - 1, 400).astype(np.int64))]
    fl = np.nonzero(flagged)[0]
    fl = fl[np.unique(np.linspace(0, fl.size - 1, 200).astype(np.int64))]
    cells = np.concatenate([nb, fl])
    _, lo, hi = _cell_boxes(hdr, cells)
    # (interior points only as SAMPLES: a corner of the guarded box classifies into a neighbouring cell - pulled 2 guard bands inside)
    g = 2 * N.GRID_GUARD
    pts = _box_points(lo + g, hi - g, np.random.default_rng(6))
    own = np.repeat(cells, pts.shape[1])
    pts = pts.reshape(-1, 3)
    assert np.array_equal(N.cell_of(hdr, pts), own)
    # one ray per point, every one of its S samples AT the point: o = p - d, near = far = 1 (uniform sampling)
    S = 4
    rng = np.random.default_rng(7)
    dirs = rng.standard_normal(pts.shape)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * 1e-3).astype(np.float32)
    o, d = T((pts - dirs).astype(np.float32)), T(dirs)
    near = far = T(np.ones(pts.shape[0], np.float32))
    R = pts.shape[0]
    monkeypatch.setenv("DSN_CELLMAJOR_MIN", "1")
    r._set_frame(batch, lazy=True)
    ws, z = geometry(r.scene, pk, o, d, near, far, S, uniform=True)
    got = read_geometry(ws, R, S)
    hdr2, _, clear2 = _fine_arrays(r.scene)
    assert hdr2["lazy"] == 2
    p2 = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).cpu().numpy()
    c2 = N.cell_of(hdr2, p2)
    assert np.isin(c2, cells).mean() > 0.99                      # (o + d rounds: a few land across a wall, still compared)
    assert (clear2[fl] == 1).all() and (clear2[nb] == 0).all()   # the flag is the cell's, whichever rays visit it
    r._set_frame(batch, lazy=False)
    ref_ws, z_ref = geometry(r.scene, pk, o, d, near, far, S, uniform=True, exhaustive=True)
    assert torch.equal(z, z_ref)
    ref = read_geometry(ref_ws, R, S)
    same_geometry(got, ref, "cells next to flagged ones")
    in_fl, in_nb = np.isin(c2, fl), np.isin(c2, nb)
    print(f"{nb.size} unflagged neighbours, {fl.size} flagged cells; non-transparent samples: {int((ref['transparent'][in_nb] == 0).sum())} of "
          f"{int(in_nb.sum())} in the neighbours, {int((ref['transparent'][in_fl] == 0).sum())} of {int(in_fl.sum())} in flagged cells")
    assert ref["transparent"][in_fl].all()


# ---------------------------------------------------------------------------------------------------------------------------
# degenerate faces among the members
# ---------------------------------------------------------------------------------------------------------------------------
def test_zero_area_and_sliver_faces_among_the_members(monkeypatch):
    """the lattice body + a zero-area face (n, u, v, h are NaN: its samples are NOT transparent), a sliver whose 1 / det is beyond the
    bound of the u / v margins and a milder one within it, all 6 cm off the body where far cells have them as candidates: frames
    equal the exhaustive form, and no cell whose list holds the zero-area face is flagged"""
    canon, faces, batch = full_frame(hw=256)
    faces = np.asarray(faces, np.int64)
    xyz = batch["xyz"][0].numpy()
    V = xyz.shape[0]
    top = int(np.argmax(xyz[:, 2]))
    side = int(np.argmax(xyz[:, 0]))
    front = int(np.argmax(xyz[:, 1]))
    new_x = np.array([xyz[top] + [0, 0, 0.06]] * 3 +                                                        # zero area
                     [xyz[side] + [0.06, 0, 0], xyz[side] + [0.06, 0.02, 0], xyz[side] + [0.06, 0.04, 1e-7]] +    # det ~ 4e-18
                     [xyz[front] + [0, 0.06, 0], xyz[front] + [0.02, 0.06, 0], xyz[front] + [0.04, 0.06, 1e-4]],   # det ~ 4e-12
                    np.float32)
    new_c = np.concatenate([canon[[top] * 3], canon[[side] * 3] + new_x[3:6] - xyz[side], canon[[front] * 3] + new_x[6:9] - xyz[front]])
    F0 = faces.shape[0]
    faces2 = np.concatenate([faces, V + np.arange(9).reshape(3, 3)])
    batch["xyz"] = torch.from_numpy(np.concatenate([xyz, new_x]).astype(np.float32))[None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = renderer_with(state("x_w4"), np.concatenate([canon, new_c]).astype(np.float32), faces2, density_screen=False)
    r.eval()
    flagged, per_cell, hdr, geo, pts, (h_off, off, ids) = _three_forms(r, batch, 64, monkeypatch, "degenerate faces")
    entry_cell = np.repeat(np.arange(hdr["ncell"]), np.diff(off))
    holds = lambda f: np.bincount(entry_cell[ids == f], minlength=hdr["ncell"]) > 0
    zero, sliver, mild = holds(F0), holds(F0 + 1), holds(F0 + 2)
    print(f"cells whose list holds the zero-area face: {int(zero.sum())} ({int((zero & flagged).sum())} flagged), the sliver: "
          f"{int(sliver.sum())} ({int((sliver & flagged).sum())} flagged), the milder sliver: {int(mild.sum())} ({int((mild & flagged).sum())} flagged)")
    assert zero.sum() >= 8 and sliver.sum() >= 8 and mild.sum() >= 8
    assert not (zero & flagged).any()
    # the zero-area face is the nearest one of some samples, and they are not transparent (NaN compares false)
    cell = N.cell_of(hdr, pts)
    assert (geo["transparent"][np.isin(cell, np.nonzero(zero)[0])] == 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# every other build and call keeps its lists
# ---------------------------------------------------------------------------------------------------------------------------
def test_full_and_completing_builds_and_a_training_batch_are_untouched(monkeypatch):
    """offsets and lists of a build of every cell (set_frame) and of a completing build (a lazily set frame rendered through the
    exhaustive form, after a fused eval frame left flags and empty lists behind) are entry for entry those without the flag pass
    (DSN_NN_NO_CLEAR_CELLS=1) and those of the fill pass that sweeps again (DSN_NN_NO_MEMBER=1); a lazily set training batch's fused
    search builds the list of every cell it visits and gives the outputs of the exhaustive search"""
    from dsnerf_amd import _lib
    from test_gpu_round6 import _fine_level_lists
    r, batch, _ = _frame("lattice")
    o, d, near, far = _inputs(r, batch)
    pk = r.net.packed(r.device)
    S = 64

    def full():
        r._set_frame(batch, lazy=False)
        torch.cuda.synchronize()
        return _fine_level_lists(r.scene)

    def completed():
        r._set_frame(batch, lazy=True)
        geometry(r.scene, pk, o, d, near, far, S)                         # fused eval frame: flags, empty lists of clear cells
        assert N.read_header(r.scene, "world_fine")["lazy"] == 2
        geometry(r.scene, pk, o[:4096], d[:4096], near[:4096], far[:4096], S, exhaustive=True)      # completes the level
        return _fine_level_lists(r.scene)

    sel = torch.linspace(0, o.shape[0] - 1, 8192, device=DEV).long()
    noise = torch.randn(8192, S, generator=torch.Generator().manual_seed(11)).to(DEV)

    def train(**kw):
        r._set_frame(batch, lazy=True)
        out = _lib.render_rays(r.scene, pk, _lib.RenderWorkspace(DEV), o[sel].contiguous(), d[sel].contiguous(), near[sel].clone(),
                               far[sel].clone(), S, r._t_vals(S), None, noise, skip_transparent=False, train_cache=_lib.GradWorkspace(DEV), **kw)
        torch.cuda.synchronize()
        return {k: out[k].clone() for k in ("color", "acc_map", "depth_map", "weights", "z_vals")}, N.read_header(r.scene, "world_fine")

    # (a build of every cell never consults DSN_NN_NO_CLEAR_CELLS: under that switch "full" compares the build with itself and only says
    #  that nothing else moved; what the switch can change is "completed" and the training batch, and DSN_NN_NO_MEMBER changes both builds)
    base = {"full": full(), "completed": completed()}
    t_on, h_on = train()
    for env in ("DSN_NN_NO_CLEAR_CELLS", "DSN_NN_NO_MEMBER"):
        monkeypatch.setenv(env, "1")
        other = {"full": full(), "completed": completed()}
        t_off, h_off = train()
        monkeypatch.delenv(env)
        for name in base:
            (nc_a, ok_a, lz_a, tot_a, offs_a, ent_a), (nc_b, ok_b, lz_b, tot_b, offs_b, ent_b) = base[name], other[name]
            assert (nc_a, ok_a, lz_a, tot_a) == (nc_b, ok_b, lz_b, tot_b) and ok_a == 1 and lz_a == 0 and tot_a > 100000, (env, name)
            assert torch.equal(offs_a, offs_b) and torch.equal(ent_a, ent_b), (env, name)
        assert h_on["lazy"] == 2 and h_on["total"] == h_off["total"] > 0, (env, h_on, h_off)
        for k in t_on:
            assert torch.equal(torch.nan_to_num(t_on[k], nan=-1.0), torch.nan_to_num(t_off[k], nan=-1.0)), (env, k)
    assert torch.equal(base["full"][4], base["completed"][4]) and torch.equal(base["full"][5], base["completed"][5])
    t_ref, _ = train(exhaustive=True)
    for k in t_on:
        assert torch.equal(torch.nan_to_num(t_on[k], nan=-1.0), torch.nan_to_num(t_ref[k], nan=-1.0)), k
