"""GPU: the block-deferred winner of the nearest-centroid scans (DsnBlk, csrc/dsn_nn.h) against the exhaustive search.

k_nns_search (survivors in LDS, drained in rounds; the unpruned scalar-load path of lists under 96 entries; the coarse path with its
one-sample-per-lane form), k_nns_search_far and the brute-force tile scan resolve the winning index per block of eight list entries
instead of per candidate.  The index must stay the serial strict-'<' scan's, ties included (tests/test_nns_block_rule_host.py pins the
rule itself).  Here every path runs on bodies with duplicated faces - a tie wherever a twinned face is nearest - and what the search
leaves behind (face index where the path stores one, transparency, canonical point, the active list as a set) is compared bit for
bit with DSN_NN_EXHAUSTIVE, whose own indices are compared with the oracle's float32 restatement."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import oracle as O
import nn_cases as N
from helpers import state
from test_gpu_round2 import full_frame, renderer_with

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK = 8                      # = DSN_NN_BLOCK (csrc/dsn_nn.h)
SURVIVORS = 320                # = NNS_SURVIVORS (csrc/dsn_nn.hip)
FINE_MAXCELL = 65536           # = DSN_NN_FINE_MAXCELL


def a256(b):
    return (b + 255) // 256 * 256


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _packed():
    from dsnerf_amd import _lib
    return _lib.PackedParams(DEV).update({k: torch.from_numpy(v) for k, v in state().items()})


def read_geometry(ws, R, S, with_nn=False):
    """what a frame's geometry phase left in its workspace (layout of dsn_carve, csrc/dsn_api.hip): the active list as a sorted array,
    transparent [N], x_c [N, 3] and - DSN_NN_UNFUSED - the face index k_nns_search<false> wrote for every sample inside the fine grid"""
    from dsnerf_amd import _lib
    n = R * S
    b = ws.buf
    cnt = int(b[:4].view(torch.int32)[_lib.CNT_ACTIVE])
    o = _lib.CNT_BYTES
    act = np.sort(b[o:o + 4 * n].view(torch.int32)[:cnt].cpu().numpy())
    o += a256(4 * n)
    tr = b[o:o + n].cpu().numpy().copy()
    o += a256(n) + a256(4 * n)                       # (transparent, z)
    xc = b[o:o + 12 * n].view(torch.float32).reshape(n, 3).cpu().numpy().copy()
    o += a256(12 * n) + a256(4 * n)                  # (x_c, sigma): G begins here, the unfused search's nn[] is its second N ints
    nn = b[o + 4 * n:o + 8 * n].view(torch.int32).cpu().numpy().copy() if with_nn else None
    return dict(active=act, transparent=tr, x_c=xc, nn=nn)


def read_fine_lists(scene, level="world_fine"):
    """(header, offsets, face index of every list entry) of a fine level (layout of dsn_grid_view, csrc/dsn_nn.h: 16-byte entries)"""
    o = scene._nn_off[N.LEVELS.index(level)]
    h = N.read_header(scene, level)
    p = 256 + a256(4 * (FINE_MAXCELL + 1)) + a256(4 * FINE_MAXCELL)
    b = scene.buf[o:o + p + 16 * h["total"]].cpu().numpy()
    off = b[256:256 + 4 * (h["ncell"] + 1)].view(np.int32).copy()
    ids = b[p:p + 16 * h["total"]].view(np.int32).reshape(-1, 4)[:, 3].copy()
    return h, off, ids


def geometry(scene, pk, o, d, near, far, S, **kw):
    from dsnerf_amd import _lib
    ws = _lib.RenderWorkspace(DEV)
    t_vals = torch.linspace(0.0, 1.0, steps=S, device=DEV)
    out = _lib.render_rays(scene, pk, ws, o, d, near.clone(), far.clone(), S, t_vals, screen=False, phases=_lib.PHASE_GEOMETRY, **kw)
    torch.cuda.synchronize()
    return ws, out["z_vals"]


def same_geometry(got, ref, what):
    assert np.array_equal(got["transparent"], ref["transparent"]), what
    assert got["x_c"].tobytes() == ref["x_c"].tobytes(), what
    assert np.array_equal(got["active"], ref["active"]), what


def block_places(lists_of):
    """for (cell list, (first face, second face)) items: how many pairs sit inside one block of their list, how many in different blocks"""
    inside = across = 0
    for li, (fa, fb) in lists_of:
        pa, pb = np.nonzero(li == fa)[0], np.nonzero(li == fb)[0]
        if pa.size and pb.size:
            if pa[0] // BLOCK == pb[0] // BLOCK:
                inside += 1
            else:
                across += 1
    return inside, across


# ---------------------------------------------------------------------------------------------------------------------------
# frames of the two synthetic bodies with twinned faces: fused cell-major search, lazily built lists, DSN_NN_UNFUSED
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonuniform", [False, True])
def test_frame_searches_equal_the_exhaustive_search(nonuniform, monkeypatch):
    """a 256 x 256 x 64 frame (4.2 M samples: the sampler's classification, k_nns_search<true> on pruned survivor lists): the fused
    search on every cell's lists and on lazily built ones, and DSN_NN_UNFUSED (k_nns_search<false> writes the index, k_warp reads it),
    leave the transparency flags, canonical points and active set of the exhaustive sweep, bit for bit; the unfused index equals the
    sweep's wherever the search took the sample, and the sweep's equals the oracle's on a subset"""
    from dsnerf_amd import _lib
    S, HW = 64, 256
    assert HW * HW * S >= 1 << 20           # = DSN_CELLMAJOR_MIN: the cell-major search runs
    case = N.twin_case(nonuniform, "orig")
    canon, faces, batch = full_frame(hw=HW, nonuniform=nonuniform)
    assert np.array_equal(canon, case["base_canon"]) and np.array_equal(batch["xyz"][0].numpy(), case["base_xyz"])
    batch["xyz"] = torch.from_numpy(case["xyz"])[None]
    r = renderer_with(state(), case["canon"], case["faces"])
    r.eval()
    o, d = r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0])
    near, far = r._dev(batch["near"][0]), r._dev(batch["far"][0])
    pk = r.net.packed(r.device)
    R = o.shape[0]

    def run(lazy, with_nn=False, **kw):
        r._set_frame(batch, lazy=lazy)
        ws, z = geometry(r.scene, pk, o, d, near, far, S, **kw)
        assert r.scene.nn_overflow == {}
        h = N.read_header(r.scene, "world_fine")
        assert h["total"] <= h["cap"] and (h["lazy"] == 2 if lazy and not kw and not with_nn else h["ok"] == 1), (lazy, kw, h)
        return read_geometry(ws, R, S, with_nn), z

    ref, z = run(False, exhaustive=True)
    assert ref["active"].size > 100000
    same_geometry(run(False)[0], ref, "fused, every cell's lists")
    same_geometry(run(True)[0], ref, "fused, lazily built lists")
    monkeypatch.setenv("DSN_NN_UNFUSED", "1")
    unf, _ = run(False, with_nn=True)
    monkeypatch.delenv("DSN_NN_UNFUSED")
    same_geometry(unf, ref, "DSN_NN_UNFUSED")
    # the index itself: the exhaustive sweep's on the frame's own points
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    idx = _lib.warp(r.scene, pts, None, 1, want_dir=False, exhaustive=True)["face_idx"].cpu().numpy()
    took = unf["nn"] >= 0
    assert took.mean() > 0.99, took.mean()
    assert np.array_equal(unf["nn"][took], idx[took])
    tied = N.tie_mask(case, idx, "world")
    print(f"nonuniform {nonuniform}: {int(tied.sum())} tied samples among {idx.size}, {int((tied & took).sum())} of them in the cell-major search")
    assert (tied & took).sum() >= 200, int((tied & took).sum())
    assert np.isin(idx[tied], case["first"]).all()          # the FIRST face of every tied pair
    sel = np.nonzero(tied)[0][::max(1, int(tied.sum()) // 3000)][:3000]
    assert np.array_equal(idx[sel], O.nearest_face(pts.cpu().numpy()[sel], O.centroids(case["xyz"], case["faces"])))


# ---------------------------------------------------------------------------------------------------------------------------
# lists under 96 entries: the unpruned scalar-load path
# ---------------------------------------------------------------------------------------------------------------------------
def test_short_lists_take_the_unpruned_path_and_equal_the_exhaustive_search(monkeypatch):
    """a 72-face soup (64 lattice triangles + 8 twins: every fine list is shorter than 96 entries, so k_nns_search never prunes) seen by
    a small ray batch with DSN_CELLMAJOR_MIN=1: fused and unfused searches against the sweep; the tied pairs sit inside one block of
    their cell's list for some cells and in different blocks for others, and the lists' lengths cover every tail length"""
    from dsnerf_amd import _lib, synth
    s = N.dyadic_soup(n=4)
    c = N.twin_faces((s["verts"] * np.float32(0.5)).astype(np.float32), s["faces"], s["verts"], [3, 9, 17, 22, 30, 41, 50, 60], [], "orig")
    assert c["faces"].shape[0] == 72 < 96
    sc = _lib.Scene(torch.from_numpy(c["canon"]), torch.from_numpy(c["faces"]), DEV)
    pk = _packed()
    sc.set_frame(pk, torch.from_numpy(c["xyz"]), torch.from_numpy(synth.make_poses()), 5)
    S, HW = 64, 64
    rays = synth.make_rays(HW, HW, c["xyz"], fit_box=True)
    o, d, near, far = (T(rays[k]) for k in ("ray_o", "ray_d", "near", "far"))
    R = o.shape[0]
    monkeypatch.setenv("DSN_CELLMAJOR_MIN", "1")
    ref_ws, z = geometry(sc, pk, o, d, near, far, S, exhaustive=True)
    ref = read_geometry(ref_ws, R, S)
    same_geometry(read_geometry(geometry(sc, pk, o, d, near, far, S)[0], R, S), ref, "fused")
    monkeypatch.setenv("DSN_NN_UNFUSED", "1")
    unf = read_geometry(geometry(sc, pk, o, d, near, far, S)[0], R, S, with_nn=True)
    monkeypatch.delenv("DSN_NN_UNFUSED")
    same_geometry(unf, ref, "DSN_NN_UNFUSED")
    assert N.read_header(sc, "world_fine")["ok"] == 1
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    idx = _lib.warp(sc, pts, None, 1, want_dir=False, exhaustive=True)["face_idx"].cpu().numpy()
    took = unf["nn"] >= 0
    assert took.sum() >= 10000, int(took.sum())
    assert np.array_equal(unf["nn"][took], idx[took])
    assert np.array_equal(idx, O.nearest_face(pts.cpu().numpy(), O.centroids(c["xyz"], c["faces"])))
    h, off, ids = read_fine_lists(sc)
    cell = N.cell_of(h, pts.cpu().numpy())
    assert np.array_equal(cell >= 0, took)
    lens = np.diff(off)
    visited = np.unique(cell[took])
    assert 0 < lens[visited].min() and lens[visited].max() < 96, (lens[visited].min(), lens[visited].max())
    tails = sorted(set(int(x) % BLOCK for x in lens[visited]))
    print(f"{visited.size} visited cells, lists of {lens[visited].min()} .. {lens[visited].max()} entries, tail lengths {tails}")
    assert len(tails) >= 4                                                   # short last blocks of several lengths
    pair = N.pair_of(c)
    tied = took & (pair[idx] >= 0)
    assert tied.sum() >= 1000 and np.isin(idx[tied], c["first"]).all(), int(tied.sum())
    combos = {(int(cc), int(pair[i])) for cc, i in zip(cell[tied], idx[tied])}
    inside, across = block_places([(ids[off[cc]:off[cc + 1]], (c["first"][k], c["second"][k])) for cc, k in combos])
    print(f"{int(tied.sum())} tied samples; (cell, pair) combinations with both faces in one block: {inside}, in different blocks: {across}")
    assert inside >= 1 and across >= 1


# ---------------------------------------------------------------------------------------------------------------------------
# more survivors than the wave's array holds: drained in rounds
# ---------------------------------------------------------------------------------------------------------------------------
def _shell_body(n_faces=720, rho=0.05, eps=0.002, n_twins=40):
    """small triangles whose centroids lie on a sphere of radius rho around the origin (+ twins of some): from the centre every face is
    the nearest one to within rounding"""
    k = np.arange(n_faces) + 0.5
    phi = np.arccos(1.0 - 2.0 * k / n_faces)
    th = np.pi * (1.0 + 5.0 ** 0.5) * k
    u = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)
    t1 = np.cross(u, np.where(np.abs(u[:, 2:3]) < 0.9, [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0]]))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(u, t1)
    c = rho * u
    verts = np.stack([c + eps * t1, c + eps * (-0.5 * t1 + 0.75 ** 0.5 * t2), c + eps * (-0.5 * t1 - 0.75 ** 0.5 * t2)], 1)
    verts = verts.reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n_faces).reshape(n_faces, 3)
    picks = [int(x) for x in np.random.default_rng(3).permutation(n_faces)[:n_twins]]
    return N.twin_faces((verts * np.float32(0.5)).astype(np.float32), faces, verts, picks, [], "orig")


def test_lists_drained_in_rounds_equal_the_exhaustive_search(monkeypatch):
    """760 near-equidistant faces around a cloud of samples 4e-6 of their distance wide: no candidate can be pruned (asserted from the
    bound's own formula on the box of ALL samples, which contains every wave's), so each wave drains its list in three rounds of at most
    320 survivors; the winners change from round to round and many are one of a duplicated pair.  Lazily built lists (only the visited
    cells': a level of 760-entry lists for every cell would not fit), DSN_CELLMAJOR_MIN=1 for the small batch"""
    from dsnerf_amd import _lib, synth
    c = _shell_body()
    F = c["faces"].shape[0]
    assert F > 2 * SURVIVORS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the canonical levels of this body may not fit their capacity: not used here)
        sc = _lib.Scene(torch.from_numpy(c["canon"]), torch.from_numpy(c["faces"]), DEV)
    pk = _packed()
    R, S = 2048, 64
    rng = np.random.default_rng(11)
    dirs = rng.standard_normal((R, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    o, d = T((-1e-3 * dirs).astype(np.float32)), T(dirs)
    near, far = T(np.full(R, 1e-3 * (1 - 1e-4), np.float32)), T(np.full(R, 1e-3 * (1 + 1e-4), np.float32))      # points within 1e-7 of the centre
    monkeypatch.setenv("DSN_CELLMAJOR_MIN", "1")
    poses = torch.from_numpy(synth.make_poses())
    sc.set_frame(pk, torch.from_numpy(c["xyz"]), poses, 5, lazy=True)
    ws, z = geometry(sc, pk, o, d, near, far, S, uniform=True)
    got = read_geometry(ws, R, S)
    h, off, ids = read_fine_lists(sc)
    assert h["lazy"] == 2 and h["total"] <= h["cap"], h          # the visited cells' lists were built and fit: the fused search ran on them
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)
    p = pts.cpu().numpy()
    cell = N.cell_of(h, p)
    assert (cell >= 0).all()
    lens = np.diff(off)[np.unique(cell)]
    assert lens.min() > 2 * SURVIVORS, lens
    # nothing can be pruned: T (1 + 1e-4) >= the nearest-point distance of every candidate, for any box inside the box of all samples
    cent = O.centroids(c["xyz"], c["faces"]).astype(np.float64)
    lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    dmax2 = (np.maximum(np.abs(cent - lo), np.abs(cent - hi)) ** 2).sum(1)
    dmin2 = (np.maximum(np.maximum(lo - cent, cent - hi), 0.0) ** 2).sum(1)
    assert dmax2.max() <= dmin2.min() * 1.00005, (dmax2.max(), dmin2.min())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the exhaustive call completes the level for every cell, which may not fit: not used)
        ref_ws, z2 = geometry(sc, pk, o, d, near, far, S, uniform=True, exhaustive=True)
    assert torch.equal(z, z2)
    ref = read_geometry(ref_ws, R, S)
    same_geometry(got, ref, "fused, three rounds")
    assert ref["active"].size > 0.9 * R * S               # (5 cm from every face: the canonical points carry the index)
    idx = _lib.warp(sc, pts, None, 1, want_dir=False, exhaustive=True)["face_idx"].cpu().numpy()
    assert np.array_equal(idx, O.nearest_face(p, O.centroids(c["xyz"], c["faces"])))
    pair = N.pair_of(c)
    tied = pair[idx] >= 0
    pos = np.empty(idx.size, np.int64)                                       # (nothing pruned: position among the survivors = in the list)
    for cc in np.unique(cell):
        m = cell == cc
        li = ids[off[cc]:off[cc + 1]]
        pos[m] = np.searchsorted(li, idx[m])
        assert np.array_equal(li[pos[m]], idx[m])
    rounds = np.bincount(pos // SURVIVORS, minlength=3)
    print(f"{int(tied.sum())} tied samples among {idx.size}; winners per round: {rounds.tolist()}")
    assert tied.sum() >= 1000 and np.isin(idx[tied], c["first"]).all() and (rounds > 1000).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the coarse / far path of training batches
# ---------------------------------------------------------------------------------------------------------------------------
def _training_forward_forms(nonuniform):
    """the forward of an 8192 x 64 training batch of the twinned body (noise 1: transparent samples are evaluated, their canonical
    points lie far from the body - the far canonical search) with the default geometry, with per-lane walks only and with the
    exhaustive search; returns the outputs of the three and what is needed to look at the far points"""
    from dsnerf_amd import _lib, synth
    R, S, HW = 8192, 64, 512
    case = N.twin_case(nonuniform, "orig")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sc = _lib.Scene(torch.from_numpy(case["canon"]), torch.from_numpy(case["faces"]), DEV)
    pk = _lib.PackedParams(DEV).update({k: torch.from_numpy(v) for k, v in state("x_w4").items()})
    sc.set_frame(pk, torch.from_numpy(case["xyz"]), torch.from_numpy(synth.make_poses()), 5)
    rays = synth.make_rays(HW, HW, case["base_xyz"], fit_box=True)
    sel = np.linspace(0, HW * HW - 1, R).astype(np.int64)
    o, d, near, far = (T(rays[k][sel]) for k in ("ray_o", "ray_d", "near", "far"))
    noise = torch.randn(R, S, generator=torch.Generator().manual_seed(11)).to(DEV)
    t_vals = torch.linspace(0.0, 1.0, steps=S, device=DEV)

    def run(**kw):
        out = _lib.render_rays(sc, pk, _lib.RenderWorkspace(DEV), o, d, near.clone(), far.clone(), S, t_vals, None, noise,
                               skip_transparent=False, train_cache=_lib.GradWorkspace(DEV), **kw)
        torch.cuda.synchronize()
        return {k: out[k].clone() for k in ("color", "acc_map", "depth_map", "weights", "z_vals")}

    forms = {"default": run(), "exhaustive": run(exhaustive=True)}
    os.environ["DSN_NN_UNFUSED"] = "1"
    os.environ["DSN_TRAIN_FAR_SEARCH_MIN"] = str(1 << 40)
    try:
        forms["walks"] = run()
    finally:
        del os.environ["DSN_NN_UNFUSED"], os.environ["DSN_TRAIN_FAR_SEARCH_MIN"]
    return forms, case, sc, o, d


def _assert_forms_equal(forms, what):
    for name in ("default", "walks"):
        for k, v in forms["exhaustive"].items():
            assert torch.equal(torch.nan_to_num(forms[name][k], nan=-1.0), torch.nan_to_num(v, nan=-1.0)), (what, name, k)
    assert float(forms["exhaustive"]["acc_map"].max()) > 0.05


@pytest.mark.parametrize("nonuniform", [False, True])
def test_training_batch_far_search_equals_the_exhaustive_search(nonuniform):
    """k_nns_search_far (segments of the coarse lists, the winner per block inside a segment, 64-bit atomicMin across segments) and the
    fused search of the training forward: outputs bit for bit those of the exhaustive search and of the per-lane walks.  Among the
    batch's far canonical points many are nearest to a duplicated face, with the two faces inside one block of the coarse list for some
    and in different blocks for others"""
    from dsnerf_amd import _lib
    R, S = 8192, 64
    assert R * S >= 1 << 18 and R * S >= 1 << 15         # = DSN_TRAIN_CELLMAJOR_MIN, DSN_TRAIN_FAR_SEARCH_MIN: both on by default
    forms, case, sc, o, d = _training_forward_forms(nonuniform)
    _assert_forms_equal(forms, "segmented far search")
    pts = (o[:, None, :] + d[:, None, :] * forms["exhaustive"]["z_vals"][..., None]).reshape(-1, 3)
    x_c = _lib.warp(sc, pts, None, 1, want_dir=False, exhaustive=True)["x_c"].cpu().numpy()
    cf = N.cell_of(N.read_header(sc, "canon_fine"), x_c)
    cc = N.cell_of(N.read_header(sc, "canon_coarse"), x_c)
    farp = x_c[(cf < 0) & (cc >= 0)]
    assert farp.shape[0] >= 10000, farp.shape
    z3 = np.zeros_like(farp)
    idx = _lib.shade(sc, _packed(), T(farp), T(z3), T(farp), T(z3 + 1), T(z3), 1, exhaustive=True)[0].cpu().numpy()
    tied = N.tie_mask(case, idx, "canon")
    assert tied.sum() >= 200, int(tied.sum())
    off, lst = N.read_coarse_lists(sc)
    cell = N.cell_of(N.read_header(sc, "canon_coarse"), farp[tied])
    pair = N.pair_of(case)
    combos = {(int(c_), int(pair[i])) for c_, i in zip(cell, idx[tied])}
    inside, across = block_places([(lst[off[c_]:off[c_ + 1]], (case["first"][k], case["second"][k])) for c_, k in combos])
    print(f"nonuniform {nonuniform}: {farp.shape[0]} far canonical points, {int(tied.sum())} tied; (cell, pair) combinations with both "
          f"faces in one block of the coarse list: {inside}, in different blocks: {across}")
    assert inside >= 1 and across >= 1


def test_unsegmented_coarse_search_equals_the_exhaustive_search():
    """DSN_FAR_SEGMENTS=0 (read once per process: a child process): the far points take k_nns_search<false> on the coarse lists - one
    wave per list, two samples per lane and, for waves of at most 64 samples, its one-sample-per-lane form - on both bodies"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DSN_FAR_SEGMENTS="0",
               PYTHONPATH=os.pathsep.join([root, os.path.join(root, "oracle"), os.path.join(root, "tests")]))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "UNSEGMENTED_OK" in p.stdout


if __name__ == "__main__":
    assert os.environ.get("DSN_FAR_SEGMENTS") == "0"
    for nu in (False, True):
        _assert_forms_equal(_training_forward_forms(nu)[0], f"unsegmented coarse search, nonuniform {nu}")
    print("UNSEGMENTED_OK")
