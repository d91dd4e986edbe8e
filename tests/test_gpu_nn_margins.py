"""GPU: the float margins of the nearest-face list build (DSN_GRID_GUARD, the pruning margin of dsn_in_list; csrc/dsn_nn.hip) on
cases that need them - tests/nn_margin_cases.py: probe cells on both synthetic bodies in which a float32 point that classifies into
the cell lies outside the cell's own box, and whose nearest face a list built without the margins lacks (the host verdicts,
tests/test_nn_margins_host.py).

  * the device's grids are the recorded ones the cases were built on (tests/golden/nn_margin_headers.json), its lists hold every
    certainly-in face of the restatement and no certainly-out one, its U(B)^2 lies in the restated bracket - on all four levels, for
    every cell a probe point lies in;
  * every search path returns what the exhaustive sweep and the oracle return, bit for bit, on the probe points: dsn_warp and
    dsn_lbs_warp (lists / sweep; on a scene whose fine levels do not fit, DSN_NN_FINE_CAP, the same queries walk the COARSE lists, the
    only way a search reaches the coarse probe cells), dsn_shade (k_normal's per-lane walk and its cooperative sweep), the fused
    cell-major search of an eval batch (every cell's lists and lazily built ones, with and without DSN_NN_NO_SUPER / DSN_NN_NO_MEMBER)
    and a training batch (fused search on lazily built lists, far canonical search).

That the battery bites: mutated builds of the library, each run once on the MI355X against this module (sources restored afterwards;
the runs are not part of the suite; the first two were made with the first six points of every probe cell, before the further
points were added).

  * DSN_GRID_GUARD 0.0f and dsn_in_list reduced to dmin2 <= u2 (host verdict: 64 / 60 posed fine cells, 64 / 64 canonical fine cells,
    4 or 5 per coarse level lose their probe point's nearest face): all 8 tests fail.
      test_device_lists_against_the_restatement   [uniform] "certainly-in faces the device list lacks" (world_fine, a body face: every
                                                  list shrinks), [SMPL-like] U(B)^2 below the restated bracket
      test_stage_calls_equal_the_sweep_...        "wrong face index at points" in _warp_checks, lists (exhaustive=False): 114 / 62 posed
                                                  points, the first of every probe cell's six among them (points 0, 6, 12, ...)
      test_fused_cell_major_search_...            same_geometry: x_c of the fused search on every cell's lists != the sweep's
      test_training_batch_...                     `color` of the lazily set batch != exhaustive
  * DSN_GRID_GUARD 0.0f alone (host verdict: 19 / 0 posed fine cells, 56 / 63 canonical fine cells): 6 of 8 fail.
      test_device_lists_against_the_restatement   as above, both bodies
      test_stage_calls_equal_the_sweep_...        [uniform] 53 wrong posed points in _warp_checks; [SMPL-like] the posed points pass and
                                                  _shade_checks reports 60 wrong canonical face indices (lists)
      test_fused_... / test_training_batch_...    [uniform] fail as above; [SMPL-like] pass - no posed cell of that body needs the guard
                                                  beside the shipped margin, as the host verdict says
  * the shipped guard with dmin2 <= u2 was not built: the host verdict finds no cell that needs the pruning margin beside the guard.

  * DSN_CLEAR_MARGIN 0.0f (the host finds no position that margin 0 flags with a non-transparent sample, so no frame can differ;
    the flag itself does): test_clear_cell_flag_at_its_limits fails at its first position between the two flips, ("h", k = 2):
    "device flag 1, restated False".  The other 8 tests do not look at flags.

The clear-cell margin (test_clear_cell_flag_at_its_limits): one cell whose list holds a single face, placed float by float at the
limits of dsn_face_clears_box - 66 positions, 40 of them with the guarded box's nearest corner within 8 ulp of |h| = 0.1 or of
u / v = 5, -4.  The device's flag equals the restated one everywhere, frames equal DSN_NN_NO_CLEAR_CELLS=1 and the sweep, no flagged
cell holds a non-transparent sample, and NO position is flagged by margin 0 while a sample of the cell is not transparent (nor, on the
host, while a float64 point of the guarded box is not): the flag is decided on the guarded box, 1e-4 m beyond any sample, against
roundings of 1e-8 m.  In these families the margin covers only the restated decision's own rounding; a sample-level failure needs a
face whose u / v gradient is thousands of times steeper, which DSN_CLEAR_INV_MAX keeps from the u / v test.
"""
import warnings

import numpy as np
import pytest
import torch

import oracle as O
import nn_cases as N
import nn_margin_cases as M
from test_gpu_nn_ties import T, _packed, _same, _scene, _waves
from test_gpu_nns_block import a256, geometry, read_fine_lists, read_geometry, same_geometry
from test_gpu_clear_cells import _fine_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BODIES = [False, True]


def _u2(scene, level):
    """U(B)^2 of every cell of a level (layout of dsn_grid_view, csrc/dsn_nn.h; test_gpu_clear_cells._fine_arrays reads the posed
    fine level's the same way)"""
    maxcell = M.FINE_MAXCELL if level.endswith("fine") else M.COARSE_MAXCELL
    o = scene._nn_off[N.LEVELS.index(level)] + 256 + a256(4 * (maxcell + 1))
    n = N.read_header(scene, level)["ncell"]
    return scene.buf[o:o + 4 * n].view(torch.float32).cpu().numpy().copy()


def _lists(scene, level):
    """(offsets, face index of every entry) of a level"""
    if level.endswith("fine"):
        _, off, ids = read_fine_lists(scene, level)
        return off, ids
    return N.read_coarse_lists(scene, level)


def _capped_scene(c):
    """the case's scene with fine levels that do not fit (DSN_NN_FINE_CAP=1000, set by the caller): both fine levels are switched off
    and every query inside them walks the coarse lists"""
    from dsnerf_amd import _lib, synth
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the overflow warning is the point)
        sc = _lib.Scene(torch.from_numpy(c["canon"]), torch.from_numpy(c["faces"]), DEV)
        sc.set_frame(_packed(), torch.from_numpy(c["xyz"]), torch.from_numpy(synth.make_poses()), 5)
        st = _lib.nn_stats(sc)
    for name, (ncell, ok, total, cap) in st.items():
        assert ok == (0 if name.endswith("fine") else 1), (name, st)
    return sc


@pytest.mark.parametrize("nonuniform", BODIES)
def test_device_lists_against_the_restatement(nonuniform):
    """all four levels: the device's grid is the recorded one the case was built on; for every cell a probe point lies in, every
    certainly-in face is in the device's list and no certainly-out face is, U(B)^2 lies in the restated bracket, and the restatement
    leaves at most 1 % of the entries open.  The face each probe cell loses without the margins is in its list."""
    c = M.margin_case(nonuniform)
    sc = _scene(c["canon"], c["faces"], c["xyz"])
    for lv in N.LEVELS:
        h = N.read_header(sc, lv)
        assert M.same_header(h, c["headers"][lv]), (lv, h, c["headers"][lv])
        off, ids = _lists(sc, lv)
        u2 = _u2(sc, lv)
        lists, _ = M.shipped_lists(nonuniform, lv)
        entries = open_ = plain = 0
        for cell, r in lists.items():
            li = ids[off[cell]:off[cell + 1]]
            assert np.all(np.diff(li) > 0), (lv, cell)                    # ascending face order
            have = np.zeros(c["faces"].shape[0], bool)
            have[li] = True
            missing, extra = np.nonzero(r["sure_in"] & ~have)[0], np.nonzero(r["sure_out"] & have)[0]
            assert missing.size == 0, (lv, cell, "certainly-in faces the device list lacks", missing[:8])
            assert extra.size == 0, (lv, cell, "certainly-out faces in the device list", extra[:8])
            assert r["u2_lo"] <= u2[cell] <= r["u2_hi"], (lv, cell, u2[cell], r["u2_lo"], r["u2_hi"])
            plain += int(u2[cell] == r["u2_plain"])
            entries += li.size
            open_ += int((have & ~r["sure_in"]).sum())
        print(f"nonuniform {nonuniform} {lv}: {len(lists)} cells, {entries} entries, {open_} undetermined, U^2 = the unfused value in {plain}")
        assert open_ <= 0.01 * entries, (lv, open_, entries)
        for pr in c["probes"][lv]:
            li = ids[off[pr["cell"]]:off[pr["cell"] + 1]]
            assert pr["face_s"] in li and pr["face_g"] in li, (lv, pr["ijk"])


def _cells_of(c, space, bad):
    """which probe cells the points `bad` (positions in the space's fine points followed by its coarse points) belong to"""
    n_fine = c["points"][space + "_fine"].shape[0]
    out = []
    for i in bad:
        lv, j = (space + "_fine", i) if i < n_fine else (space + "_coarse", i - n_fine)
        if j < c["owner"][lv].size:
            out.append((lv, tuple(int(x) for x in c["probes"][lv][c["owner"][lv][j]]["ijk"]),
                        int(j % 6) if j < 6 * len(c["probes"][lv]) else "further point"))
    return out[:6]


def _warp_checks(sc, c, pts, what):
    from dsnerf_amd import _lib, synth
    o = O.warp(pts, None, c["xyz"], c["canon"], c["faces"])
    for exhaustive in (False, True):
        a = _lib.warp(sc, T(pts), None, 1, want_dir=False, want_uvh=True, exhaustive=exhaustive)
        got = a["face_idx"].cpu().numpy()
        bad = np.nonzero(got != o["idx"])[0]
        assert bad.size == 0, (what, exhaustive, "wrong face index at points", bad[:8], got[bad[:8]], o["idx"][bad[:8]],
                               "probe cells (level, cell, which of its six points)", _cells_of(c, "world", bad))
        for k in ("uv", "h", "x_c"):
            assert _same(a[k].cpu().numpy(), o[k]), (what, k, exhaustive)
        assert _same(a["transparent"].cpu().numpy().astype(bool), o["transparent"]), (what, exhaustive)
    W = synth.make_skin_weights(c["xyz"].shape[0])
    A = synth.make_joint_transforms()
    ol = O.lbs_warp(pts, c["xyz"], c["faces"], W, A, 0)
    for exhaustive in (False, True):
        b = _lib.lbs_warp(sc, T(pts), torch.from_numpy(W), torch.from_numpy(A), "rigid_center", exhaustive=exhaustive)
        assert _same(b["face_idx"].cpu().numpy(), ol["idx"]), (what, "lbs_warp", exhaustive)
    return o


def _shade_checks(sc, c, x_c, what):
    from dsnerf_amd import _lib
    rng = np.random.default_rng(23)
    n = x_c.shape[0]
    grad, x_w, rd = (rng.standard_normal((n, 3)).astype(np.float32) for _ in range(3))
    ess = rng.random((n, 3)).astype(np.float32)
    oi, on = O.normal_world(x_c, grad, c["canon"], c["xyz"], c["faces"])
    for exhaustive in (False, True):
        idx, n_w, _ = _lib.shade(sc, _packed(), T(x_c), T(grad), T(x_w), T(rd), T(ess), 1, exhaustive=exhaustive)
        got = idx.cpu().numpy()
        bad = np.nonzero(got != oi)[0]
        assert bad.size == 0, (what, exhaustive, "wrong canonical face index at points", bad[:8], got[bad[:8]], oi[bad[:8]])
        assert _same(n_w.cpu().numpy(), on), (what, exhaustive)
    return oi


@pytest.mark.parametrize("nonuniform", BODIES)
def test_stage_calls_equal_the_sweep_and_the_oracle(nonuniform, monkeypatch):
    """dsn_warp / dsn_lbs_warp on the posed probe points and dsn_shade on the canonical ones (in waves with 1 - 3 lanes outside the
    canonical fine grid: k_normal's cooperative sweep; with all lanes outside; with none: the per-lane walk), through the lists and
    through the sweep: face index, uv, h, x_c, transparent / index and world normal equal the oracle bit for bit.  Then the same on a
    scene whose fine levels do not fit: the probe points of the COARSE cells (and all others) walk the coarse lists."""
    c = M.margin_case(nonuniform)
    pw = np.concatenate([c["points"]["world_fine"], c["points"]["world_coarse"]])
    pc = np.concatenate([c["points"]["canon_fine"], c["points"]["canon_coarse"]])
    sc = _scene(c["canon"], c["faces"], c["xyz"])
    assert (N.cell_of(N.read_header(sc, "world_fine"), pw) >= 0).all() and (N.cell_of(N.read_header(sc, "canon_fine"), pc) >= 0).all()
    o = _warp_checks(sc, c, pw, "every level")
    probe_hit = np.isin(o["idx"], np.arange(c["base_F"], c["faces"].shape[0]))
    assert probe_hit.mean() > 0.9 and (~o["transparent"][:c["points"]["world_fine"].shape[0]]).mean() > 0.5
    # canonical: the probe points + as many far points (outside the canonical fine grid: in the coarse shell and beyond both)
    rng = np.random.default_rng(29)
    far = np.concatenate([pc[::2] + np.float32(0.3) * np.sign(pc[::2]), pc[1::2] + np.float32(3.0)]).astype(np.float32)
    q = np.concatenate([pc, far])
    inside = N.cell_of(N.read_header(sc, "canon_fine"), q) >= 0
    rows, kind = _waves(np.nonzero(inside)[0], np.nonzero(~inside)[0], rng)
    assert (kind == 0).sum() >= pc.shape[0] // 2 and (kind == 1).sum() >= 8 and (kind == 2).sum() >= 64
    assert np.isin(np.arange(pc.shape[0]), rows).mean() > 0.9
    _shade_checks(sc, c, q[rows], "every level")
    del sc
    monkeypatch.setenv("DSN_NN_FINE_CAP", "1000")
    sc = _capped_scene(c)
    monkeypatch.delenv("DSN_NN_FINE_CAP")
    for lv, pts in (("world_coarse", pw), ("canon_coarse", pc)):
        assert (N.cell_of(N.read_header(sc, lv), pts) >= 0).all()
    _warp_checks(sc, c, pw, "coarse lists")
    _shade_checks(sc, c, pc, "coarse lists")


def _point_rays(pts):
    """one ray per point whose samples all sit AT the point: per axis d = a power of two with the point's sign, at most 2^-10 and at
    most half the coordinate (o = p - d then stays within one binade below p and is exact, and o + d * 1 gives p back), near = far = 1"""
    k = np.minimum(np.floor(np.log2(np.maximum(np.abs(pts.astype(np.float64)), 2.0 ** -100))) - 1, -10)
    d = (np.where(pts < 0, -1.0, 1.0) * 2.0 ** k).astype(np.float32)
    o = (pts - d).astype(np.float32)
    one = np.ones(pts.shape[0], np.float32)
    return T(o), T(d), T(one), T(one)


@pytest.mark.parametrize("nonuniform", BODIES)
def test_fused_cell_major_search_equals_the_sweep(nonuniform, monkeypatch):
    """one ray per posed probe point, every sample at the point (DSN_CELLMAJOR_MIN=1, uniform sampling, near = far): the fused
    cell-major search + warp on every cell's lists and on lazily built ones, each with the build's supersets and membership words and
    without them (DSN_NN_NO_SUPER, DSN_NN_NO_MEMBER), leaves the transparency flags, canonical points and active set of the
    exhaustive sweep bit for bit, and the sweep's are the oracle's"""
    from dsnerf_amd import _lib, synth
    c = M.margin_case(nonuniform)
    pts = np.concatenate([c["points"]["world_fine"], c["points"]["world_coarse"]])
    o, d, near, far = _point_rays(pts)
    R, S = pts.shape[0], 4
    pk = _packed()
    sc = _lib.Scene(torch.from_numpy(c["canon"]), torch.from_numpy(c["faces"]), DEV)
    xyz, poses = torch.from_numpy(c["xyz"]), torch.from_numpy(synth.make_poses())
    monkeypatch.setenv("DSN_CELLMAJOR_MIN", "1")

    def run(lazy, **kw):
        sc.set_frame(pk, xyz, poses, 5, lazy=lazy)
        ws, z = geometry(sc, pk, o, d, near, far, S, uniform=True, **kw)
        h = N.read_header(sc, "world_fine")
        assert h["total"] <= h["cap"] and (h["lazy"] == 2 if lazy and not kw else h["ok"] == 1), (lazy, kw, h)
        return read_geometry(ws, R, S), z

    ref, z = run(False, exhaustive=True)
    p2 = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).cpu().numpy()
    kept = (p2.reshape(R, S, 3) == pts[:, None, :]).all(-1)
    print(f"nonuniform {nonuniform}: {kept.mean():.3f} of the samples have the probe point's bits")
    assert kept.mean() >= 0.9
    ow = O.warp(p2, None, c["xyz"], c["canon"], c["faces"])
    assert np.array_equal(ref["transparent"].astype(bool), ow["transparent"])
    live = ~ow["transparent"]
    assert live.sum() >= 0.3 * live.size and ref["x_c"][live].tobytes() == ow["x_c"][live].tobytes()
    assert ref["active"].size > 0
    for env in (None, "DSN_NN_NO_SUPER", "DSN_NN_NO_MEMBER"):
        if env:
            monkeypatch.setenv(env, "1")
        for lazy in (False, True):
            got, z2 = run(lazy)
            assert torch.equal(z, z2)
            same_geometry(got, ref, (env, "lazy" if lazy else "every cell"))
        if env:
            monkeypatch.delenv(env)


@pytest.mark.parametrize("nonuniform", BODIES)
def test_training_batch_equals_the_exhaustive_search(nonuniform):
    """a training batch of 4352 rays x 64 samples (above DSN_TRAIN_CELLMAJOR_MIN = 2^18 and DSN_TRAIN_FAR_SEARCH_MIN: the fused search
    on lazily built lists and the far canonical search) whose rays hold the posed probe points, every sample at its point: every
    output equals the call with exhaustive=True bit for bit"""
    from dsnerf_amd import _lib, synth
    from helpers import state
    c = M.margin_case(nonuniform)
    pts = np.concatenate([c["points"]["world_fine"], c["points"]["world_coarse"]])
    R, S = 4352, 64
    assert R * S >= 1 << 18 and pts.shape[0] <= R
    pts = pts[np.arange(R) % pts.shape[0]]
    o, d, near, far = _point_rays(pts)
    pk = _lib.PackedParams(DEV).update({k: torch.from_numpy(v) for k, v in state("x_w4").items()})
    sc = _lib.Scene(torch.from_numpy(c["canon"]), torch.from_numpy(c["faces"]), DEV)
    xyz, poses = torch.from_numpy(c["xyz"]), torch.from_numpy(synth.make_poses())
    noise = torch.randn(R, S, generator=torch.Generator().manual_seed(11)).to(DEV)
    t_vals = torch.linspace(0.0, 1.0, steps=S, device=DEV)

    def run(lazy, **kw):
        sc.set_frame(pk, xyz, poses, 5, lazy=lazy)
        out = _lib.render_rays(sc, pk, _lib.RenderWorkspace(DEV), o, d, near.clone(), far.clone(), S, t_vals, None, noise,
                               skip_transparent=False, uniform=True, train_cache=_lib.GradWorkspace(DEV), **kw)
        torch.cuda.synchronize()
        return {k: out[k].clone() for k in ("color", "acc_map", "depth_map", "weights", "z_vals")}, N.read_header(sc, "world_fine")

    ref, _ = run(False, exhaustive=True)
    p2 = o[:, None, :] + d[:, None, :] * ref["z_vals"][..., None]
    assert float((p2 == T(pts)[:, None, :]).all(-1).float().mean()) >= 0.9
    assert float(ref["acc_map"].max()) > 0.05
    for lazy in (True, False):
        got, h = run(lazy)
        assert (h["lazy"] == 2) if lazy else (h["ok"] == 1), (lazy, h)
        for k, v in ref.items():
            assert torch.equal(torch.nan_to_num(got[k], nan=-1.0), torch.nan_to_num(v, nan=-1.0)), (lazy, k)


# ---------------------------------------------------------------------------------------------------------------------------
# the clear-cell margin
# ---------------------------------------------------------------------------------------------------------------------------
def test_clear_cell_flag_at_its_limits(monkeypatch):
    """one cell of an otherwise empty grid with ONE member face (nn_margin_cases.clear_scene), placed float by float around the
    limits of dsn_face_clears_box: where the guarded box's nearest corner has |h| = 0.1 (u, v = 5, -4) to within 8 ulp, where the
    restated flag flips with margin 0, and where it flips with DSN_CLEAR_MARGIN.  Per position a lazily set fused eval batch of 27
    samples of the cell (its first / middle / last float32 per axis): the device's flag is the restated one (both values occur per
    kind), transparent / x_c / the active set equal the run with DSN_NN_NO_CLEAR_CELLS=1 and the exhaustive sweep bit for bit, the
    sweep's transparency is the restated dsn_project's, and a flagged cell holds no non-transparent sample.  Host side: the number of
    positions that margin 0 flags although a sample of the cell is not transparent is 0 - the flag is decided on the guarded box,
    1e-4 m beyond any sample, against roundings of 1e-8 m: no biting cell exists in these families."""
    from dsnerf_amd import _lib, synth
    verts, faces = M.clear_scene()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the canonical levels of 2 x 1000 coincident faces do not fit: not used here)
        sc = _lib.Scene(torch.from_numpy(verts), torch.from_numpy(faces), DEV)
    pk = _packed()
    poses = torch.from_numpy(synth.make_poses())
    sc.set_frame(pk, torch.from_numpy(verts), poses, 5)
    hdr = N.read_header(sc, "world_fine")
    assert hdr["ok"] == 1
    ijk = np.array([int(x) // 2 for x in hdr["n"]])
    cell = int(M.cell_index(hdr, ijk))
    pts = M.cell_sample_points(hdr, ijk)
    assert (N.cell_of(hdr, pts) == cell).all()
    o, d, near, far = _point_rays(pts)
    R, S = pts.shape[0], 2
    configs = M.clear_configs(hdr, ijk)
    assert len(configs) >= 40
    monkeypatch.setenv("DSN_CELLMAJOR_MIN", "1")
    seen, bites, at_limit = set(), 0, 0
    for cf in configs:
        v = verts.copy()
        v[-3:] = cf["tri"]
        xyz = torch.from_numpy(v)
        cent = M.centroids(v, faces)
        r = M.restate_cell(hdr, cent, cell)
        assert np.array_equal(np.nonzero(r["sure_in"])[0], [faces.shape[0] - 1]) and np.array_equal(r["sure_in"], ~r["sure_out"])
        assert r["u2_lo"] >= M.CLEAR_MIN_U2

        def run(lazy, **kw):
            sc.set_frame(pk, xyz, poses, 5, lazy=lazy)
            ws, z = geometry(sc, pk, o, d, near, far, S, uniform=True, **kw)
            h, u2, clear = _fine_arrays(sc)
            assert M.same_header(h, hdr), (cf["kind"], cf["k"])
            return read_geometry(ws, R, S), z, h, u2, clear

        on = run(True)
        assert on[2]["lazy"] == 2
        assert int(on[4][cell]) == int(cf["flag"]), (cf["kind"], cf["k"], "device flag", int(on[4][cell]), "restated", cf["flag"])
        assert r["u2_lo"] <= on[3][cell] <= r["u2_hi"]
        monkeypatch.setenv("DSN_NN_NO_CLEAR_CELLS", "1")
        off = run(True)
        monkeypatch.delenv("DSN_NN_NO_CLEAR_CELLS")
        ref = run(False, exhaustive=True)
        p2 = (o[:, None, :] + d[:, None, :] * ref[1][..., None]).reshape(-1, 3).cpu().numpy()
        assert np.array_equal(p2.reshape(R, S, 3), np.repeat(pts[:, None, :], S, 1))
        same_geometry(on[0], ref[0], (cf["kind"], cf["k"], "flags"))
        same_geometry(off[0], ref[0], (cf["kind"], cf["k"], "no flags"))
        assert (M.nearest_d2(pts, cent) == faces.shape[0] - 1).all()
        f = M.make_face(cf["tri"][0], cf["tri"][1], cf["tri"][2])
        tr = M.transparent(*M.project(pts, f))
        assert np.array_equal(ref[0]["transparent"].reshape(R, S).astype(bool), np.repeat(tr[:, None], S, 1)), (cf["kind"], cf["k"])
        if cf["flag"]:
            assert tr.all(), (cf["kind"], cf["k"], "a flagged cell holds a non-transparent sample")
        bites += int(cf["flag0"] and not tr.all())
        at_limit += int(cf["at_limit"])
        seen.add((cf["kind"], cf["flag"]))
    print(f"{len(configs)} positions, {at_limit} with the nearest corner within 8 ulp of its limit; flagged by margin 0 with a "
          f"non-transparent sample: {bites}")
    assert seen == {(k, fl) for k in M.CLEAR_KINDS for fl in (False, True)}
    assert at_limit >= 20 and bites == 0
