"""The float margins of the nearest-face list build on the host: tests/nn_margin_cases.py (restatement of list membership and the
probe cases on both synthetic bodies) on its own, before tests/test_gpu_nn_margins.py judges the kernels by it.  No GPU.

What the committed cases reach, asserted below as exact counts - probe cells whose restated list CERTAINLY lacks the face that the
float64 brute force and the dsn_d2 restatement both name nearest to the cell's probe point p (uniform body / SMPL-like body):

                 probe cells   guard 0, margin 1   guard 0, shipped margin   shipped guard, margin 1   shipped
  world_fine       64 / 64         64 / 60              19 /  0                     0 / 0               0 / 0
  world_coarse      5 /  5          4 /  5               0 /  0                     0 / 0               0 / 0
  canon_fine       64 / 64         64 / 64              56 / 63                     0 / 0               0 / 0
  canon_coarse      4 /  4          4 /  4               0 /  0                     0 / 0               0 / 0

  * DSN_GRID_GUARD is needed on its own: with the shipped pruning margin and no guard, 56 / 63 canonical fine cells and 19 posed ones
    (uniform body) lose p's nearest face.  c* has to sit in the window between "pruned" (dmin > U (1 + 5e-6)) and "nearest"
    (U rel < excursion x 1.58), and it moves in float32 steps: the canonical coordinates are small (|x| < 1 m, ulp <= 6e-8) against
    cells of 0.0335 m; at the posed mesh's coordinates (ulp 6e-8 .. 1.2e-7, cells of 0.0426 m, U >= 0.037 m) the window is about one
    step wide, and whether a cell reaches it hangs on the last place of the cell size (none does on the SMPL-like body).
  * the pruning margin (1 + 1e-5, + 1e-12) is never needed once the guard is there: shipped guard with margin 1 loses nothing in any
    configuration the builder tried (both placements of c_g, c* stepped float by float from U (1 - 2e-6) to U (1 + 3e-5)).  The guard
    grows the box by 1e-4 m where a point strays by 1e-7 m and U^2 rounds by 1e-7 of itself: at these magnitudes the margin is implied
    by the guard.
  * coarse levels: 4 or 5 cells, not the 8 aimed at.  Both probe centroids must lie inside the centroid box, the cells 4 cells apart and
    clear of the body: the box is 10 x 10 x 3 coarse cells with the body through its middle, which leaves two positions along x, three
    along y and one along z (posed), two by two by one (canonical).  Where U is 0.14 m the bracket of U^2 (4 evaluation orders) is also
    as wide as the window, so some cells stay undetermined."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import oracle as O
import nn_cases as N
import nn_margin_cases as M

BODIES = [False, True]
PROBES = {False: {"world_fine": 64, "world_coarse": 5, "canon_fine": 64, "canon_coarse": 4},
          True: {"world_fine": 64, "world_coarse": 5, "canon_fine": 64, "canon_coarse": 4}}
LOST = {False: {"world_fine": (64, 19, 0, 0), "world_coarse": (4, 0, 0, 0), "canon_fine": (64, 56, 0, 0), "canon_coarse": (4, 0, 0, 0)},
        True: {"world_fine": (60, 0, 0, 0), "world_coarse": (5, 0, 0, 0), "canon_fine": (64, 63, 0, 0), "canon_coarse": (4, 0, 0, 0)}}
SETS = ("none", "margin_only", "guard_only", "shipped")


def test_fma_restatement_is_fmaf():
    """fma32 (float64 product, TwoSum, ties decided by the error term) against the C library's fmaf: random operands, operands of
    dsn_d2's magnitudes and sums built to land exactly half way between two float32"""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 3, 4000)).astype(np.float32)
    # half-way cases: c = 1, a * b = 2^-24 (1 + tiny) and 2^-24 (1 - tiny), 3 * 2^-24 +- tiny
    t = np.float32(2.0 ** -12)
    a = np.concatenate([a, [t, t, np.float32(3) * t, np.float32(3) * t, t]]).astype(np.float32)
    b = np.concatenate([b, [np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)),
                            np.nextafter(t, np.float32(0)), t]]).astype(np.float32)
    c = np.concatenate([c, [1, 1, 1, 1, 1]]).astype(np.float32)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    got = M.fma32(a, b, c)
    assert got.tobytes() == want.tobytes()
    assert len(set(want[-5:].tolist())) >= 2            # the half-way cases round both ways


@pytest.mark.parametrize("nonuniform", BODIES)
def test_cases_are_what_they_claim(nonuniform):
    """the probes did not move the grids (asserted by the builder), sit in their cells, are 4 cells apart, have centroids strictly
    inside the body's centroid box; the restated centroids and dsn_d2 winners are the oracle's; c_g attains U(B) and c* is p's nearest
    face in float64 and float32 for every probe that counts"""
    c = M.margin_case(nonuniform)
    F0 = c["base_F"]
    assert c["faces"].shape[0] == F0 + 4 * (M.N_FINE + M.N_COARSE)
    for space, v in (("world", c["xyz"]), ("canon", c["canon"])):
        cent = c["cent"][space]
        assert cent.tobytes() == O.centroids(v, c["faces"]).tobytes()
        assert (cent[F0:] > cent[:F0].min(0)).all() and (cent[F0:] < cent[:F0].max(0)).all()
    for lv in N.LEVELS:
        hdr, cent, pr = c["headers"][lv], c["cent"][lv.split("_")[0]], c["probes"][lv]
        assert len(pr) == PROBES[nonuniform][lv], (lv, len(pr))
        ijk = np.array([p["ijk"] for p in pr])
        for k in range(len(pr)):
            others = np.delete(ijk, k, 0)
            assert others.shape[0] == 0 or np.abs(others - ijk[k]).max(1).min() >= 4
        p = np.array([q["p"] for q in pr], np.float32)
        assert np.array_equal(N.cell_of(hdr, p), [q["cell"] for q in pr])
        # p lies outside its cell's own unguarded box on the crossed axis
        for q in pr:
            blo, bhi = M.cell_box(hdr, q["ijk"], np.float32(0))
            a = q["axis"]
            assert (q["p"][a] > bhi[a]) if q["side"] else (q["p"][a] < blo[a]), (lv, q["ijk"])
        n32 = M.nearest_d2(p, cent)
        assert np.array_equal(n32, O.nearest_face(p, cent))
        lost = c["verdict"][lv]["none"]
        n64 = M.nearest_f64(p, cent)[0]
        assert np.array_equal(n64[lost], [q["face_s"] for q, l in zip(pr, lost) if l])
        for q, l in zip(pr, lost):
            if l:
                r = M.restate_cell(hdr, cent, q["cell"], *M.PARAM_SETS["none"])
                blo, bhi = M.cell_box(hdr, q["ijk"], np.float32(0))
                assert int(np.argmin(M.box_dmax2(cent, blo, bhi)[0])) == q["face_g"] and r["u2_lo"] <= r["u2_plain"] <= r["u2_hi"]
        rels = [q["rel"] for q in pr]
        assert min(rels) >= M.REL_FROM - 1e-6 and max(rels) <= M.REL_TO and (len(pr) < 8 or len(set(np.round(rels, 9))) >= len(pr) // 4)


@pytest.mark.parametrize("nonuniform", BODIES)
def test_shipped_lists_certainly_hold_the_nearest_face_of_every_probe_point(nonuniform):
    """shipped guard and margin: on all four levels the restated list of the cell a probe point lies in (p, its +-1 / +-2 ulp
    neighbours, p pulled inside) certainly holds the point's float64 nearest face; the undetermined entries of the restatement stay
    under 1 % of the probe cells' entries"""
    c = M.margin_case(nonuniform)
    for lv in N.LEVELS:
        lists, cells = M.shipped_lists(nonuniform, lv)
        cent = c["cent"][lv.split("_")[0]]
        n64, ties = M.nearest_f64(c["points"][lv], cent)
        assert (ties == 1).all()
        held = np.array([lists[int(k)]["sure_in"][f] for k, f in zip(cells, n64)])
        assert held.all(), (lv, np.nonzero(~held)[0])
        entries = sum(int((~r["sure_out"]).sum()) for r in lists.values())
        open_ = sum(int((~r["sure_out"] & ~r["sure_in"]).sum()) for r in lists.values())
        print(f"nonuniform {nonuniform} {lv}: {len(lists)} cells, {entries} possible entries, {open_} undetermined")
        assert entries > 0 and open_ <= 0.01 * entries, (lv, open_, entries)


@pytest.mark.parametrize("nonuniform", BODIES)
def test_lists_without_the_margins_lose_the_nearest_face(nonuniform):
    """the counts of the module docstring, exactly: guard 0 and margin 1 lose p's nearest face in at least 32 cells of each fine level
    (and in every coarse cell the builder could make certain); guard 0 with the shipped margin loses it in the canonical fine level;
    the shipped guard with margin 1, and the shipped constants, lose nothing"""
    c = M.margin_case(nonuniform)
    for lv in N.LEVELS:
        got = tuple(int(c["verdict"][lv][s].sum()) for s in SETS)
        print(f"nonuniform {nonuniform} {lv}: lost under {dict(zip(SETS, got))}")
        assert got == LOST[nonuniform][lv], (lv, got)
        if lv.endswith("fine"):
            assert got[0] >= 32
        else:
            assert got[0] >= 4
        # a cell that loses the face with the shipped margin loses it with margin 1 too
        assert not (c["verdict"][lv]["margin_only"] & ~c["verdict"][lv]["none"]).any()


@pytest.mark.parametrize("nonuniform", BODIES)
def test_oracle_agrees_with_float64_on_every_probe_point(nonuniform):
    """O.nearest_face, O.warp (posed probes) and O.normal_world (canonical probes) name the float64 brute force's face on every probe
    point - there are no ties, so the two agree exactly - and a probe face as nearest face gives a canonical point / normal of its own"""
    c = M.margin_case(nonuniform)
    for lv in N.LEVELS:
        space = lv.split("_")[0]
        pts, cent = c["points"][lv], c["cent"][space]
        n64, ties = M.nearest_f64(pts, cent)
        assert (ties == 1).all()
        assert np.array_equal(O.nearest_face(pts, cent), n64), lv
        if space == "world":
            w = O.warp(pts, None, c["xyz"], c["canon"], c["faces"])
            assert np.array_equal(w["idx"], n64), lv
            if lv.endswith("fine"):
                assert (~w["transparent"]).mean() > 0.5, (lv, (~w["transparent"]).mean())      # a wrong index shows in x_c
        else:
            g = np.ones_like(pts)
            idx, n_w = O.normal_world(pts, g, c["canon"], c["xyz"], c["faces"])
            assert np.array_equal(idx, n64), lv


# ---------------------------------------------------------------------------------------------------------------------------
# the clear-cell margin: the restatement of dsn_make_face / dsn_project / dsn_face_clears_box
# ---------------------------------------------------------------------------------------------------------------------------
def _uvh64(p, tri):
    """(u, v, h) of points p for one triangle, in float64 from the formulas (utils/geo_utils.py project_point2mesh)"""
    v0, v1, v2 = (np.asarray(x, np.float64) for x in tri)
    a, b = v1 - v0, v2 - v0
    n = np.cross(a, b)
    n /= np.linalg.norm(n)
    t = np.asarray(p, np.float64) - v0
    h = t @ n
    w = t - h[:, None] * n
    d00, d01, d11 = b @ b, b @ a, a @ a
    d02, d12 = w @ b, w @ a
    inv = 1.0 / (d00 * d11 - d01 * d01)
    return (d11 * d02 - d01 * d12) * inv, (d00 * d12 - d01 * d02) * inv, h


def test_project_restatement_is_the_oracles():
    """make_face + project (float32 numpy) give the oracle's uv, h and transparency bit for bit: the posed probe points of the
    uniform body, each in the frame of its nearest face"""
    c = M.margin_case(False)
    pts = np.concatenate([c["points"]["world_fine"], c["points"]["world_coarse"]])
    o = O.warp(pts, None, c["xyz"], c["canon"], c["faces"])
    tri = c["xyz"][c["faces"][o["idx"]]]
    f = M.make_face(tri[:, 0], tri[:, 1], tri[:, 2])
    u, v, h = M.project(pts, f)
    assert np.stack([u, v], 1).tobytes() == o["uv"].tobytes() and h.tobytes() == o["h"].tobytes()
    tr = M.transparent(u, v, h)
    assert np.array_equal(tr, o["transparent"]) and tr.any() and not tr.all()


def test_clear_flag_restatement_at_its_limits():
    """the probe positions of nn_margin_cases.clear_configs on the restated grid of clear_scene: at least 20 have the guarded box's
    nearest corner within 8 ulp of its limit, both values of the flag occur for every kind, the shipped margin never flags what
    margin 0 does not, and where the restatement flags the cell every corner, face centre and 200 random points of the guarded box
    are transparent in float64.  Positions margin 0 flags although a float64 point of the GUARDED box is not transparent are counted
    (the margin's own job; samples never reach the guard band - test_gpu_nn_margins.py counts those)."""
    verts, faces = M.clear_scene()
    hdr = M.grid_header(M.centroids(verts, faces), "world_fine")
    ijk = np.array([int(x) // 2 for x in hdr["n"]])
    configs = M.clear_configs(hdr, ijk)
    blo, bhi = M.cell_box(hdr, ijk)
    rng = np.random.default_rng(3)
    t = np.concatenate([np.stack(np.meshgrid(*[[0.0, 0.5, 1.0]] * 3, indexing="ij"), -1).reshape(-1, 3), rng.uniform(0, 1, (200, 3))])
    box = blo.astype(np.float64) + t * (bhi.astype(np.float64) - blo)
    seen, wrong0 = set(), 0
    for cf in configs:
        u, v, h = _uvh64(box, cf["tri"])
        clear64 = (np.abs(h) > 0.1) | (u > 5) | (u < -4) | (v > 5) | (v < -4)
        if cf["flag"]:
            assert cf["flag0"] and clear64.all(), (cf["kind"], cf["k"])
        wrong0 += int(cf["flag0"] and not clear64.all())
        seen.add((cf["kind"], cf["flag"]))
    print(f"{len(configs)} positions; flagged with margin 0 although a float64 point of the guarded box is not transparent: {wrong0}")
    assert sum(cf["at_limit"] for cf in configs) >= 20
    assert seen == {(k, fl) for k in M.CLEAR_KINDS for fl in (False, True)}
