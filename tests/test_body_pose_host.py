"""The body model's rule (include/dsnerf.h, dsn_body_shape / dsn_body_pose) on the CPU: the numpy restatement tests/body_pose_restate.py
against the reference's own outputs (tests/golden/body_pose.npz, made by tests/golden/make_golden_body_pose.py), against its float64
twin and against closed forms; BodyModel's loaders; the library's argument checks.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import body_pose_restate as BP
from helpers import GOLDEN

U = 2.0 ** -24          # unit roundoff of float32


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "body_pose.npz"))


@pytest.fixture(scope="module")
def bars():
    with open(os.path.join(GOLDEN, "body_pose_errors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def clip(g):
    """the fixture's clip on the small body, recomputed: (model arrays, v_shaped, joints, the restatement's outputs)"""
    from dsnerf_amd import synth
    canon, _ = synth.make_small_body()
    vt, w, Jr, sd, pd = BP.make_model(canon)
    vs, jn = BP.shape(vt, sd, g["clip:betas"], Jr)
    e = BP.pose(vs, jn, BP.SMPL_PARENTS, w, pd, g["clip:poses"], g["clip:Rh"], g["clip:Th"])
    return (vt, w, Jr, sd, pd), vs, jn, e


def ulps(a, b):
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return np.where((a == 0) & (b == 0), 0, d)


TABLES = {"smpl": BP.SMPL_PARENTS, "chain": BP.CHAIN_PARENTS, "star": BP.STAR_PARENTS}


def test_joint_transforms_are_the_references(g):
    """A against utils/h36m_utils.get_rigid_transformation run in float64 on the same values: both sides compute in float64 and round
    once, so an element may differ by one float32 ulp where a float64 last-bit difference straddles a rounding boundary - and on
    the fixture's cases at least 99 % of the elements agree bit for bit"""
    equal = total = 0
    for tn, parents in TABLES.items():
        assert np.array_equal(g[f"parents:{tn}"], parents)
        for pn in ("poses", "zero", "beyond_pi", "tiny"):
            A, pf = BP.chain(g[f"poses:{pn}"], g["joints"], parents)
            ref = g[f"A:{tn}:{pn}"]
            assert A.dtype == np.float32 and A.shape == ref.shape and pf.shape == (ref.shape[0], 207)
            u = ulps(A, ref)
            assert int(u.max()) <= 1, (tn, pn, int(u.max()))
            equal, total = equal + int((u == 0).sum()), total + u.size
    assert equal / total >= 0.99, equal / total
    assert (np.linalg.norm(g["poses:beyond_pi"], axis=-1) > np.pi).any() and float(np.abs(g["poses:tiny"]).max()) <= 2e-9
    assert not g["poses:zero"].any()


def test_bounds_are_the_references(g, clip):
    e = clip[3]
    assert np.array_equal(e["xyz"].view(np.uint32), g["clip:xyz"].view(np.uint32))      # the vertices the reference padded
    for key, mode in (("zju_train", BP.PAD_ZJU_TRAIN), ("zju_eval", BP.PAD_ZJU_EVAL), ("h36m", BP.PAD_H36M)):
        got = BP.bounds(e["xyz"], mode)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), g[f"bounds:{key}"].view(np.uint32)), key
    none = BP.bounds(e["xyz"], BP.PAD_NONE)
    assert np.array_equal(none[:, 0], e["xyz"].min(axis=1)) and np.array_equal(none[:, 1], e["xyz"].max(axis=1))


def test_bounds_order_and_nan_rule():
    x = np.array([[[0.0, 1.0, -2.0], [-0.0, 3.0, np.nan], [0.0, -1.0, 5.0]]], np.float32)
    b = BP.bounds(x, BP.PAD_NONE)
    assert np.signbit(b[0, 0, 0]) and not np.signbit(b[0, 1, 0])            # -0 below +0
    assert b[0, 0, 1] == -1.0 and b[0, 1, 1] == 3.0
    assert np.isnan(b[0, :, 2]).all()                                       # a NaN on the axis: both bounds
    assert np.isnan(BP.bounds(x, BP.PAD_H36M)[0, :, 2]).all()


def vertex_bar(pf, pd, w, A, vp, xs, Rh32, Th):
    """|float32 result - float64 twin| of the vertex work, from its operation counts (u = 2^-24, gamma(n) = n u / (1 - n u), the
    standard bound of an n-operation chain relative to the sum of the magnitudes of its terms):
      v_posed   207 products and 207 additions in a chain (gamma(208) S, S = sum_k |pf_k posedirs_k|) and the addition of v_shaped (u M_v)
      T         24 products, 24 additions (gamma(25) M_T, M_T = sum_j w_j |A_j|, per element, maximum taken)
      xyz_smpl  3 products, 3 additions on inexact operands: 3 (e_T M_v + M_T e_vp) + e_T + gamma(4) (3 M_T M_v + M_T)
      xyz       the same with Rh_mat (exact float32 input, |R| <= M_R) and Th: 3 M_R e_xs + gamma(4) (3 M_R M_xs + M_Th)
    Returns (e_vp, e_xs, e_xyz)."""
    f = lambda a: np.abs(np.asarray(a, np.float64))      # noqa: E731
    S = float((f(pf) @ f(pd)).max()) if pd is not None else 0.0
    M_v, M_xs = float(f(vp).max()), float(f(xs).max())
    M_T = float(np.einsum("vj,pje->pve", f(w), f(A).reshape(A.shape[0], 24, 16)).max())
    M_R, M_Th = float(f(Rh32).max()), float(f(Th).max()) if Th is not None else 0.0
    e_vp = gamma(208) * S + U * M_v
    e_T = gamma(25) * M_T
    e_xs = 3 * (e_T * M_v + M_T * e_vp) + e_T + gamma(4) * (3 * M_T * M_v + M_T)
    e_xyz = 3 * M_R * e_xs + gamma(4) * (3 * M_R * M_xs + M_Th)
    return e_vp, e_xs, e_xyz


def test_float32_vertices_against_the_float64_twin(g, clip):
    (vt, w, Jr, sd, pd), vs, jn, e = clip
    vp64, xs64, xyz64 = BP.vertices(vs, w, pd, e["pf"], e["A"], e["Rh_mat"], g["clip:Th"], dtype=np.float64)
    assert vp64.dtype == np.float64
    e_vp, e_xs, e_xyz = vertex_bar(e["pf"], pd, w, e["A"], e["v_posed"], e["xyz_smpl"], e["Rh_mat"], g["clip:Th"])
    assert e_xyz < 2e-4                                   # the bar is a float32 bar, not a loose one
    for name, got, want, bar in (("v_posed", e["v_posed"], vp64, e_vp), ("xyz_smpl", e["xyz_smpl"], xs64, e_xs), ("xyz", e["xyz"], xyz64, e_xyz)):
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{name}: |float32 - float64| = {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (name, err, bar)


def one_hot_model(V=96, seed=5):
    from dsnerf_amd import synth
    vt = ((synth.hash_uniform(3 * V, seed).reshape(V, 3) - np.float32(0.5)) * np.float32(1.5)).astype(np.float32)
    owner = (np.arange(V) * 7) % 24
    w = np.zeros((V, 24), np.float32)
    w[np.arange(V), owner] = 1.0
    joints = ((synth.hash_uniform(72, seed + 1).reshape(24, 3) - np.float32(0.5)) * np.float32(1.2)).astype(np.float32)
    return vt, w, joints, owner


def test_a_single_rotated_joint_moves_its_subtree_rigidly():
    vt, w, joints, owner = one_hot_model()
    j = 16                                                 # SMPL's left shoulder: the subtree 16, 18, 20, 22
    subtree = np.isin(owner, [16, 18, 20, 22])
    poses = np.zeros((1, 24, 3), np.float32)
    poses[0, j] = (0.3, -0.8, 0.5)
    e = BP.pose(vt, joints, BP.SMPL_PARENTS, w, None, poses)
    R = BP.rodrigues(poses[0, j:j + 1].astype(np.float64))[0]
    want = vt.astype(np.float64).copy()
    want[subtree] = (vt[subtree].astype(np.float64) - joints[j]) @ R.T + joints[j]
    bar = vertex_bar(e["pf"], None, w, e["A"], e["v_posed"], e["xyz_smpl"], e["Rh_mat"], None)[2] + 4 * U * 2.0      # + A's own rounding
    assert subtree.any() and not subtree.all()
    assert float(np.abs(e["xyz"][0] - want).max()) <= bar
    assert np.array_equal(e["xyz"][0][~subtree], vt[~subtree])            # the rest of the body does not move at all
    assert float(np.abs(e["xyz"][0][subtree] - vt[subtree]).max()) > 0.05


def test_identity_pose_posedirs_zero_and_rh_th(clip):
    (vt, w, Jr, sd, pd), vs, jn, e = clip
    V = vs.shape[0]
    zero = np.zeros((2, 24, 3), np.float32)
    z = BP.pose(vs, jn, BP.SMPL_PARENTS, w, pd, zero)
    bar = vertex_bar(z["pf"], pd, w, z["A"], z["v_posed"], z["xyz_smpl"], z["Rh_mat"], None)[2] + 4 * U * 2.0
    assert not z["pf"].any() and np.array_equal(z["v_posed"][0], vs)      # R = I exactly: no pose feature, no blend-shape offset
    assert float(np.abs(z["xyz"][0].astype(np.float64) - vs).max()) <= bar
    assert np.array_equal(z["Rh_mat"][0], np.eye(3, dtype=np.float32))
    # posedirs = 0 is the call without posedirs
    from dsnerf_amd import synth
    poses = np.stack([synth.make_poses(s) for s in (61, 62)])
    a = BP.pose(vs, jn, BP.SMPL_PARENTS, w, np.zeros((207, 3 * V), np.float32), poses)
    b = BP.pose(vs, jn, BP.SMPL_PARENTS, w, None, poses)
    for k in ("xyz", "xyz_smpl", "v_posed", "bounds"):
        assert np.array_equal(a[k], b[k]), k
    # Rh / Th: xyz = Rh_mat . xyz_smpl + Th, and xyz_smpl does not know about them
    Rh = (synth.hash_normal(6, 71) * np.float32(0.9)).reshape(2, 3)
    Th = (synth.hash_normal(6, 72) * np.float32(1.1)).reshape(2, 3)
    c = BP.pose(vs, jn, BP.SMPL_PARENTS, w, pd, poses, Rh, Th)
    d = BP.pose(vs, jn, BP.SMPL_PARENTS, w, pd, poses)
    assert np.array_equal(c["xyz_smpl"], d["xyz_smpl"]) and np.array_equal(d["xyz"], d["xyz_smpl"])
    want = np.einsum("prc,pvc->pvr", c["Rh_mat"].astype(np.float64), c["xyz_smpl"].astype(np.float64)) + Th.astype(np.float64)[:, None]
    assert float(np.abs(c["xyz"] - want).max()) <= gamma(4) * (3 * float(np.abs(c["xyz_smpl"]).max()) + float(np.abs(Th).max()))
    only_th = BP.pose(vs, jn, BP.SMPL_PARENTS, w, pd, poses, None, Th)
    assert np.array_equal(only_th["xyz"], d["xyz_smpl"] + Th[:, None].astype(np.float32))
    R64 = BP.rodrigues(Rh.astype(np.float64))
    # a rotation up to the reference's 1e-8 in the angle (the axis p / |p + 1e-8| is not quite a unit vector: 1.7e-8 / |p| at most)
    assert float(np.abs(R64 @ R64.transpose(0, 2, 1) - np.eye(3)).max()) < 4 * 1.74e-8 / float(np.linalg.norm(Rh, axis=1).min())


def test_pose_feature_layout_is_smpls():
    """SMPL's pose feature is (R_1 .. R_23 minus I) flattened row-major, and posedirs[v, c, k] (the pickle's layout) moves coordinate c
    of vertex v by feature k: one non-zero entry of posedirs and one joint turned about z by a known angle moves exactly one
    coordinate by a known amount.  Feature 9 (j - 1) + 3 r + c of joint j = 7 is R_7[r, c] - (r == c): [0, 1] is -sin, [1, 0] is
    +sin, [0, 0] is cos - 1 (each to the reference's 1e-8 in the angle)."""
    from dsnerf_amd.body import BodyModel
    V, j, v, theta, d = 40, 7, 13, 0.7, 0.5
    vt, _, Jr, _, _ = BP.make_model(V)
    w = np.zeros((V, 24), np.float32)
    w[:, 0] = 1.0                                                  # the body rides on the root, which does not move
    joints = BP.shape(vt, None, None, Jr)[1]
    poses = np.zeros((1, 24, 3), np.float32)
    poses[0, j, 2] = theta
    for (r, c), coord, want in (((0, 1), 0, -np.sin(theta)), ((1, 0), 2, np.sin(theta)), ((0, 0), 1, np.cos(theta) - 1.0)):
        pickled = np.zeros((V, 3, 207), np.float32)
        pickled[v, coord, 9 * (j - 1) + 3 * r + c] = d
        pd = BodyModel(vt, w, BP.SMPL_PARENTS, joints=joints, posedirs=pickled, device="cpu").posedirs.numpy()
        e = BP.pose(vt, joints, BP.SMPL_PARENTS, w, pd, poses)
        assert abs(float(e["pf"][0, 9 * (j - 1) + 3 * r + c]) - want) < 1e-6
        moved = e["xyz"][0].astype(np.float64) - vt
        assert abs(moved[v, coord] - want * d) < 1e-6 and abs(want * d) > 0.1
        moved[v, coord] = 0.0
        assert float(np.abs(moved).max()) < 1e-6, ((r, c), float(np.abs(moved).max()))      # nothing else moves
        # the neighbouring feature indices are other entries of R_7 - I: zero for a turn about z, or a different value
        other = np.zeros((V, 3, 207), np.float32)
        other[v, coord, 9 * (j - 1) + 3 * 2 + 2] = d                # R_7[2, 2] - 1 = 0
        e0 = BP.pose(vt, joints, BP.SMPL_PARENTS, w, np.ascontiguousarray(other.reshape(3 * V, 207).T), poses)
        assert float(np.abs(e0["xyz"][0].astype(np.float64) - vt).max()) < 1e-6


def test_round_trip_through_the_references_inverse(g, clip, bars):
    """utils/blend_utils.ppts_to_pts(xyz_smpl, weights, A), run by the fixture's generator in float32 on this restatement's outputs,
    returns v_posed within twice the reference's own float32 distance from its float64 run on the same inputs"""
    e = clip[3]
    for k in ("xyz_smpl", "v_posed", "A"):                 # what the generator handed the reference is what the restatement makes today
        assert np.array_equal(e[k].view(np.uint32), g[f"clip:{k}"].view(np.uint32)), k
    own = bars["ppts_to_pts_f32_vs_f64"]
    assert 1e-8 < own < 1e-5
    err = float(np.abs(g["clip:ppts_to_pts"].astype(np.float64) - e["v_posed"].astype(np.float64)).max())
    print(f"round trip: {err:.3e}, the reference's float32 - float64 distance {own:.3e}")
    assert err <= 2 * own, (err, own)


def test_bad_parents_are_rejected():
    for bad in (np.r_[-1, np.arange(1, 24)], np.r_[-1, 0, -1, np.zeros(21, int)], np.arange(-1, 22)):
        with pytest.raises(ValueError):
            BP.check_parents(bad)


# ---- BodyModel's loaders (device="cpu": layouts only) ------------------------------------------------------------------------------
def test_body_model_from_a_pickle_shaped_dict():
    import scipy.sparse
    from dsnerf_amd.body import BodyModel
    V, B = 37, 10
    vt, w, Jr, sd, pd = BP.make_model(V)
    kin = np.stack([BP.SMPL_PARENTS.astype(np.int64), np.arange(24)]).astype(np.uint32)      # 2^32 - 1 in front, as in the pickle
    assert kin[0, 0] == 2 ** 32 - 1
    pickle_pd = np.ascontiguousarray(pd.T.reshape(V, 3, 207))
    m = BodyModel.from_smpl_dict({"v_template": vt.astype(np.float64), "weights": w.astype(np.float64), "kintree_table": kin,
                                  "J_regressor": scipy.sparse.csc_matrix(Jr.astype(np.float64)), "shapedirs": sd.astype(np.float64),
                                  "posedirs": pickle_pd.astype(np.float64), "f": np.zeros((1, 3), np.uint32)}, device="cpu")
    assert m.V == V and np.array_equal(m.parents, BP.SMPL_PARENTS) and list(m._parents_c) == list(BP.SMPL_PARENTS)
    assert tuple(m.posedirs.shape) == (207, 3 * V) and m.posedirs.is_contiguous() and np.array_equal(m.posedirs.numpy(), pd)
    assert m.posedirs[5, 3 * 11 + 2] == float(pickle_pd[11, 2, 5])
    assert np.array_equal(m.J_regressor.numpy(), Jr) and np.array_equal(m.shapedirs.numpy(), sd) and tuple(m.shapedirs.shape) == (V, 3, B)
    assert np.array_equal(m.v_template.numpy(), vt) and np.array_equal(m.weights.numpy(), w)
    assert all(t.dtype.is_floating_point and t.element_size() == 4 for t in (m.v_template, m.weights, m.posedirs, m.shapedirs, m.J_regressor))
    same = BodyModel(vt, w, BP.SMPL_PARENTS, J_regressor=Jr, posedirs=pd, device="cpu")      # the kernel's layout is taken as it is
    assert np.array_equal(same.posedirs.numpy(), pd)
    with pytest.raises(ValueError):
        BodyModel(vt, w, BP.SMPL_PARENTS, J_regressor=Jr, posedirs=pd[:, :-3], device="cpu")
    with pytest.raises(ValueError):
        BodyModel(vt, w, np.r_[-1, np.arange(1, 24)], J_regressor=Jr, device="cpu")          # a parent that is not an earlier joint
    with pytest.raises(ValueError):
        BodyModel(vt, w, BP.SMPL_PARENTS, device="cpu")                                      # neither a regressor nor joints
    with pytest.raises(ValueError):
        BodyModel(vt, w[:, :23], BP.SMPL_PARENTS, J_regressor=Jr, device="cpu")


def test_body_model_from_the_lbs_arrays(tmp_path):
    from dsnerf_amd.body import BodyModel
    V = 29
    vt, w, Jr, _, _ = BP.make_model(V)
    joints = BP.shape(vt, None, None, Jr)[1]
    arrays = {"joints": joints, "parents": BP.SMPL_PARENTS.astype(np.int64), "weights": w, "tvertices": vt}
    for k, a in arrays.items():
        np.save(tmp_path / f"{k}.npy", a)
    for src in (arrays, str(tmp_path)):
        m = BodyModel.from_lbs_dir(src, device="cpu")
        assert m.V == V and m.posedirs is None and m.shapedirs is None and m.J_regressor is None
        assert np.array_equal(m.joints.numpy(), joints) and np.array_equal(m.v_shaped.numpy(), vt) and np.array_equal(m.weights.numpy(), w)
        assert np.array_equal(m.parents, BP.SMPL_PARENTS)


# ---- the library's argument checks (no device work is reached) ---------------------------------------------------------------------------
def test_library_argument_checks():
    import dsnerf_amd
    lib = dsnerf_amd._lib.lib()
    one, z = C.c_void_p(256), None
    good = (C.c_int32 * 24)(*[int(x) for x in BP.SMPL_PARENTS])

    def pose(v_shaped=one, joints=one, parents=good, weights=one, V=5, poses=one, P=2, pad=0, xyz=one, ws=one, ws_bytes=1 << 30):
        return lib.dsn_body_pose(v_shaped, joints, parents, weights, z, V, poses, z, z, P, pad, xyz, z, z, z, z, ws, ws_bytes, z)

    def refused(rc, text):
        assert rc != 0 and b"dsn_body_pose" in lib.dsn_last_error() and text in lib.dsn_last_error(), lib.dsn_last_error()

    refused(pose(v_shaped=z), b"null")
    refused(pose(joints=z), b"null")
    refused(pose(parents=z), b"null")
    refused(pose(weights=z), b"null")
    refused(pose(poses=z), b"null")
    refused(pose(xyz=z), b"null")
    refused(pose(ws=z), b"workspace")
    refused(pose(ws=C.c_void_p(8)), b"aligned")
    refused(pose(ws_bytes=16), b"too small")
    refused(pose(V=0), b"V must be")
    refused(pose(V=-3), b"V must be")
    refused(pose(P=-1), b"negative")
    refused(pose(pad=4), b"pad_mode")
    refused(pose(pad=-1), b"pad_mode")
    for i, v in ((1, 1), (5, 7), (23, -1), (2, 2)):
        bad = (C.c_int32 * 24)(*[int(x) for x in BP.SMPL_PARENTS])
        bad[i] = v
        refused(pose(parents=bad), b"parents")
    anything = (C.c_int32 * 24)(*[int(x) for x in BP.SMPL_PARENTS])
    anything[0] = 12345                                    # entry 0 is ignored
    # P = 0: an empty clip is a valid call that launches nothing - outputs, poses and workspace may be null
    assert pose(parents=anything, P=0, poses=z, xyz=z, ws=z, ws_bytes=0) == 0
    refused(pose(P=0, weights=z), b"null")                 # ... but the model is still checked
    wsb = lib.dsn_body_pose_workspace_bytes
    assert wsb(6890, 0) == 0 and wsb(0, 4) == 0 and wsb(-1, 4) == 0 and wsb(6890, -1) == 0
    assert 0 < wsb(1, 1) <= wsb(6890, 1) < wsb(6890, 64) < wsb(6890, 512) and wsb(6890, 64) % 256 == 0
    assert wsb(6890, 512) < 512 * 4096                     # a few KB per pose: features, transforms, partial bounds

    def shape(vt=one, sd=z, betas=z, B=0, Jr=z, V=5, vs=one, joints=z):
        return lib.dsn_body_shape(vt, sd, betas, B, Jr, V, vs, joints, z)
    for rc in (shape(vt=z), shape(vs=z), shape(V=0), shape(B=-1), shape(sd=one, B=3), shape(betas=one, B=3), shape(Jr=one), shape(joints=one)):
        assert rc != 0 and b"dsn_body_shape" in lib.dsn_last_error(), lib.dsn_last_error()
