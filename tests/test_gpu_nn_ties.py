"""GPU: the nearest-face tie rule and the grids' cell edges on every search path.

Every path of the exact nearest-face search (exhaustive sweep, per-lane list walks, the fused cell-major search with its per-wave
pruning, lazily built lists, k_normal's cooperative sweep, the segmented far search of training batches) must return the index the
serial ascending sweep with strict '<' returns - among equal distances the FIRST index.  Random points never tie; the cases of
tests/nn_cases.py do: twinned faces on both bodies in both face orders, a dyadic lattice soup with exact 2-, 4- and 8-way ties, and
points on the cell boundaries and outer faces of the grids.  Each test also asserts that its ties are present and that the intended
path ran (levels ok = 1, sample counts above the fused / far-search thresholds)."""
import functools
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


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _packed():
    from dsnerf_amd import _lib
    return _lib.PackedParams(DEV).update({k: torch.from_numpy(v) for k, v in state().items()})


def _scene(canon, faces, xyz):
    """a Scene with every level of both meshes built (no lazy, not fine-only), each asserted to fit (ok = 1, no overflow warning)"""
    from dsnerf_amd import _lib, synth
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sc = _lib.Scene(torch.from_numpy(canon), torch.from_numpy(np.asarray(faces, np.int64)), DEV)
        sc.set_frame(_packed(), torch.from_numpy(xyz), torch.from_numpy(synth.make_poses()), 5)
        st = _lib.nn_stats(sc)
        assert sc.nn_watch(wait=True) == {}
    for name, (ncell, ok, total, cap) in st.items():
        assert ok == 1 and 0 < total <= cap, (name, st)
    return sc


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _classes(sc, pts, mesh):
    """0: inside the fine grid, 1: outside it and inside the coarse one, 2: outside both"""
    cf = N.cell_of(N.read_header(sc, mesh + "_fine"), pts)
    cc = N.cell_of(N.read_header(sc, mesh + "_coarse"), pts)
    return np.where(cf >= 0, 0, np.where(cc >= 0, 1, 2))


def _world_points(sc, case):
    """the world queries around the twinned faces + points on the cell boundaries of both posed levels and on their outer faces"""
    q = case["q_world"]
    k = q.shape[0] // 3
    hf, hc = N.read_header(sc, "world_fine"), N.read_header(sc, "world_coarse")
    edges = [N.edge_points(hf, q[:k:2]), N.edge_points(hf, q[:k:5], outer=True), N.edge_points(hc, q[k:2 * k:2]),
             N.edge_points(hc, q[k:2 * k:5], outer=True)]
    return np.concatenate([q] + edges), q.shape[0]


# ---------------------------------------------------------------------------------------------------------------------------
# stage calls on the twinned bodies
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", N.ORDERS)
@pytest.mark.parametrize("nonuniform", [False, True])
def test_warp_and_lbs_warp_keep_the_first_index_of_a_tie(nonuniform, order):
    """dsn_warp through the lists and through the exhaustive sweep, dsn_lbs_warp both ways: face index, uv, h, x_c and the
    transparency flag equal the oracle bit for bit, on tied points in the fine grid, the coarse shell and beyond, and on the cell
    boundaries / outer faces of both posed levels"""
    from dsnerf_amd import _lib, synth
    case = N.twin_case(nonuniform, order)
    sc = _scene(case["canon"], case["faces"], case["xyz"])
    pts, nq = _world_points(sc, case)
    o = O.warp(pts, None, case["xyz"], case["canon"], case["faces"])
    tied = N.tie_mask(case, o["idx"], "world")
    cls = _classes(sc, pts, "world")
    for c in range(3):          # ties in every level (the queries' thirds: surface, shell, beyond)
        assert tied[:nq][cls[:nq] == c].sum() >= 100, (c, tied[:nq][cls[:nq] == c].sum())
    assert tied[nq:].sum() >= 200 and (cls[nq:] == 0).sum() > 0 and (cls[nq:] == 1).sum() > 0 and (cls[nq:] == 2).sum() > 0
    assert np.isin(o["idx"][tied], case["first"]).all()
    for exhaustive in (False, True):
        a = _lib.warp(sc, T(pts), None, 1, want_dir=False, want_uvh=True, exhaustive=exhaustive)
        assert _same(a["face_idx"].cpu().numpy(), o["idx"]), exhaustive
        for k in ("uv", "h", "x_c"):
            assert _same(a[k].cpu().numpy(), o[k]), (k, exhaustive)
        assert _same(a["transparent"].cpu().numpy().astype(bool), o["transparent"]), exhaustive
    W = synth.make_skin_weights(case["xyz"].shape[0])
    A = synth.make_joint_transforms()
    ol = O.lbs_warp(pts, case["xyz"], case["faces"], W, A, 0)
    for exhaustive in (False, True):
        b = _lib.lbs_warp(sc, T(pts), torch.from_numpy(W), torch.from_numpy(A), "rigid_center", exhaustive=exhaustive)
        assert _same(b["face_idx"].cpu().numpy(), ol["idx"]), exhaustive


def _waves(inside, outside, rng):
    """x_c rows laid out in waves of 64 for k_normal: waves with 1-3 lanes outside the canonical fine grid (the cooperative sweep,
    dsn_wave_argmin), waves with every lane outside (the per-lane walk) and waves inside only.  Returns (rows, kind per row)."""
    inside, outside = list(rng.permutation(inside)), list(rng.permutation(outside))
    rows, kind = [], []
    n_all = len(outside) // 2 // 64
    for _ in range(n_all):
        rows += [outside.pop() for _ in range(64)]
        kind += [2] * 64
    j = 0
    while outside and len(inside) >= 63:
        m = min(1 + j % 3, len(outside))
        w = [inside.pop() for _ in range(64 - m)] + [outside.pop() for _ in range(m)]
        lane = rng.permutation(64)
        rows += [w[i] for i in lane]
        kind += [1 if lane_i >= 64 - m else 0 for lane_i in lane]
        j += 1
    while len(inside) >= 64:
        rows += [inside.pop() for _ in range(64)]
        kind += [0] * 64
    return np.array(rows), np.array(kind)


@pytest.mark.parametrize("order", N.ORDERS)
@pytest.mark.parametrize("nonuniform", [False, True])
def test_normals_keep_the_first_index_of_a_canonical_tie(nonuniform, order):
    """dsn_shade (k_normal): the canonical face index and the world normal of the list search equal the exhaustive sweep's and the
    oracle's bit for bit - on tied points inside the canonical fine grid (per-lane walk), outside it in waves where 1-3 lanes are
    (the wave-cooperative coarse / full sweep and its (distance, index) shuffle reduction) and in waves where all lanes are"""
    from dsnerf_amd import _lib
    case = N.twin_case(nonuniform, order)
    sc = _scene(case["canon"], case["faces"], case["xyz"])
    q = case["q_canon"]
    k = q.shape[0] // 3
    hf, hc = N.read_header(sc, "canon_fine"), N.read_header(sc, "canon_coarse")
    q = np.concatenate([q, N.edge_points(hf, q[:k:3]), N.edge_points(hf, q[:k:7], outer=True), N.edge_points(hc, q[k:2 * k:7], outer=True)])
    cls = _classes(sc, q, "canon")
    rng = np.random.default_rng(17)
    rows, kind = _waves(np.nonzero(cls == 0)[0], np.nonzero(cls > 0)[0], rng)
    x_c = q[rows]
    n = x_c.shape[0]
    grad = rng.standard_normal((n, 3)).astype(np.float32)
    x_w = rng.standard_normal((n, 3)).astype(np.float32)
    rd = rng.standard_normal((n, 3)).astype(np.float32)
    ess = rng.random((n, 3)).astype(np.float32)
    oi, on = O.normal_world(x_c, grad, case["canon"], case["xyz"], case["faces"])
    tied = N.tie_mask(case, oi, "canon")
    assert tied[kind == 0].sum() >= 300 and tied[kind == 1].sum() >= 20 and tied[kind == 2].sum() >= 300, \
        [int(tied[kind == c].sum()) for c in range(3)]
    assert (cls[rows][kind == 1] == 1).any() and (cls[rows][kind == 1] == 2).any()      # coarse lists and the full sweep, cooperatively
    res = {}
    for exhaustive in (False, True):
        idx, n_w, _ = _lib.shade(sc, _packed(), T(x_c), T(grad), T(x_w), T(rd), T(ess), 1, exhaustive=exhaustive)
        res[exhaustive] = (idx.cpu().numpy(), n_w.cpu().numpy())
        assert _same(res[exhaustive][0], oi), exhaustive
        assert _same(res[exhaustive][1], on), exhaustive
    assert _same(res[False][1], res[True][1])


def test_dyadic_soup_exact_ties_on_every_stage_path():
    """the lattice soup's exact 2-, 4- and 8-way ties between distinct centroids (shuffled face order): warp (lists / sweep),
    lbs_warp and k_normal (lists / sweep) return the smallest index of every tied set - the float64 lexicographic minimum"""
    from dsnerf_amd import _lib, synth
    s = N.dyadic_soup()
    verts, faces = s["verts"], s["faces"]
    canon = (verts * np.float32(0.5)).astype(np.float32)          # (exact: ties survive the scaling)
    sc = _scene(canon, faces, verts)
    pts = s["pts"]
    assert (s["mult"] > 1).sum() >= 800
    hf = N.read_header(sc, "world_fine")
    assert (N.cell_of(hf, pts) >= 0).all()
    o = O.warp(pts, None, verts, canon, faces)
    assert _same(o["idx"], s["win"])
    for exhaustive in (False, True):
        a = _lib.warp(sc, T(pts), None, 1, want_dir=False, want_uvh=True, exhaustive=exhaustive)
        assert _same(a["face_idx"].cpu().numpy(), s["win"]), exhaustive
        for k in ("uv", "h", "x_c"):
            assert _same(a[k].cpu().numpy(), o[k]), (k, exhaustive)
        W = synth.make_skin_weights(verts.shape[0])
        b = _lib.lbs_warp(sc, T(pts), torch.from_numpy(W), torch.from_numpy(synth.make_joint_transforms()), "rigid_center",
                          exhaustive=exhaustive)
        assert _same(b["face_idx"].cpu().numpy(), s["win"]), exhaustive
        # canonical: the same ties at half scale, and the same queries moved 3 m out (the cooperative / full sweeps of k_normal)
        x_c = np.concatenate([pts * np.float32(0.5), pts * np.float32(0.5) + np.float32(3.0)]).astype(np.float32)
        rng = np.random.default_rng(5)
        g = rng.standard_normal(x_c.shape).astype(np.float32)
        idx, n_w, _ = _lib.shade(sc, _packed(), T(x_c), T(g), T(x_c), T(g), T(np.abs(g)), 1, exhaustive=exhaustive)
        assert _same(idx.cpu().numpy()[:pts.shape[0]], s["win"]), exhaustive
        assert _same(idx.cpu().numpy(), O.nearest_face(x_c, O.centroids(canon, faces))), exhaustive


# ---------------------------------------------------------------------------------------------------------------------------
# frames and a training batch on the twinned body
# ---------------------------------------------------------------------------------------------------------------------------
def test_twinned_frame_every_search_form_equals_the_sweep(monkeypatch):
    """a 256 x 256 x 64 frame of the twinned body (4.2 M samples: the sampler's classification, the fused cell-major search + warp
    with its per-wave pruning): lazily built lists, every cell's lists and DSN_NN_UNFUSED (k_warp's per-lane walk) give the frame
    of the exhaustive sweep bit for bit, in both face orders; the two orders give different frames (the ties reach the image) and
    both equal the oracle on a ray subset"""
    from dsnerf_amd import _lib
    S, HW = 64, 256
    assert HW * HW * S >= 1 << 20           # = DSN_CELLMAJOR_MIN: the fused search runs
    colour = {}
    for order in N.ORDERS:
        case = N.twin_case(False, order)
        canon, faces, batch = full_frame(hw=HW)
        assert np.array_equal(canon, case["base_canon"]) and np.array_equal(batch["xyz"][0].numpy(), case["base_xyz"])
        batch["xyz"] = torch.from_numpy(case["xyz"])[None]
        r = renderer_with(state(), case["canon"], case["faces"])
        r.eval()
        r.early_stop = False
        o, d = r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0])
        pk = r.net.packed(r.device)

        def run(lazy, **kw):
            r._set_frame(batch, lazy=lazy)
            assert r.scene.lazy == lazy
            n, f = r._dev(batch["near"][0]).clone(), r._dev(batch["far"][0]).clone()
            out = _lib.render_rays(r.scene, pk, _lib.RenderWorkspace(r.device), o, d, n, f, S, r._t_vals(S), screen=False, **kw)
            torch.cuda.synchronize()
            assert r.scene.nn_overflow == {}
            h = N.read_header(r.scene, "world_fine")
            assert h["total"] <= h["cap"] and (h["lazy"] == 2 if lazy and not kw else h["ok"] == 1), (lazy, kw, h)
            return out

        ref = run(False, exhaustive=True)
        forms = {"lazy": run(True), "full": run(False)}
        monkeypatch.setenv("DSN_NN_UNFUSED", "1")
        forms["unfused"] = run(False)
        monkeypatch.delenv("DSN_NN_UNFUSED")
        for name, out in forms.items():
            for k in ("color", "acc_map", "depth_map", "weights", "z_vals"):
                assert torch.equal(torch.nan_to_num(out[k], nan=-1.0), torch.nan_to_num(ref[k], nan=-1.0)), (order, name, k)
        assert float(ref["acc_map"].max()) > 0.05
        # ties among the frame's samples (every 5th ray), inside the posed fine grid
        z = ref["z_vals"][::5]
        pts = (o[::5, None, :] + d[::5, None, :] * z[..., None]).reshape(-1, 3)
        w = _lib.warp(r.scene, pts, None, 1, want_dir=False, exhaustive=True)
        nt = int(N.tie_mask(case, w["face_idx"].cpu().numpy(), "world").sum())
        print(f"order {order}: {nt} tied samples among {pts.shape[0]}")
        assert nt >= 2000, nt
        colour[order] = ref["color"].cpu().numpy()
        sel = np.arange(0, HW * HW, 509)[:96]
        sd = state()
        e = O.render(batch["ray_o"][0].numpy()[sel], batch["ray_d"][0].numpy()[sel], batch["near"][0].numpy()[sel].copy(),
                     batch["far"][0].numpy()[sel].copy(), S, case["xyz"], case["canon"], case["faces"], O.Params(sd),
                     batch["poses"][0].numpy(), sd["nerf.embedding.weight"][5], t_vals=torch.linspace(0.0, 1.0, steps=S).numpy())
        assert np.array_equal(ref["z_vals"].cpu().numpy()[sel], e["z_vals"])
        big = max(1.0, float(np.abs(e["color"]).max()))
        assert float(np.abs(ref["color"].cpu().numpy()[sel] - e["color"]).max()) < 1e-4 * big
        assert float(np.abs(ref["acc_map"].cpu().numpy()[sel] - e["acc_map"]).max()) < 1e-4
    differ = np.any(colour["orig"] != colour["twin"], 1)
    assert differ.sum() >= 100, int(differ.sum())


def test_twinned_training_batch_fused_and_far_search_equal_the_per_lane_walk(monkeypatch):
    """an 8192 x 64 training batch of the twinned body, both face orders: the default geometry (fused cell-major search + warp on
    lazily built lists, segmented far canonical search in front of k_normal) against DSN_NN_UNFUSED + DSN_TRAIN_FAR_SEARCH_MIN=2^40
    (per-lane walks only): forward outputs bit for bit, gradients as in test_training_geometry_fused_and_lazy_equals_the_per_lane_walk.
    The batch has canonical points outside the fine grid (inside the coarse one) whose nearest face is tied, and some of those ties
    lie in different 768-entry segments of their coarse list."""
    import dsnerf_amd
    from dsnerf_amd import _lib, synth
    from cases import make_cfg
    R, S, HW = 8192, 64, 512
    assert R * S >= 1 << 18 and R * S >= 1 << 15         # = DSN_TRAIN_CELLMAJOR_MIN, DSN_TRAIN_FAR_SEARCH_MIN: both on by default
    sd = state("x_w4")
    cfg = make_cfg(S)
    dev = torch.device(DEV)
    fwd_by_order = {}
    for order in N.ORDERS:
        case = N.twin_case(False, order)
        canon, faces, xyz = case["canon"], case["faces"], case["xyz"]
        rays = synth.make_rays(HW, HW, case["base_xyz"], fit_box=True)
        sel = np.linspace(0, HW * HW - 1, R).astype(np.int64)
        Tc = lambda a: torch.from_numpy(np.ascontiguousarray(a))

        def run(lazy):
            net = dsnerf_amd.DualSpaceNeRF(cfg)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            net.to(dev)
            r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
            r.cfg.MODEL.raw_noise_std = 1.0
            r.train_lazy_lists = lazy
            r.train()
            b = {"ray_o": Tc(rays["ray_o"][sel])[None], "ray_d": Tc(rays["ray_d"][sel])[None], "near": Tc(rays["near"][sel])[None],
                 "far": Tc(rays["far"][sel])[None], "xyz": Tc(xyz)[None], "poses": Tc(synth.make_poses())[None],
                 "Th": torch.zeros(1, 1, 3), "frame": torch.tensor([5])}
            torch.manual_seed(11)
            out = r.render(b)["coarse"]
            assert r.scene.lazy == lazy
            target = Tc(synth.hash_uniform(R * 3, 77).reshape(R, 3).astype(np.float32)).to(dev)
            torch.nn.functional.mse_loss(out["color"], target).backward()
            torch.cuda.synchronize()
            assert r.range_overflow_count() == 0 and r.scene.nn_watch(wait=True) == {}
            fwd = {k: out[k].detach().clone() for k in ("color", "acc_map", "depth_map", "weights", "z_vals")}
            return fwd, {k: p.grad.detach().clone() for k, p in net.named_parameters()}, r

        fa, ga, ra = run(True)
        _, ga2, _ = run(True)
        monkeypatch.setenv("DSN_NN_UNFUSED", "1")
        monkeypatch.setenv("DSN_TRAIN_FAR_SEARCH_MIN", str(1 << 40))
        fb, gb, _ = run(False)
        monkeypatch.delenv("DSN_NN_UNFUSED")
        monkeypatch.delenv("DSN_TRAIN_FAR_SEARCH_MIN")
        for k in fa:
            assert torch.equal(torch.nan_to_num(fa[k], nan=-1.0), torch.nan_to_num(fb[k], nan=-1.0)), (order, k)
        stable = [k for k in ga if "stage" in k and torch.equal(ga[k], ga2[k])]
        assert len(stable) >= 12
        for k in stable:
            assert torch.equal(ga[k], gb[k]), (order, k)
        for k in ga:
            dd = float((ga[k] - gb[k]).norm() / gb[k].norm().clamp_min(1e-30))
            assert dd < 1e-4, (order, k, dd)
        fwd_by_order[order] = fa["color"]
        # what the far search saw: the batch's canonical points (the warp of its samples, exact on any scene) outside the canonical
        # fine grid and inside the coarse one, whose nearest face is one of a tied pair
        sc = _scene(canon, faces, xyz)
        o, d = Tc(rays["ray_o"][sel]).to(dev), Tc(rays["ray_d"][sel]).to(dev)
        pts = (o[:, None, :] + d[:, None, :] * fa["z_vals"][..., None]).reshape(-1, 3)
        x_c = _lib.warp(sc, pts, None, 1, want_dir=False)["x_c"].cpu().numpy()
        cls = _classes(sc, x_c, "canon")
        far = x_c[cls == 1]
        assert far.shape[0] >= 10000, far.shape
        z3 = np.zeros_like(far)
        idx, _, _ = _lib.shade(sc, _packed(), T(far), T(z3), T(far), T(z3 + 1), T(z3), 1, exhaustive=True)
        idx = idx.cpu().numpy()
        tied = N.tie_mask(case, idx, "canon")
        print(f"order {order}: {far.shape[0]} canonical points in the coarse shell, {int(tied.sum())} of them tied")
        assert tied.sum() >= 200, int(tied.sum())
        off, lst = N.read_coarse_lists(sc)
        cell = N.cell_of(N.read_header(sc, "canon_coarse"), far[tied])
        k = N.pair_of(case)[idx[tied]]
        split = 0
        for c, kk in zip(cell, k):
            li = lst[off[c]:off[c + 1]]
            if li.size > N.FAR_SEG:
                pa, pb = np.searchsorted(li, case["first"][kk]), np.searchsorted(li, case["second"][kk])
                assert li[pa] == case["first"][kk] and li[pb] == case["second"][kk]
                split += int(pa // N.FAR_SEG != pb // N.FAR_SEG)
        print(f"order {order}: {split} tied pairs in different far-search segments of their coarse list")
        assert split >= 1, split
    assert not torch.equal(fwd_by_order["orig"], fwd_by_order["twin"])
