"""dsn_train_loss / dsn_train_loss_grad and dsnerf_amd.loss on the device, against the float64 restatement of include/dsnerf.h's rule
(tests/train_loss_restate.py): the four fp64 results within 1e-10 relative (the only freedom is the order of the fp64 sums and
fused multiply-add over at most 3 x 2^20 terms: dsn_image_ssim's bar), the seeds and the overwritten acc bit for bit; the
reference's own utils/loss.py run (tests/golden/train_loss.npz) at the bars of tests/test_train_loss_host.py; and the loss end to
end behind Renderer.sample_batch / render on the small body."""
import os

import numpy as np
import pytest
import torch

import train_loss_restate as LR
from helpers import GOLDEN, load

pytestmark = pytest.mark.gpu

SUM_BAR = 1e-10
SHARE = LR.SHARE
SIZES = [0, 1, 63, 64, 65, 257, SHARE - 1, SHARE, SHARE + 1, 2 * SHARE + 1, 8192, (1 << 20) + 37]


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert dsnerf_amd._lib.LOSS_SHARE == SHARE
    return dsnerf_amd._lib


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def close(a, b):
    a, b = float(a), float(b)
    return (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= SUM_BAR * abs(b)


_inputs = {}


def make_inputs(R):
    """one set of host arrays per R (shared by the tests): colours around the targets with a tail beyond |d| = 1, acc in [0, 1] with
    rays where acc == occupancy, occupancy 0 / 1 and a few other labels"""
    if R not in _inputs:
        rng = np.random.RandomState(100 + R % 9973)
        t64 = rng.rand(R, 3)
        color = (t64 + rng.randn(R, 3) * 0.6).astype(np.float32)
        acc = rng.rand(R).astype(np.float32)
        occ = (rng.rand(R) < 0.5).astype(np.uint8)
        if R > 8:
            occ[rng.permutation(R)[: max(1, R // 16)]] = 2
            acc[rng.permutation(R)[: max(1, R // 16)]] = 0.0
        _inputs[R] = dict(color=color, t64=t64, t32=t64.astype(np.float32), acc=acc, occ_u8=occ, occ_bool=occ == 1,
                          occ_f32=np.where(occ == 2, 0.5, occ).astype(np.float32))
    return _inputs[R]


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_and_compare(L, color, target, acc=None, occ=None, kind="L2", ups=(1.0, 1.0), overwrite=True, workspace=None, want_acc=True):
    """the forward and the backward on the device against the restatement; returns the device results as numpy"""
    k = LR.KINDS[kind]
    e = LR.forward(color, target, acc, occ, k, overwrite)
    d_acc = cuda(acc)
    res = L.train_loss(cuda(color), cuda(target), d_acc, cuda(occ), kind=kind, overwrite_acc=overwrite, workspace=workspace)
    out4 = res["out4"].cpu().numpy()
    assert out4.dtype == np.float64 and res["loss_rgb"].dtype == torch.float32 and res["loss_mask"].dtype == torch.float32
    assert res["mse"].dtype == torch.float64 and res["psnr"].dtype == torch.float64 and res["mse"].dim() == 0 and res["loss_rgb"].dim() == 0
    got = dict(zip(("loss_rgb", "loss_mask", "mse", "psnr"), out4))
    print(kind, "R", np.asarray(color).reshape(-1, 3).shape[0], {n: (float(got[n]), float(e[n])) for n in got})
    for n in got:
        assert close(got[n], e[n]), (n, got[n], e[n])
    assert np.array_equal(bits(res["loss_rgb"].cpu().numpy()), bits(np.float32(out4[0])))
    assert np.array_equal(bits(res["loss_mask"].cpu().numpy()), bits(np.float32(out4[1])))
    assert float(res["mse"]) == out4[2] or np.isnan(out4[2])
    acc_after = None
    if acc is not None:
        acc_after = d_acc.cpu().numpy()
        assert np.array_equal(bits(acc_after), bits(e["acc"]))
    up = [None if u is None else torch.tensor(u, dtype=torch.float32, device="cuda") for u in ups]
    for a_dev in ((d_acc, cuda(acc)) if (acc is not None and occ is not None) else (d_acc,)):     # acc after and before the overwrite
        g_color, g_acc = L.train_loss_grad(cuda(color), cuda(target), a_dev, cuda(occ), kind=kind, up_rgb=up[0], up_mask=up[1],
                                           want_acc=want_acc)
        eg_color, eg_acc = LR.grad(color, target, acc, occ, k, ups[0], ups[1])
        assert g_color.dtype == torch.float32 and tuple(g_color.shape) == eg_color.shape
        assert np.array_equal(bits(g_color.cpu().numpy()), bits(eg_color))
        if acc is not None and want_acc:
            assert np.array_equal(bits(g_acc.cpu().numpy()), bits(eg_acc))
        else:
            assert g_acc is None
    return dict(out4=out4, g_color=g_color.cpu().numpy(), g_acc=None if g_acc is None else g_acc.cpu().numpy(), acc=acc_after)


@pytest.mark.parametrize("R", SIZES)
def test_sizes_kinds_and_dtypes(L, R):
    """every size around a workgroup's share of the forward, the batch size of the trainer and a whole 1024 x 1024 frame's rays:
    both kinds with the mask term on (uint8 occupancy, float32 target) and off; the float64 target and the bool / float32
    occupancies take turns over the sizes (all of them at 257 and 8192)"""
    x = make_inputs(R)
    big = R > 100000
    i = SIZES.index(R)
    run_and_compare(L, x["color"], x["t32"], x["acc"], x["occ_u8"], "L2")
    run_and_compare(L, x["color"], x["t64"], x["acc"], x["occ_f32"] if i % 2 else x["occ_bool"], "L1")
    if big:
        return
    run_and_compare(L, x["color"], x["t32"], None, None, "L1")
    run_and_compare(L, x["color"], x["t64"], x["acc"], None, "L2")
    if R in (257, 8192):
        for kind in ("L2", "L1"):
            for occ in ("occ_u8", "occ_bool", "occ_f32"):
                for t in ("t32", "t64"):
                    run_and_compare(L, x["color"], x[t], x["acc"], x[occ], kind)


def test_upstream_gradients_and_null_g_acc(L):
    x = make_inputs(257)
    rng = np.random.RandomState(8)
    pair = tuple(float(np.float32(v)) for v in rng.randn(2))
    for kind in ("L2", "L1"):
        for ups in ((1.0, 1.0), (0.1, 0.1), (None, 1.0), (1.0, None), (None, None), pair):
            run_and_compare(L, x["color"], x["t32"], x["acc"], x["occ_u8"], kind, ups=ups)
        run_and_compare(L, x["color"], x["t64"], x["acc"], x["occ_u8"], kind, ups=pair, want_acc=False)
        run_and_compare(L, x["color"], x["t64"], x["acc"], x["occ_u8"], kind, overwrite=False)


def test_shapes_and_non_contiguous_inputs(L):
    R = 2 * SHARE + 1
    x = make_inputs(R)
    e = LR.forward(x["color"], x["t64"], x["acc"], x["occ_u8"], LR.SMOOTH_L1)
    eg = LR.grad(x["color"], x["t64"], x["acc"], x["occ_u8"], LR.SMOOTH_L1, 1.0, 1.0)
    wide = torch.zeros(R, 5, device="cuda")
    wide[:, 1:4] = cuda(x["color"])
    twide = torch.zeros(1, R, 4, dtype=torch.float64, device="cuda")
    twide[0, :, :3] = cuda(x["t64"])
    acc2 = torch.zeros(R, 2, device="cuda")
    acc2[:, 1] = cuda(x["acc"])
    occ2 = torch.zeros(1, 2 * R, dtype=torch.uint8, device="cuda")
    occ2[0, ::2] = cuda(x["occ_u8"])
    color, target, acc, occ = wide[:, 1:4][None], twide[:, :, :3], acc2[:, 1][None], occ2[:, ::2]
    assert not color.is_contiguous() and not target.is_contiguous() and not acc.is_contiguous() and not occ.is_contiguous()
    g_color, g_acc = L.train_loss_grad(color, target, acc, occ, kind="L1", up_rgb=torch.ones((), device="cuda"), up_mask=1.0)
    assert np.array_equal(bits(g_color.cpu().numpy()), bits(eg[0])) and np.array_equal(bits(g_acc.cpu().numpy()), bits(eg[1]))
    res = L.train_loss(color, target, acc, occ, kind="L1")
    for i, n in enumerate(("loss_rgb", "loss_mask", "mse", "psnr")):
        assert close(res["out4"][i], e[n]), n
    assert np.array_equal(bits(acc2[:, 1].cpu().numpy()), bits(e["acc"]))          # written back through the strided view
    assert not acc2[:, 0].any() and np.array_equal(wide[:, 1:4].cpu().numpy(), x["color"])
    host = L.train_loss(cuda(x["color"]), torch.from_numpy(x["t64"])[None], cuda(x["acc"])[None], torch.from_numpy(x["occ_u8"])[None], kind="L1")
    assert torch.equal(host["out4"], res["out4"])            # host targets / occupancy are moved over
    with pytest.raises(ValueError):
        L.train_loss(cuda(x["color"]), cuda(x["t32"]), None, cuda(x["occ_u8"]))
    with pytest.raises(ValueError):
        L.train_loss(cuda(x["color"]), cuda(x["t32"]), kind="huber")
    with pytest.raises(TypeError):
        L.train_loss(cuda(x["color"]).double(), cuda(x["t32"]))


def test_same_bits_whatever_the_workspace_holds(L, monkeypatch):
    for R in (8192, 2 * SHARE + 1):
        x = make_inputs(R)
        first = run_and_compare(L, x["color"], x["t32"], x["acc"], x["occ_u8"], "L2")
        again = run_and_compare(L, x["color"], x["t32"], x["acc"], x["occ_u8"], "L2")
        n = L.lib().dsn_train_loss_workspace_bytes(R)
        runs = [again]
        for size, fill in ((n, 0xFF), (4 * n + 4096, 0xFF), (n + 256, 0x00), (2 * n, None)):
            ws = torch.empty(size, dtype=torch.uint8, device="cuda")
            if fill is None:
                ws.copy_(torch.from_numpy(np.random.RandomState(1).randint(0, 256, size).astype(np.uint8)))
            else:
                ws.fill_(fill)
            runs.append(run_and_compare(L, x["color"], x["t32"], x["acc"], x["occ_u8"], "L2", workspace=ws))
        monkeypatch.setenv("DSN_POISON_SCRATCH", "1")
        runs.append(run_and_compare(L, x["color"], x["t32"], x["acc"], x["occ_u8"], "L2"))
        monkeypatch.delenv("DSN_POISON_SCRATCH")
        for other in runs:
            for k in ("out4", "g_color", "g_acc", "acc"):
                assert np.array_equal(bits(first[k]).view(np.uint8), bits(other[k]).view(np.uint8)), k


def test_edge_values(L):
    R = SHARE + 7
    rng = np.random.RandomState(6)
    t = rng.rand(R, 3).astype(np.float32)
    for kind in ("L2", "L1"):
        out = run_and_compare(L, t, t, None, None, kind)                              # d = 0: mse 0, psnr +inf
        assert out["out4"][0] == 0.0 and out["out4"][2] == 0.0 and out["out4"][3] == np.inf
    below, above = np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))
    d = np.resize(np.array([1.0, -1.0, below, -below, above, -above, 0.0, 0.5], np.float32), (R, 3))
    out = run_and_compare(L, d, np.zeros_like(d), None, None, "L1")
    assert set(np.unique(np.abs(out["g_color"]))) == {np.float32((1.0 / (3.0 * R)) * v) for v in (0.0, 0.5, float(below), 1.0)}
    acc = rng.rand(R).astype(np.float32)
    occ = (rng.rand(R) < 0.5).astype(np.uint8)
    acc[::3] = occ[::3]                                                                # acc == occ: sign 0
    out = run_and_compare(L, t, t, acc, occ, "L2", ups=(1.0, -0.3))
    assert (out["g_acc"][::3] == 0).all()
    out = run_and_compare(L, t, t, acc, np.ones(R, np.uint8), "L2")                    # all ones
    assert out["out4"][1] == 0.0 and (out["acc"] == 1).all() and not out["g_acc"].any()
    out = run_and_compare(L, t, t, acc, np.zeros(R, np.uint8), "L1")                   # all zeros
    assert np.array_equal(out["acc"], acc)
    c = t.copy()
    c[R - 1, 2] = np.nan
    acc_n = acc.copy()
    acc_n[1] = np.nan
    for kind in ("L2", "L1"):                                                          # NaN in, NaN out
        out = run_and_compare(L, c, t, acc_n, np.zeros(R, np.uint8), kind)
        assert np.isnan(out["out4"]).all() and np.isnan(out["g_color"]).sum() == 1 and np.isnan(out["g_acc"]).sum() == 1
    out = run_and_compare(L, t, t, acc_n, np.ones(R, np.uint8), "L2")                  # ... but acc under occupancy 1 is never read
    assert out["out4"][1] == 0.0
    empty = run_and_compare(L, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint8))
    assert np.isnan(empty["out4"]).all()
    empty = run_and_compare(L, np.zeros((0, 3), np.float32), np.zeros((0, 3)), None, None)
    assert np.isnan(empty["out4"][[0, 2, 3]]).all() and empty["out4"][1] == 0.0


def test_fixture_cases_against_the_reference(L):
    from test_train_loss_host import check_against_reference
    g = np.load(os.path.join(GOLDEN, "train_loss.npz"))
    for name in g["cases"]:
        c = {k.split(":", 1)[1]: g[k] for k in g.files if k.startswith(name + ":")}
        R = int(c["R"])
        color, acc = g[f"in{R}:color"], g[f"in{R}:acc"]
        target = g[f"in{R}:target32" if str(c["target_dtype"]) == "float32" else f"in{R}:target64"]
        c["occ"] = g[f"in{R}:occ_u8" if str(c["occ_dtype"]) == "uint8" else f"in{R}:occ_f32"]
        occ = c["occ"] if bool(c["mask"]) else None
        d_acc = cuda(acc)
        res = L.train_loss(cuda(color), cuda(target), d_acc, cuda(occ), kind=str(c["kind"]))
        g_color, g_acc = L.train_loss_grad(cuda(color), cuda(target), d_acc, cuda(occ), kind=str(c["kind"]), up_rgb=1.0, up_mask=1.0)
        got = {"loss_rgb": res["loss_rgb"].cpu().numpy(), "loss_mask": res["loss_mask"].cpu().numpy()}      # the float32 losses
        check_against_reference(c, got, g_color.cpu().numpy(), g_acc.cpu().numpy(), d_acc.cpu().numpy())


# ---- end to end on the small body -----------------------------------------------------------------------------------------------
def _cfg(kind, mask=True):
    from types import SimpleNamespace
    return SimpleNamespace(MODEL=SimpleNamespace(LOSS=kind, LOSSwMask=mask))


def _torch_op_loss(kind, out, target, occ, mask=True):
    """utils/loss.py + trainer.py:73-76 written in torch ops: what a user has without dsnerf_amd.loss"""
    F = torch.nn.functional
    loss = (F.mse_loss if kind == "L2" else F.smooth_l1_loss)(out["color"], target)
    if mask:
        acc = out["acc_map"]
        acc[occ == 1] = 1
        loss = loss + 0.1 * F.l1_loss(acc, occ)
    return loss


@pytest.mark.parametrize("kind", ["L2", "L1"])
def test_parameter_gradients_match_the_torch_op_loss(L, kind):
    """the golden training batch: render -> make_loss(cfg)(coarse, batch) -> sum -> backward() against the same render driven by the
    reference's loss in torch ops, all 33 tensors within the bars of tests/golden/achieved_grad_errors.json (and, for L2, against the
    reference's own autograd in the fixture at the same bars)"""
    import dsnerf_amd
    from cases import make_batch, make_renderer, rel, sample_index, FULL_LIMIT
    from test_gpu_train import achieved, bar
    g = load("small_train_grads")
    rec = achieved("reference", "small_train_grads")
    r = make_renderer(g, "small_train_grads")
    r.cfg.MODEL.raw_noise_std = float(g["raw_noise_std"])
    r.train()
    target, occ = torch.from_numpy(g["target_rgb"]), torch.from_numpy(g["occupancy"])
    grads, losses = [], []
    for which in ("device", "torch"):
        torch.manual_seed(int(g["seed"]))
        out = r.render(make_batch(g))["coarse"]
        r.net.zero_grad()
        if which == "device":
            loss_fn = dsnerf_amd.loss.make_loss(_cfg(kind))
            loss1 = loss_fn(out, {"rgb": target[None], "occupancy": occ[None]})            # host tensors in the batch, as the loader's
            assert set(loss1) == {"loss_rgb", "loss_mask"}
            assert all(v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda and v.requires_grad for v in loss1.values())
            loss = 0
            for key in loss1:
                loss += loss1[key]
            assert bool((out["acc_map"][occ.cuda() == 1] == 1).all())
        else:
            loss = _torch_op_loss(kind, out, target.cuda(), occ.cuda())
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append({k: p.grad.detach().cpu().numpy().reshape(-1).copy() for k, p in r.net.named_parameters()})
    assert abs(losses[0] - losses[1]) <= 2e-6 * max(1.0, abs(losses[1])), losses
    assert len(grads[0]) == 33
    for k in grads[0]:
        assert rel(grads[0][k], grads[1][k]) <= bar(rec[k]), (k, rel(grads[0][k], grads[1][k]), rec[k])
        if kind == "L2":
            a = grads[0][k] if grads[0][k].size <= FULL_LIMIT else grads[0][k][sample_index(grads[0][k].size)]
            assert rel(a, g["grad:" + k]) <= bar(rec[k]), (k, rel(a, g["grad:" + k]), rec[k])
    assert r.range_overflow_count() == 0


def test_sample_batch_render_loss_backward(L, monkeypatch):
    """sample_batch -> render -> make_loss(cfg)(coarse, batch) -> sum -> backward(): the seeds that reach _RenderRays.backward are
    dsn_train_loss_grad's, acc_map reads 1 where occupancy == 1 (and is left alone with overwrite_acc=False), loss_fn.last holds the
    batch's psnr, a few Adam steps lower the loss, and render_view gives the same bits before and after"""
    import dsnerf_amd
    import train_rays_restate as TR
    from cases import make_batch, make_renderer
    g = load("small_eval")
    r = make_renderer(g, "small_eval")
    gv = load("small_view")
    Hv, Wv = int(gv["H"]), int(gv["W"])

    def view():
        r.eval()
        b = make_batch(gv)
        b["img"] = torch.zeros(1, Hv, Wv, 3, dtype=torch.float64)
        b["mask_at_box"] = torch.from_numpy(gv["mask_at_box"])[None]
        return {k: v.clone() for k, v in r.render_view(b).items() if torch.is_tensor(v)}

    before = view()
    xyz = g["xyz"]
    lo, hi = xyz.min(0) - 0.05, xyz.max(0) + 0.05
    H, W = 37, 53
    f = 0.9 * W
    K = np.array([[f, 0.0, W / 2 - 0.5], [0.0, f, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    Rm, T = np.eye(3), np.array([0.0, 0.0, 3.0]) - (lo + hi) / 2
    bounds = np.stack([lo, hi]).astype(np.float64)
    assert TR.half_integer_distance(K, Rm, T, bounds) > 1e-6
    rng = np.random.RandomState(2)
    img = torch.from_numpy(rng.rand(H, W, 3)).cuda()
    mask = torch.from_numpy(TR.bound_mask(K, Rm, T, bounds, H, W) * (rng.rand(H, W) < 0.5)).cuda()
    batch = r.sample_batch(img, K, Rm, T, bounds, mask, 64, 77, occupancy_from=mask)
    assert batch["rgb"].dtype == torch.float32 and batch["occupancy"].dtype == torch.uint8 and bool((batch["occupancy"] == 1).any())
    extra = make_batch(g)
    batch.update(xyz=extra["xyz"], poses=extra["poses"], frame=extra["frame"], Th=extra["Th"])
    r.train()
    seeds = []
    real = L.render_rays_grad

    def spy(*a, **kw):
        seeds.append((a[9].clone(), None if a[11] is None else a[11].clone()))      # g_color, g_acc as _RenderRays.backward hands them on
        assert a[10] is None and a[12] is None and a[13] is None
        return real(*a, **kw)

    monkeypatch.setattr(L, "render_rays_grad", spy)
    occ = batch["occupancy"].reshape(-1)
    for kind in ("L2", "L1"):
        loss_fn = dsnerf_amd.loss.make_loss(_cfg(kind))
        torch.manual_seed(5)
        coarse = r.render(batch)["coarse"]
        color0, acc0 = coarse["color"].detach().clone(), coarse["acc_map"].detach().clone()
        quiet = loss_fn(coarse, dict(batch, rgb=batch["rgb"].double()), overwrite_acc=False)      # (a float64 target of the same values)
        assert torch.equal(coarse["acc_map"], acc0)
        loss1 = loss_fn(coarse, batch)
        assert torch.equal(loss1["loss_rgb"], quiet["loss_rgb"]) and torch.equal(loss1["loss_mask"], quiet["loss_mask"])
        assert bool((coarse["acc_map"][occ == 1] == 1).all()) and torch.equal(coarse["acc_map"][occ != 1], acc0[occ != 1])
        loss = 0
        for key in loss1:
            loss += loss1[key]
        r.net.zero_grad()
        del seeds[:]
        loss.backward()
        one = torch.ones((), device="cuda")
        g_color, g_acc = L.train_loss_grad(color0, batch["rgb"], acc0, batch["occupancy"], kind=kind, up_rgb=one, up_mask=one)
        assert len(seeds) == 1 and torch.equal(seeds[0][0], g_color) and torch.equal(seeds[0][1], g_acc)
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in r.net.parameters())
        c, t = color0.cpu().numpy().astype(np.float64), batch["rgb"][0].cpu().numpy()
        want = -10.0 * np.log10(np.mean((c - t) ** 2))
        last = loss_fn.last
        assert set(last) == {"mse", "psnr", "loss_rgb", "loss_mask"} and all(v.is_cuda for v in last.values())
        assert abs(float(last["psnr"]) - want) <= 1e-10 * abs(want) and last["psnr"].dtype == torch.float64
        assert float(last["loss_rgb"]) == float(loss1["loss_rgb"]) and float(last["loss_mask"]) == float(loss1["loss_mask"])
        # without the mask term: one key, acc_map untouched, no seed for it
        plain = dsnerf_amd.loss.make_loss(_cfg(kind, mask=False))
        coarse = r.render(batch)["coarse"]
        color1, acc1 = coarse["color"].detach().clone(), coarse["acc_map"].detach().clone()
        only = plain(coarse, batch)
        assert set(only) == {"loss_rgb"} and torch.equal(coarse["acc_map"], acc1) and float(plain.last["loss_mask"]) == 0.0
        r.net.zero_grad()
        del seeds[:]
        only["loss_rgb"].backward()
        g_color1, _ = L.train_loss_grad(color1, batch["rgb"], kind=kind, up_rgb=one)
        assert len(seeds) == 1 and torch.equal(seeds[0][0], g_color1) and seeds[0][1] is None
    monkeypatch.undo()
    # the eval path is untouched: the same bits from render_view as before the loss was ever used
    after = view()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
    r.train()
    # trainer.py:66-81 in miniature
    loss_fn = dsnerf_amd.loss.make_loss(_cfg("L2"))
    opt = torch.optim.Adam(r.net.parameters(), lr=5e-4)
    torch.manual_seed(0)
    losses, psnrs = [], []
    for _ in range(12):
        opt.zero_grad()
        loss1 = loss_fn(r.render(batch)["coarse"], batch)
        loss = 0
        for key in loss1:
            loss += loss1[key]
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        psnrs.append(loss_fn.last["psnr"])
    losses = [float(v) for v in losses]
    assert np.isfinite(losses).all() and np.isfinite([float(p) for p in psnrs]).all()
    assert np.mean(losses[-3:]) < 0.9 * np.mean(losses[:3]), losses
