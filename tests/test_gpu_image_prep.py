"""dsn_image_undistort, dsn_image_morph, dsn_image_resize and the fused dsn_image_prep on the GPU: every output byte for byte against
the numpy restatement of the rule (tests/image_prep_restate.py), on outputs pre-filled with 0xFF (DSN_POISON_SCRATCH), at sizes around
the kernels' 64 x 16 tile; the fused launch against the composition of the stand-alone device calls; prepare_zju into
Renderer.sample_batch; prepare_h36m against the restatement's composition."""
import numpy as np
import pytest
import torch

import image_prep_restate as IP
from helpers import load

pytestmark = pytest.mark.gpu

TW, TH = 64, 16          # dsnerf_amd.imageprep.TILE_W / TILE_H (asserted below)
SIZES = [(1, 1), (2, 2), (37, 53), (40, 48), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1)]


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    assert (dsnerf_amd.imageprep.TILE_W, dsnerf_amd.imageprep.TILE_H) == (TW, TH)
    return dsnerf_amd._lib


@pytest.fixture(scope="module")
def P():
    import dsnerf_amd
    return dsnerf_amd.imageprep


@pytest.fixture(autouse=True)
def poisoned_outputs(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")          # every output tensor starts as 0xFF bytes


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(t, a):
    """a device tensor and a numpy array: the same shape, dtype and bytes"""
    h = t.cpu().numpy()
    return h.shape == a.shape and h.dtype == a.dtype and h.tobytes() == np.ascontiguousarray(a).tobytes()


def camera(H, W, shift=0.0):
    return np.array([[0.9 * W + 0.37, 0.0, W / 2 - 0.3 + shift], [0.0, 0.92 * W + 0.11, H / 2 + 0.2 - shift], [0.0, 0.0, 1.0]])


D_ZERO = np.zeros(5)
D_REAL = np.array([-0.3, 0.12, 1.5e-3, -2e-3, 0.03])
D_STRONG = np.array([2.5, 0.0, 0.0, 0.0])
D_EIGHT = np.array([-0.28, 0.09, -1e-3, 2e-3, 0.02, 0.015, -0.03, 0.004])
D_PUSH = np.array([0.6, 0.0, 1e-3, 1e-3])
DISTORTIONS = {"zero": D_ZERO, "real": D_REAL, "strong": D_STRONG, "eight": D_EIGHT}


def images(rng, H, W):
    return {"u8": rng.randint(0, 256, (H, W)).astype(np.uint8), "u8x3": rng.randint(0, 256, (H, W, 3)).astype(np.uint8),
            "f32": rng.randn(H, W).astype(np.float32), "f32x3": rng.rand(H, W, 3).astype(np.float32)}


# ---- undistort ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_undistort_is_the_restatement(L, H, W):
    rng = np.random.RandomState(H * 100 + W)
    K = camera(H, W)
    src = images(rng, H, W)
    for dname, D in DISTORTIONS.items():
        iu, iv, ok = IP.undistort_map(K, D, H, W)
        if dname == "strong" and H >= 37:          # a band of border pixels maps outside the image: every tap is zero there
            sx, sy = iu >> 5, iv >> 5
            gone = (sx < -1) | (sx >= W) | (sy < -1) | (sy >= H)
            assert gone[0].all() and gone[:, 0].all() and not gone[H // 2, W // 2]
        if dname == "zero":
            assert np.array_equal(iu >> 5, np.broadcast_to(np.arange(W), (H, W))) and not (iu & 31).any()
        for name, a in src.items():
            want = IP.remap(a, iu, iv, ok)
            got = L.image_undistort(dev(a[None]), K, D)
            assert same(got[0], want), (dname, name, int((got[0].cpu().numpy() != want).sum()))


def test_undistort_rint_ties_and_border_taps(L):
    """u 32 = n + 0.5 exactly (K = I, row 0: u = j (1 + k1 j^2)): rint goes to even, which a float32 image shows in its weights; and
    taps that straddle the border read partial zeros"""
    K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    rng = np.random.RandomState(11)
    a = (rng.rand(5, 7).astype(np.float32) + np.float32(1.0))
    for k1, want_iu in ((1 / 64, 32), (5 / 64, 34), (-3 / 64, 30)):
        iu, iv, ok = IP.undistort_map(K, [k1, 0, 0, 0], 5, 7)
        assert iu[0, 1] == want_iu and abs((1.0 + k1) * 32.0 - want_iu) == 0.5          # a tie, resolved to even
        want = IP.remap(a, iu, iv, ok)
        up = iu.copy()
        up[0, 1] = int(np.floor((1.0 + k1) * 32.0 + 0.5))          # what rounding half up would have taken
        assert IP.remap(a, up, iv, ok)[0, 1] != want[0, 1]
        assert same(L.image_undistort(dev(a[None]), K, [k1, 0, 0, 0])[0], want)
    # a lens that pushes the border pixels' taps across the image's edge
    H, W = 9, 12
    Kc = camera(H, W)
    full = np.full((H, W, 3), 255, np.uint8)
    iu, iv, ok = IP.undistort_map(Kc, D_PUSH, H, W)
    want = IP.remap(full, iu, iv, ok)
    assert ((want > 0) & (want < 255)).any()          # partial zeros exist
    assert same(L.image_undistort(dev(full[None]), Kc, D_PUSH)[0], want)


def test_undistort_batches_and_nan_camera(L):
    H, W, N = 37, 53, 3
    rng = np.random.RandomState(7)
    Ks = np.stack([camera(H, W, s) for s in (0.0, 0.4, -0.7)])
    Ds = np.stack([D_EIGHT, D_EIGHT * 0.5, D_EIGHT * -0.3])
    for name in ("u8x3", "f32"):
        batch = np.stack([images(rng, H, W)[name] for _ in range(N)])
        got = L.image_undistort(dev(batch), Ks, Ds)
        for n in range(N):
            assert same(got[n], IP.undistort(batch[n], Ks[n], Ds[n])), (name, n)
            assert torch.equal(got[n], L.image_undistort(dev(batch[n:n + 1]), Ks[n], Ds[n])[0])
        # one [3, 3] camera for the whole batch, device-resident cameras
        shared = L.image_undistort(dev(batch), dev(Ks[1]), dev(Ds[1]))
        assert all(same(shared[n], IP.undistort(batch[n], Ks[1], Ds[1])) for n in range(N))
        # NaN in one image's K stays in that image, whose outputs are all 0
        Kn = Ks.copy()
        Kn[1, 0, 0] = np.nan
        bad = L.image_undistort(dev(batch), Kn, Ds)
        assert torch.equal(bad[0], got[0]) and torch.equal(bad[2], got[2])
        assert not bool(bad[1].view(torch.uint8).any())
        empty = L.image_undistort(dev(batch[:0]), Ks[:0], Ds[:0])
        assert tuple(empty.shape) == (0,) + batch.shape[1:]


# ---- morphology ---------------------------------------------------------------------------------------------------------------------------
def morph_masks():
    rng = np.random.RandomState(3)
    H, W = 2 * TH + 5, 2 * TW + 3          # 37 x 131: two tile seams in each axis
    ms = [(rng.rand(H, W) < d).astype(np.uint8) for d in (0.01, 0.5, 0.99)]
    for (y, x) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (TH - 1, TW - 1), (TH, TW), (TH - 1, TW), (2 * TH, 2 * TW - 1)):
        m = np.zeros((H, W), np.uint8)
        m[y, x] = 1
        ms += [m, (255 - 254 * m).astype(np.uint8)]          # a lone pixel, and a lone hole of level 1 in 255
    ms.append(rng.randint(0, 20, (H, W)).astype(np.uint8))          # a label map
    ms.append(rng.randint(0, 256, (H, W)).astype(np.uint8))
    return np.stack(ms)


@pytest.fixture(scope="module")
def masks():
    return morph_masks()


@pytest.mark.parametrize("k", [1, 2, 5, 10, 15])
@pytest.mark.parametrize("op", ["dilate", "erode"])
def test_morphology_is_the_restatement(L, P, masks, k, op):
    code = L.PREP_DILATE if op == "dilate" else L.PREP_ERODE
    got = L.image_morph(dev(masks), k, code)
    for n in range(len(masks)):
        want = IP.morph(masks[n], k, op == "dilate")
        assert same(got[n], want), (n, int((got[n].cpu().numpy() != want).sum()))
    # an even box is not symmetric: the anchor convention shows
    if k % 2 == 0:
        assert not np.array_equal(IP.morph(masks[-1], k, op == "dilate"), IP.morph(masks[-1][::-1, ::-1], k, op == "dilate")[::-1, ::-1])
    small = masks[1][:TH + 1, :TW - 1].copy()
    one = (P.dilate if op == "dilate" else P.erode)(small, k)
    assert same(one, IP.morph(small, k, op == "dilate"))
    assert tuple(L.image_morph(dev(masks[:0]), k, code).shape) == (0,) + masks.shape[1:]


# ---- resizes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 4])
def test_resizes_are_the_restatement(L, P, c):
    rng = np.random.RandomState(c)
    H, W = 36, 52
    low = rng.randint(0, 4, (H, W, 3)).astype(np.uint8)          # small levels: block sums land on the rounding ties
    low[:, :W // 2] = rng.randint(0, 2, (H, W // 2, 3))          # (sums around 8: the tie above the even quotient 0 for c = 4)
    if c > 1:
        s = sum(low[dy::c, dx::c].astype(np.int64) for dy in range(c) for dx in range(c))
        q = s >> (2 if c == 2 else 4)
        tie = (s & (c * c - 1)) == c * c // 2
        assert (tie & (q % 2 == 0)).any() and (tie & (q % 2 == 1)).any()          # ties above even and above odd quotients
        if c == 4:          # half up would differ on the even ones
            assert not np.array_equal((s + 8) >> 4, IP.area_u8(s, 4))
    cases = {"low": low, "u8": rng.randint(0, 256, (H, W)).astype(np.uint8), "u8x3": rng.randint(0, 256, (H, W, 3)).astype(np.uint8),
             "f32": (rng.randn(H, W) * 1e3).astype(np.float32), "f32x3": rng.rand(H, W, 3).astype(np.float32)}
    for name, a in cases.items():
        batch = np.stack([a, a[::-1].copy()])
        area = L.image_resize(dev(batch), c, L.PREP_AREA)
        near = L.image_resize(dev(batch), c, L.PREP_NEAREST)
        for n in range(2):
            assert same(area[n], IP.resize_area(batch[n], c)), (name, n)
            assert same(near[n], batch[n][::c, ::c]), (name, n)
        assert same(P.resize_area(a, c), IP.resize_area(a, c)) and same(P.resize_nearest(a, c), a[::c, ::c])
    if c > 1:          # sizes the factor does not divide are refused
        for bad in (cases["u8"][None, :H - 1], cases["u8"][None, :, :W - 1]):
            with pytest.raises(ValueError):
                L.image_resize(dev(bad), c, L.PREP_AREA)


# ---- the fused ZJU item -------------------------------------------------------------------------------------------------------------------
def zju_inputs(H, W, seed=5, blobs=()):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    cihp = np.zeros((H, W), np.uint8)
    cihp[H // 4:3 * H // 4, W // 3:2 * W // 3] = rng.randint(1, 20, (3 * H // 4 - H // 4, 2 * W // 3 - W // 3))
    cihp[rng.rand(H, W) < 0.01] = 7
    for (y0, y1, x0, x1) in blobs:
        cihp[y0:y1, x0:x1] = 3
    return img, cihp


def composed_on_device(L, img, cihp, K, D, c, border):
    """the ZJU item as the composition of the three stand-alone device calls (and torch for != 0 and the product)"""
    fg_u = L.image_undistort((dev(cihp[None]) != 0).to(torch.uint8), K, D)
    msk_fg = L.image_morph(fg_u, border, L.PREP_DILATE)
    im = L.image_undistort(dev(img[None]), K, D) * msk_fg[..., None]
    return (L.image_resize(im, c, L.PREP_AREA)[0], L.image_resize(msk_fg, c, L.PREP_NEAREST)[0],
            L.image_resize(dev(cihp[None]), c, L.PREP_NEAREST)[0])


def check_fused(L, img, cihp, K, D, c, border):
    want64 = IP.prepare_zju(img, cihp, K, D, c=c, border=border)
    want32 = IP.prepare_zju(img, cihp, K, D, c=c, border=border, dtype=np.float32)
    comp_u8, comp_fg, comp_ci = composed_on_device(L, img, cihp, K, D, c, border)
    for dtype, want in ((torch.float64, want64), (torch.float32, want32)):
        o_img, o_u8, o_fg, o_ci = L.image_prep(dev(img[None]), dev(cihp[None]), K, D, c=c, border=border, dtype=dtype, want_u8=True)
        assert same(o_img[0], want["img"]), (dtype, int((o_img[0].cpu().numpy() != want["img"]).sum()))
        assert same(o_u8[0], want["img_u8"]) and same(o_fg[0], want["msk_fg"]) and same(o_ci[0], want["msk_cihp"])
        assert torch.equal(o_u8[0], comp_u8) and torch.equal(o_fg[0], comp_fg) and torch.equal(o_ci[0], comp_ci)
        # null optional outputs; a repeated call gives the same bytes
        p_img, p_u8, p_fg, p_ci = L.image_prep(dev(img[None]), dev(cihp[None]), K, D, c=c, border=border, dtype=dtype, want_u8=False, want_masks=False)
        assert p_u8 is None and p_fg is None and p_ci is None and torch.equal(p_img, o_img)
    return want64


@pytest.mark.parametrize("c", [1, 2, 4])
@pytest.mark.parametrize("border", [1, 5, 10])
def test_fused_prep_40x48(L, c, border):
    H, W = 40, 48
    img, cihp = zju_inputs(H, W)
    want = check_fused(L, img, cihp, camera(H, W), D_REAL, c, border)
    assert want["msk_fg"].any() and not want["msk_fg"].all()
    assert not np.array_equal(want["msk_cihp"], IP.undistort(cihp, camera(H, W), D_REAL)[::c, ::c])          # the raw mask, not the undistorted one


@pytest.mark.parametrize("c,border", [(1, 5), (2, 5), (4, 10), (2, 10), (2, 15)])
def test_fused_prep_halo_decides_across_tile_seams(L, c, border):
    """foreground blobs that end exactly at the tile seams (x = 64, 128; y = 16, 32): pixels on the far side get their mask from the
    neighbouring tile's foreground through the halo.  The restatement shows that a dilation without halo would change the outputs."""
    H, W = 2 * TH + 8, 2 * TW + 16          # 40 x 144
    blobs = ((6, TH, 40, TW), (TH, 22, TW, 90), (2 * TH - 3, 2 * TH, 2 * TW - 9, 2 * TW), (2 * TH, 2 * TH + 4, 100, 110))
    img, cihp = zju_inputs(H, W, seed=9, blobs=blobs)
    cihp[:, :34] = 0
    K, D = camera(H, W), D_REAL * 0.05          # a nearly straight lens: the blobs' edges stay at the seams
    st = IP.zju_steps(img, cihp, K, D, c, border)
    no_halo = IP.dilate_per_tile(st["fg_u"], border, TH, TW)
    assert not np.array_equal(no_halo[::c, ::c], st["msk_fg"])
    assert not np.array_equal(IP.resize_area(IP.undistort(img, K, D) * no_halo[..., None], c), st["img_u8"])
    for (ys, xs) in ((slice(0, TH), slice(TW, 2 * TW)), (slice(TH, 2 * TH), slice(0, TW))):          # on both sides of a seam
        assert (no_halo[ys, xs] != st["msk_fg_full"][ys, xs]).any()
    check_fused(L, img, cihp, K, D, c, border)


def test_fused_prep_batches_sizes_and_strong_lens(L, P):
    rng = np.random.RandomState(21)
    for (H, W, c) in ((4, 4, 4), (2, 2, 2), (1, 1, 1), (TH + 4, TW + 4, 4), (TH, TW, 2), (52, 36, 2)):
        N = 3
        imgs = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
        cihps = (rng.rand(N, H, W) < 0.3).astype(np.uint8) * rng.randint(1, 255, (N, H, W)).astype(np.uint8)
        Ks = np.stack([camera(H, W, s) for s in (0.0, 0.3, -0.2)])
        Ds = np.stack([np.concatenate([D_STRONG, np.zeros(4)]), D_EIGHT, D_EIGHT * 0])
        Ks[1, 1, 2] = np.nan if H > 4 else Ks[1, 1, 2]          # a NaN camera stays in its image
        out = P.prepare_zju(imgs, cihps, Ks, Ds, ratio=1.0 / c, border=5, want_u8=True)
        for n in range(N):
            want = IP.prepare_zju(imgs[n], cihps[n], Ks[n], Ds[n], c=c, border=5)
            for k in ("img", "img_u8", "msk_fg", "msk_cihp"):
                assert same(out[k][n], want[k]), (H, W, c, n, k)
            assert np.array_equal(out["K"][n], want["K"], equal_nan=True)
        if H > 4:
            assert not bool(out["img_u8"][1].any()) and not bool(out["msk_fg"][1].any()) and same(out["msk_cihp"][1], cihps[1][::c, ::c])
        single = P.prepare_zju(imgs[2], cihps[2], Ks[2], Ds[2], ratio=1.0 / c, dtype=torch.float32)
        assert single["img"].dtype == torch.float32 and same(single["img"], IP.prepare_zju(imgs[2], cihps[2], Ks[2], Ds[2], c=c, dtype=np.float32)["img"])
        assert "img_u8" not in single and tuple(single["msk_fg"].shape) == (H // c, W // c)
    empty = P.prepare_zju(imgs[:0], cihps[:0], Ks[:0], Ds[:0], ratio=0.5)
    assert tuple(empty["img"].shape) == (0, 26, 18, 3)


def test_unpoisoned_outputs_have_the_same_bytes(L, monkeypatch):
    H, W = 40, 48
    img, cihp = zju_inputs(H, W)
    args = (dev(img[None]), dev(cihp[None]), camera(H, W), D_REAL)
    a = L.image_prep(*args, c=2, want_u8=True)
    monkeypatch.delenv("DSN_POISON_SCRATCH")
    b = L.image_prep(*args, c=2, want_u8=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def renderer():
    from cases import make_renderer
    g = load("small_eval")
    r = make_renderer(g, "small_eval")
    r.eval()
    return g, r


def test_prepare_zju_feeds_sample_batch(L, P, renderer):
    """prepare_zju -> Renderer.sample_batch on the small body's camera equals sample_batch fed the restatement's host arrays, key for
    key and bit for bit; render takes the batch; render_view of the fixture frame is unchanged"""
    import train_rays_restate as TR
    from cases import make_batch
    g, r = renderer
    gv = load("small_view")
    Hv, Wv = int(gv["H"]), int(gv["W"])

    def view():
        b = make_batch(gv)
        b["img"] = torch.zeros(1, Hv, Wv, 3, dtype=torch.float64)
        b["mask_at_box"] = torch.from_numpy(gv["mask_at_box"])[None]
        return {k: v.clone() for k, v in r.render_view(b).items() if torch.is_tensor(v)}

    before = view()
    xyz = g["xyz"]
    lo, hi = xyz.min(0) - 0.05, xyz.max(0) + 0.05
    H, W, c = 37, 53, 2
    f = 0.9 * W
    Ksmall = np.array([[f, 0.0, W / 2 - 0.5], [0.0, f, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    K0 = Ksmall.copy()
    K0[:2] *= c          # the full-size camera: prepare_zju hands back Ksmall (powers of two: exact)
    R = np.eye(3)
    T = np.array([0.0, 0.0, 3.0]) - (lo + hi) / 2
    bounds = np.stack([lo, hi]).astype(np.float64)
    rng = np.random.RandomState(2)
    small_mask = (TR.bound_mask(Ksmall, R, T, bounds, H, W) * (rng.rand(H, W) < 0.5) * rng.randint(1, 20, (H, W))).astype(np.uint8)
    cihp = np.kron(small_mask, np.ones((c, c), np.uint8))
    img = rng.randint(0, 256, (c * H, c * W, 3)).astype(np.uint8)
    want = IP.prepare_zju(img, cihp, K0, D_REAL, c=c)
    assert np.array_equal(want["K"], Ksmall) and np.array_equal(want["msk_cihp"], small_mask)
    out = P.prepare_zju(img, cihp, K0, D_REAL, ratio=0.5)
    assert out["img"].is_cuda and out["msk_fg"].is_cuda and out["msk_cihp"].is_cuda and out["img"].dtype == torch.float64
    batch = r.sample_batch(out["img"], out["K"], R, T, bounds, out["msk_cihp"], 64, 77, occupancy_from=out["msk_fg"])
    host = r.sample_batch(torch.from_numpy(want["img"]).cuda(), want["K"], R, T, bounds, torch.from_numpy(want["msk_cihp"]).cuda(), 64, 77,
                          occupancy_from=torch.from_numpy(want["msk_fg"]).cuda())
    assert batch.keys() == host.keys() and "occupancy" in batch
    for k in batch:
        a, b = torch.as_tensor(batch[k]), torch.as_tensor(host[k])
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), k
    assert bool(batch["occupancy"].any())
    extra = make_batch(g)
    batch.update(xyz=extra["xyz"], poses=extra["poses"], frame=extra["frame"], Th=extra["Th"])
    coarse = r.render(batch)["coarse"]
    assert tuple(coarse["color"].shape[-2:]) == (64, 3) and bool(torch.isfinite(coarse["color"]).all())
    after = view()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k


@pytest.mark.parametrize("is_eval", [False, True])
def test_prepare_h36m_is_the_restatements_composition(P, is_eval):
    H, W = 48, 40
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[:H, :W]
    msk = np.zeros((H, W), np.uint8)
    msk[((y - 24) / 17.0) ** 2 + ((x - 19) / 11.0) ** 2 <= 1.0] = 5
    msk[(msk != 0) & (y > 30)] = 2
    K, D = camera(H, W), D_REAL
    for c in (2, 1):
        want = IP.prepare_h36m(img, msk, K, D, c=c, is_eval=is_eval)
        got = P.prepare_h36m(img, msk, K, D, ratio=1.0 / c, is_eval=is_eval)
        assert got.keys() == want.keys()
        for k in ("img", "msk", "orig_msk", "msk_cihp", "msk_cihp_eroded"):
            assert same(got[k], want[k]), (c, k)
        assert np.array_equal(got["K"], want["K"])
        assert (100 in want["msk"]) == (not is_eval) and want["msk_cihp_eroded"].any() and want["img"].dtype == np.float32
