"""The step after the hot path on the device (csrc/dsn_image.hip) beyond what one trip of its loops covers.

dsn_image_scatter: bit for bit against numpy boolean-mask assignment past 1024 count blocks, where the single-workgroup scan carries
between trips - on outputs and a workspace pre-filled with 0xFF (DSN_POISON_SCRATCH) and on plain ones, and again from a dirty
workspace.
dsn_image_psnr: against math.fsum over the per-pixel float64 squared errors, within a bar derived from the number of additions a term
passes through (tests/image_epilogue_restate.py), from 1 x 1 to the grid-stride loop at 1024 x 1024, with empty and full masks,
identical images and NaN pixels."""
import numpy as np
import pytest
import torch

import image_epilogue_restate as IE

pytestmark = pytest.mark.gpu

SLOTS = (("color", "coarse_color", 3), ("disp_map", "coarse_disp", 1), ("acc_map", "coarse_acc", 1), ("depth_map", "coarse_depth", 1))


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dsnerf_amd._lib


@pytest.fixture(autouse=True, params=["poisoned", "plain"])
def allocations(request, monkeypatch):
    if request.param == "poisoned":
        monkeypatch.setenv("DSN_POISON_SCRATCH", "1")          # every output tensor and workspace starts as 0xFF bytes
    else:
        monkeypatch.delenv("DSN_POISON_SCRATCH", raising=False)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


_sources = {}


def sources(rows):
    """per-ray arrays of `rows` rays (shared by the cases of one size): colours outside [0, 1], a NaN disparity and a NaN colour"""
    if rows not in _sources:
        rng = np.random.default_rng(rows)
        src = {"color": rng.standard_normal((rows, 3)).astype(np.float32), "disp_map": rng.random(rows).astype(np.float32),
               "acc_map": rng.random(rows).astype(np.float32), "depth_map": rng.random(rows).astype(np.float32)}
        for r in (0, rows // 2, rows - 1):
            src["disp_map"][r] = np.nan                     # disparity is NaN where a ray hit nothing
        src["color"][rows // 3, 1] = np.nan
        src["color"][rows - 1, 2] = np.nan
        _sources[rows] = (src, {k: cuda(v) for k, v in src.items()})
    return _sources[rows]


def check_scatter(L, H, W, mask, R, clamps=(False, True)):
    src, dev = sources(H * W)
    out = {k: v[:R] for k, v in dev.items()}
    m = cuda(mask)
    for clamp in clamps:
        img = L.image_scatter(out, m, H, W, clamp=clamp)
        for key, name, c in SLOTS:
            want = IE.scatter(src[key], mask, R, clamp=clamp and key == "color")
            got = img[name].cpu().numpy()
            assert got.shape == (H, W, c) and same_words(got.reshape(H * W, c), want), (name, clamp, R)
    return img


@pytest.mark.parametrize("H,W", IE.SCATTER_SIZES)
def test_scatter_past_one_scan_trip(L, H, W):
    """512 x 512 is exactly 1024 count blocks (one trip of k_img_scan), 513 x 512 the first carry, 1024 x 513 two carries: random,
    empty and full masks, single pixels on either side of the trip edge, exactly the blocks around it; R = popcount and popcount - 3
    (rank < R: the last three set pixels become zero); clamp and no clamp; NaN carried through"""
    for name, mask in IE.scatter_masks(H, W).items():
        pop = int(mask.sum())
        for R in sorted({pop, max(pop - 3, 0)}):
            check_scatter(L, H, W, mask, R)
        if pop > 3 and name == "random":
            three = np.flatnonzero(mask)[-3:]
            img = check_scatter(L, H, W, mask, pop - 3, clamps=(False,))
            assert not img["coarse_acc"].reshape(-1)[cuda(three)].any() and img["coarse_acc"].reshape(-1)[int(np.flatnonzero(mask)[-4])] != 0


def test_scatter_of_no_rays(L):
    """R = 0 with an empty mask: null sources are allowed, every image is zero"""
    H, W = 513, 512
    e = torch.zeros(0, device="cuda")
    img = L.image_scatter({"color": e.reshape(0, 3), "disp_map": e, "acc_map": e, "depth_map": e}, torch.zeros(H * W, dtype=torch.bool), H, W)
    for _, name, c in SLOTS:
        assert img[name].shape == (H, W, c) and not img[name].view(torch.int32).any()


def test_scatter_from_a_dirty_workspace(L, monkeypatch):
    """the count / offset array is rebuilt by every call: a workspace full of an earlier call's offsets, or of noise, changes nothing"""
    H, W = 1024, 513
    masks = IE.scatter_masks(H, W)
    nbytes = L.lib().dsn_image_workspace_bytes(H, W)
    ws = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
    clean = {name: check_scatter(L, H, W, masks[name], int(masks[name].sum()), clamps=(False,)) for name in ("random", "full")}
    handed = []

    def dirty(n, dev):
        assert n <= nbytes
        handed.append(n)
        return ws

    monkeypatch.setattr(L, "_scratch", dirty)
    for name in ("random", "full", "random"):          # noise first, then each other's offsets
        img = check_scatter(L, H, W, masks[name], int(masks[name].sum()), clamps=(False,))
        for _, key, _ in SLOTS:
            assert same_words(img[key].cpu().numpy(), clean[name][key].cpu().numpy()), (name, key)
    assert len(handed) == 3


def test_scatter_maps_null_slots(L):
    """image_scatter_maps at 513 x 512: one colour with one scalar (two null slots), and four scalars without a colour (the spare
    colour, then a call with two null slots)"""
    H, W = 513, 512
    mask = IE.scatter_masks(H, W)["random"]
    R = int(mask.sum())
    src, dev = sources(H * W)
    m = cuda(mask)
    rgb, sc = L.image_scatter_maps([dev["color"][:R]], [dev["disp_map"][:R]], m, H, W)
    assert len(rgb) == 1 and len(sc) == 1
    assert same_words(rgb[0].cpu().numpy().reshape(-1, 3), IE.scatter(src["color"], mask, R))          # (never clamped)
    assert same_words(sc[0].cpu().numpy().reshape(-1, 1), IE.scatter(src["disp_map"], mask, R))
    four = ["disp_map", "acc_map", "depth_map", "disp_map"]
    rgb, sc = L.image_scatter_maps([], [dev[k][:R] for k in four], m, H, W)
    assert rgb == [] and len(sc) == 4
    for k, img in zip(four, sc):
        assert img.shape == (H, W, 1) and same_words(img.cpu().numpy().reshape(-1, 1), IE.scatter(src[k], mask, R)), k


# ---- PSNR against an exact sum -----------------------------------------------------------------------------------------------------
PSNR_SIZES = [(1, 1), (15, 17), (16, 16), (1, 257), (512, 512), (513, 512), (1024, 1024)]
_images = {}


def images(H, W, gt_dtype):
    """(img float32, gt, their device copies, per-pixel float64 squared errors), made once per size and ground-truth type"""
    key = (H, W, np.dtype(gt_dtype).name)
    if key not in _images:
        rng = np.random.default_rng(H * 4099 + W)
        img = rng.random((H, W, 3)).astype(np.float32)
        gt = rng.random((H, W, 3)).astype(gt_dtype)
        _images[key] = (img, gt, cuda(img), cuda(gt), IE.squared_errors(img, gt))
    return _images[key]


def psnr_masks(H, W):
    n = H * W
    rng = np.random.default_rng(n)
    one = np.zeros(n, bool)
    one[(2 * n) // 3] = True
    return {"none": None, "empty": np.zeros(n, bool), "full": np.ones(n, bool), "one pixel": one, "random": rng.random(n) < 0.4}


@pytest.mark.parametrize("gt_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("H,W", PSNR_SIZES)
def test_psnr_against_the_exact_sum(L, H, W, gt_dtype):
    """bars (derived, tests/image_epilogue_restate.py): relative D 2^-53 on mse, absolute 10 D 2^-53 / ln 10 on psnr, D = ceil(n /
    (256 B)) + 8 + B, B = min(1024, blocks); two calls may differ by twice that.  The largest errors seen on the MI355X are in
    docs/LAB_NOTEBOOK.md (at 1024 x 1024: D = 1036, bars 1.15e-13 and 5.0e-13)."""
    img, gt, d_img, d_gt, e = images(H, W, gt_dtype)
    rel_bar, abs_bar = IE.psnr_bars(H * W)
    worst = [0.0, 0.0, 0.0, 0.0]
    for name, mask in psnr_masks(H, W).items():
        want = IE.psnr_reference(e, mask)
        m = None if mask is None else cuda(mask)
        got = L.image_psnr(d_img, d_gt, m).cpu().numpy()
        again = L.image_psnr(d_img, d_gt, m).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (4,)
        if name in ("none", "empty"):
            assert np.isnan(want[1]) and np.isnan(want[3]) and np.isfinite(want[[0, 2]]).all()      # the reference's mean of nothing
        if name == "full":
            assert want[1] == want[0]
        rel, ab = IE.psnr_errors(got, want)
        rel2, ab2 = IE.psnr_errors(again, got)
        worst = [max(a, b) for a, b in zip(worst, (rel, ab, rel2, ab2))]
        assert rel <= rel_bar and ab <= abs_bar, (name, rel, rel_bar, ab, abs_bar)
        assert rel2 <= 2 * rel_bar and ab2 <= 2 * abs_bar, (name, rel2, ab2)
    print(f"psnr {H} x {W} gt {np.dtype(gt_dtype).name}: D = {IE.additions(H * W)}, mse rel. error {worst[0]:.2e} (bar {rel_bar:.2e}), "
          f"psnr abs. error {worst[1]:.2e} (bar {abs_bar:.2e}); two calls: {worst[2]:.2e}, {worst[3]:.2e}")


def test_psnr_of_identical_images_is_infinite(L):
    H, W = 513, 512
    img, _, d_img, _, _ = images(H, W, np.float32)
    mask = psnr_masks(H, W)["random"]
    for gt in (d_img, d_img.double()):
        got = L.image_psnr(d_img, gt, cuda(mask)).cpu().numpy()
        assert got[0] == 0 and got[1] == 0 and got[2] == np.inf and got[3] == np.inf
    got = L.image_psnr(d_img, d_img, cuda(np.zeros(H * W, bool))).cpu().numpy()
    assert got[0] == 0 and got[2] == np.inf and np.isnan(got[1]) and np.isnan(got[3])


@pytest.mark.parametrize("where", ["img", "gt"])
def test_psnr_nan_pixel_reaches_only_its_sums(L, where):
    """a NaN pixel outside the mask: the unmasked pair is NaN, the masked pair keeps its value; inside the mask: all four"""
    H, W = 513, 512
    img, gt, _, _, _ = images(H, W, np.float64)
    mask = psnr_masks(H, W)["random"]
    rel_bar, abs_bar = IE.psnr_bars(H * W)
    outside, inside = int(np.flatnonzero(~mask)[-1]), int(np.flatnonzero(mask)[-1])      # both in the grid-stride loop's second trip
    assert min(outside, inside) >= 1024 * 256
    for p, masked in ((outside, False), (inside, True)):
        a, b = img.copy(), gt.copy()
        (a if where == "img" else b).reshape(-1, 3)[p, 1] = np.nan
        want = IE.psnr_reference(IE.squared_errors(a, b), mask)
        assert np.isnan(want[[0, 2]]).all() and np.isnan(want[[1, 3]]).all() == masked
        got = L.image_psnr(cuda(a), cuda(b), cuda(mask)).cpu().numpy()
        rel, ab = IE.psnr_errors(got, want)
        assert rel <= rel_bar and ab <= abs_bar


def test_image_metrics_on_a_synthetic_frame(L):
    """Renderer.image_metrics (clamp, then dsn_image_psnr) at 513 x 512 without a render, against the same exact-sum reference"""
    from cases import load, make_renderer
    r = make_renderer(load("small_eval"))
    H, W = 513, 512
    rng = np.random.default_rng(12)
    img = (1.4 * rng.random((H, W, 3)) - 0.2).astype(np.float32)          # a fifth of the values leave [0, 1]
    gt = rng.random((H, W, 3))
    mask = psnr_masks(H, W)["random"]
    m = r.image_metrics(cuda(img), {"img": torch.from_numpy(gt)[None], "mask_at_box": torch.from_numpy(mask)[None]})
    want = IE.psnr_reference(IE.squared_errors(np.clip(img, 0.0, 1.0), gt), mask)
    got = np.array([m["mse"], m["mse_wMask"], m["psnr_woMask"], m["psnr_wMask"]])
    rel_bar, abs_bar = IE.psnr_bars(H * W)
    rel, ab = IE.psnr_errors(got, want)
    assert set(m) == {"mse", "mse_wMask", "psnr_woMask", "psnr_wMask"} and rel <= rel_bar and ab <= abs_bar, (rel, ab)
    unclamped = IE.psnr_reference(IE.squared_errors(img, gt), mask)
    assert abs(unclamped[0] / want[0] - 1.0) > 1e-3          # (the clamp is visible in this frame)
