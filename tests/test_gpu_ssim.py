"""dsn_image_ssim (metrics.py:23-38 ssim_metric on the device) against the float64 oracle of tests/ssim_oracle.py, its error
cases, its determinism across calls and batches, and Renderer.image_metrics(ssim=True) / image_metrics_views end to end."""
import numpy as np
import pytest
import torch

from helpers import load
from cases import make_batch, make_renderer
from ssim_oracle import bounding_rect, ssim_metric

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _lib():
    from dsnerf_amd import _lib
    return _lib


def blob_mask(H, W, seed):
    """a few filled ellipses: the body-shaped masks of mask_at_box"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(3):
        cy, cx = rng.uniform(0.25, 0.75) * H, rng.uniform(0.25, 0.75) * W
        ry, rx = rng.uniform(0.15, 0.35) * H, rng.uniform(0.15, 0.35) * W
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return m


def make_mask(kind, H, W, seed=0):
    rng = np.random.default_rng(seed + 100)
    m = np.zeros((H, W), bool)
    if kind == "blobs":
        m = blob_mask(H, W, seed)
    elif kind == "full":
        m[:] = True
    elif kind == "borders":                      # touches all four image borders, holes inside
        m = rng.random((H, W)) < 0.7
        m[0, W // 3] = m[H - 1, W // 2] = m[H // 2, 0] = m[H // 3, W - 1] = True
    elif kind == "strip7":
        x0 = W // 3
        m[1:H - 2, x0:x0 + 7] = rng.random((H - 3, 7)) < 0.9
        m[1, x0] = m[1, x0 + 6] = True
    elif kind == "strip6":
        m[2:H - 1, 5:11] = True
    elif kind == "pixel":
        m[H // 2, W // 2] = True
    elif kind == "empty":
        pass
    else:
        raise ValueError(kind)
    return m


def make_images(H, W, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(lo, hi, (H, W, 3)).astype(np.float32)
    gt = np.clip(pred.astype(np.float64) * 0.8 + 0.1 + rng.normal(0, 0.05, (H, W, 3)), 0, 1)
    return pred, gt


def device_ssim(pred, gt, mask, clamp=False):
    s, rect, status = _lib().image_ssim(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(),
                                        torch.from_numpy(mask).cuda(), clamp=clamp)
    torch.cuda.synchronize()
    return s.cpu().numpy(), rect.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("H,W", [(37, 53), (96, 80), (512, 512), (1024, 1024)])
@pytest.mark.parametrize("kind", ["blobs", "full", "borders", "strip7"])
def test_ssim_matches_oracle(H, W, kind):
    seed = H * 7 + W + len(kind)
    pred, gt = make_images(H, W, seed)
    mask = make_mask(kind, H, W, seed)
    s, rect, status = device_ssim(pred, gt, mask)
    assert status.tolist() == [0]
    assert tuple(rect[0]) == bounding_rect(mask)
    want = ssim_metric(pred, gt, mask)
    assert abs(float(s[0]) - want) <= TOL, (float(s[0]), want)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("gt_dtype", [np.float64, np.float32])
def test_ssim_out_of_range_pred_and_gt_dtype(clamp, gt_dtype):
    H, W = 96, 80
    pred, gt = make_images(H, W, 11, lo=-0.5, hi=1.5)
    gt = gt.astype(gt_dtype)
    mask = make_mask("blobs", H, W, 5)
    s, _, status = device_ssim(pred, gt, mask, clamp=clamp)
    ref_pred = np.clip(pred, 0, 1) if clamp else pred
    want = ssim_metric(ref_pred.astype(np.float64), gt.astype(np.float64), mask)
    assert status.tolist() == [0]
    assert abs(float(s[0]) - want) <= TOL, (float(s[0]), want)


def test_identical_images_give_exactly_one():
    pred, _ = make_images(64, 72, 3)
    mask = make_mask("blobs", 64, 72, 3)
    s, _, _ = device_ssim(pred, pred.astype(np.float64), mask)
    assert float(s[0]) == 1.0


@pytest.mark.parametrize("kind,status", [("strip6", 1), ("pixel", 1), ("empty", 2)])
def test_too_small_crops_have_no_value(kind, status):
    H, W = 40, 50
    pred, gt = make_images(H, W, 1)
    mask = make_mask(kind, H, W)
    s, rect, st = device_ssim(pred, gt, mask)
    assert st.tolist() == [status] and np.isnan(s[0])
    assert tuple(rect[0]) == bounding_rect(mask)
    with pytest.raises(ValueError):
        ssim_metric(pred, gt, mask)               # (the oracle agrees: skimage raises)
    # the Renderer raises ValueError too, and never returns a number
    r = make_renderer(load("small_view"))
    batch = {"img": torch.from_numpy(gt)[None], "mask_at_box": torch.from_numpy(mask.reshape(-1))[None]}
    with pytest.raises(ValueError):
        r.image_metrics(torch.from_numpy(pred).cuda(), batch, ssim=True)
    m = r.image_metrics(torch.from_numpy(pred).cuda(), batch)      # psnr alone is still defined (mask=empty: nan)
    assert "ssim" not in m


def test_repeat_calls_and_batches_are_bit_identical():
    H, W = 96, 80
    kinds = ["blobs", "full", "borders", "strip7", "blobs"]
    preds, gts, masks = [], [], []
    for k, kind in enumerate(kinds):
        p, g = make_images(H, W, 40 + k, lo=-0.2, hi=1.2)
        preds.append(p), gts.append(g), masks.append(make_mask(kind, H, W, 40 + k))
    P, G, M = np.stack(preds), np.stack(gts), np.stack(masks)
    first = device_ssim(P, G, M, clamp=True)
    for _ in range(3):
        again = device_ssim(P, G, M, clamp=True)
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
    for k in range(len(kinds)):
        one = device_ssim(preds[k], gts[k], masks[k], clamp=True)
        assert one[0].tobytes() == first[0][k:k + 1].tobytes(), k
        assert np.array_equal(one[1][0], first[1][k]) and one[2][0] == first[2][k]
        want = ssim_metric(np.clip(preds[k], 0, 1), gts[k], masks[k])
        assert abs(float(first[0][k]) - want) <= TOL


def test_batch_mixes_valid_and_invalid_frames():
    H, W = 37, 53
    kinds = ["blobs", "empty", "strip6", "full"]
    data = [make_images(H, W, 60 + k) for k in range(len(kinds))]
    M = np.stack([make_mask(kind, H, W, 60 + k) for k, kind in enumerate(kinds)])
    s, _, st = device_ssim(np.stack([d[0] for d in data]), np.stack([d[1] for d in data]), M)
    assert st.tolist() == [0, 2, 1, 0]
    assert np.isnan(s[1]) and np.isnan(s[2])
    for k in (0, 3):
        assert abs(float(s[k]) - ssim_metric(data[k][0], data[k][1], M[k])) <= TOL


def _view_batch(g, seed):
    H, W = int(g["H"]), int(g["W"])
    b = make_batch(g)
    b["img"] = torch.from_numpy(np.random.default_rng(seed).random((1, H, W, 3)))
    b["mask_at_box"] = torch.from_numpy(g["mask_at_box"])[None]
    return b


def test_image_metrics_ssim_end_to_end():
    g = load("small_view")
    r = make_renderer(g)
    r.eval()
    H, W = int(g["H"]), int(g["W"])
    b = _view_batch(g, 0)
    dev = r.render_view(b, device_output=True)
    m = r.image_metrics(dev["coarse_color"], b, ssim=True)
    plain = r.image_metrics(dev["coarse_color"], b)
    assert set(m) == set(plain) | {"ssim"}
    assert all(abs(m[k] - plain[k]) <= 1e-12 * abs(plain[k]) for k in plain)     # (dsn_image_psnr sums with float atomics)
    host = np.clip(dev["coarse_color"].cpu().numpy().astype(np.float64), 0, 1)
    want = ssim_metric(host, b["img"][0].numpy(), g["mask_at_box"].reshape(H, W))
    assert abs(m["ssim"] - want) <= TOL, (m["ssim"], want)


def test_image_metrics_views_matches_per_frame_metrics():
    g = load("small_view")
    r = make_renderer(g)
    r.eval()
    batches = [_view_batch(g, s) for s in (1, 2, 3)]
    views = r.render_views(batches, device_output=True)
    imgs = [v["coarse_color"] for v in views]
    seq = r.image_metrics_views(imgs, batches)
    assert len(seq) == 3
    for img, b, m in zip(imgs, batches, seq):
        one = r.image_metrics(img, b, ssim=True)
        assert set(m) == set(one)
        assert m["ssim"] == one["ssim"]                                         # bit-identical in a batch
        assert all(abs(m[k] - one[k]) <= 1e-12 * abs(one[k]) for k in one)      # (dsn_image_psnr sums with float atomics)
    # without ssim: the keys of image_metrics' default
    plain = r.image_metrics_views(imgs, batches, ssim=False)
    assert [set(m) for m in plain] == [set(r.image_metrics(i, b)) for i, b in zip(imgs, batches)]
