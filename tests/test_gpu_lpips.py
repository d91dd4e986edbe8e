"""dsn_lpips / dsn_lpips_features (include/dsnerf.h "LPIPS", csrc/dsn_lpips.hip) against the float64 restatement of the rule
(tests/lpips_restate.py): the five taps of both backbones at sizes that straddle the kernel's tiles, the distance against the recorded
float64 values (tests/golden/lpips_golden.json), determinism, the status paths, the Python surface, and the sensitivity of these tests
to six deliberate mistakes in the rule.

Bars.  Taps: max|dev - f64| / max|f64| <= 4 x the float32 twin's pooled value of tests/golden/lpips_errors.json (two significand bits:
the split operands carry 22 against float32's 24), never looser than 1e-5.  Distance: relative error <= 4 x the twin's pooled scalar
error, never looser than 1e-5.  Parity with the `lpips` package itself: tests/test_lpips_package.py, where the package imports."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import lpips_restate as R
from helpers import load
from cases import make_batch, make_renderer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "lpips_golden.json")) as _f:
    GOLD = json.load(_f)
with open(os.path.join(GOLDEN, "lpips_errors.json")) as _f:
    ERR = json.load(_f)
NETS = ("alex", "vgg")
CASES = [(net, H, W) for net in NETS for H, W in R.SIZES[net]]
CASE_IDS = [f"{net}-{H}x{W}" for net, H, W in CASES]
BATCH_SIZE = (37, 53)


def tap_bar(net, l):
    return min(4.0 * ERR[net]["tap"][l], 1e-5)


def scalar_bar(net):
    return min(4.0 * ERR[net]["scalar"], 1e-5)


def L():
    from dsnerf_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def weights(net):
    return R.make_weights(net)


TINY = 1e-4


@functools.lru_cache(maxsize=None)
def tiny_weights(net):
    """the same network with every feature scaled by TINY (first convolution and all biases x TINY: the backbone is positively
    homogeneous): feature norms of order 1e-3, where the 1e-10 beside the root is 1e-7 of the norm and one inside the root would be
    1e-4 of it - the one place the eps placement shows"""
    w = weights(net)
    s = np.float32(TINY)
    conv = [((cw * s if i == 0 else cw), cb * s) for i, (cw, cb) in enumerate(w["conv"])]
    return {"conv": conv, "lin": w["lin"]}


@functools.lru_cache(maxsize=None)
def packed(net, tiny=False):
    w = tiny_weights(net) if tiny else weights(net)
    return L().lpips_pack(net, w["conv"], w["lin"], "cuda")


@functools.lru_cache(maxsize=None)
def pair(net, H, W):
    return R.make_pair(H, W, GOLD[net][f"{H}x{W}"]["seed"])


@functools.lru_cache(maxsize=None)
def ref_taps(net, H, W):
    """float64 taps of the case's two images: ([5 x [1,C,h,w]], [5 x [1,C,h,w]]) numpy - computed once, never written to"""
    img, gt = pair(net, H, W)
    out = tuple([t.numpy() for t in R.features(net, weights(net), s[None])] for s in (img, gt))
    for taps in out:
        for t in taps:
            t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch_frames(net):
    """five frames of BATCH_SIZE (img float32, gt float64) and their float64 distances"""
    H, W = BATCH_SIZE
    frames = [R.make_pair(H, W, 300 + k) for k in range(5)]
    img, gt = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    want, _ = R.lpips(net, weights(net), img, gt)
    return img, gt, want


def dev_lpips(net, img, gt, rgb_pm1=False, pk=None):
    out, layers, status = L().lpips(net, pk if pk is not None else packed(net), torch.as_tensor(img).cuda(), torch.as_tensor(gt).cuda(),
                                    rgb_pm1=rgb_pm1)
    return out.cpu().numpy(), layers.cpu().numpy(), status.cpu().numpy()


@pytest.fixture
def poisoned(monkeypatch):
    """workspaces, packed images and outputs start as 0xFF bytes (_lib._scratch / _lib._output)"""
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")


# ---- taps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,H,W", CASES, ids=CASE_IDS)
def test_taps(net, H, W, poisoned):
    img, gt = pair(net, H, W)
    stack = torch.from_numpy(np.stack([img, gt.astype(np.float32)])).cuda()
    taps, status = L().lpips_features(net, packed(net), stack)
    assert status.cpu().tolist() == [0, 0]
    want = ref_taps(net, H, W)
    assert [tuple(t.shape[1:]) for t in taps] == R.tap_shapes(net, H, W)
    for l, t in enumerate(taps):
        got = t.cpu().numpy().astype(np.float64)
        border = R.border_mask(*got.shape[2:])
        for i in range(2):
            ref = want[i][l][0]
            scale = np.abs(ref).max()
            err = np.abs(got[i] - ref) / scale
            e_border, e_inner = err[:, border].max(), (err[:, ~border].max() if (~border).any() else 0.0)
            print(f"{net} {H}x{W} tap {l} image {i}: border {e_border:.3e} interior {e_inner:.3e} bar {tap_bar(net, l):.3e}")
            assert e_border <= tap_bar(net, l), (l, i, "border", e_border, tap_bar(net, l))
            assert e_inner <= tap_bar(net, l), (l, i, "interior", e_inner, tap_bar(net, l))


# ---- the distance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,H,W", CASES + [("alex", 512, 512), ("vgg", 512, 512)], ids=CASE_IDS + ["alex-512x512", "vgg-512x512"])
def test_distance(net, H, W, poisoned):
    img, gt = pair(net, H, W)
    g = GOLD[net][f"{H}x{W}"]
    out, layers, status = dev_lpips(net, img[None], gt[None])
    assert status.tolist() == [0]
    rel = abs(out[0] - g["out"]) / g["out"]
    print(f"{net} {H}x{W}: {out[0]!r} want {g['out']!r} rel {rel:.3e} bar {scalar_bar(net):.3e}")
    assert rel <= scalar_bar(net), (out[0], g["out"], rel, scalar_bar(net))
    assert np.abs(layers[0] - np.array(g["layers"])).max() <= scalar_bar(net) * g["out"]
    assert out[0] == (((layers[0, 0] + layers[0, 1]) + layers[0, 2]) + layers[0, 3]) + layers[0, 4]
    out32, layers32, _ = dev_lpips(net, img[None], gt[None].astype(np.float32))     # (the ground truth is float32-exact: the cast changes nothing)
    assert out32.tobytes() == out.tobytes() and layers32.tobytes() == layers.tobytes()


@pytest.mark.parametrize("net", NETS)
def test_distance_with_small_feature_norms(net):
    """the eps placement: see tiny_weights"""
    img, gt, _ = batch_frames(net)
    want, _ = R.lpips(net, tiny_weights(net), img[:2], gt[:2])
    out, _, status = dev_lpips(net, img[:2], gt[:2], pk=packed(net, True))
    assert status.tolist() == [0, 0]
    rel = np.abs(out - want) / want
    print(f"{net} small norms: rel {rel} bar {scalar_bar(net):.3e}")
    assert rel.max() <= scalar_bar(net)


@pytest.mark.parametrize("net", NETS)
def test_batches_and_repeats_are_bit_identical(net, poisoned):
    img, gt, want = batch_frames(net)
    whole = dev_lpips(net, img, gt)
    assert whole[2].tolist() == [0] * 5
    assert np.abs(whole[0] - want).max() <= scalar_bar(net) * want.max()
    again = dev_lpips(net, img, gt)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
    singles = [dev_lpips(net, img[k:k + 1], gt[k:k + 1]) for k in range(5)]
    for k in range(5):
        assert singles[k][0].tobytes() == whole[0][k:k + 1].tobytes() and singles[k][1].tobytes() == whole[1][k:k + 1].tobytes(), k
    for F in (2, 3):
        part = dev_lpips(net, img[:F], gt[:F])
        assert part[0].tobytes() == whole[0][:F].tobytes() and part[1].tobytes() == whole[1][:F].tobytes(), F
    perm = [3, 0, 4, 2, 1]
    mixed = dev_lpips(net, img[perm], gt[perm])
    assert mixed[0].tobytes() == whole[0][perm].tobytes() and mixed[1].tobytes() == whole[1][perm].tobytes()


@pytest.mark.parametrize("net", NETS)
def test_symmetric_and_zero_on_identical_stacks(net):
    img, gt, _ = batch_frames(net)
    g32 = gt.astype(np.float32)
    ab, ba = dev_lpips(net, img[:3], g32[:3]), dev_lpips(net, g32[:3], img[:3])
    assert ab[0].tobytes() == ba[0].tobytes() and ab[1].tobytes() == ba[1].tobytes() and (ab[0] > 0.1).all()
    for other in (img[:3].copy(), img[:3].astype(np.float64)):
        same = dev_lpips(net, img[:3], other)
        assert same[2].tolist() == [0, 0, 0]
        assert same[0].tobytes() == np.zeros(3).tobytes() and same[1].tobytes() == np.zeros((3, 5)).tobytes()


@pytest.mark.parametrize("net", NETS)
def test_rgb_pm1_and_the_flip(net):
    img, gt, want = batch_frames(net)
    img, gt, want = img[:2], gt[:2], want[:2]
    bgr = dev_lpips(net, img, gt)
    # the package's call surface: RGB in [-1, 1] (the same float32 operations, done by the caller) gives the same bits
    to_pm1 = lambda a: np.ascontiguousarray((2.0 * torch.as_tensor(a).float() - 1.0).flip(-1).numpy())      # noqa: E731
    pm1 = dev_lpips(net, to_pm1(img), to_pm1(gt), rgb_pm1=True)
    assert pm1[0].tobytes() == bgr[0].tobytes()
    want_pm1, _ = R.lpips(net, weights(net), to_pm1(img), to_pm1(gt), rgb_pm1=True)
    assert np.abs(pm1[0] - want_pm1).max() <= scalar_bar(net) * want_pm1.max()
    # without the flip the value moves by far more than the bar, and the restatement WITH the flip is the one the device matches
    unflipped, _ = R.lpips(net, weights(net), img, gt, variant="no_flip")
    assert (np.abs(unflipped - want) / want).min() > 100 * scalar_bar(net)
    assert (np.abs(bgr[0] - want) / want).max() <= scalar_bar(net)
    # and the flag itself matters: the same arrays read as RGB in [-1, 1] are another image
    other = dev_lpips(net, img, gt, rgb_pm1=True)
    assert (np.abs(other[0] - bgr[0]) / bgr[0]).min() > 100 * scalar_bar(net)


# ---- status paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,H,W", [("alex", 30, 31), ("alex", 31, 30), ("vgg", 15, 16), ("vgg", 16, 15)])
def test_too_small(net, H, W, poisoned):
    img, gt = R.make_pair(H, W, 5)
    out, layers, status = dev_lpips(net, np.stack([img, img]), np.stack([gt, gt]))
    assert status.tolist() == [L().LPIPS_TOO_SMALL] * 2
    assert np.isnan(out).all() and np.isnan(layers).all()
    _, st = L().lpips_features(net, packed(net), torch.from_numpy(img[None]).cuda())
    assert st.cpu().tolist() == [L().LPIPS_TOO_SMALL]
    H2, W2 = max(H, R.MIN_SIDE[net]), max(W, R.MIN_SIDE[net])                # the smallest image itself has a value
    img, gt = R.make_pair(H2, W2, 5)
    assert dev_lpips(net, img[None], gt[None])[2].tolist() == [0]


@pytest.mark.parametrize("net", NETS)
def test_range_flag_is_confined_to_its_frame(net):
    """the first convolution scaled by 2e5: an ordinary image's activations leave the split's range (|v| >= 32768), while the image on
    which the scaling layer's output is zero - v = (shift + 1) / 2 per channel - sees the biases alone"""
    w = weights(net)
    wmax = float(np.abs(w["conv"][0][0]).max())
    big = {"conv": [(w["conv"][0][0] * np.float32(16000.0 / wmax), w["conv"][0][1])] + w["conv"][1:], "lin": w["lin"]}
    assert float(np.abs(big["conv"][0][0]).max()) < L().LPIPS_RANGE_MAX / 2
    pk = L().lpips_pack(net, big["conv"], big["lin"], "cuda")
    H, W = BATCH_SIZE
    img, gt, _ = batch_frames(net)
    zero_rgb = (np.array(R.SHIFT, np.float32) + np.float32(1.0)) * np.float32(0.5)
    flat = np.broadcast_to(zero_rgb[::-1], (H, W, 3)).astype(np.float32)      # BGR
    assert float(np.abs(R.scaling_layer(flat[None]).numpy()).max()) < 1e-7
    imgs = np.stack([flat, img[0], flat])
    gts = np.stack([flat, gt[0], flat]).astype(np.float64)
    gts[2] = gt[1]                                                           # frame 2: its ground truth alone leaves the range
    out, layers, status = dev_lpips(net, imgs, gts, pk=pk)
    assert status.tolist() == [0, L().LPIPS_RANGE, L().LPIPS_RANGE]
    assert out[0] == 0.0 and np.isnan(out[1:]).all() and np.isnan(layers[1:]).all()
    # a weight outside the range flags every frame of a call with that packed image
    huge = {"conv": [(w["conv"][0][0] * np.float32(40000.0 / wmax), w["conv"][0][1])] + w["conv"][1:], "lin": w["lin"]}
    assert float(np.abs(huge["conv"][0][0]).max()) >= L().LPIPS_RANGE_MAX
    pk2 = L().lpips_pack(net, huge["conv"], huge["lin"], "cuda")
    out, _, status = dev_lpips(net, imgs[:1], gts[:1], pk=pk2)
    assert status.tolist() == [L().LPIPS_RANGE] and np.isnan(out).all()
    # the ordinary weights are in range with room to spare
    assert GOLD[net]["128x96"]["max_activation"] < 32.0


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_pixel_is_confined_to_its_frame(net, bad):
    img, gt, _ = batch_frames(net)
    img, gt = img[:3].copy(), gt[:3].copy()
    clean = dev_lpips(net, img, gt)
    img[1, 17, 20, 1] = bad
    gt[2, 3, 4, 0] = bad
    out, layers, status = dev_lpips(net, img, gt)
    assert status.tolist() == [0, L().LPIPS_NONFINITE, L().LPIPS_NONFINITE]
    assert np.isnan(out[1:]).all() and np.isnan(layers[1:]).all()
    assert out[:1].tobytes() == clean[0][:1].tobytes() and layers[:1].tobytes() == clean[1][:1].tobytes()


# ---- frame chunks under the workspace cap ----------------------------------------------------------------------------------------
def cap_of(net, k):
    """the workspace of k frames (lpips) / k pairs (lpips_features) of BATCH_SIZE: as LPIPS_WORKSPACE_CAP it allows k per call"""
    return L().lib().dsn_lpips_workspace_bytes(L()._lpips_net(net), k, *BATCH_SIZE)


def recorded_calls(monkeypatch, name):
    """the frame counts of the C calls `name` that follow"""
    lib, calls = L().lib(), []
    real = getattr(lib, name)

    def spy(*args):
        calls.append(int(args[5 if name == "dsn_lpips" else 3]))
        return real(*args)

    monkeypatch.setattr(lib, name, spy, raising=False)
    return calls


@pytest.mark.parametrize("k,steps", [(1, [1, 1, 1, 1, 1]), (2, [2, 2, 1])])
@pytest.mark.parametrize("net", NETS)
def test_chunked_distance_is_the_uncapped_call(net, k, steps, poisoned, monkeypatch):
    """five frames under a cap of one and of two frames' workspace: the slices of out, layers and status, the even split and the
    short last chunk give the bits of the single call; a NaN pixel in frame 4 flags frame 4 alone"""
    img, gt, _ = batch_frames(net)
    whole = dev_lpips(net, img, gt)
    bad = img.copy()
    bad[4, 17, 20, 1] = np.nan
    whole_bad = dev_lpips(net, bad, gt)
    assert whole[2].tolist() == [0] * 5 and whole_bad[2].tolist() == [0, 0, 0, 0, L().LPIPS_NONFINITE]
    monkeypatch.setattr(L(), "LPIPS_WORKSPACE_CAP", cap_of(net, k))
    calls = recorded_calls(monkeypatch, "dsn_lpips")
    chunked = dev_lpips(net, img, gt)
    assert calls == steps
    assert all(a.tobytes() == b.tobytes() for a, b in zip(chunked, whole))
    chunked_bad = dev_lpips(net, bad, gt)
    assert chunked_bad[2].tolist() == [0, 0, 0, 0, L().LPIPS_NONFINITE]
    assert np.isnan(chunked_bad[0][4]) and np.isnan(chunked_bad[1][4]).all()
    assert chunked_bad[0][:4].tobytes() == whole[0][:4].tobytes() and chunked_bad[1][:4].tobytes() == whole[1][:4].tobytes()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(chunked_bad, whole_bad))


@pytest.mark.parametrize("net", NETS)
def test_chunked_features_are_the_uncapped_call(net, poisoned, monkeypatch):
    """lpips_features on an odd stack (n = 5) under the cap of one pair: calls of 2 + 2 + 1 images write the slices of the five taps
    and of status that the single call writes"""
    img, _, _ = batch_frames(net)
    stack = torch.from_numpy(img).cuda()
    taps, status = L().lpips_features(net, packed(net), stack)
    assert status.cpu().tolist() == [0] * 5 and [tuple(t.shape) for t in taps] == [(5, *s) for s in R.tap_shapes(net, *BATCH_SIZE)]
    monkeypatch.setattr(L(), "LPIPS_WORKSPACE_CAP", cap_of(net, 1))
    calls = recorded_calls(monkeypatch, "dsn_lpips_features")
    c_taps, c_status = L().lpips_features(net, packed(net), stack)
    assert calls == [2, 2, 1]
    assert c_status.cpu().numpy().tobytes() == status.cpu().numpy().tobytes()
    for l, (a, b) in enumerate(zip(c_taps, taps)):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), l


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def package_state_dict(net):
    w = weights(net)
    from dsnerf_amd.lpips import FEATURE_INDEX, _slice_of
    sd = {}
    for i, (cw, cb) in zip(FEATURE_INDEX[net], w["conv"]):
        sd[f"net.slice{_slice_of(net, i)}.{i}.weight"] = torch.from_numpy(cw)
        sd[f"net.slice{_slice_of(net, i)}.{i}.bias"] = torch.from_numpy(cb)
    for k, lw in enumerate(w["lin"]):
        sd[f"lin{k}.model.1.weight"] = sd[f"lins.{k}.model.1.weight"] = torch.from_numpy(lw).reshape(1, -1, 1, 1)
    sd["scaling_layer.shift"] = torch.tensor(R.SHIFT).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(R.SCALE).view(1, 3, 1, 1)
    return sd


@functools.lru_cache(maxsize=None)
def loss_fn(net):
    import dsnerf_amd
    return dsnerf_amd.lpips.LPIPS(net=net, state_dict=package_state_dict(net)).to("cuda")


@pytest.mark.parametrize("net", NETS)
def test_lpips_object_equals_the_binding(net):
    img, gt, want = batch_frames(net)
    pred = (2.0 * torch.from_numpy(img[:2]) - 1.0).flip(-1).permute(0, 3, 1, 2).cuda()        # test.py:77-84: NCHW RGB in [-1, 1]
    target = (2.0 * torch.from_numpy(gt[:2]).float() - 1.0).flip(-1).permute(0, 3, 1, 2).cuda()
    fn = loss_fn(net)
    d = fn(pred, target)
    assert d.shape == (2, 1, 1, 1) and d.dtype == torch.float32 and d.is_cuda
    direct = dev_lpips(net, img[:2], gt[:2])
    assert fn.last.cpu().numpy().tobytes() == direct[0].tobytes()
    assert fn.last_layers.cpu().numpy().tobytes() == direct[1].tobytes() and fn.last_status.cpu().tolist() == [0, 0]
    assert np.array_equal(d.reshape(-1).cpu().numpy(), direct[0].astype(np.float32))
    assert np.abs(direct[0] - want[:2]).max() <= scalar_bar(net) * want.max()


def small_body_views(n):
    """a renderer of the small body and n view batches of BATCH_SIZE with random ground truth"""
    g = load("small_eval")
    r = make_renderer(g)
    r.eval()
    H, W = BATCH_SIZE
    xyz = g["xyz"]
    lo, hi = xyz.min(0) - 0.05, xyz.max(0) + 0.05
    f = 0.9 * W
    K = np.array([[f, 0.0, W / 2 - 0.5], [0.0, f, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    batches = []
    for k in range(n):
        T = np.array([0.02 * k, 0.0, 3.0]) - (lo + hi) / 2
        ray_o, ray_d, near, far, mask = L().camera_rays(K, np.eye(3), T, np.stack([lo, hi]).astype(np.float64), H, W, device="cuda")
        idx = mask.nonzero().reshape(-1)
        b = make_batch(g)
        b.update(ray_o=ray_o[idx][None], ray_d=ray_d[idx][None], near=near[idx][None], far=far[idx][None], mask_at_box=mask[None],
                 img=torch.from_numpy(R.make_image(H, W, 900 + k).astype(np.float64))[None])
        batches.append(b)
    return r, batches


def _same_but_float_atomics(a, b):
    """dsn_image_psnr sums with float atomics (tests/test_gpu_ssim.py): its four keys repeat to 1e-12, not to the bit"""
    return all(abs(a[k] - b[k]) <= 1e-12 * abs(b[k]) for k in ("mse", "mse_wMask", "psnr_woMask", "psnr_wMask"))


def test_image_metrics_carries_both_keys():
    r, (b,) = small_body_views(1)
    nets = {"alex": loss_fn("alex"), "vgg": loss_fn("vgg")}
    dev = r.render_view(b, device_output=True)
    plain = r.image_metrics(dev["coarse_color"], b, ssim=True)
    m = r.image_metrics(dev["coarse_color"], b, ssim=True, lpips=nets)
    assert set(m) == set(plain) | {"lpips_alex", "lpips_vgg"}
    assert m["ssim"] == plain["ssim"] and _same_but_float_atomics(m, plain)
    assert set(r.image_metrics(dev["coarse_color"], b, lpips={"vgg": nets["vgg"]})) == {"mse", "mse_wMask", "psnr_woMask", "psnr_wMask", "lpips_vgg"}
    img = torch.clamp(dev["coarse_color"], 0.0, 1.0)
    for net in NETS:
        direct = dev_lpips(net, img[None].cpu().numpy(), b["img"].numpy())
        assert m[f"lpips_{net}"] == direct[0][0]
        want, _ = R.lpips(net, weights(net), img[None].cpu().numpy(), b["img"].numpy())
        assert abs(m[f"lpips_{net}"] - want[0]) <= scalar_bar(net) * want[0]
    with pytest.raises(ValueError, match="alex"):
        r.image_metrics(dev["coarse_color"], b, lpips={"squeeze": nets["alex"]})


def test_image_metrics_views_equals_single_calls():
    r, batches = small_body_views(3)
    nets = {"alex": loss_fn("alex"), "vgg": loss_fn("vgg")}
    imgs = [v["coarse_color"] for v in r.render_views(batches, device_output=True)]
    seq = r.image_metrics_views(imgs, batches, lpips=nets)
    assert len(seq) == 3
    for img, b, m in zip(imgs, batches, seq):
        one = r.image_metrics(img, b, ssim=True, lpips=nets)
        assert set(m) == set(one)
        assert all(m[k] == one[k] for k in ("ssim", "lpips_alex", "lpips_vgg")) and _same_but_float_atomics(m, one)
    assert [set(m) for m in r.image_metrics_views(imgs, batches)] == [set(r.image_metrics(i, b, ssim=True)) for i, b in zip(imgs, batches)]


@pytest.mark.parametrize("poison", [False, True])
def test_render_view_is_untouched_by_an_lpips_call_on_its_stream(poison, monkeypatch):
    if poison:
        monkeypatch.setenv("DSN_POISON_SCRATCH", "1")
    r, (b,) = small_body_views(1)
    before = {k: v.clone() for k, v in r.render_view(b, device_output=True).items() if torch.is_tensor(v)}
    img, gt, _ = batch_frames("vgg")
    first = [dev_lpips(net, img[:2], gt[:2]) for net in NETS]
    after = {k: v.clone() for k, v in r.render_view(b, device_output=True).items() if torch.is_tensor(v)}
    assert set(before) == set(after)
    for k in before:
        assert torch.equal(before[k].view(torch.uint8), after[k].view(torch.uint8)), k
    second = [dev_lpips(net, img[:2], gt[:2]) for net in NETS]
    assert all(a[0].tobytes() == c[0].tobytes() for a, c in zip(first, second))


# ---- sensitivity: each deliberate mistake in the rule is caught by the named check ---------------------------------------------------
def _tap_check_fails(net, H, W, variant):
    """would test_taps fail if the device computed `variant`?  (the device's taps stand in as the correct rule's: the distance of the
    variant's float64 taps from the correct float64 taps, against the bar)"""
    img, _ = pair(net, H, W)
    good = ref_taps(net, H, W)[0]
    shapes_differ, worst = False, 0.0
    for l, t in enumerate(R.features(net, weights(net), img[None], variant=variant)):
        t = t.numpy()
        if t.shape != good[l].shape:
            shapes_differ = True
            continue
        worst = max(worst, float(np.abs(t - good[l]).max() / np.abs(good[l]).max()) / tap_bar(net, l))
    return shapes_differ or worst > 10.0


def _distance_check_fails(net, H, W, variant):
    img, gt = pair(net, H, W)
    out, _ = R.lpips(net, weights(net), img[None], gt[None], variant=variant)
    g = GOLD[net][f"{H}x{W}"]["out"]
    return abs(out[0] - g) / g > 10.0 * scalar_bar(net)


def _small_norm_check_fails(net, H, W, variant):
    """test_distance_with_small_feature_norms"""
    img, gt, _ = batch_frames(net)
    want, _ = R.lpips(net, tiny_weights(net), img[:2], gt[:2])
    out, _ = R.lpips(net, tiny_weights(net), img[:2], gt[:2], variant=variant)
    return float((np.abs(out - want) / want).max()) > 10.0 * scalar_bar(net)


@pytest.mark.parametrize("variant,net,H,W,check", [
    ("no_flip", "alex", 64, 64, "taps"), ("no_flip", "vgg", 64, 64, "distance"),
    ("replicate_pad", "alex", 37, 53, "taps"), ("replicate_pad", "vgg", 17, 31, "taps"),
    ("ceil_pool", "alex", 35, 67, "taps"), ("ceil_pool", "vgg", 65, 63, "taps"),
    ("eps_inside", "alex", 37, 53, "small_norms"), ("eps_inside", "vgg", 37, 53, "small_norms"),
    ("pre_relu_taps", "alex", 31, 31, "taps"), ("pre_relu_taps", "vgg", 16, 16, "taps"),
    ("alex_stride3", "alex", 127, 129, "taps"),
])
def test_sensitivity(variant, net, H, W, check):
    """test_taps / test_distance of this case pass on the device (they run above) and would not with the mistake: the mistake moves the
    checked quantity by more than ten bars"""
    fails = {"taps": _tap_check_fails, "distance": _distance_check_fails, "small_norms": _small_norm_check_fails}[check]
    assert fails(net, H, W, variant), (variant, net, H, W, check)
    assert not fails(net, H, W, None)
