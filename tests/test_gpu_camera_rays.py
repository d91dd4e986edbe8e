"""dsn_camera_rays on the device against the per-pixel numpy restatement (tests/camera_rays_restate.py), word for word, on outputs
pre-filled with 0xFF (DSN_POISON_SCRATCH) and plain: the edge cameras of tests/golden/camera_rays_edges.npz (zero direction
components, three planes within the slack, camera inside the box, box behind the camera, origin on a box plane), the generic
rotated camera, pixel counts around the 256-thread block, a singular K; then the two consumers - a training batch drawn on the
front camera and Renderer.view_batch."""
import numpy as np
import pytest
import torch

import camera_rays_restate as CR
import train_rays_restate as TR
from camera_rays_cases import CONVENTIONS, NAMES, camera, recorded, within_bars

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dsnerf_amd._lib


@pytest.fixture(autouse=True, params=["poisoned", "plain"])
def outputs(request, monkeypatch):
    if request.param == "poisoned":
        monkeypatch.setenv("DSN_POISON_SCRATCH", "1")          # every output tensor starts as 0xFF bytes
    else:
        monkeypatch.delenv("DSN_POISON_SCRATCH", raising=False)


def device(L, K, R, T, bounds, H, W, convention):
    return tuple(t.cpu().numpy() for t in L.camera_rays(K, R, T, bounds, H, W, device="cuda", convention=convention))


def same_words(a, b):
    """float32 arrays equal as 32-bit words; a NaN equals a NaN (its payload is the hardware's)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def assert_is_the_restatement(got, want, what):
    for k, a, b in zip(("ray_o", "ray_d", "near", "far"), got, want):
        assert same_words(a, b), (what, k, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
    assert got[4].dtype == np.bool_ and np.array_equal(got[4], want[4]), (what, "mask")


@pytest.mark.parametrize("convention", CONVENTIONS)
@pytest.mark.parametrize("name", NAMES)
def test_every_camera_is_the_restatement_word_for_word(L, name, convention):
    args = camera(name, convention)
    got = device(L, *args, convention)
    assert_is_the_restatement(got, CR.rays(*args, convention), (name, convention))
    again = device(L, *args, convention)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    # and, through the restatement, the reference's own arrays: mask equal, values within the older tests' bars
    g = recorded(name, convention)
    assert np.array_equal(got[4], g[4]) and all(within_bars(a, b) for a, b in zip(got[:4], g[:4]))


@pytest.mark.parametrize("convention", CONVENTIONS)
def test_singular_K_gives_nan_rays_and_no_hit(L, convention):
    """det K = 0: every direction is NaN, no ray hits, near = far = 0 (the reference's near < far is False on NaN)"""
    K = np.array([[40.0, 0.0, 26.0], [0.0, 0.0, 18.0], [0.0, 0.0, 1.0]])
    _, R, T, bounds, H, W = camera("front", convention)
    got = device(L, K, R, T, bounds, H, W, convention)
    assert_is_the_restatement(got, CR.rays(K, R, T, bounds, H, W, convention), ("singular", convention))
    assert np.isnan(got[1]).all() and np.isfinite(got[0]).all() and not got[4].any() and not got[2].any() and not got[3].any()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, device(L, K, R, T, bounds, H, W, convention)))


def test_wrapper_refuses_malformed_cameras(L):
    K, R, T, bounds, H, W = camera("front", CR.ZJU)
    with pytest.raises(ValueError):
        L.camera_rays(K[:2], R, T, bounds, H, W, device="cuda")
    with pytest.raises(ValueError):
        L.camera_rays(K, R, T, bounds[:1], H, W, device="cuda")
    with pytest.raises(ValueError):
        L.camera_rays(K, R, T, bounds, H, W, device="cuda", convention="blender")


# ---- consumers ---------------------------------------------------------------------------------------------------------------
def front_training_case():
    """an image and a body mask on the front camera (zju), and a seed - chosen with the restatement alone - whose batch draws from
    column 26 and from row 18, where a direction component is exactly zero"""
    K, R, T, bounds, H, W = camera("front", CR.ZJU)
    rng = np.random.default_rng(5)
    img = rng.random((H, W, 3))
    mask = np.zeros((H, W), np.uint8)
    mask[8:30, 14:40] = 1
    mask[10:14, 24:29] = 2
    rays = CR.rays(K, R, T, bounds, H, W, CR.ZJU)
    for seed in range(100):
        e = TR.sample(img, K, R, T, bounds, mask, 64, seed, rays=rays)
        if e["status"] == TR.OK and (e["coord"][:, 1] == 26).any() and (e["coord"][:, 0] == 18).any():
            return img, mask, seed, rays, e
    raise AssertionError("no seed below 100 draws from column 26 and row 18")


def test_training_batch_carries_the_whole_image_bits_on_the_zero_components(L):
    K, R, T, bounds, H, W = camera("front", CR.ZJU)
    img, mask, seed, rays, e = front_training_case()
    whole = device(L, K, R, T, bounds, H, W, CR.ZJU)
    out = L.train_rays(torch.from_numpy(img).cuda(), K, R, T, bounds, torch.from_numpy(mask).cuda(), 64, seed)
    assert int(out["status"]) == TR.OK
    coord = out["coord"].cpu().numpy()
    assert np.array_equal(coord, e["coord"])
    assert (coord[:, 1] == 26).any() and (coord[:, 0] == 18).any()
    p = coord[:, 0] * W + coord[:, 1]
    for k, full, restated in zip(("ray_o", "ray_d", "near", "far"), whole, rays):
        a = out[k].cpu().numpy()
        assert same_words(a, full[p]) and same_words(a, restated[p]), k
    zero = (coord[:, 1] == 26)
    assert (out["ray_d"].cpu().numpy()[zero, 0] == 0).all() and whole[4][p].all() and out["mask_at_box"].all()


@pytest.mark.parametrize("convention", CONVENTIONS)
def test_view_batch_returns_the_masked_rays(L, convention):
    from cases import load, make_renderer
    r = make_renderer(load("small_eval"))
    K, R, T, bounds, H, W = camera("front", convention)
    dev = torch.device("cuda")
    posed = {"xyz": torch.zeros(1, 4, 3, device=dev), "bounds": torch.from_numpy(np.asarray(bounds, np.float64))[None].to(dev),
             "poses": torch.zeros(1, 24, 3, device=dev), "Th": torch.zeros(1, 3, device=dev), "Rh_mat": torch.eye(3, device=dev)[None]}
    b = r.view_batch(posed, 0, K, R, T, H, W, convention=convention)
    want = CR.rays(K, R, T, bounds, H, W, convention)
    m = want[4]
    n = int(m.sum())
    assert n == (466 if convention == CR.ZJU else 425)
    assert np.array_equal(b["mask_at_box"][0].cpu().numpy(), m) and b["img"].shape == (1, H, W, 3)
    for k, full in zip(("ray_o", "ray_d", "near", "far"), want):
        a = b[k][0].cpu().numpy()
        assert a.shape == full[m].shape and same_words(a, full[m]), k
