"""dsn_train_rays / dsn_bound_mask on the device against the numpy restatement (tests/train_rays_restate.py), bit for bit.

The restatement is given the device's own whole-image rays (_lib.camera_rays): the rule says a drawn pixel carries the bits
dsn_camera_rays writes for it, and the box test that accepts it is that call's mask_at_box.  On the fixture cameras that mask is
also the oracle's, so the device batch is the reference's own coord / rgb as well (tests/golden/train_rays.npz)."""
import os

import numpy as np
import pytest
import torch

import train_rays_restate as TR
from helpers import GOLDEN, load

pytestmark = pytest.mark.gpu

KEYS = ("ray_o", "ray_d", "near", "far", "coord", "rgb", "mask_at_box", "bound_mask")


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dsnerf_amd._lib


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "train_rays.npz"))
    return {n: {k.split(":", 1)[1]: g[k] for k in g.files if k.startswith(n + ":")} for n in ("zju", "zju_half", "zju_noface", "h36m")}


_rays = {}


def device_rays(L, K, R, T, bounds, H, W, conv):
    """the whole-image call once per camera: numpy (ray_o, ray_d, near, far, hit)"""
    key = (K.tobytes(), R.tobytes(), T.tobytes(), np.asarray(bounds, np.float64).tobytes(), H, W, conv)
    if key not in _rays:
        _rays[key] = tuple(t.cpu().numpy() for t in L.camera_rays(K, R, T, bounds, H, W, convention=conv))
    return _rays[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_and_compare(L, img, K, R, T, bounds, mask, nrays, seed, conv="zju", mask_b=None, bound_mask=None, occ=None, workspace=None):
    """device batch (numpy) after comparing every output with the restatement, bit for bit"""
    H, W = img.shape[:2]
    rays = device_rays(L, K, R, T, bounds, H, W, conv)
    e = TR.sample(img, K, R, T, bounds, mask, nrays, seed, convention=conv, mask_b=mask_b, bound_mask_in=bound_mask, occupancy_src=occ,
                  rays=rays)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = L.train_rays(t(img), K, R, T, bounds, t(mask), nrays, seed, convention=conv, mask_b=t(mask_b), occupancy_src=t(occ),
                     bound_mask_in=t(bound_mask), workspace=workspace)
    out = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items() if k != "workspace"}
    assert int(out["status"]) == e["status"] and int(out["rounds"]) == e["rounds"], (out["status"], out["rounds"], e["status"], e["rounds"])
    for k in KEYS:
        assert out[k].shape == e[k].shape and out[k].dtype == e[k].dtype, (k, out[k].shape, out[k].dtype, e[k].dtype)
        assert np.array_equal(bits(out[k]), bits(e[k])), k
    if occ is not None:
        assert np.array_equal(out["occupancy"], e["occupancy"])
    else:
        assert out["occupancy"] is None
    if e["status"] == TR.OK:          # the bits of the whole-image call at coord
        p = out["coord"][:, 0] * W + out["coord"][:, 1]
        for k, full in zip(("ray_o", "ray_d", "near", "far"), rays):
            assert np.array_equal(bits(out[k]), bits(full[p])), k
        assert rays[4][p].all() and out["mask_at_box"].all()
    out["expected"] = e
    return out


def fixture_args(c, name):
    return dict(img=c["img"], K=c["K"], R=c["R"], T=c["T"], bounds=c["bounds"], mask=c["mask"], conv="h36m" if name == "h36m" else "zju",
                mask_b=c.get("mask_b"))


@pytest.mark.parametrize("name", ["zju", "zju_half", "zju_noface", "h36m"])
def test_fixture_cases_are_the_references_batch(L, golden, name):
    """40 x 48 and 37 x 53 (off every tile and ballot-word boundary), both conventions, both image dtypes, an empty face class, a body
    half beside the box (several rounds), msk == 100: the restatement's bits, which here are the reference's coord and rgb"""
    c = golden[name]
    a = fixture_args(c, name)
    H, W = c["mask"].shape
    occ = (c["mask"] != 0).astype(np.uint8) * 7
    out = run_and_compare(L, nrays=int(c["nrays"]), seed=int(c["seed"]), occ=occ, **a)
    assert int(out["status"]) == TR.OK and int(out["rounds"]) == int(c["rounds"])
    assert np.array_equal(device_rays(L, c["K"], c["R"], c["T"], c["bounds"], H, W, a["conv"])[4],
                          TR.whole_image_rays(c["K"], c["R"], c["T"], c["bounds"], H, W, a["conv"])[4])
    assert np.array_equal(out["coord"], c["coord"]) and np.array_equal(out["rgb"], c["rgb"])
    assert np.array_equal(out["bound_mask"], c["bound_mask"])
    assert np.array_equal(out["occupancy"], occ[c["coord"][:, 0], c["coord"][:, 1]])
    # dsn_bound_mask on its own
    m = L.bound_mask(c["K"], c["R"], c["T"], c["bounds"], H, W).cpu().numpy()
    assert m.dtype == np.uint8 and np.array_equal(m, c["bound_mask"])
    assert np.array_equal(m, TR.bound_mask(c["K"], c["R"], c["T"], c["bounds"], H, W))


@pytest.mark.parametrize("conv", ["zju", "h36m"])
@pytest.mark.parametrize("nrays", [1, 7, 64, 1000, 4096])
def test_batch_sizes(L, golden, conv, nrays):
    name = "h36m" if conv == "h36m" else "zju_half"
    out = run_and_compare(L, nrays=nrays, seed=1000 + nrays, **fixture_args(golden[name], name))
    assert int(out["status"]) == TR.OK and out["coord"].shape == (nrays, 2)


def test_other_image_dtype_same_batch(L, golden):
    c = golden["zju"]
    a = fixture_args(c, "zju")
    assert a["img"].dtype == np.float64
    o64 = run_and_compare(L, nrays=64, seed=2, **a)
    a["img"] = a["img"].astype(np.float32)
    o32 = run_and_compare(L, nrays=64, seed=2, **a)
    assert np.array_equal(o64["coord"], o32["coord"]) and np.array_equal(o64["rgb"], o32["rgb"])
    h = golden["h36m"]
    a = fixture_args(h, "h36m")
    a["img"] = a["img"].astype(np.float64) + 1e-9          # float64 values that are no float32: the cast is the kernel's
    run_and_compare(L, nrays=50, seed=2, **a)


def wide_camera(H, W):
    """every pixel's ray meets the box (checked by the caller), every corner in front of the camera"""
    f = 0.35 * W
    K = np.array([[f, 0.0, W / 2 - 0.5], [0.0, f, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    return K, np.eye(3), np.array([0.02, -0.01, 3.0]), np.array([[-6.0, -6.0, -0.3], [6.0, 6.0, 0.3]])


@pytest.mark.parametrize("conv", ["zju", "h36m"])
def test_class_edges(L, conv):
    """the rank-select's ends and the counts at which a ballot word or a tile fills: a class of one pixel, body pixels at the first
    and the last pixel of the image, classes of exactly 64, 65 and 256 (one tile) pixels, scattered and packed"""
    H, W = 37, 53
    K, R, T, bounds = wide_camera(H, W)
    assert device_rays(L, K, R, T, bounds, H, W, conv)[4].all()
    rng = np.random.RandomState(5)
    img = rng.rand(H, W, 3).astype(np.float32)
    ones = np.ones((H, W), np.uint8)
    cihp = np.zeros((H, W), np.uint8)
    cihp.reshape(-1)[[3, 700, 1960]] = 2
    body_value = 1
    masks = {}
    for n in (1, 64, 65, 256):
        m = np.zeros(H * W, np.uint8)
        m[rng.permutation(H * W)[:n]] = body_value
        masks[f"scattered{n}"] = m.reshape(H, W)
        m = np.zeros(H * W, np.uint8)
        m[192:192 + n] = body_value                   # packed from a word boundary on: whole words, then one bit more
        masks[f"packed{n}"] = m.reshape(H, W)
    ends = np.zeros(H * W, np.uint8)
    ends[[0, H * W - 1]] = body_value
    masks["ends"] = ends.reshape(H, W)
    last = np.zeros(H * W, np.uint8)
    last[H * W - 1] = body_value
    masks["last"] = last.reshape(H, W)
    for name, m in masks.items():
        out = run_and_compare(L, img, K, R, T, bounds, m, 64, 17, conv=conv, mask_b=cihp, bound_mask=ones)
        # (zju: these masks hold no 2, the face draws are left out: 38 + 23 rays in round 0, the last 3 in round 1)
        assert int(out["status"]) == TR.OK and int(out["rounds"]) == (1 if conv == "h36m" else 2), name
        body = out["coord"][:38]                      # int(64 * 0.6) body slots
        assert m[body[:, 0], body[:, 1]].all(), name
        if name == "ends":
            assert {tuple(v) for v in body} == {(0, 0), (H - 1, W - 1)}
        if name == "last":
            assert {tuple(v) for v in body} == {(H - 1, W - 1)}
    # a random class of one pixel (the caller's box mask), a face class of one pixel
    one = np.zeros((H, W), np.uint8)
    one[20, 31] = 1
    body = (rng.rand(H, W) < 0.3).astype(np.uint8)
    body[20, 31] = 1
    face1 = np.zeros((H, W), np.uint8)
    face1[36, 52] = 2
    cm = np.where(face1 == 2, 2, body).astype(np.uint8) if conv == "zju" else body
    out = run_and_compare(L, img, K, R, T, bounds, cm, 64, 3, conv=conv, mask_b=face1, bound_mask=one)
    assert int(out["status"]) == TR.OK
    if conv == "zju":
        assert (out["coord"][38:41] == (36, 52)).all() and (out["coord"][41:] == (20, 31)).all()
    else:
        assert (out["coord"][:38] == (20, 31)).all()      # body = msk == 1 inside the box: that one pixel


def rejection_case(L, golden):
    """zju_half's camera with the caller's box mask set everywhere and the body lying almost wholly beside the box: a round keeps about one draw in eight"""
    c = golden["zju_half"]
    H, W = c["mask"].shape
    hit = device_rays(L, c["K"], c["R"], c["T"], c["bounds"], H, W, "zju")[4].reshape(H, W)
    body = (~hit).astype(np.uint8)
    ys, xs = np.nonzero(hit)
    body[ys[:100], xs[:100]] = 1
    bound = (~hit).astype(np.uint8)
    bound[ys[-200:], xs[-200:]] = 1
    return c, body, bound


def test_rejection_heavy_takes_tens_of_rounds(L, golden):
    c, body, bound = rejection_case(L, golden)
    out = run_and_compare(L, c["img"], c["K"], c["R"], c["T"], c["bounds"], body, 64, 4, bound_mask=bound)
    print("rounds", int(out["rounds"]), "status", int(out["status"]))
    assert int(out["status"]) == TR.OK and 10 <= int(out["rounds"]) <= TR.MAX_ROUNDS
    assert int(out["rounds"]) == out["expected"]["rounds"]


def test_callers_bound_mask(L, golden):
    """a box mask of the caller's replaces the computed one: it is the random class, it blanks the h36m colours, it comes back"""
    for name in ("zju", "h36m"):
        c = golden[name]
        a = fixture_args(c, name)
        mine = c["bound_mask"].copy()
        mine[:, : mine.shape[1] // 2] = 0
        mine[5:30, 20:24] = 1
        out = run_and_compare(L, nrays=100, seed=8, bound_mask=mine, **a)
        assert np.array_equal(out["bound_mask"], mine) and int(out["status"]) == TR.OK
        assert not np.array_equal(out["coord"], run_and_compare(L, nrays=100, seed=8, **a)["coord"])


def test_same_seed_same_bits_and_dirty_workspace(L, golden):
    c = golden["zju_half"]
    a = fixture_args(c, "zju_half")
    first = run_and_compare(L, nrays=200, seed=5, **a)
    again = run_and_compare(L, nrays=200, seed=5, **a)
    other = run_and_compare(L, nrays=200, seed=6, **a)
    for k in KEYS:
        assert np.array_equal(bits(first[k]), bits(again[k])), k
    assert not np.array_equal(first["coord"], other["coord"])
    n = L.lib().dsn_train_rays_workspace_bytes(37, 53, 200)
    for fill in (0xFF, 0x00, None):
        ws = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        if fill is None:
            ws.copy_(torch.from_numpy(np.random.RandomState(1).randint(0, 256, n + 64).astype(np.uint8)))
        else:
            ws.fill_(fill)
        dirty = run_and_compare(L, nrays=200, seed=5, workspace=ws, **a)
        for k in KEYS:
            assert np.array_equal(bits(first[k]), bits(dirty[k])), (k, fill)


def test_1024_square_8192_rays(L):
    """the frame size of the Human3.6M config: pixel indices and word offsets past 2^16 rows of tiles, 4096 tiles per class"""
    H = W = 1024
    g = np.load(os.path.join(GOLDEN, "camera_rays_h36m.npz"))
    K, R, T, bounds = g["K2"], g["R"], g["T2"], g["bounds"]
    assert TR.half_integer_distance(K, R, T, bounds) > 1e-6
    rng = np.random.RandomState(11)
    img = rng.rand(H, W, 3).astype(np.float32)
    y, x = np.mgrid[:H, :W]
    cihp = np.zeros((H, W), np.uint8)
    cihp[((y - 520) / 330.0) ** 2 + ((x - 500) / 150.0) ** 2 <= 1] = 4
    cihp[(cihp != 0) & (y < 300)] = 2
    msk = (cihp != 0).astype(np.uint8)
    msk[(msk == 1) & (rng.rand(H, W) < 0.02)] = 100
    msk[H - 1, W - 1] = 1
    occ = (rng.rand(H, W) < 0.5).astype(np.uint8)
    out = run_and_compare(L, img, K, R, T, bounds, msk, 8192, 2024, conv="h36m", mask_b=cihp, occ=occ)
    assert int(out["status"]) == TR.OK
    assert out["coord"][:, 0].max() > 700 and (out["coord"][:, 0] * W + out["coord"][:, 1]).max() > 1 << 19
    out = run_and_compare(L, img, K, R, T, bounds, cihp, 8192, 2025, conv="zju")
    assert int(out["status"]) == TR.OK


@pytest.fixture(scope="module")
def renderer():
    from cases import make_renderer
    g = load("small_eval")
    r = make_renderer(g, "small_eval")
    r.eval()
    return g, r


def test_status_paths_raise(L, golden, renderer):
    _, r = renderer
    c = golden["zju"]
    a = (c["K"], c["R"], c["T"], c["bounds"])
    img = torch.from_numpy(c["img"]).cuda()
    with pytest.raises(ValueError, match="empty"):
        r.sample_batch(img, *a, np.zeros_like(c["mask"]), 16, 1)
    b = r.sample_batch(img, *a, np.zeros_like(c["mask"]), 16, 1, check=False)
    assert int(b["status"]) == L.TRAIN_RAYS_EMPTY_CLASS and not bool(b["mask_at_box"].any())
    # nothing acceptable: the caller's box mask and the body lie wholly beside the box
    H, W = c["mask"].shape
    miss = (~device_rays(L, *a, H, W, "zju")[4].reshape(H, W)).astype(np.uint8)
    assert miss.any()
    with pytest.raises(RuntimeError, match="64 rounds"):
        r.sample_batch(img, *a, miss, 16, 1, bound_mask=miss)
    b = r.sample_batch(img, *a, miss, 16, 1, bound_mask=miss, check=False)
    assert int(b["status"]) == L.TRAIN_RAYS_SHORT and int(b["rounds"]) == L.TRAIN_RAYS_MAX_ROUNDS
    out = run_and_compare(L, c["img"], *a, miss, 16, 1, bound_mask=miss)
    assert int(out["status"]) == TR.SHORT and not out["mask_at_box"].any()
    # a box corner behind the camera
    T = c["T"].copy()
    T[2] = 0.1
    with pytest.raises(ValueError, match="behind the camera"):
        r.sample_batch(img, c["K"], c["R"], T, c["bounds"], c["mask"], 16, 1)
    assert not bool(L.bound_mask(c["K"], c["R"], T, c["bounds"], H, W).any())
    with pytest.raises(ValueError):
        r.sample_batch(img, *a, c["mask"], 0, 1)
    with pytest.raises(ValueError):
        r.sample_batch(img, *a, c["mask"], 65537, 1)
    with pytest.raises(ValueError):
        r.sample_batch(img, *a, c["mask"], 16, 1, convention="blender")


def test_render_takes_the_batch_and_render_view_is_untouched(L, renderer):
    """Renderer.render on a sample_batch batch (device tensors, no copy) equals render on the same arrays passed through the host;
    render_view of a golden frame is the same before and after a sample_batch call"""
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
    H, W = 37, 53
    f = 0.9 * W
    K = np.array([[f, 0.0, W / 2 - 0.5], [0.0, f, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    R = np.eye(3)
    T = np.array([0.0, 0.0, 3.0]) - (lo + hi) / 2
    bounds = np.stack([lo, hi]).astype(np.float64)
    assert TR.half_integer_distance(K, R, T, bounds) > 1e-6
    rng = np.random.RandomState(2)
    img = torch.from_numpy(rng.rand(H, W, 3)).cuda()
    mask = torch.from_numpy(TR.bound_mask(K, R, T, bounds, H, W) * (rng.rand(H, W) < 0.5)).cuda()
    batch = r.sample_batch(img, K, R, T, bounds, mask, 64, 77, occupancy_from=mask)
    assert all(batch[k].is_cuda for k in ("rgb", "ray_o", "ray_d", "near", "far", "coord", "mask_at_box", "occupancy", "mybound_mask"))
    assert batch["ray_o"].shape == (1, 64, 3) and batch["near"].shape == (1, 64) and batch["coord"].shape == (1, 64, 2)
    assert batch["mybound_mask"].shape == (1, H, W) and batch["coord"].dtype == torch.int64
    extra = make_batch(g)
    host = {k: batch[k].cpu() for k in ("ray_o", "ray_d", "near", "far")}
    for b in (batch, host):
        b.update(xyz=extra["xyz"], poses=extra["poses"], frame=extra["frame"], Th=extra["Th"])
    ptr = batch["ray_o"].data_ptr()
    a = {k: v.clone() for k, v in r.render(batch)["coarse"].items() if torch.is_tensor(v)}
    assert batch["ray_o"].data_ptr() == ptr
    h = r.render(host)["coarse"]
    for k in ("color", "acc_map", "depth_map", "weights", "z_vals"):
        assert torch.equal(a[k], h[k]), k
    after = view()
    assert before.keys() == after.keys()
    for k in before:      # bit patterns (NaN-safe: disp is NaN where acc is 0, like the reference)
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
