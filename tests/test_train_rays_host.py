"""The training-batch sampler's rule (include/dsnerf.h: dsn_train_rays / dsn_bound_mask) without a GPU: the numpy restatement against
the reference's own my_sample_ray / sample_ray_h36m (tests/golden/train_rays.npz, made by tests/golden/make_golden_train_rays.py),
the pieces of the rule on closed forms, and the argument checks of the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import train_rays_restate as TR
from helpers import GOLDEN, maxdiff

CASES = ("zju", "zju_half", "zju_noface", "h36m")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "train_rays.npz"))


def case(g, name):
    return {k.split(":", 1)[1]: g[k] for k in g.files if k.startswith(name + ":")}


def restated(c, name):
    conv = TR.H36M if name == "h36m" else TR.ZJU
    return TR.sample(c["img"], c["K"], c["R"], c["T"], c["bounds"], c["mask"], int(c["nrays"]), int(c["seed"]), convention=conv,
                     mask_b=c.get("mask_b"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(golden, name):
    """coord, rgb, mask_at_box and the box mask exactly; near and far as tests/test_gpu_stages.py compares camera_rays.npz (the
    reference's training path evaluates the box test on the float64 rays, the rule on the float32 rays dsn_camera_rays writes)"""
    c = case(golden, name)
    e = restated(c, name)
    assert e["status"] == TR.OK and e["rounds"] == int(c["rounds"])
    n = int(c["nrays"])
    assert c["coord"].shape == (n, 2) and c["coord"].dtype == np.int64
    assert np.array_equal(e["coord"], c["coord"])
    assert c["rgb"].dtype == np.float32 and np.array_equal(e["rgb"], c["rgb"])
    assert np.array_equal(e["mask_at_box"], c["mask_at_box"]) and c["mask_at_box"].all()
    assert np.array_equal(e["bound_mask"], c["bound_mask"]) and 0 < c["bound_mask"].sum() < c["bound_mask"].size
    assert maxdiff(e["ray_o"], c["ray_o"]) <= 2.4e-7 and maxdiff(e["ray_d"], c["ray_d"]) <= 1.2e-7
    dn, df = maxdiff(e["near"], c["near"]), maxdiff(e["far"], c["far"])
    print(name, "near", dn, "far", df)
    assert dn <= 2.4e-7 and df <= 4.8e-7
    # the fixture's cameras stay clear of rounding ties, and the recorded corners are the rounded projections
    assert TR.half_integer_distance(c["K"], c["R"], c["T"], c["bounds"]) > 1e-6
    assert np.array_equal(TR.rounded_corners(c["K"], c["R"], c["T"], c["bounds"]), c["corners"])


def test_fixture_covers_the_cases_it_is_there_for(golden):
    c = case(golden, "zju_half")
    hit = TR.whole_image_rays(c["K"], c["R"], c["T"], c["bounds"], *c["mask"].shape, TR.ZJU)[4].reshape(c["mask"].shape)
    assert 0.35 < hit[c["mask"] != 0].mean() < 0.65 and int(c["rounds"]) >= 3          # the reference itself needs several rounds
    assert not (case(golden, "zju_noface")["mask"] == 2).any()
    assert (case(golden, "zju")["mask"] == 2).any()
    h = case(golden, "h36m")
    assert ((h["mask"] == 100) & (h["bound_mask"] == 1)).any()
    assert ((h["mask_b"] == 2) & (h["bound_mask"] != 1)).any()                       # a face pixel the box does not cut away
    assert {tuple(case(golden, n)["mask"].shape) for n in CASES} == {(40, 48), (37, 53)}
    # sample_ray_h36m blanks the image outside the box mask: a drawn face pixel beside it is black
    out = h["bound_mask"][h["coord"][:, 0], h["coord"][:, 1]] != 1
    assert np.all(h["rgb"][out] == 0) and np.all(h["rgb"][~out] == h["img"][h["coord"][~out, 0], h["coord"][~out, 1]])


def test_quotas_are_pythons_int():
    rem = np.arange(1, 65537)
    body = np.array([int(r * 0.6) for r in rem])
    face = np.array([int(r * 0.05) for r in rem])
    assert np.array_equal(rem * 6 // 10, body) and np.array_equal(rem * 5 // 100, face)
    q = [TR.quotas(int(r)) for r in (1, 7, 64, 1000, 65536)]
    assert q == [(0, 0, 1), (4, 0, 3), (38, 3, 23), (600, 50, 350), (39321, 3276, 22939)]


def _triangle(a, b, c, H, W):
    """independent of the winding rule: inclusive sign test of the three edge functions"""
    y, x = np.mgrid[:H, :W]
    e = [(q[0] - p[0]) * (y - p[1]) - (q[1] - p[1]) * (x - p[0]) for p, q in ((a, b), (b, c), (c, a))]
    return (np.all([v >= 0 for v in e], axis=0) | np.all([v <= 0 for v in e], axis=0))


def _segment(a, b, H, W):
    y, x = np.mgrid[:H, :W]
    cross = (b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0])
    return (cross == 0) & (x >= min(a[0], b[0])) & (x <= max(a[0], b[0])) & (y >= min(a[1], b[1])) & (y <= max(a[1], b[1]))


def test_union_rule_on_closed_forms():
    H, W = 14, 17
    # an axis-aligned box face: the inclusive rectangle, either orientation, with or without the repeated closing vertex
    want = np.zeros((H, W), bool)
    want[3:9, 2:11] = True
    for pts in ([(2, 3), (10, 3), (10, 8), (2, 8)], [(2, 8), (10, 8), (10, 3), (2, 3)], [(2, 3), (10, 3), (10, 8), (2, 8), (2, 3)]):
        assert np.array_equal(TR.loop_mask(pts, H, W), want)
    # a loop that leaves the image is cut, not wrapped
    cut = np.zeros((H, W), bool)
    cut[0:4, 12:17] = True
    assert np.array_equal(TR.loop_mask([(12, -5), (30, -5), (30, 3), (12, 3)], H, W), cut)
    assert not TR.loop_mask([(20, 20), (30, 20), (30, 30)], H, W).any()
    # a degenerate loop of collinear corners: its segments' pixels and nothing else
    diag = np.zeros((H, W), bool)
    diag[np.arange(1, 8), np.arange(1, 8)] = True
    assert np.array_equal(TR.loop_mask([(1, 1), (4, 4), (7, 7), (2, 2)], H, W), diag)
    row = np.zeros((H, W), bool)
    row[5, 3:13] = True
    assert np.array_equal(TR.loop_mask([(3, 5), (12, 5), (8, 5), (6, 5)], H, W), row)
    one = np.zeros((H, W), bool)
    one[6, 4] = True
    assert np.array_equal(TR.loop_mask([(4, 6), (4, 6), (4, 6), (4, 6)], H, W), one)
    # the reference's typo loop [4, 5, 7, 6, 5] is the triangle 5-7-6 plus the segment 4-5
    c = {4: (1, 2), 5: (6, 9), 7: (15, 11), 6: (12, 1)}
    typo = TR.loop_mask([c[4], c[5], c[7], c[6], c[5]], H, W)
    assert np.array_equal(typo, _triangle(c[5], c[7], c[6], H, W) | _segment(c[4], c[5], H, W))
    assert typo.sum() > _triangle(c[5], c[7], c[6], H, W).sum()                        # (the segment adds pixels)
    assert not np.array_equal(typo, TR.loop_mask([c[4], c[5], c[7], c[6]], H, W))     # ... and it is not the quadrilateral
    # triangles in general position against the independent sign test
    rng = np.random.RandomState(3)
    for _ in range(50):
        a, b, d = (tuple(int(v) for v in rng.randint(-3, 20, 2)) for _ in range(3))
        if (b[0] - a[0]) * (d[1] - a[1]) == (b[1] - a[1]) * (d[0] - a[0]):
            continue          # (collinear: the sign test below describes a whole line; the degenerate loops are checked above)
        assert np.array_equal(TR.loop_mask([a, b, d], H, W), _triangle(a, b, d, H, W)), (a, b, d)


def test_box_mask_is_the_union_not_the_hull(golden):
    """the six loops of a convex box's faces cover its silhouette; what the rule adds over any single face is the union"""
    c = case(golden, "zju")
    H, W = c["mask"].shape
    m = TR.bound_mask(c["K"], c["R"], c["T"], c["bounds"], H, W)
    assert np.array_equal(m, c["bound_mask"])
    faces = [TR.loop_mask(c["corners"][list(l)], H, W) for l in TR.LOOPS]
    assert np.array_equal(m.astype(bool), np.any(faces, axis=0)) and any(f.sum() < m.sum() for f in faces)
    # a corner behind the camera: no mask, and the batch says so
    T = c["T"].copy()
    T[2] = 0.1
    assert TR.rounded_corners(c["K"], c["R"], T, c["bounds"]) is None and not TR.bound_mask(c["K"], c["R"], T, c["bounds"], H, W).any()
    assert TR.sample(c["img"], c["K"], c["R"], T, c["bounds"], c["mask"], 8, 1)["status"] == TR.BAD_CAMERA


def _mix_int(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def test_draws():
    # the header's hash in plain Python integers
    for seed, r, c, k in ((0, 0, 0, 0), (11, 3, 2, 4095), (2 ** 32 - 1, 63, 1, 65535)):
        want = _mix_int(_mix_int((seed + 0x9E3779B9 * (3 * r + c)) & 0xFFFFFFFF) ^ k)
        assert int(TR.hash32(seed, r, c, k)) == want
    assert int(TR.hash32(0, 0, 0, 0)) == 0 and int(TR.hash32(0, 0, 0, 1)) == _mix_int(1)
    # always below the count, count 1 included; a pure function of (seed, r, c, k)
    for count in (1, 2, 63, 64, 65, 1000, 2 ** 31 - 1):
        d = TR.draw_indices(5, 2, 1, 4096, count)
        assert d.min() >= 0 and d.max() < count and (count > 1) == (len(np.unique(d)) > 1)
        assert np.array_equal(d, TR.draw_indices(5, 2, 1, 4096, count))
        assert np.array_equal(d[:100], TR.draw_indices(5, 2, 1, 100, count))          # slot k does not depend on the round's size
    assert not np.array_equal(TR.draw_indices(5, 2, 1, 64, 1000), TR.draw_indices(6, 2, 1, 64, 1000))
    assert not np.array_equal(TR.draw_indices(5, 2, 1, 64, 1000), TR.draw_indices(5, 3, 1, 64, 1000))
    assert not np.array_equal(TR.draw_indices(5, 2, 1, 64, 1000), TR.draw_indices(5, 2, 2, 64, 1000))
    # spread: 65536 slots over 64 bins
    for seed, r, c in ((0, 0, 0), (11, 1, 2), (123456789, 40, 1)):
        bins = np.bincount(TR.draw_indices(seed, r, c, 65536, 64), minlength=64)
        assert 0.8 * 1024 <= bins.min() and bins.max() <= 1.25 * 1024, (seed, r, c, bins.min(), bins.max())


def test_rounds_statuses_and_determinism(golden):
    c = case(golden, "zju_half")
    H, W = c["mask"].shape
    rays = TR.whole_image_rays(c["K"], c["R"], c["T"], c["bounds"], H, W, TR.ZJU)
    kw = dict(rays=rays)
    a = TR.sample(c["img"], c["K"], c["R"], c["T"], c["bounds"], c["mask"], 200, 5, **kw)
    b = TR.sample(c["img"], c["K"], c["R"], c["T"], c["bounds"], c["mask"], 200, 5, **kw)
    other = TR.sample(c["img"], c["K"], c["R"], c["T"], c["bounds"], c["mask"], 200, 6, **kw)
    assert np.array_equal(a["coord"], b["coord"]) and not np.array_equal(a["coord"], other["coord"])
    assert rays[4][a["coord"][:, 0] * W + a["coord"][:, 1]].all()
    # no body pixel: EMPTY_CLASS; nothing acceptable: SHORT after MAX_ROUNDS rounds
    assert TR.sample(c["img"], c["K"], c["R"], c["T"], c["bounds"], np.zeros_like(c["mask"]), 16, 1, **kw)["status"] == TR.EMPTY_CLASS
    hit = rays[4].reshape(H, W)
    miss = (~hit).astype(np.uint8)
    s = TR.sample(c["img"], c["K"], c["R"], c["T"], c["bounds"], miss, 16, 1, bound_mask_in=miss, **kw)
    assert s["status"] == TR.SHORT and s["rounds"] == TR.MAX_ROUNDS and not s["mask_at_box"].any()


def test_abi_argument_checks():
    import dsnerf_amd
    L = dsnerf_amd._lib
    lib = L.lib()
    assert {"dsn_bound_mask", "dsn_train_rays_workspace_bytes", "dsn_train_rays"} <= set(L.EXPORTS)
    assert lib.dsn_abi_version() == 8
    assert (L.TRAIN_RAYS_OK, L.TRAIN_RAYS_EMPTY_CLASS, L.TRAIN_RAYS_SHORT, L.TRAIN_RAYS_BAD_CAMERA) == (TR.OK, TR.EMPTY_CLASS, TR.SHORT, TR.BAD_CAMERA)
    assert (L.TRAIN_RAYS_MAX_ROUNDS, L.TRAIN_RAYS_MAX_RAYS) == (TR.MAX_ROUNDS, TR.MAX_RAYS)
    wsb = lib.dsn_train_rays_workspace_bytes
    n = wsb(512, 512, 4096)
    assert n >= 3 * 512 * 512 // 8 + 2 * 4 * 4096 and n < 1 << 20                     # three bit planes and two slot lists
    assert wsb(1024, 1024, 8192) < 2 << 20
    assert wsb(0, 4, 1) == 0 and wsb(4, 4, 0) == 0 and wsb(4, 4, 65537) == 0 and wsb(65536, 32768, 1) == 0 and wsb(4, 4, 65536) > 0
    one, z = C.c_void_p(256), None
    big = C.c_size_t(1 << 30)

    def call(K=one, H=8, W=8, conv=0, i64=one, i32=z, mask_a=one, mask_b=z, occ_src=z, nrays=4, occ=z, status=one, ws=one, nbytes=big):
        return lib.dsn_train_rays(K, one, one, one, H, W, conv, i64, i32, mask_a, mask_b, z, occ_src, nrays, 1, one, one, one, one, one,
                                  one, occ, one, one, status, one, ws, nbytes, z)

    for kw, msg in ((dict(K=z), b"null argument"), (dict(mask_a=z), b"null argument"), (dict(status=z), b"null argument"),
                    (dict(ws=z), b"null argument"), (dict(H=0), b"empty image"), (dict(H=65536, W=32768), b"2^31"),
                    (dict(nrays=0), b"nrays"), (dict(nrays=65537), b"nrays"), (dict(conv=2), b"unknown convention"),
                    (dict(i32=one), b"exactly one"), (dict(i64=z), b"exactly one"), (dict(conv=1), b"mask_b"),
                    (dict(occ=one), b"go together"), (dict(occ_src=one), b"go together"), (dict(nbytes=C.c_size_t(64)), b"workspace_bytes"),
                    (dict(ws=C.c_void_p(264)), b"16-byte aligned")):
        assert call(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_train_rays" in err and msg in err, (kw, err)
    assert lib.dsn_bound_mask(z, one, one, one, 8, 8, one, z) != 0 and b"dsn_bound_mask" in lib.dsn_last_error()
    assert lib.dsn_bound_mask(one, one, one, one, 8, 8, z, z) != 0 and b"null argument" in lib.dsn_last_error()
    assert lib.dsn_bound_mask(one, one, one, one, 0, 8, one, z) != 0 and b"empty image" in lib.dsn_last_error()
    assert lib.dsn_bound_mask(one, one, one, one, 65536, 32768, one, z) != 0 and b"2^31" in lib.dsn_last_error()
