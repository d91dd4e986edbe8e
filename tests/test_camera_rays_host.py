"""tests/camera_rays_restate.py (the per-pixel numpy restatement of csrc/dsn_rays.h) against the reference's own get_rays /
get_near_far / get_rays_within_bounds outputs: tests/golden/camera_rays_edges.npz (axis-aligned cameras whose rays have zero direction
components, meet three planes, start inside the box or have it behind them; tests/golden/make_golden_rays.py) and the two older
fixtures.  The fixture's edges are counted, so it provably contains each one, and every mutant of the restatement is shown to move a
named check on a named camera.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import camera_rays_restate as CR
from camera_rays_cases import CONVENTIONS, EDGES, NAMES, camera, recorded, within_bars, words
from helpers import GOLDEN

def checks(name, convention, variant=None):
    """the named checks of one camera: the restatement (or a mutant of it) against the reference's recorded arrays"""
    ro, rd, near, far, mask = CR.rays(*camera(name, convention), convention, variant=variant)
    g_ro, g_rd, g_near, g_far, g_mask = recorded(name, convention)
    n2, f2, m2 = CR.near_far(g_ro, g_rd, camera(name, convention)[3], convention, variant=variant)
    return {"mask": np.array_equal(mask, g_mask),
            "rays": within_bars(ro, g_ro) and within_bars(rd, g_rd),
            "near": within_bars(near, g_near), "far": within_bars(far, g_far),
            "own-rays mask": np.array_equal(m2, g_mask),
            "own-rays near": np.array_equal(words(n2), words(g_near)), "own-rays far": np.array_equal(words(f2), words(g_far))}


@pytest.mark.parametrize("convention", CONVENTIONS)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference_on_every_edge_camera(name, convention):
    """mask equal; rays, near and far within the bars; near / far / mask restated from the reference's own float32 rays: its bits"""
    got = checks(name, convention)
    assert all(got.values()), got


def test_restatement_matches_the_older_fixtures():
    g = np.load(os.path.join(GOLDEN, "camera_rays.npz"))
    ro, rd, near, far, mask = CR.rays(g["K"], g["R"], g["T"], g["bounds"], int(g["H"]), int(g["W"]), CR.ZJU)
    assert np.array_equal(mask, g["mask_at_box"])
    assert within_bars(ro, g["ray_o"]) and within_bars(rd, g["ray_d"])
    assert within_bars(near[mask], g["near"]) and within_bars(far[mask], g["far"])
    assert not near[~mask].any() and not far[~mask].any()
    g = np.load(os.path.join(GOLDEN, "camera_rays_h36m.npz"))
    ro, rd, near, far, mask = CR.rays(g["K"], g["R"], g["T"], g["bounds"], int(g["H"]), int(g["W"]), CR.H36M)
    assert np.array_equal(mask, g["mask_at_box"])
    assert within_bars(ro, g["ray_o"]) and within_bars(rd, g["ray_d"])
    assert within_bars(near[mask], g["near"]) and within_bars(far[mask], g["far"])
    p = g["pick2"]                                              # every 37th pixel of the 1024 x 1024 frame
    ro, rd, near, far, mask = CR.rays(g["K2"], g["R"], g["T2"], g["bounds"], int(g["H2"]), int(g["W2"]), CR.H36M, pixels=p)
    assert np.array_equal(mask, g["mask2"])
    assert within_bars(rd, g["ray_d2"]) and within_bars(near, g["near2"]) and within_bars(far, g["far2"])


def test_fixture_contains_each_edge():
    """the counts the fixture was built for: were a camera to drift, the edge it exercises would silently leave the suite"""
    H, W = 37, 53
    px = lambda r, c: r * W + c
    rd, mask = recorded("front", CR.ZJU)[1], recorded("front", CR.ZJU)[4]
    assert int(mask.sum()) == 466
    assert np.array_equal(np.flatnonzero(rd[:, 0] == 0), np.arange(H) * W + 26)          # column 26: d_x = 0 exactly, 37 pixels
    assert np.array_equal(np.flatnonzero(rd[:, 1] == 0), 18 * W + np.arange(W))          # row 18: d_y = 0 exactly, 53 pixels
    assert mask[px(18, 26)] and mask[np.arange(H) * W + 26].sum() >= 10 and mask[18 * W + np.arange(W)].sum() >= 10
    # two rays meet three planes within the 1e-6 slack (a box edge): "exactly two" leaves them out, "at least two" would not
    three = np.flatnonzero(CR.rays(*camera("front", CR.ZJU), CR.ZJU, variant="at_least_two")[4] & ~mask)
    assert three.tolist() == [px(26, 38), px(28, 41)]
    rd, mask = recorded("front", CR.H36M)[1], recorded("front", CR.H36M)[4]
    assert int(mask.sum()) == 425 and int((rd == 0).sum()) == 90                        # 37 + 53 components take the clamps
    assert mask[np.arange(H) * W + 26].sum() >= 10 and mask[18 * W + np.arange(W)].sum() >= 10
    for convention in CONVENTIONS:
        assert recorded("inside", convention)[4].all() and recorded("inside", convention)[4].size == 1961
    # the box BEHIND the camera: the reference takes |t|, so rays pointing away from the box still "hit" it
    ro, rd, near, far, mask = recorded("behind", CR.ZJU)
    assert int(mask.sum()) == 186 and ro[0].tolist() == [0.0, 0.0, 6.0] and (rd[:, 2] > 0).all()
    assert near[px(18, 26)] == np.float32(2.99) and far[px(18, 26)] == np.float32(4.01)
    assert int(recorded("behind", CR.H36M)[4].sum()) == 176
    # the origin on the float32 box's x-min plane, column 26 running along that face
    ro, rd, _, _, mask = recorded("on_plane", CR.H36M)
    assert ro[0, 0] == EDGES["on_plane:h36m:bounds"][0, 0] and int(mask.sum()) == 430 and mask[np.arange(H) * W + 26].sum() >= 10
    assert [int(EDGES[f"{n}:H"]) * int(EDGES[f"{n}:W"]) for n in NAMES[-4:]] == [1, 255, 256, 257]


def test_axis_aligned_closed_forms():
    """R = I, d = (x, y, 1) before any normalisation: a ray that crosses both z-planes inside the x and y slabs has the plane
    parameters t = z_plane - o_z.  zju reports the distances |t| (padded planes; the smaller one first, whatever the signs), h36m the
    signed parameters of the unit direction, t * sqrt(1 + x^2 + y^2).  Within 4 float32 ulps (a handful of roundings each)."""
    H, W = 37, 53
    row, col = np.divmod(np.arange(H * W), W)
    x, y = (col - 26.0) / 40.0, (row - 18.0) / 40.0
    for name, oz in (("front", 0.0), ("inside", 2.5), ("behind", 6.0)):
        for convention, pad in ((CR.ZJU, 0.01), (CR.H36M, 0.0)):
            b = np.asarray(camera(name, convention)[3], np.float64)
            t0, t1 = b[0, 2] - pad - oz, b[1, 2] + pad - oz
            both = np.ones(H * W, bool)
            for t in (t0, t1):
                both &= (x * t > b[0, 0] - pad + 1e-4) & (x * t < b[1, 0] + pad - 1e-4)
                both &= (y * t > b[0, 1] - pad + 1e-4) & (y * t < b[1, 1] + pad - 1e-4)
            _, _, near, far, mask = CR.rays(*camera(name, convention), convention)
            if convention == CR.ZJU:
                want_near, want_far = np.sort(np.abs([t0, t1]))[:, None] * np.ones(H * W)
            else:
                want_near, want_far = t0 * np.sqrt(1.0 + x * x + y * y), t1 * np.sqrt(1.0 + x * x + y * y)
            assert both.sum() >= 100 and mask[both].all(), (name, convention, int(both.sum()))
            assert np.abs(near[both] / want_near[both] - 1.0).max() <= 4 * 2.0 ** -23, (name, convention)
            assert np.abs(far[both] / want_far[both] - 1.0).max() <= 4 * 2.0 ** -23, (name, convention)
    _, _, near, far, mask = CR.rays(*camera("inside", CR.H36M), CR.H36M)          # inside the box: near < 0 < far on every ray
    assert mask.all() and (near < 0).all() and (far > 0).all() and far[18 * W + 26] == np.float32(0.5) and near[18 * W + 26] == np.float32(-0.5)


@pytest.mark.parametrize("convention", CONVENTIONS)
def test_singular_K_gives_nan_rays_and_no_hit(convention):
    K = np.array([[40.0, 0.0, 26.0], [0.0, 0.0, 18.0], [0.0, 0.0, 1.0]])
    _, R, T, bounds, H, W = camera("front", convention)
    ro, rd, near, far, mask = CR.rays(K, R, T, bounds, H, W, convention)
    assert np.isfinite(ro).all() and np.isnan(rd).all()
    assert not mask.any() and not near.any() and not far.any()
    if convention == CR.H36M:           # C's fminf / fmaxf drop the NaN: -inf < +inf, every ray a "hit" with NaN near / far
        assert CR.rays(K, R, T, bounds, H, W, convention, variant="fmin_fmax")[4].all()


MUTANTS = [  # variant, convention, camera, the check it moves, checks that stay
    ("at_least_two", CR.ZJU, "front", "mask"),
    ("signed_t", CR.ZJU, "behind", "near"),
    ("no_pad", CR.ZJU, "front", "mask"),
    ("no_clamp", CR.H36M, "on_plane", "mask"),
    ("clamp_swapped", CR.H36M, "on_plane", "mask"),
]


@pytest.mark.parametrize("variant,convention,name,moved", MUTANTS)
def test_every_mutant_moves_its_named_check(variant, convention, name, moved):
    assert all(checks(name, convention).values())
    got = checks(name, convention, variant=variant)
    assert not got[moved] and not got["own-rays " + moved], (variant, got)
    assert got["rays"]                                       # (the mutants touch the box test, never the rays)
    W = 53
    ref_mask = recorded(name, convention)[4]
    mut = CR.rays(*camera(name, convention), convention, variant=variant)
    if variant == "at_least_two":
        assert np.flatnonzero(mut[4] != ref_mask).tolist() == [26 * W + 38, 28 * W + 41]
    if variant in ("no_clamp", "clamp_swapped"):             # exactly the zero-component column that runs along the face
        diff = np.flatnonzero(mut[4] != ref_mask)
        assert len(diff) >= 10 and (diff % W == 26).all() and not mut[4][diff].any()
    if variant == "signed_t":
        assert (mut[2][ref_mask] < 0).all() and np.array_equal(mut[4], ref_mask)
    if variant == "no_pad":
        assert mut[4].sum() < ref_mask.sum() and mut[2][18 * W + 26] == np.float32(2.0)


def test_clamp_mutants_are_invisible_where_the_origin_is_off_the_planes():
    """why the fixture needs the on_plane camera: with the origin strictly inside or outside a slab the sign of a +-1e-5 component
    (and a division by zero in its place) cannot change near < far - the front camera's 90 zero components do not tell them apart"""
    for variant in ("no_clamp", "clamp_swapped"):
        assert checks("front", CR.H36M, variant=variant)["mask"]


def test_library_argument_checks():
    """dsn_camera_rays refuses an empty image, an unknown convention and more than (2^31 - 1) / 3 pixels (its kernels index the
    [H*W, 3] arrays with int) before it touches the device"""
    import dsnerf_amd
    lib = dsnerf_amd._lib.lib()
    one = C.c_void_p(256)
    call = lambda H, W, convention: lib.dsn_camera_rays(one, one, one, one, H, W, convention, one, one, one, one, one, None)
    for args, what in (((0, 5, 0), b"empty image"), ((5, -1, 0), b"empty image"), ((4, 4, 2), b"unknown convention"),
                       ((65536, 32768, 0), b"2^31"), ((46341, 46341, 1), b"2^31"),
                       ((26755, 26755, 0), b"2^31"), ((715827883, 1, 1), b"2^31")):          # 715 827 882 = (2^31 - 1) // 3 is the most
        assert call(*args) != 0 and what in lib.dsn_last_error(), (args, lib.dsn_last_error())
    assert lib.dsn_camera_rays(None, one, one, one, 4, 4, 0, one, one, one, one, one, None) != 0
    assert b"null argument" in lib.dsn_last_error()
