"""the numpy statements tests/test_gpu_image_epilogue.py compares the device with (tests/image_epilogue_restate.py), checked on their
own: the scan-shaped scatter is the boolean-mask assignment, the exact-sum PSNR is the reference's formula, and the two mutants - a
scan that drops its carry at 1024 blocks, a masked mean divided by the pixel count - move the expected values.  No GPU."""
import math

import numpy as np
import pytest

import image_epilogue_restate as IE

SIZES, masks = IE.SCATTER_SIZES, IE.scatter_masks


@pytest.mark.parametrize("H,W", SIZES)
def test_scan_shaped_scatter_is_the_mask_assignment_and_the_dropped_carry_is_not(H, W):
    n = H * W
    assert -(-n // 256) == {512: 1024, 513: 1026, 1024: 2052}[H]
    rng = np.random.default_rng(7)
    src = rng.standard_normal((n, 1)).astype(np.float32)
    for name, mask in masks(H, W).items():
        pop = int(mask.sum())
        for R in sorted({pop, max(pop - 3, 0)}):
            want = IE.scatter(src, mask, R)
            assert np.array_equal(IE.scatter_by_scan(src, mask, R), want), (name, R)
            moved = not np.array_equal(IE.scatter_by_scan(src, mask, R, carry=False), want)
            # the carry matters exactly when a set pixel lies beyond block 1023 and one before it
            needs_carry = mask[262144:].any() and mask[:262144].any() and R > 0
            assert moved == bool(needs_carry), (name, R)
        if name in ("random", "full"):
            assert moved == (n > 512 * 512)
    if n > 512 * 512:
        offs, short = IE.block_offsets(masks(H, W)["full"]), IE.block_offsets(masks(H, W)["full"], carry=False)
        assert offs[1024] == 262144 and short[1024] == 0 and np.array_equal(offs[:1024], short[:1024])


def test_rank_limit_zeroes_the_last_masked_pixels():
    mask = np.zeros(600, bool)
    mask[[3, 255, 256, 300, 599]] = True
    src = np.arange(1, 6, dtype=np.float32).reshape(5, 1)
    assert IE.scatter(src, mask, 5)[mask, 0].tolist() == [1, 2, 3, 4, 5]
    assert IE.scatter(src, mask, 2)[mask, 0].tolist() == [1, 2, 0, 0, 0]
    assert IE.scatter_by_scan(src, mask, 2)[mask, 0].tolist() == [1, 2, 0, 0, 0]
    clamped = IE.scatter(np.array([[-1.0], [np.nan], [2.0], [0.5], [1.0]], np.float32), mask, 5, clamp=True)[mask, 0]
    assert np.array_equal(clamped, np.array([0.0, np.nan, 1.0, 0.5, 1.0], np.float32), equal_nan=True)


def test_psnr_reference_is_the_reference_formula():
    """metrics.py:8-21 in float64 numpy on a small image: the exact-sum statement agrees to the rounding of numpy's own sum"""
    rng = np.random.default_rng(3)
    H, W = 15, 17
    img, gt, mask = rng.random((H, W, 3)).astype(np.float32), rng.random((H, W, 3)), rng.random((H, W)) < 0.4
    d2 = (img.astype(np.float64) - gt) ** 2
    want = np.array([d2.mean(), d2[mask].mean(), -10 * np.log10(d2.mean()), -10 * np.log10(d2[mask].mean())])
    got = IE.psnr_reference(IE.squared_errors(img, gt), mask)
    assert np.allclose(got, want, rtol=1e-14, atol=0)
    # the mutant: the masked mean over all pixels instead of the set ones - far outside the device's bar
    rel_bar, abs_bar = IE.psnr_bars(H * W)
    mutant = IE.psnr_reference(IE.squared_errors(img, gt), mask, divide_by_n=True)
    assert abs(mutant[1] / got[1] - 1.0) > 1e6 * rel_bar and abs(mutant[3] - got[3]) > 1e6 * abs_bar
    assert np.array_equal(mutant[[0, 2]], got[[0, 2]])
    full = IE.psnr_reference(IE.squared_errors(img, gt), np.ones(H * W, bool), divide_by_n=True)
    assert np.array_equal(full, IE.psnr_reference(IE.squared_errors(img, gt), np.ones(H * W, bool)))      # (invisible on a full mask)


def test_psnr_reference_edges():
    img = np.full((4, 5, 3), 0.25, np.float32)
    e = IE.squared_errors(img, img.astype(np.float64))
    got = IE.psnr_reference(e, np.ones(20, bool))
    assert got[0] == 0 and got[1] == 0 and got[2] == np.inf and got[3] == np.inf            # identical images
    got = IE.psnr_reference(e + 1.0, np.zeros(20, bool))
    assert got[0] == 1.0 / 3.0 and np.isnan(got[1]) and np.isnan(got[3]) and np.isfinite(got[2])      # the mean of nothing
    assert np.array_equal(IE.psnr_reference(e + 1.0, None), got, equal_nan=True)
    e2 = e + 1.0
    e2[7] = np.nan
    m = np.zeros(20, bool)
    m[:7] = True
    got = IE.psnr_reference(e2, m)
    assert np.isnan(got[0]) and np.isnan(got[2]) and got[1] == 1.0 / 3.0                   # a NaN outside the mask: the unmasked two
    m[7] = True
    assert np.isnan(IE.psnr_reference(e2, m)).all()


def test_bars_are_the_derived_ones():
    """D = ceil(n / (256 B)) + 8 + B with B = min(1024, blocks)"""
    assert [IE.additions(n) for n in (1, 255, 256, 257, 512 * 512, 513 * 512, 1024 * 1024)] == [10, 10, 10, 11, 1033, 1034, 1036]
    rel, ab = IE.psnr_bars(1024 * 1024)
    assert rel == 1036 * 2.0 ** -53 and ab == 10 * rel / math.log(10.0) and rel < 1.2e-13      # (the 1e-12 it replaces was 9 x wider)


def test_error_helper_rejects_what_the_bars_could_not():
    """Python's max(0.0, nan) is 0.0: a helper that folded errors with it would let a NaN result - a poisoned output left
    unwritten, a NaN leaking into the masked pair - pass every bar.  psnr_errors refuses each of them"""
    want = IE.psnr_reference(np.array([0.25, 0.5, 1.0, 2.0]), np.array([True, False, True, False]))
    assert np.isfinite(want).all()
    assert IE.psnr_errors(want, want) == [0.0, 0.0]
    poisoned = np.frombuffer(b"\xff" * 32, np.float64)
    assert np.isnan(poisoned).all()
    with pytest.raises(AssertionError):
        IE.psnr_errors(poisoned, want)                                   # an output nobody wrote
    for i in range(4):                                                   # a NaN in any single slot
        got = want.copy()
        got[i] = np.nan
        with pytest.raises(AssertionError):
            IE.psnr_errors(got, want)
    nan_outside = np.array([np.nan, want[1], np.nan, want[3]])           # a NaN pixel outside the mask: the masked pair keeps its value
    assert IE.psnr_errors(nan_outside, nan_outside) == [0.0, 0.0]
    with pytest.raises(AssertionError):
        IE.psnr_errors([np.nan] * 4, nan_outside)                        # ... the NaN leaking into the masked pair
    with pytest.raises(AssertionError):
        IE.psnr_errors(want, nan_outside)                                # ... or the NaN lost
    inf = np.array([0.0, 0.0, np.inf, np.inf])                           # identical images
    assert IE.psnr_errors(inf, inf) == [0.0, 0.0]
    with pytest.raises(AssertionError):
        IE.psnr_errors([0.0, 1e-300, np.inf, 3000.0], inf)
    rel, ab = IE.psnr_errors(want * (1.0 + 1e-9), want)                  # and a finite error is reported, not folded away
    assert 0.9e-9 < rel < 1.1e-9 and ab > 0.9e-9 * abs(want[2:]).max()
    rel_bar, abs_bar = IE.psnr_bars(4)
    assert rel > rel_bar and ab > abs_bar
