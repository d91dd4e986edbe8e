"""tests/stop_slices_restate.py (the interval restatement of DSN_EARLY_STOP's transmittance that test_gpu_stop_slices.py judges the
kernels by) on its own, on the reference's golden rays: the intervals are ordered and monotone, dead stays dead, every decision on the
goldens is determined - with the derived m and nearly all with eight times that - and the slicings reach every variant of k_advance_T.
No GPU.

Colour scales as the callers would set them (EARLY_STOP_COLOUR_HEADROOM x the largest colour): 2400 for w3 (colours ~ 1200), 2 for the
others.  Cases with S != 64 run on the golden rays resampled to S samples (stop_slices_restate.resample).
Measured at S = 64 (terminated rays / certainly-dead decisions / undetermined, uniform 8): full_eval_w4 56 / 312 / 0, full_eval_w3 22 / 127 / 0,
full_eval_w2 18 / 39 / 0, full_eval 0 / 0 / 0; the largest m that matters (arg < 40) is 3.4e-6 / 7e-6 / 6e-7 / 2.7e-7."""
import numpy as np
import pytest

import stop_slices_restate as SR
from helpers import load

SCALE = {"full_eval_w4": 2.0, "full_eval_w3": 2400.0, "full_eval_w2": 2.0, "full_eval": 2.0}
TERMINATING = ["full_eval_w4", "full_eval_w3", "full_eval_w2"]
IDS = [SR.slicing_id(s) for s in SR.SLICINGS]
_CACHE = {}


def frame(name, sl, widen=1.0):
    key = (name, SR.slicing_id(sl), widen)
    if key not in _CACHE:
        S, kind, v = sl
        g = load(name)
        sg, tr, z = SR.resample(g["sigma"], g["transparent"], g["z_vals"], S)
        eps = SR.eps_scaled(S, SCALE[name])
        _CACHE[key] = SR.restate(sg, tr, z, g["ray_d"], SR.bounds_of(S, kind, v), eps, widen)
    return _CACHE[key]


def test_threshold_is_the_librarys():
    """dsn_early_stop_eps_scaled = min(2^-20, 1e-4 / (2 (S + 1) max(1, c))) in float32, and the slice-length rules restated beside it"""
    F = np.float32
    for S, c in ((64, 1.0), (64, 2.0), (64, 2400.0), (24, 2.0), (100, 2400.0), (128, 0.5)):
        want = min(F(2.0 ** -20), F(1e-4) / (F(2) * F(S + 1) * F(max(c, 1.0))))
        assert SR.eps_scaled(S, c) == want, (S, c)
    assert SR.uniform_len(1, 24) == 1 and SR.uniform_len(1, 64) == 2 and SR.uniform_len(3, 100) == 4 and SR.uniform_len(99, 128) == 64
    assert SR.stats_len(8, 64) == 4 and SR.stats_len(1, 24) == 1 and SR.stats_len(3, 64) == 3 and SR.stats_len(5, 128) == 5
    assert SR.bounds_of(100, "uniform", 8)[-3:] == [88, 96, 100] and SR.bounds_of(64, "schedule", [33, 31]) == [0, 33, 64]


def test_slicings_reach_every_advance_variant():
    """every G of dsn_launch_advance_T, slice lengths 1, 2, 3, 5, 13, 17, 33 and 64, and ragged last slices"""
    reached, lengths, ragged = set(), set(), 0
    for S, kind, v in SR.SLICINGS:
        b = SR.bounds_of(S, kind, v)
        reached |= SR.variants_of(b)
        lens = [b[k + 1] - b[k] for k in range(len(b) - 1)]
        lengths |= set(lens)
        ragged += kind == "uniform" and lens[-1] != lens[0]
    assert reached == {1, 2, 4, 8, 16, 32, 64}, reached
    assert {1, 2, 3, 5, 13, 17, 33, 64} <= lengths, lengths
    assert ragged >= 3
    assert [SR.advance_variant(n) for n in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    for sl in SR.LIST_MODE_SLICINGS:
        assert sl in SR.SLICINGS


@pytest.mark.parametrize("sl", SR.SLICINGS, ids=IDS)
@pytest.mark.parametrize("name", TERMINATING + ["full_eval"])
def test_intervals_and_decisions_on_the_goldens(name, sl):
    r = frame(name, sl)
    T_lo, T_nom, T_hi = r["T_lo"], r["T_nom"], r["T_hi"]
    assert (T_lo <= T_nom).all() and (T_nom <= T_hi).all()
    for T in (T_lo, T_nom, T_hi):
        assert (T[:, 1:] <= T[:, :-1]).all() and (T[:, 0] == 1).all() and (T >= 0).all()
    dead, alive, undet = r["dead"], r["alive"], r["undet"]
    assert not (dead & alive).any()
    assert (dead[:, 1:] >= dead[:, :-1]).all()                   # a slice found dead stays dead
    assert (alive[:, 1:] <= alive[:, :-1]).all()
    c = SR.counts(r)
    print(name, SR.slicing_id(sl), c, "eps %.3g m_max %.3g" % (r["eps"], r["m_max"]))
    assert c["undetermined"] == 0, c
    if name == "full_eval":
        assert c["terminated_rays"] == 0 and c["dead_decisions"] == 0, c
    elif len(r["bounds"]) == 2:
        assert c["dead_decisions"] == 0                           # a single slice: nothing is decided
    elif name != "full_eval_w2" or 4 * r["bounds"][1] <= sl[0]:
        # (w2, trained briefly: a thinner body whose rays end between a quarter and a half of the way - a slicing whose first border
        #  lies beyond the first quarter of the ray comes too late for them; w4 and w3 terminate under every slicing)
        assert c["terminated_rays"] >= 10, c
    # eightfold m: the inputs are not balanced on the threshold
    wide = SR.counts(frame(name, sl, widen=8.0))
    assert wide["undetermined"] <= 0.01 * wide["dead_decisions"], wide
    assert wide["dead_decisions"] <= c["dead_decisions"]


@pytest.mark.parametrize("name", TERMINATING)
def test_running_order_and_statistics(name):
    """k_stop_stats' running product against the slice-wise one (they may differ in the last bits, never by a decision on these rays),
    would_skip equal to the restated `skipped`, and the histogram: its column sums are the non-transparent samples per slice, and
    pricing the uniform slicing from it gives would_skip back"""
    g = load(name)
    S, L = 64, 8
    eps = SR.eps_scaled(S, SCALE[name])
    b = SR.bounds_of(S, "uniform", L)
    a = SR.restate(g["sigma"], g["transparent"], g["z_vals"], g["ray_d"], b, eps)
    o = SR.restate(g["sigma"], g["transparent"], g["z_vals"], g["ray_d"], b, eps, order="running")
    assert np.array_equal(a["dead"], o["dead"]) and not o["undet"].any()
    rel = np.abs(a["T_nom"].astype(np.float64) - o["T_nom"]) / np.maximum(o["T_nom"].astype(np.float64), 1e-300)
    assert float(rel[o["T_nom"] > 1e-30].max()) < 64 * 2.0 ** -23          # (normal numbers: 64 roundings at the most)
    would, hist, open_rays = SR.stop_stats(g["sigma"], g["transparent"], g["z_vals"], g["ray_d"], S, L, SR.stats_len(L, S), eps)
    assert would == (SR.counts(a)["skipped_certain"], 0) and not open_rays
    live = ~g["transparent"].reshape(-1, S)
    Lh = SR.stats_len(L, S)
    assert np.array_equal(hist.sum(0), live.reshape(-1, S // Lh, Lh).sum((0, 2)))
    K = hist.shape[1]
    priced = sum(int(hist[:2 * u + 1, 2 * u:2 * u + 2].sum()) for u in range(K // 2))     # first dead slice <= 2 u: dead at the start of uniform slice u
    assert priced == would[0], (priced, would)


def test_unshaded_and_gaps():
    F = np.float32
    sg = np.array([1.0, 1.0, 0.0, -1.0, np.nan, 2.0, 3.0], F)
    w = np.array([1e-9, 1e-3, 0.0, 0.0, 0.0, np.nan, 1e-7], F)
    assert SR.unshaded(sg, w, F(1e-7)).tolist() == [True, False, False, False, False, False, False]
    tr = np.ones((3, 12), bool)
    tr[0, [0, 9]] = False            # entries in slices 0 and 2 of [0, 4, 8, 12]: a gap
    tr[1, [0, 5]] = False            # slices 0 and 1: none
    tr[2, [9]] = False               # leading transparent slices only: none
    assert SR.gap_rays(tr, [0, 4, 8, 12], 3, 12) == 1
