"""The builders and bars of tests/train_rows_cases.py with the oracle alone (no GPU): every case holds the row counts it states by the
oracle's own flags, the float32 oracle passes the bar the float64 oracle sets (so the reference alone passes), the bar has room above
float32 rounding, and the row the bar is measured on - the last listed one - weighs as much as the others."""
import numpy as np
import pytest
import torch

import train_rows_cases as C

CASES = C.all_cases()


def test_both_parameter_sets_share_the_rays_and_the_pools_are_pure():
    """the 64 pure-pool rays are all-transparent and the 8 hit rays all non-transparent - for both parameter sets, which share body,
    pose and rays (transparency is geometry: it does not depend on the parameters)"""
    assert C.same_rays()
    tr = C.geometry()["transparent"]
    assert tr.shape == (128, C.S)
    pure, hit = C.pure_rays(), C.hit_rays()
    assert len(pure) == C.PURE_RAYS and tr[pure].all()
    assert len(hit) == C.HIT_RAYS and not tr[hit].any()
    assert len(np.intersect1d(pure, hit)) == 0
    for name in C.PARAM_SETS:
        c = C.mixed_case(name, 192, hit_scale=1.0)
        assert c.R == 40 and not c.transparent[:128].any() and c.transparent[128:].all()
    assert len(C.module_points()["x_c"]) == C.A2_N


@pytest.mark.parametrize("kind", C.SUPPORTS)
@pytest.mark.parametrize("B", C.COUNTS)
def test_supports_take_the_staging_form_they_are_built_for(kind, B):
    rows = C.support(kind, B)
    assert len(rows) == B and np.all(np.diff(rows) > 0)
    one = C.staging_forms(rows)          # per group of four listed rows: one DMA address (consecutive rows) or four
    if len(one) == 0:
        return
    if kind == "prefix":
        assert one.all()
    elif kind == "stride":
        if 2 * B <= C.A2_N:
            assert not one.any()
        else:                            # (255 ... 257 of 320 rows: four addresses on most steps, see support())
            assert np.mean(~one) >= 0.75
    else:
        if B >= 8:
            assert one.any() and (~one).any()
        changes = np.count_nonzero(np.diff(one.astype(int)))
        if B <= 196:                     # (what the pattern holds in 320 rows)
            assert changes >= len(one) - 2                                          # the form changes from step to step
        else:                            # (255 ... 257: the pattern, then rows from the top - the first hundred listed rows alternate)
            assert changes >= 24


def test_fill_order_and_counts_of_the_ray_pools():
    order = C.fill_order(64)
    assert list(order[:8]) == [0, 1, 2, 3, 16, 17, 18, 19] and order[256] == 4 and len(np.unique(order)) == 1024
    c = C.pure_case(C.PARAM_SETS[0], 80)
    n = c.noise.reshape(-1)
    assert set(np.unique(n)) == {np.float32(C.DEAD), np.float32(C.LIVE)} and int((n > 0).sum()) == 80
    live = np.nonzero(C.live_rows(c))[0]
    assert live[-1] == 19 * 16 + 3 and c.noise.reshape(-1)[live[-1]] == np.float32(C.LIVE)      # the last listed row is a filled one


def test_forward_batch_without_a_live_row():
    for name in C.PARAM_SETS:
        b = C.forward_f0_batch(name)
        assert b.R == C.PURE_RAYS and b.z.shape == (64, C.S) and b.transparent.all() and (b.dead_noise <= 0).all()


def test_module_fill_covers_every_row_of_a_ray_batch():
    f = C.module_fill(C.PARAM_SETS[0], 1024)
    assert f.backward == 1024 and ((f.gs != 0) | (f.gc != 0).any(1)).all() and f.x_c.shape == (1024, 3)


def test_renderer_draw_holds_the_chosen_count():
    for name in C.PARAM_SETS:
        c = C.renderer_case(name, C.RENDERER_F)
        assert c.R == C.RENDERER_RAYS and c.forward == C.RENDERER_F and c.transparent.all()
        z = C.renderer_case(name, 0)
        assert z.noise is None and z.forward == 0


@pytest.mark.parametrize("cid,family,build", CASES, ids=[c[0] for c in CASES])
def test_reference_alone_passes_its_own_bar(cid, family, build):
    c = build()
    full = C.reference(c)                                   # float64
    # the counts, by the oracle's own flags
    if c.mode == "module":
        on = (c.gs != 0) | (c.gc != 0).any(1)
        assert int(on.sum()) == c.backward == len(c.rows) and np.array_equal(np.nonzero(on)[0], c.rows)
    else:
        assert c.forward == int(C.live_rows(c).sum())
        if "pure" in cid:
            F = int(cid.rsplit("F", 1)[1])
            assert c.forward == F and c.backward == F, (c.forward, c.backward)
        if "mixed" in cid:
            F = int(cid.rsplit("F", 1)[1])
            assert c.forward == F and F - 128 <= c.backward <= F, (c.forward, c.backward)
        if "zerocot" in cid:
            assert c.forward == 256 and 0 < c.backward <= c.live_with_cotangent == 64 + 64      # (the even rays: 4 hit rays x 16, 16 transparent rays x 4)
        if "C-F0" in cid:
            assert c.forward == 0
        if "C-B0" in cid:
            assert c.forward == 64 and c.backward == 0
        if "tiny" in cid:
            assert c.forward == c.N and not c.transparent.any()
            assert c.backward > 0, cid                      # a hit ray that HAS a gradient: not another B = 0 case
            if c.S <= 2:
                assert c.backward == c.N, (cid, c.backward)
        if c.last is not None and c.transparent[c.true_last]:
            assert c.last == c.true_last, (cid, c.last, c.true_last)      # on the filled samples the bar's row IS the last listed row
    zero = [k for k, v in full.items() if not np.any(v)]
    if c.backward == 0:
        assert len(zero) == 33, cid                         # F = 0 / B = 0: exactly zero float64 gradients
        return
    bar, med = C.bar(c, full)
    f32 = C.reference(c, torch.float32)
    err, nonzero = C.errors(f32, full)
    worst = max(err.values())
    print(f"{c.label}: median delta {med:.2e}, bar {bar:.2e}, float32 oracle {worst:.2e}")
    assert not nonzero, nonzero
    assert worst <= min(bar, C.CEILING), (worst, bar)       # the reference alone passes
    assert med >= 20.0 * worst, (med, worst)                # and the bar has room above float32 rounding
    # the last listed row carries weight: against the rows of the list at large (a sample of them)
    rows = C.listed_rows(c)
    pick = np.unique(rows[np.linspace(0, len(rows) - 1, 5).astype(np.int64)])
    others = [C.row_weight(c, full, int(r)) for r in pick]
    assert med > np.median(others) / 10.0, (med, others)
    if c.mode == "rays" and c.transparent.any():
        assert zero == ["nerf.density_net.0.bias"] if c.transparent.all() else zero == [], zero
