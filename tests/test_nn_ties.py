"""CPU checks of the tie and cell-edge cases (tests/nn_cases.py): the ties they build are real in the oracle's own arithmetic and
visible downstream, so that the GPU tests of tests/test_gpu_nn_ties.py can pin every search path to the first-index-wins rule."""
import numpy as np
import pytest

import oracle as O
import nn_cases as N


@pytest.mark.parametrize("order", N.ORDERS)
@pytest.mark.parametrize("nonuniform", [False, True])
def test_twins_share_their_centroid_bit_for_bit(nonuniform, order):
    c = N.twin_case(nonuniform, order)
    F0 = c["base_faces"].shape[0]
    assert c["faces"].shape[0] == F0 + c["first"].size and np.all(c["first"] < c["second"])
    world = c["space"] == "world"
    assert 100 <= world.sum() and 100 <= (~world).sum()
    cw, cc = O.centroids(c["xyz"], c["faces"]), O.centroids(c["canon"], c["faces"])
    assert np.array_equal(cw[c["first"][world]], cw[c["second"][world]])
    assert np.array_equal(cc[c["first"][~world]], cc[c["second"][~world]])
    # the other space is rotated by one vertex: the affine map of the warp / the normal differs for every pair
    f1, f2 = c["faces"][c["first"]], c["faces"][c["second"]]
    other = np.where(world[:, None, None], c["canon"][f1], c["xyz"][f1]), np.where(world[:, None, None], c["canon"][f2], c["xyz"][f2])
    assert not np.any(np.all(other[0] == other[1], axis=(1, 2)))
    assert np.array_equal(other[0][:, [1, 2, 0]], other[1]) or np.array_equal(other[1][:, [1, 2, 0]], other[0])
    # gaps: the same lane group, other lanes of a wave, other segments of the far search
    g = c["second"] - c["first"]
    assert (g == 1).sum() >= 50 and ((g > 64) & (g < N.FAR_SEG)).sum() >= 50 and (g > N.FAR_SEG).sum() >= 100
    # the untouched faces keep their order
    keep = np.ones(c["faces"].shape[0], bool)
    keep[c["first"]] = keep[c["second"]] = False
    assert np.array_equal(c["faces"][keep], np.delete(c["base_faces"], c["base"], 0))
    assert np.array_equal(c["faces"][c["orig"]], c["base_faces"][c["base"]])


@pytest.mark.parametrize("nonuniform", [False, True])
def test_face_order_decides_the_oracle_and_the_warp(nonuniform):
    """the ties are real in the oracle's float32 arithmetic: with the original first the original wins, with the twin first the twin
    - the same index (the pair's first position), a different face - and the warp's outputs differ with it"""
    a, b = N.twin_case(nonuniform, "orig"), N.twin_case(nonuniform, "twin")
    assert np.array_equal(a["first"], b["first"]) and np.array_equal(a["second"], b["second"])
    for space, q, v in (("world", "q_world", "xyz"), ("canon", "q_canon", "canon")):
        ia = O.nearest_face(a[q], O.centroids(a[v], a["faces"]))
        ib = O.nearest_face(b[q], O.centroids(b[v], b["faces"]))
        pair = N.pair_of(a, space)
        tied = pair[ia] >= 0
        assert tied.mean() >= 0.35, (space, tied.mean())
        assert np.array_equal(ia[tied], a["first"][pair[ia[tied]]])         # first index wins ...
        # (near the OTHER space's pairs the two orders differ in rounding - a rotated vertex order sums differently - not in ties)
        plain = (N.pair_of(a, "canon" if space == "world" else "world")[ia] < 0) & (N.pair_of(b, "canon" if space == "world" else "world")[ib] < 0)
        assert plain.mean() > 0.9 and np.array_equal(ia[plain], ib[plain])
        flipped = np.any(a["faces"][ia] != b["faces"][ib], 1)              # ... and which face that is depends on the order
        assert np.array_equal(flipped[plain], tied[plain])
        # the tied queries reach the fine grid, the coarse shell and beyond (thirds of the query set)
        n3 = a[q].shape[0] // 3
        assert min(tied[:n3].mean(), tied[n3:2 * n3].mean(), tied[2 * n3:].mean()) >= 0.1
    wa = O.warp(a["q_world"], None, a["xyz"], a["canon"], a["faces"])
    wb = O.warp(b["q_world"], None, b["xyz"], b["canon"], b["faces"])
    tied = N.pair_of(a, "world")[wa["idx"]] >= 0
    plain = (N.pair_of(a, "canon")[wa["idx"]] < 0) & (N.pair_of(b, "canon")[wb["idx"]] < 0)
    assert np.array_equal(wa["idx"][plain], wb["idx"][plain])
    moved = np.any(wa["x_c"] != wb["x_c"], 1)
    assert moved[tied].mean() > 0.99 and not moved[plain & ~tied].any()
    # (both faces of a world pair are the same posed triangle: the projection is the same, the canonical point is not)
    assert np.array_equal(wa["uv"][plain], wb["uv"][plain]) and np.array_equal(wa["h"][plain], wb["h"][plain])
    # canonical ties: the world normal made from the canonical gradient differs
    rng = np.random.default_rng(3)
    g = rng.standard_normal(a["q_canon"].shape).astype(np.float32)
    ia, na = O.normal_world(a["q_canon"], g, a["canon"], a["xyz"], a["faces"])
    ib, nb = O.normal_world(b["q_canon"], g, b["canon"], b["xyz"], b["faces"])
    tied = N.pair_of(a, "canon")[ia] >= 0
    assert np.array_equal(ia[tied], ib[tied]) and np.any(na != nb, 1)[tied].mean() > 0.99


def test_dyadic_soup_ties_are_exact():
    """lattice midpoints, face centres and cube centres: 2-, 4- and 8-way exact ties between distinct centroids; the oracle returns
    the float64 (distance, index) lexicographic minimum, i.e. the smallest index of the tied set, and the warp depends on it"""
    s = N.dyadic_soup()
    cent = O.centroids(s["verts"], s["faces"])
    assert np.array_equal(cent, s["cent"])
    assert sorted(set(s["mult"].tolist())) == [1, 2, 4, 8] and (s["mult"] > 1).sum() >= 800
    j, m = N.lexmin_f64(s["pts"], cent)
    assert np.array_equal(m, s["mult"]) and np.array_equal(j, s["win"])
    assert np.array_equal(O.nearest_face(s["pts"], cent), j)
    # the winner is not tied to position: in most tied sets it is not the lattice site that comes first
    assert len(set((s["win"][s["mult"] == 8] % 7).tolist())) == 7
    # the reversed face order picks a different face of every tied set (the sets are exact ties)
    rev = s["faces"][::-1].copy()
    ir = O.nearest_face(s["pts"], O.centroids(s["verts"], rev))
    tied = s["mult"] > 1
    assert np.all(rev[ir][tied] != s["faces"][j][tied]) and np.array_equal(rev[ir][~tied], s["faces"][j][~tied])


def test_edge_points_sit_on_the_cell_boundaries():
    """the cell-edge builder on a header like the library's: the first float32 of each boundary reaches the next cell, one ulp below
    it does not; outer points sit on the grid's first / last plane (the hand-over to the next level)"""
    raw = np.zeros(64, np.uint8)
    f, i = raw.view(np.float32), raw.view(np.int32)
    f[0:3] = np.float32([-0.913, -1.271, -0.231])
    f[3] = np.float32(0.0317)
    f[4] = np.float32(1.0) / f[3]
    i[5:8] = [58, 60, 16]
    h = N.parse_header(raw)
    assert h["n"].tolist() == [58, 60, 16] and h["cell"] == f[3]
    rng = np.random.default_rng(2)
    base = (h["lo"] + rng.uniform(0.05, 0.95, (300, 3)) * h["n"] * h["cell"]).astype(np.float32)
    for outer in (False, True):
        e = N.edge_points(h, base, outer=outer).reshape(-1, 4, 3)
        for j in range(e.shape[0]):
            a = j % 3
            x, below = e[j, 0, a], e[j, 1, a]
            fx = lambda v: np.float32(np.float32(v - h["lo"][a]) * h["inv_cell"])
            k = int(fx(x))
            assert fx(x) >= k and fx(below) < k and np.nextafter(below, np.float32(1e9)) == x
            assert abs(float(e[j, 2, a]) - float(x) - 1e-4) < 1e-6 and abs(float(x) - float(e[j, 3, a]) - 1e-4) < 1e-6
            if outer:
                assert k in (0, int(h["n"][a]))
        c = N.cell_of(h, e.reshape(-1, 3))
        if outer:        # the last plane is outside, one ulp below it inside; the first plane inside, one ulp below outside
            assert (c[0::4] < 0).sum() == (c[1::4] >= 0).sum() == e.shape[0] - (c[0::4] >= 0).sum()
        else:
            assert np.all(c >= 0)
