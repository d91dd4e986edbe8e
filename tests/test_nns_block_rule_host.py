"""Host: the block-deferred winner rule of the nearest-centroid scans (DsnBlk / dsn_blk_resolve, csrc/dsn_nn.h) as a numpy float32
model, for blocks of 8 and 16, against the serial strict-'<' scan it replaces.

The serial scan keeps (best, index) current after every candidate.  The block rule keeps only the running minimum per candidate and,
per block of B consecutive list entries, the position of the block that lowered it strictly; one strict scan over that block from
+inf then gives the index.  blk is the first block whose minimum is strictly below everything in front of it - the first block that
attains the list's minimum - and the scan inside it finds the first entry that attains it: the serial scan's entry, ties included.
The model follows the kernels step by step: v_min3_f32 ignores a NaN operand (np.fmin), '<' with a NaN is false, a short last block
is padded with +inf, lists drained in rounds (k_nns_search's survivor array) resolve the lanes whose block changed in that round,
and a sample without a candidate below +inf keeps index 0."""
import numpy as np
import pytest

INF = np.float32(np.inf)
NAN = np.float32(np.nan)
BLOCKS = (8, 16)


def serial(d):
    """the per-candidate rule: strict '<' in list order, index 0 when nothing is below +inf"""
    best, bi = INF, 0
    for k, x in enumerate(d):
        if x < best:
            best, bi = x, k
    return bi, best


def block_rule(d, B, round_len=None):
    """pass 1 per block (running minimum through fmin, strict compare against the minimum at the previous close), pass 2 per round
    (round_len entries, a multiple of B; None: one round)"""
    d = np.asarray(d, np.float32)
    n = d.size
    round_len = round_len or max(B, -(-n // B) * B)
    assert round_len % B == 0
    run = best = INF
    bi = 0
    for r0 in range(0, n, round_len):
        seg = d[r0:min(n, r0 + round_len)]
        seg = np.concatenate([seg, np.full((-seg.size) % B, INF, np.float32)])      # the padded last block of the round
        blk = -1
        for pos in range(0, seg.size, B):
            run = np.fmin.reduce(np.concatenate([seg[pos:pos + B], [run]]).astype(np.float32))      # v_min3 tree: NaN operands ignored
            if run < best:
                blk = pos
            best = run
        if blk >= 0:                                                                 # resolve before the round's entries go away
            b, idx = INF, bi
            for j in range(B):
                if seg[blk + j] < b:
                    b, idx = seg[blk + j], r0 + blk + j
            bi = idx
    return bi, best


def _same_best(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def check(d):
    d = np.asarray(d, np.float32)
    want, wbest = serial(d)
    for B in BLOCKS:
        for round_len in (None, B, 2 * B, 320 if 320 % B == 0 else None):
            got, gbest = block_rule(d, B, round_len)
            assert got == want, (B, round_len, got, want, d.size)
            assert _same_best(np.float32(gbest), np.float32(wbest)), (B, round_len, gbest, wbest)


def dist(p, cent):
    """squared distances in float32, term by term as the kernels add them (the rule only sees the values)"""
    dx, dy, dz = (np.float32(p[i]) - cent[:, i].astype(np.float32) for i in range(3))
    return ((dx * dx + dy * dy).astype(np.float32) + dz * dz).astype(np.float32)


def test_random_lists_of_1_to_700_entries():
    rng = np.random.default_rng(0)
    for n in list(range(1, 40)) + [int(x) for x in rng.integers(40, 701, 160)] + [700]:
        cent = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        check(dist(rng.uniform(-1, 1, 3), cent))
    for n in rng.integers(1, 701, 60):        # few distinct values: ties everywhere
        check(rng.integers(0, 4, int(n)).astype(np.float32))


@pytest.mark.parametrize("B", BLOCKS)
def test_duplicated_centroids_inside_a_block_across_an_edge_and_at_the_ends(B):
    rng = np.random.default_rng(B)
    for n in (3 * B, 3 * B + 5, 700):
        cent = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        p = rng.uniform(-1, 1, 3).astype(np.float32)
        near = (p + np.float32(1e-3)).astype(np.float32)        # nearer than every random centroid
        places = [(B + 1, B + 4), (B + 2, B + 3),               # inside one block
                  (B - 1, B), (2 * B - 1, 2 * B), (B - 1, 2 * B + 3),      # across a block edge, neighbours and apart
                  (0, 1), (0, n - 1), (n - 2, n - 1), (0, B), (B, n - 1),  # first / last position
                  (1, B, 2 * B + 1), (B - 1, B, B + 1)]         # three-way
        for pl in places:
            c = cent.copy()
            for k in pl:
                c[k] = near
            d = dist(p, c)
            assert len({float(d[k]) for k in pl}) == 1 and float(d[pl[0]]) < float(np.delete(d, pl).min())
            assert serial(d)[0] == min(pl)
            check(d)


@pytest.mark.parametrize("B", BLOCKS)
def test_list_lengths_around_multiples_of_the_block(B):
    rng = np.random.default_rng(100 + B)
    for k in (1, 2, 3, 5, 20, 40):
        for n in (B * k - 1, B * k, B * k + 1):
            for _ in range(4):
                d = rng.uniform(0, 4, n).astype(np.float32)
                check(d)
                for at in (0, n - 1, max(0, n - 2), (n - 1) // B * B, max(0, (n - 1) // B * B - 1)):      # the winner in the tail / at its edge
                    e = d.copy()
                    e[at] = np.float32(0.0)
                    check(e)
                    e[(at + 1) % n] = e[at]
                    check(e)


def test_inf_and_nan_distances():
    rng = np.random.default_rng(7)
    for n in (1, 7, 8, 9, 15, 16, 17, 64, 333, 700):
        for _ in range(6):
            d = rng.uniform(0, 4, n).astype(np.float32)
            m = rng.random(n)
            d[m < 0.2] = NAN
            d[(m >= 0.2) & (m < 0.4)] = INF
            check(d)
        d = np.full(n, INF, np.float32)
        assert serial(d)[0] == 0
        check(d)                                   # nothing below +inf: index 0
        d[n // 2] = np.float32(3.0)
        check(d)
        d = np.full(n, NAN, np.float32)
        d[n - 1] = np.float32(2.0)                 # one candidate behind NaNs, in the last (short) block
        check(d)
        d[0] = np.float32(2.0)                     # ... tied with the first
        check(d)


def test_every_candidate_nan_keeps_index_zero():
    for n in (1, 5, 8, 16, 17, 320, 321, 700):
        d = np.full(n, NAN, np.float32)
        assert serial(d)[0] == 0
        for B in BLOCKS:
            for round_len in (None, B, 320 if 320 % B == 0 else None):
                assert block_rule(d, B, round_len)[0] == 0
        check(d)
