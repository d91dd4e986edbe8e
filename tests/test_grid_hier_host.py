"""The coarse-to-fine density grid's rule (include/dsnerf.h, dsn_grid_hier_*) without a GPU: the numpy restatement
(tests/grid_hier_restate.py) on analytic volumes - what the certificate `leaks` says with 0, 1 and 2 rings of dilation, what it cannot
see (a blob smaller than a coarse cell) - the lattice on short axes, NaN and infinities, the retry rule of
Renderer.extract_mesh(coarse=...) and the library's argument checks.

The volumes are this file's own (off-centre spheres and a torus on [-1, 1]^3): with no ring the spheres and the torus leak at factors 2
and 4 on every grid (27 - 1571 edges) and at factor 8 (17 - 113 edges) except in three cases where the few core cells of so coarse a
lattice already cover every stencil (NO_LEAK_WITHOUT_A_RING: asserted as 0)."""
import ctypes as C

import numpy as np
import pytest

import grid_hier_restate as H

LEVELS = {"step": 0.5}
# factor 8 on these grids: the core cells alone hold every sign-changing edge and its stencil (at most eight cells along an axis)
NO_LEAK_WITHOUT_A_RING = {("sphere", (33, 33, 33), 8), ("torus", (33, 33, 33), 8), ("torus", (64, 50, 47), 8)}
VOLUMES = dict(H.CASES, step=H.step_sphere)


@pytest.fixture(scope="module")
def lib():
    import dsnerf_amd
    return dsnerf_amd._lib.lib()


@pytest.fixture(scope="module")
def volumes():
    cache = {}

    def get(name, shape):
        if (name, shape) not in cache:
            v = VOLUMES[name](shape)
            v.setflags(write=False)
            cache[name, shape] = v
        return cache[name, shape]
    return get


@pytest.mark.parametrize("shape", H.GRIDS)
@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_analytic_volumes(volumes, name, shape):
    d = volumes(name, shape)
    level = LEVELS.get(name, 0.0)
    for c in (2, 4, 8):
        h0 = H.hier(d, level, c, 0)
        if name in ("sphere", "two_spheres", "torus"):
            if (name, shape, c) in NO_LEAK_WITHOUT_A_RING:
                assert h0["leaks"] == 0, (c, h0["leaks"])
            else:
                assert h0["leaks"] > 0, (c, h0["leaks"])
        frac = [h0["evaluated_points"]]
        for r in (1, 2):
            h = H.hier(d, level, c, r)
            assert h["leaks"] == 0 and H.hidden(d, h["volume"], level) == 0, (c, r, h["leaks"])
            assert H.reads_equal(d, h["volume"], level), (c, r)
            frac.append(h["evaluated_points"])
        assert frac[0] <= frac[1] <= frac[2] <= d.size          # monotone in r
        assert frac[0] < d.size


def test_blob_smaller_than_a_cell_is_hidden_not_counted():
    shape = (64, 50, 47)
    d = H.sphere_with_blob(shape)
    for c in (2, 4, 8):
        h = H.hier(d, 0.0, c, 1)
        assert h["leaks"] == 0 and H.hidden(d, h["volume"], 0.0) == 4, c
        assert not H.reads_equal(d, h["volume"], 0.0)


def test_all_active_lattice_is_the_dense_volume(volumes):
    for shape in H.GRIDS:
        d = volumes("noisy_sphere", shape)
        for c in H.FACTORS:
            h = H.hier(d, 0.0, c, 0, evaluate_all=True)
            assert np.array_equal(h["volume"].view(np.uint32), d.view(np.uint32)) and h["leaks"] == 0
            assert h["evaluated_points"] == d.size and np.array_equal(h["index"], np.arange(d.size))
        # enough rings reach every cell
        h = H.hier(d, 0.0, 8, 8)
        assert h["evaluated_points"] == d.size and np.array_equal(h["volume"].view(np.uint32), d.view(np.uint32))


def test_level_not_crossed(volumes):
    d = volumes("sphere", (33, 33, 33))
    for level in (5.0, -5.0):
        for r in (0, 1, 2):
            h = H.hier(d, level, 4, r)
            assert h["core_cells"] == 0 and h["active_cells"] == 0 and h["index"].size == 0 and h["leaks"] == 0
            assert H.hidden(d, h["volume"], level) == 0


def fill_rule_holds(h, level):
    """rule 5's claim: two filled neighbours never differ in side, so every sign-changing edge has an evaluated end"""
    ins, filled = H.inside(h["volume"], level), ~h["evaluated"]
    for d in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[d], hi[d] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        if ((ins[lo] != ins[hi]) & filled[lo] & filled[hi]).any():
            return False
    return True


@pytest.mark.parametrize("c", H.FACTORS)
def test_short_axes(c, lib):
    import dsnerf_amd
    rng = np.random.default_rng(c)
    for n in sorted({2, 3, c, c + 1, c + 2}):
        idx = H.coarse_index(n, c)
        assert idx[0] == 0 and idx[-1] == n - 1 and (np.diff(idx) > 0).all() and (np.diff(idx) <= c).all()
        assert (np.diff(idx)[:-1] == c).all() and len(idx) == -(-(n - 1) // c) + 1
        assert np.array_equal(dsnerf_amd._lib.grid_hier_axes((n, 2, 3), c)[0], idx)
        own = H.owner(n, idx)
        assert own.min() == 0 and own.max() == len(idx) - 2 and (idx[own] <= np.arange(n)).all() and (np.arange(n) <= idx[own + 1]).all()
        for shape in ((n, 5, 2 * c + 3), (3, n, n), (n, n, n)):
            d = rng.standard_normal(shape).astype(np.float32)
            for r in (0, 1):
                h = H.hier(d, 0.0, c, r)
                assert fill_rule_holds(h, 0.0)
                assert h["coarse_shape"] == tuple(-(-(s - 1) // c) + 1 for s in shape)
                ev = h["evaluated"]
                assert np.array_equal(h["volume"][ev].view(np.uint32), d[ev].view(np.uint32))
                assert h["index"].dtype == np.int32 and (np.diff(h["index"]) > 0).all()
                assert lib.dsn_grid_hier_workspace_bytes(*shape, c) >= 2 * h["core"].size + 8


def test_nan_and_infinities_among_the_values():
    for shape in ((33, 33, 33), (37, 41, 35)):
        d = H.nan_inf_volume(shape)
        assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any()
        for level in (0.0, 0.5):
            for c in (2, 4):
                for r in (0, 1):
                    h = H.hier(d, level, c, r)
                    assert fill_rule_holds(h, level)
                    # NaN and -inf are outside, +inf inside: the core cells follow the sides, not the values
                    ins = H.inside(h["coarse"], level).astype(int)
                    mx, my, mz = ins.shape
                    s = sum(ins[a:mx - 1 + a, b:my - 1 + b, e:mz - 1 + e] for a in (0, 1) for b in (0, 1) for e in (0, 1))
                    assert np.array_equal(h["core"], (s > 0) & (s < 8))
    # a volume of NaN only: nothing is inside, nothing is evaluated
    h = H.hier(np.full((9, 9, 9), np.nan, np.float32), 0.0, 4, 1)
    assert h["index"].size == 0 and h["leaks"] == 0 and np.isnan(h["volume"]).all()


def test_retry_rule_against_the_restatement(volumes):
    from dsnerf_amd.can_render import hier_retry
    d = volumes("torus", (37, 41, 35))
    seen = []

    def attempt(r):
        seen.append(r)
        h = H.hier(d, 0.0, 4, r)
        return h["volume"], {"leaks": h["leaks"], "dilate": r}
    assert H.hier(d, 0.0, 4, 0)["leaks"] > 0
    vol, info = hier_retry(attempt, dilate=0, max_dilate=3)
    assert seen == [0, 1] and info["dilate"] == 1 and info["attempts"] == 2 and not info["fell_back"] and info["leaks"] == 0
    assert np.array_equal(vol, H.hier(d, 0.0, 4, 1)["volume"])
    del seen[:]
    vol, info = hier_retry(attempt, dilate=0, max_dilate=0)          # no ring allowed: the dense grid
    assert seen == [0] and vol is None and info["fell_back"] and info["attempts"] == 1 and info["leaks"] > 0
    del seen[:]
    vol, info = hier_retry(attempt, dilate=1, max_dilate=3)
    assert seen == [1] and vol is not None and info["attempts"] == 1 and not info["fell_back"]
    # a certificate that never holds: every ring up to max_dilate, then the fallback
    calls = []
    vol, info = hier_retry(lambda r: (calls.append(r) or "v", {"leaks": 7}), dilate=1, max_dilate=3)
    assert calls == [1, 2, 3] and vol is None and info == {"leaks": 7, "attempts": 3, "fell_back": True}


def test_abi_argument_errors(lib):
    z, i64, f = None, C.c_int64, C.c_float
    one = C.c_void_p(1)
    calls = {
        "dsn_grid_hier_mark": lambda: lib.dsn_grid_hier_mark(z, 2, 2, 2, 2, 2, 2, 2, 1, f(0.0), z, 0, z, z),
        "dsn_grid_hier_list": lambda: lib.dsn_grid_hier_list(2, 2, 2, 2, z, 0, i64(0), z, z),
        "dsn_grid_hier_assemble": lambda: lib.dsn_grid_hier_assemble(z, 2, 2, 2, 2, 2, 2, 2, f(0.0), z, 0, z, z, i64(0), z, z, z),
        "dsn_density_points": lambda: lib.dsn_density_points(z, 1, 1, z, z, 2, z, 2, z, 2, z, i64(0), 0, z, i64(8), z, 0, z),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert name.encode() in lib.dsn_last_error() and b"null" in lib.dsn_last_error(), (name, lib.dsn_last_error())
    # every check comes before any device work
    big = 1 << 40
    mark = lambda m=(9, 9, 9), n=(33, 33, 33), c=4, r=1, level=0.0: lib.dsn_grid_hier_mark(one, *m, *n, c, r, f(level), one, big, one, z)
    for kw, msg in ((dict(c=3), b"factor"), (dict(c=32), b"factor"), (dict(c=0), b"factor"), (dict(r=-1), b"negative dilate"),
                    (dict(level=float("nan")), b"NaN level"), (dict(n=(33, 1, 33)), b"grid size"),
                    (dict(n=(2048, 1024, 1024), m=(513, 257, 257)), b"2^31"), (dict(m=(9, 9, 8)), b"coarse shape"),
                    (dict(m=(33, 33, 33)), b"coarse shape"), (dict(n=(34, 33, 33)), b"coarse shape")):
        assert mark(**kw) != 0 and msg in lib.dsn_last_error(), (kw, lib.dsn_last_error())
    assert lib.dsn_grid_hier_mark(one, 9, 9, 9, 33, 33, 33, 4, 1, f(0.0), one, 16, one, z) != 0 and b"workspace" in lib.dsn_last_error()
    lst = lambda n=(33, 33, 33), c=4, m=10, out=one, ws=big: lib.dsn_grid_hier_list(*n, c, one, ws, i64(m), out, z)
    for kw, msg in ((dict(c=5), b"factor"), (dict(n=(1, 33, 33)), b"grid size"), (dict(m=-1), b"n_points"), (dict(m=33 ** 3 + 1), b"n_points"),
                    (dict(out=z), b"null output"), (dict(ws=8), b"workspace")):
        assert lst(**kw) != 0 and msg in lib.dsn_last_error(), (kw, lib.dsn_last_error())
    asm = lambda m=(9, 9, 9), n=(33, 33, 33), c=4, level=0.0, M=10, idx=one, ws=big: lib.dsn_grid_hier_assemble(
        one, *m, *n, c, f(level), one, ws, idx, one, i64(M), one, one, z)
    for kw, msg in ((dict(c=6), b"factor"), (dict(level=float("nan")), b"NaN level"), (dict(n=(33, 33, 1)), b"grid size"),
                    (dict(m=(8, 9, 9)), b"coarse shape"), (dict(M=-2), b"n_points"), (dict(idx=z), b"null point list"), (dict(ws=8), b"workspace")):
        assert asm(**kw) != 0 and msg in lib.dsn_last_error(), (kw, lib.dsn_last_error())
    # sizes
    assert lib.dsn_grid_hier_workspace_bytes(33, 33, 33, 3) == 0 and lib.dsn_grid_hier_workspace_bytes(33, 1, 33, 4) == 0
    assert lib.dsn_grid_hier_workspace_bytes(2048, 1024, 1024, 4) == 0
    assert 0 < lib.dsn_grid_hier_workspace_bytes(512, 512, 512, 4) < 2 * 128 ** 3 + 8 * (512 ** 3 // 4096 + 2) + 3 * 256 + 1
    assert lib.dsn_density_points_workspace_bytes(i64(0)) == 0 and lib.dsn_density_points_workspace_bytes(i64(1 << 20)) >= 28 * (1 << 20)
    ws = lib.dsn_density_points_workspace_bytes(i64(64))
    pts = lambda n=(4, 4, 4), M=10, idx=one, flags=0, slab=64, nbytes=ws: lib.dsn_density_points(
        one, 1, 1, one, one, n[0], one, n[1], one, n[2], idx, i64(M), flags, one, i64(slab), one, nbytes, z)
    for kw, msg in ((dict(n=(0, 4, 4)), b"empty"), (dict(n=(2048, 1024, 1024)), b"2^31"), (dict(M=-1), b"negative"), (dict(idx=z), b"null point list"),
                    (dict(slab=0), b"slab_points"), (dict(nbytes=16), b"workspace"), (dict(flags=1), b"flags")):
        assert pts(**kw) != 0 and msg in lib.dsn_last_error(), (kw, lib.dsn_last_error())
