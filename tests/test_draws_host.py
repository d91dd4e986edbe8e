"""dsn_train_draws' rule without a GPU: the numpy restatement (tests/draws_restate.py) against the generator's known answers, the
ranges and lattices of both conversions, the distribution of 2^20 values per kind at fixed seeds, the addressing, and the library's
argument checks."""
import ctypes as C

import numpy as np
import pytest

import draws_restate as DR

R_STAT, S_STAT = 16384, 64          # 2^20 values per kind
N_STAT = R_STAT * S_STAT
SEEDS = (20261019, (0x5eed << 32) | 7)          # fixed; the second one has a non-zero high word
STEP = 3


# ---- 1. the generator -----------------------------------------------------------------------------------------------------------------
def test_known_answers():
    for counter, key, want in DR.KNOWN_ANSWERS:
        got = DR.philox4x32(counter, key)
        assert got.dtype == np.uint32 and got.shape == (4,)
        assert tuple(int(v) for v in got) == want, ([hex(int(v)) for v in got], [hex(v) for v in want])
    # vectorised over counters and keys: the same words
    cs = np.array([k[0] for k in DR.KNOWN_ANSWERS], dtype=np.uint64)
    ks = np.array([k[1] for k in DR.KNOWN_ANSWERS], dtype=np.uint64)
    got = DR.philox4x32([cs[:, i] for i in range(4)], [ks[:, i] for i in range(2)])
    assert np.array_equal(got, np.array([k[2] for k in DR.KNOWN_ANSWERS], dtype=np.uint32))


# ---- 2. the conversions ---------------------------------------------------------------------------------------------------------------
def test_jitter_range_and_lattice():
    edge = DR.jitter_from_words(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint32))
    assert edge.dtype == np.float32
    assert edge[0] == 0.0 and edge[1] == 0.0 and edge[2] == np.float32(2.0 ** -24) and edge[3] == np.float32(1.0 - 2.0 ** -24)
    j, _ = DR.draws(4096, 64, SEEDS[0], STEP, want_noise=False)
    assert j.dtype == np.float32 and j.min() >= 0.0 and j.max() <= np.float32(1.0 - 2.0 ** -24)
    scaled = j.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(scaled, np.floor(scaled))          # on the 2^-24 lattice
    w = DR.words(4096, 64, SEEDS[0], STEP, DR.KIND_JITTER).reshape(4096, 64)
    assert np.array_equal(scaled.astype(np.uint32), w >> np.uint32(8))          # exact: no rounding anywhere


def test_noise_range():
    with np.errstate(all="raise"):          # no log(0), no invalid operation at the edges
        z0, z1, r = DR.box_muller(np.array([0xFFFFFFFF] * 3, dtype=np.uint32), np.array([0, 0x40000000, 0xFFFFFFFF], dtype=np.uint32))
        assert np.all(r == 0.0) and np.all(z0 == 0.0) and np.all(z1 == 0.0)
        z0, z1, r = DR.box_muller(np.uint32(0), np.uint32(0))
        assert z0 == np.float32(np.sqrt(64.0 * np.log(2.0))) and z1 == 0.0 and z0 == np.float32(DR.Z_MAX)
        # the smallest u1 under every angle of a sweep: |z| never passes sqrt(64 ln 2)
        b = np.linspace(0, 2 ** 32 - 1, 4097).astype(np.uint64).astype(np.uint32)
        z0, z1, _ = DR.box_muller(np.zeros_like(b), b)
        assert np.all(np.isfinite(z0)) and np.all(np.isfinite(z1)) and max(np.abs(z0).max(), np.abs(z1).max()) <= np.float32(DR.Z_MAX)
    edge = DR.noise_from_words(np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 0, 0, 0x80000000]], dtype=np.uint32), 0.5)
    assert edge.dtype == np.float32 and np.all(np.isfinite(edge))
    assert edge[0, 0] == np.float32(DR.Z_MAX) * np.float32(0.5) and edge[0, 2] == 0.0 and edge[1, 2] == -edge[0, 0]


# ---- 3. the distribution ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    out = {}
    for seed in SEEDS:
        j, n = DR.draws(R_STAT, S_STAT, seed, STEP)
        j1, n1 = DR.draws(R_STAT, S_STAT, seed, STEP + 1)
        out[seed] = (j, n, j1, n1)
    return out


def corr(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("seed", SEEDS)
def test_moments_and_ks(sample, seed):
    """mean and variance within 5 standard errors: the variance of a sample variance is (mu4 - sigma^4) / n, i.e. (1/80 - 1/144) / n
    for the uniform and 2 / n for the normal distribution"""
    from scipy import stats
    j, n, _, _ = sample[seed]
    assert j.size == n.size == N_STAT == 1 << 20 and np.all(np.isfinite(n)) and np.abs(n).max() <= np.float32(DR.Z_MAX)
    for name, x, mean, var, var_of_var, dist in (("jitter", j, 0.5, 1.0 / 12.0, 1.0 / 80.0 - 1.0 / 144.0, "uniform"),
                                                 ("noise", n, 0.0, 1.0, 2.0, "norm")):
        x = x.astype(np.float64).ravel()
        m, v = x.mean(), x.var()
        p = stats.kstest(x, dist).pvalue
        print(f"seed {seed:#x} {name}: mean {m:.6f} ({(m - mean) / np.sqrt(var / N_STAT):+.2f} s.e.), variance {v:.6f} "
              f"({(v - var) / np.sqrt(var_of_var / N_STAT):+.2f} s.e.), ks p {p:.3g}")
        assert abs(m - mean) <= 5.0 * np.sqrt(var / N_STAT), (name, m)
        assert abs(v - var) <= 5.0 * np.sqrt(var_of_var / N_STAT), (name, v)
        assert p > 1e-6, (name, p)


@pytest.mark.parametrize("seed", SEEDS)
def test_correlations(sample, seed):
    j, n, j1, n1 = sample[seed]
    for name, x, x1 in (("jitter", j, j1), ("noise", n, n1)):
        pairs = {"neighbouring samples": (x[:, :-1], x[:, 1:]), "neighbouring rays": (x[:-1], x[1:]), "steps t, t + 1": (x, x1)}
        for what, (a, b) in pairs.items():
            c = corr(a, b)
            print(f"seed {seed:#x} {name}, {what}: {c:+.2e} (bar {5.0 / np.sqrt(a.size):.2e})")
            assert abs(c) < 5.0 / np.sqrt(a.size), (name, what, c)
    c = corr(j, n)
    print(f"seed {seed:#x} jitter against noise: {c:+.2e}")
    assert abs(c) < 5.0 / np.sqrt(N_STAT), c


# ---- 4. the addressing -----------------------------------------------------------------------------------------------------------------
def test_columns_do_not_depend_on_S():
    j8, n8 = DR.draws(7, 8, SEEDS[1], 5)
    j5, n5 = DR.draws(7, 5, SEEDS[1], 5)
    assert j5.shape == n5.shape == (7, 5)
    assert np.array_equal(j5.view(np.uint32), j8[:, :5].view(np.uint32)) and np.array_equal(n5.view(np.uint32), n8[:, :5].view(np.uint32))
    j1, n1 = DR.draws(7, 1, SEEDS[1], 5)
    assert np.array_equal(j1, j8[:, :1]) and np.array_equal(n1, n8[:, :1])
    for R, S in ((0, 5), (3, 0), (0, 0)):          # nothing to draw
        j0, n0 = DR.draws(R, S, SEEDS[1], 5)
        assert j0.shape == n0.shape == (R, S) and j0.dtype == n0.dtype == np.float32


def test_rows_depend_on_their_ray_id_only():
    R, S = 40, 13
    j, n = DR.draws(R, S, SEEDS[0], 9)
    # split into calls with ray_base offsets
    for lo, hi in ((0, 11), (11, 40)):
        a, b = DR.draws(hi - lo, S, SEEDS[0], 9, ray_base=lo)
        assert np.array_equal(a, j[lo:hi]) and np.array_equal(b, n[lo:hi])
    # ids as a permutation, with repeats, and negative int32 ids taken modulo 2^32
    perm = np.random.RandomState(0).permutation(R).astype(np.int32)
    a, b = DR.draws(R, S, SEEDS[0], 9, ray_ids=perm)
    assert np.array_equal(a, j[perm]) and np.array_equal(b, n[perm])
    rep = np.array([3, 3, 17, 3], dtype=np.int32)
    a, b = DR.draws(4, S, SEEDS[0], 9, ray_ids=rep)
    assert np.array_equal(a, j[rep]) and np.array_equal(b, n[rep])
    wrap_j, wrap_n = DR.draws(6, S, SEEDS[0], 9, ray_base=2 ** 32 - 3)
    assert np.array_equal(wrap_j[3:], j[:3]) and np.array_equal(wrap_n[3:], n[:3])
    neg_j, _ = DR.draws(3, S, SEEDS[0], 9, ray_ids=np.array([-3, -2, -1], dtype=np.int32))
    assert np.array_equal(neg_j, wrap_j[:3])
    # distinct ids, steps and kinds give distinct rows
    assert len({row.tobytes() for row in j}) == R and not np.array_equal(j, DR.draws(R, S, SEEDS[0], 10)[0])
    assert not np.array_equal(DR.words(R, S, SEEDS[0], 9, DR.KIND_JITTER), DR.words(R, S, SEEDS[0], 9, DR.KIND_NOISE))


def test_both_seed_words_count():
    base = DR.draws(4, 8, 0x00000001_00000002, 0)
    high = DR.draws(4, 8, 0x00000003_00000002, 0)
    low = DR.draws(4, 8, 0x00000001_00000004, 0)
    for k in range(2):
        assert not np.array_equal(base[k], high[k]) and not np.array_equal(base[k], low[k])
    # the seed is taken modulo 2^64, the step modulo 2^32
    again = DR.draws(4, 8, 0x00000001_00000002 + (1 << 64), 1 << 32)
    assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1])


def test_noise_std_scales_in_float32():
    _, n1 = DR.draws(5, 7, SEEDS[0], 1)
    _, nh = DR.draws(5, 7, SEEDS[0], 1, noise_std=0.3)
    _, n0 = DR.draws(5, 7, SEEDS[0], 1, noise_std=0.0)
    assert np.array_equal(nh, n1 * np.float32(0.3)) and np.all(n0 == 0.0)
    assert np.array_equal(np.signbit(n0), np.signbit(n1))          # 0 x z keeps z's sign, as mul_ does


# ---- 5. the library's host side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    return dsnerf_amd._lib


def test_abi_version_and_export(L):
    assert L.lib().dsn_abi_version() == 8
    assert "dsn_train_draws" in L.EXPORTS and hasattr(L.lib(), "dsn_train_draws") and callable(L.train_draws)


def test_argument_checks(L):
    lib = L.lib()
    one = C.c_void_p(64)          # (never dereferenced: every call below returns before anything is enqueued)

    def call(R=4, S=8, ray_ids=None, jitter=one, noise=one):
        return lib.dsn_train_draws(1, 0, 0, ray_ids, R, S, 1.0, jitter, noise, None)

    def refused(msg, **kw):
        assert call(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_train_draws" in err and msg in err, (kw, err)

    refused(b"both null", jitter=None, noise=None)
    refused(b"negative", R=-1)
    refused(b"negative", S=-1)
    refused(b"negative", R=-4, S=-8)          # (a positive product)
    refused(b"INT_MAX", R=65536, S=32768)          # 2^31 = INT_MAX + 1
    refused(b"INT_MAX", R=2 ** 31 - 1, S=2)
    refused(b"4-byte", jitter=C.c_void_p(66))
    refused(b"4-byte", noise=C.c_void_p(65))
    refused(b"4-byte", ray_ids=C.c_void_p(2))
    # nothing to draw: success without a launch, whatever the pointers
    assert call(R=0) == 0 and call(S=0) == 0 and call(R=0, jitter=None, noise=None) == 0
    # the binding refuses before it reaches the library
    if not __import__("torch").cuda.is_available():
        with pytest.raises(RuntimeError):
            L.train_draws(4, 8, 1, 0)
