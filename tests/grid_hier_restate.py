"""numpy restatement of the coarse-to-fine density grid of include/dsnerf.h (dsn_grid_hier_mark / _list / _assemble), rules 1 - 7,
written from the rule and not from the kernels: the evaluated points are painted cell by cell, the leaks are counted over all edges.

hier(dense, level, c, r) takes the DENSE volume as the source of every evaluated value and returns what the stages must return, bit
for bit; hidden(dense, assembled, level) counts the points whose inside differs; reads_equal() says whether every value marching cubes
and its normal stencil read on the dense volume is the assembled volume's."""
import numpy as np

FACTORS = (2, 4, 8, 16)


def coarse_index(n, c):
    """rule 1: 0, c, 2c, ... < n, plus n - 1 if it is not among them"""
    idx = list(range(0, n, c))
    if idx[-1] != n - 1:
        idx.append(n - 1)
    return np.asarray(idx, dtype=np.int64)


def inside(v, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(v, np.float32) > np.float32(level)          # (strict; NaN is outside)


def core_cells(coarse, level):
    """rule 2: cells whose eight corners are not all on the same side"""
    ins = inside(coarse, level).astype(np.int64)
    mx, my, mz = ins.shape
    s = sum(ins[dx:mx - 1 + dx, dy:my - 1 + dy, dz:mz - 1 + dz] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    return (s != 0) & (s != 8)


def dilate(mask, r):
    """rule 3: r times the 26-neighbourhood, clipped at the border"""
    m = mask.copy()
    for _ in range(int(r)):
        p = np.pad(m, 1)
        out = np.zeros_like(m)
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    out |= p[dx:dx + m.shape[0], dy:dy + m.shape[1], dz:dz + m.shape[2]]
        m = out
    return m


def evaluated_mask(active, idx3, shape):
    """rule 4: every fine point in the closed index box of an active cell"""
    ev = np.zeros(shape, dtype=bool)
    for a, b, c in zip(*np.nonzero(active)):
        ev[idx3[0][a]:idx3[0][a + 1] + 1, idx3[1][b]:idx3[1][b + 1] + 1, idx3[2][c]:idx3[2][c + 1] + 1] = True
    return ev


def owner(n, idx):
    """rule 5, one axis: the last coarse index <= the point's index, clamped to the last cell"""
    o = np.searchsorted(idx, np.arange(n), side="right") - 1
    return np.minimum(o, len(idx) - 2)


def count_leaks(assembled, ev, level):
    """rule 7: sign-changing edges with a filled point among the two ends or their in-grid +-1 neighbours along the three axes"""
    ins = inside(assembled, level)
    filled = ~ev
    near = filled.copy()                       # a filled point in the point's own stencil
    for d in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[d], hi[d] = slice(0, -1), slice(1, None)
        near[tuple(lo)] |= filled[tuple(hi)]
        near[tuple(hi)] |= filled[tuple(lo)]
    leaks = 0
    for d in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[d], hi[d] = slice(0, -1), slice(1, None)
        cross = ins[tuple(lo)] != ins[tuple(hi)]
        leaks += int((cross & (near[tuple(lo)] | near[tuple(hi)])).sum())
    return leaks


def hier(dense, level, c, r, evaluate_all=False):
    """the stages' outputs from a dense float32 volume.  evaluate_all: every cell active (the assembled volume is then the dense one)"""
    assert c in FACTORS and r >= 0
    dense = np.ascontiguousarray(dense, dtype=np.float32)
    shape = dense.shape
    idx3 = [coarse_index(n, c) for n in shape]
    coarse = dense[np.ix_(*idx3)]
    core = core_cells(coarse, level)
    active = np.ones_like(core) if evaluate_all else dilate(core, r)
    ev = evaluated_mask(active, idx3, shape)
    index = np.flatnonzero(ev.reshape(-1)).astype(np.int32)          # ascending
    own = [owner(n, idx) for n, idx in zip(shape, idx3)]
    fill = coarse[np.ix_(*own)]
    assembled = np.where(ev, dense, fill).astype(np.float32)
    return {"coarse_index": idx3, "coarse": coarse, "core": core, "active": active, "evaluated": ev, "index": index,
            "volume": assembled, "leaks": count_leaks(assembled, ev, level),
            "core_cells": int(core.sum()), "active_cells": int(active.sum()), "evaluated_points": int(ev.sum()), "points": dense.size,
            "coarse_shape": tuple(coarse.shape)}


def hidden(dense, assembled, level):
    return int((inside(dense, level) != inside(assembled, level)).sum())


def read_mask(vol, level):
    """the points marching cubes and dsn_mc_normals read VALUES of (not just sides): the ends of the sign-changing edges and their
    in-grid +-1 neighbours along the three axes"""
    ins = inside(vol, level)
    ends = np.zeros(vol.shape, dtype=bool)
    for d in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[d], hi[d] = slice(0, -1), slice(1, None)
        cross = ins[tuple(lo)] != ins[tuple(hi)]
        ends[tuple(lo)] |= cross
        ends[tuple(hi)] |= cross
    read = ends.copy()
    for d in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[d], hi[d] = slice(0, -1), slice(1, None)
        read[tuple(lo)] |= ends[tuple(hi)]
        read[tuple(hi)] |= ends[tuple(lo)]
    return read


def reads_equal(dense, assembled, level):
    m = read_mask(dense, level)
    a = np.ascontiguousarray(dense, np.float32).view(np.uint32)
    b = np.ascontiguousarray(assembled, np.float32).view(np.uint32)
    return bool(np.array_equal(a[m], b[m]))


# ---- the analytic volumes of the tests ----
def axes_of(shape, lo=-1.0, hi=1.0):
    return tuple(np.linspace(lo, hi, n).astype(np.float32) for n in shape)


def _xyz(shape):
    return np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing="ij")


def sphere(shape, r=0.62, centre=(0.07, -0.05, 0.03)):
    x, y, z = _xyz(shape)
    return (r - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def two_spheres(shape):
    return np.maximum(sphere(shape, 0.35, (-0.45, -0.1, 0.0)), sphere(shape, 0.3, (0.45, 0.2, 0.1)))


def torus(shape):
    x, y, z = _xyz(shape)
    x, y, z = x - 0.04, y + 0.06, z - 0.05
    return (0.25 - np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).astype(np.float32)


def noisy_sphere(shape, seed=5):
    return sphere(shape) + np.random.default_rng(seed).uniform(-0.02, 0.02, shape).astype(np.float32)


def step_sphere(shape):
    """0 outside, 30 inside: the shape of a trained density around its 0.5 level"""
    return np.where(sphere(shape) > 0, np.float32(30.0), np.float32(0.0)).astype(np.float32)


def sphere_with_blob(shape):
    """a sphere plus a 0.04-radius blob in the grid's corner: smaller than a coarse cell, far from any coarse sign change"""
    return np.maximum(sphere(shape, 0.5, (0.0, 0.0, 0.0)), sphere(shape, 0.04, (-0.924, -0.876, -0.896)))


def nan_inf_volume(shape, seed=9):
    v = noisy_sphere(shape, seed)
    rng = np.random.default_rng(seed + 1)
    k = rng.integers(0, 16, shape)
    v[k == 0] = np.nan
    v[k == 1] = np.inf
    v[k == 2] = -np.inf
    return v


CASES = {"sphere": sphere, "two_spheres": two_spheres, "torus": torus, "noisy_sphere": noisy_sphere}
GRIDS = ((33, 33, 33), (37, 41, 35), (64, 50, 47))
