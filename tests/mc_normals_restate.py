"""numpy restatement of the marching-cubes vertex normals of include/dsnerf.h (dsn_mc_normals), in the vertex order of
tests/mc_restate.py (ascending edge id 3 n + d).

Gradient of the volume at a grid point along axis d: (v[i + 1] - v[i - 1]) / (ax[i + 1] - ax[i - 1]) inside, the one-sided quotient
over the first / last interval on the grid's outer faces.  A vertex of edge (n, d) mixes the gradients of the edge's two points with
the t of its position, g = g_a + t (g_b - g_a); normal = (s g) / sqrt((g0 g0 + g1 g1) + g2 g2), s = -1 for "descent" and +1 for
"ascent"; (0, 0, 0) unless the norm is positive and finite.  dtype=np.float32 reproduces the kernel bit for bit (numpy does not
fuse); dtype=np.float64 is the same rule in double precision."""
import numpy as np


def gradients(vol, axes, dtype=np.float32):
    """[nx, ny, nz, 3]: the difference quotients at every grid point"""
    v = np.ascontiguousarray(vol, dtype=np.float32).astype(dtype)
    g = np.zeros(v.shape + (3,), dtype=dtype)
    with np.errstate(all="ignore"):
        for d in range(3):
            a = np.asarray(axes[d], dtype=np.float32).astype(dtype)
            nd = v.shape[d]
            i = np.arange(nd)
            lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, nd - 1)
            shape = [1, 1, 1]
            shape[d] = nd
            g[..., d] = (np.take(v, hi, axis=d) - np.take(v, lo, axis=d)) / (a[hi] - a[lo]).reshape(shape)
    return g


def crossing_edges(vol, level):
    """(n, d) of every sign-changing grid edge in ascending edge id"""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    inside = vol > np.float32(level)
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    eid = np.flatnonzero(cross.reshape(-1))
    return eid // 3, eid % 3


def normals(vol, axes, level, gradient_direction, dtype=np.float32):
    if gradient_direction not in ("descent", "ascent"):
        raise ValueError(gradient_direction)
    T = dtype
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    n, d = crossing_edges(vol, level)
    m = n + np.array([ny * nz, nz, 1], dtype=np.int64)[d]
    g = gradients(vol, axes, T).reshape(-1, 3)
    flat = vol.reshape(-1).astype(T)
    s = T(-1.0 if gradient_direction == "descent" else 1.0)
    with np.errstate(all="ignore"):
        a, b = flat[n], flat[m]
        t = (T(np.float32(level)) - a) / (b - a)
        gv = g[n] + t[:, None] * (g[m] - g[n])
        nn = np.sqrt((gv[:, 0] * gv[:, 0] + gv[:, 1] * gv[:, 1]) + gv[:, 2] * gv[:, 2])
        out = (s * gv) / nn[:, None]
    ok = (nn > 0) & (nn < np.inf)
    out = np.where(ok[:, None], out, T(0)).astype(T)
    assert out.dtype == T
    return out
