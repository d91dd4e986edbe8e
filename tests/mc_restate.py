"""numpy restatement of the marching cubes of include/dsnerf.h (dsn_mc_count / dsn_mc_emit), from the library's case table.

Inside = v > level; one vertex per sign-changing grid edge in ascending edge id 3 n + d; t = (level - a) / (b - a) and the coordinate
ax[i] + t * (ax[i + 1] - ax[i]) in float32 (numpy does not fuse); triangles in ascending cell index, then in table order; ascent
reverses every triangle.  Returns (verts [V,3] float32, faces [T,3] int32)."""
import numpy as np

# cube numbering of include/dsnerf.h: corner c = dx + 2 dy + 4 dz; edge e = 4 d + q, q = b1 + 2 b2 over the other axes in increasing order
OTHER = {0: (1, 2), 1: (0, 2), 2: (0, 1)}


def edge_corners(e):
    d, q = e // 4, e % 4
    a1, a2 = OTHER[d]
    c0 = ((q & 1) << a1) | ((q >> 1) << a2)
    return c0, c0 | (1 << d)


def corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.int64)


def marching_cubes(vol, axes, level, gradient_direction, table):
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    level = np.float32(level)
    nx, ny, nz = vol.shape
    ax = [np.asarray(a, dtype=np.float32) for a in axes]
    inside = vol > level                              # (NaN compares False: outside)
    N = vol.size
    strides = (ny * nz, nz, 1)
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    eid = np.flatnonzero(cross.reshape(-1))           # ascending edge id 3 n + d
    n, d = eid // 3, eid % 3
    vid = np.full(3 * N, -1, dtype=np.int64)
    vid[eid] = np.arange(eid.size)
    flat = vol.reshape(-1)
    i, j, k = n // (ny * nz), (n // nz) % ny, n % nz
    verts = np.stack([ax[0][i], ax[1][j], ax[2][k]], axis=1).astype(np.float32)
    a = flat[n]
    b = flat[n + np.array(strides, dtype=np.int64)[d]]
    t = (level - a) / (b - a)
    for dd in range(3):
        s = d == dd
        idx = (i, j, k)[dd][s]
        verts[s, dd] = ax[dd][idx] + t[s] * (ax[dd][idx + 1] - ax[dd][idx])
    # cells in ascending index = base points (i < nx-1, j < ny-1, k < nz-1) in ascending n
    ins = inside.astype(np.int64)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = corner_xyz(c)
        case |= ins[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] << c
    ci, cj, ck = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")
    base = ((ci * ny + cj) * nz + ck).reshape(-1)
    case = case.reshape(-1)
    ntri = table[case, 0]
    keep = ntri > 0
    base, case, ntri = base[keep], case[keep], ntri[keep]
    cell = np.repeat(np.arange(base.size), ntri)
    tri_in_cell = np.arange(cell.size) - np.repeat(np.cumsum(ntri) - ntri, ntri)
    faces = np.zeros((cell.size, 3), dtype=np.int64)
    c0_of = np.array([edge_corners(e)[0] for e in range(12)])
    off_of = np.array([corner_xyz(c) @ np.array(strides) for c in c0_of])
    for r in range(3):
        e = table[case[cell], 1 + 3 * tri_in_cell + r]
        faces[:, r] = vid[3 * (base[cell] + off_of[e]) + e // 4]
    assert (faces >= 0).all()
    if gradient_direction == "ascent":
        faces = faces[:, ::-1]
    elif gradient_direction != "descent":
        raise ValueError(gradient_direction)
    return verts, np.ascontiguousarray(faces.astype(np.int32))


def euler_characteristic(verts, faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    E = np.unique(e, axis=0).shape[0]
    used = np.unique(faces).size
    return used - E + faces.shape[0]


def directed_edge_counts(faces):
    """(number of directed edges, how many appear more than once, how many undirected edges lack their reverse)"""
    de = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    key = de[:, 0] * (1 << 32) + de[:, 1]
    u, cnt = np.unique(key, return_counts=True)
    rev = de[:, 1] * (1 << 32) + de[:, 0]
    return de.shape[0], int((cnt > 1).sum()), int((~np.isin(rev, u)).sum())


def area(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
