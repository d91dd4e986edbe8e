"""Case builders for the nearest-face tie rule and the grid's cell edges (test infrastructure, imported by the tests).

Every search path must return what the serial sweep in ascending face order with strict '<' returns: the smallest squared
distance and, among equal distances, the FIRST index.  Random points never tie, so these builders make ties:

* twin_case(): a real body (synth.make_body, uniform or SMPL-like) with a few hundred faces given a TWIN on appended vertices.
  A world twin has the same posed vertices in the same order (posed centroid bit-identical) and its canonical vertices rotated
  by one, so the warp maps points through it differently; a canonical twin is the mirror construction (canonical centroid
  bit-identical, posed vertices rotated), for k_normal.  The two faces of a pair sit 1, ~100, ~900 or ~5000 positions apart
  (the same lane group, other lanes of a wave, other 768-entry segments of the far search); order "orig" puts the original first,
  order "twin" the twin - the index that must win is always the pair's FIRST position.  Query points are generated around the
  twinned faces: on the surface, in the coarse shell and beyond both grids.
* dyadic_soup(): small triangles whose vertices are multiples of 3 * 2^-7, centroids on a lattice of 12 * 2^-7: centroids and every
  squared distance of the queries are exact in float32 in any evaluation order, so lattice midpoints, face centres and cube
  centres tie exactly 2, 4 and 8 distinct centroids.  Face indices are shuffled.
* edge_points(): points on the cell boundaries of a level (the first float32 at which (p - lo) * inv_cell reaches an integer, one
  ulp below it, +- DSN_GRID_GUARD) and on the outer faces of the grid, from the level's 64-byte DsnGrid header.
"""
import functools

import numpy as np

GRID_GUARD = np.float32(1e-4)        # = DSN_GRID_GUARD (csrc/dsn_nn.h)
FAR_SEG = 768                        # = NNS_FAR_SEG (csrc/dsn_nn.hip): candidates per segment of the far canonical search
LEVELS = ("world_fine", "world_coarse", "canon_fine", "canon_coarse")      # = _lib.Scene._NN_NAMES (index into Scene._nn_off)
GAPS = (1, 97, 901, 5003)            # positions between the two faces of a pair (before the other pairs are inserted)
ORDERS = ("orig", "twin")            # which face of every pair comes first


# ---------------------------------------------------------------------------------------------------------------------------
# twins on the real bodies
# ---------------------------------------------------------------------------------------------------------------------------
def _normals(v, f):
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _around(cent, nrm, faces_sel, rng, n):
    """query points around the given faces: on the surface (fine grid), 0.15 - 0.6 m out (coarse shell), 1.5 - 4 m out (beyond)"""
    f = faces_sel[rng.integers(0, faces_sel.size, n)]
    c, nv = cent[f].astype(np.float64), nrm[f]
    k = n // 3
    near = c[:k] + rng.normal(0.0, 2e-3, (k, 3)) + nv[:k] * rng.uniform(-5e-3, 2e-2, (k, 1))
    shell = c[k:2 * k] + nv[k:2 * k] * rng.uniform(0.15, 0.6, (k, 1))
    far = c[2 * k:] + nv[2 * k:] * rng.uniform(1.5, 4.0, (n - 2 * k, 1))
    return np.concatenate([near, shell, far]).astype(np.float32)


def _pick(O, pts, cent, n, taken):
    """up to n faces nearest to the given points (the most frequent first), none of `taken`, each with room for its gap"""
    idx = O.nearest_face(pts, cent)
    u, cnt = np.unique(idx, return_counts=True)
    u = u[np.argsort(-cnt, kind="stable")]
    u = u[~np.isin(u, list(taken))]
    return [int(x) for x in u[:n]]


@functools.lru_cache(maxsize=None)
def _picks(nonuniform, n_world=240, n_canon=240):
    """(canon, faces, xyz, world picks, canon picks, world queries, canonical queries) of one body - the queries are those the picks
    were made for: half of the picks are the faces nearest to far / shell points, half random faces, and the queries surround them"""
    import oracle as O
    from dsnerf_amd import synth
    canon, faces = synth.make_body(nonuniform=nonuniform)
    xyz = synth.pose_body(canon)
    F = faces.shape[0]
    rng = np.random.default_rng(41 if nonuniform else 40)
    out = []
    taken = set()
    for v, n_pick in ((xyz, n_world), (canon, n_canon)):
        cent, nrm = O.centroids(v, faces), _normals(v, faces)
        seed = _around(cent, nrm, rng.permutation(F)[:2000], rng, 3000)[1000:]      # shell + far: which faces are nearest out there
        picks = _pick(O, seed, cent, n_pick // 2, taken)
        taken.update(picks)
        rest = [int(f) for f in rng.permutation(F) if int(f) not in taken][:n_pick - len(picks)]
        picks = picks + rest
        taken.update(rest)
        q = _around(cent, nrm, np.array(picks), rng, 6000)
        out.append((picks, q))
    return canon, faces, xyz, out[0][0], out[1][0], out[0][1], out[1][1]


def twin_faces(canon, faces, xyz, world_picks, canon_picks, order):
    """the body with a twin of every picked face.  Returns dict(canon, faces, xyz, first, second, space, orig): for pair k,
    first[k] < second[k] are the positions of its two faces in `faces` (the index that must win a tie is first[k]), space[k] is
    "world" / "canon" (which centroid is shared bit for bit), orig[k] is the position of the ORIGINAL face ("orig": first), base[k]
    its index in the input."""
    assert order in ORDERS
    canon, faces, xyz = np.asarray(canon, np.float32), np.asarray(faces, np.int64), np.asarray(xyz, np.float32)
    V, F = canon.shape[0], faces.shape[0]
    picks = [(int(f), "world") for f in world_picks] + [(int(f), "canon") for f in canon_picks]
    assert len({f for f, _ in picks}) == len(picks), "a face is twinned once"
    new_c, new_x, rows, keys, roles = [], [], [], [], []
    for k, (f, space) in enumerate(picks):
        a, b, c = faces[f]
        src = np.array([a, b, c])
        rot = np.array([b, c, a])
        same, turned = (xyz, canon) if space == "world" else (canon, xyz)
        vs, vt = same[src], turned[rot]          # the shared space keeps the vertex order; the other one is rotated by one
        new_c.append(vt if space == "world" else vs)
        new_x.append(vs if space == "world" else vt)
        rows.append(V + 3 * k + np.arange(3))
        gap = GAPS[k % len(GAPS)]
        eps = 1e-6 * (k + 1)                     # (distinct keys for the inserted rows)
        ka, kb = (f, f + gap - 0.5 + eps) if f + gap < F else (f - gap + 0.5 + eps, f)
        keys.append((ka, kb))
        roles.append(space)
    canon2 = np.concatenate([canon] + new_c).astype(np.float32)
    xyz2 = np.concatenate([xyz] + new_x).astype(np.float32)
    # rows of the final face list: the untouched faces at their own index, each pair's two faces at its two keys
    picked = {f for f, _ in picks}
    items = [(float(i), faces[i], None) for i in range(F) if i not in picked]
    for k, (f, space) in enumerate(picks):
        ka, kb = keys[k]
        orig_row, twin_row = faces[f], rows[k]
        a_row, b_row = (orig_row, twin_row) if order == "orig" else (twin_row, orig_row)
        items.append((float(ka), a_row, (k, 0)))
        items.append((float(kb), b_row, (k, 1)))
    items.sort(key=lambda t: t[0])
    faces2 = np.stack([np.asarray(r, np.int64) for _, r, _ in items])
    first, second = np.zeros(len(picks), np.int64), np.zeros(len(picks), np.int64)
    for pos, (_, _, tag) in enumerate(items):
        if tag is not None:
            (first if tag[1] == 0 else second)[tag[0]] = pos
    orig = first.copy() if order == "orig" else second.copy()
    return dict(canon=canon2, faces=faces2, xyz=xyz2, first=first, second=second, space=np.array(roles), orig=orig,
                base=np.array([f for f, _ in picks], np.int64))


def twin_case(nonuniform, order):
    """twin_faces() of one body + the world / canonical query points around its twinned faces (dict)"""
    canon, faces, xyz, wp, cp, qw, qc = _picks(bool(nonuniform))
    d = twin_faces(canon, faces, xyz, wp, cp, order)
    d.update(base_canon=canon, base_faces=faces, base_xyz=xyz, q_world=qw, q_canon=qc)
    return d


def pair_of(case, space=None):
    """face position -> pair number for every face of a pair (optionally of one space), -1 elsewhere"""
    m = np.full(case["faces"].shape[0], -1, np.int64)
    for k in range(case["first"].size):
        if space is None or case["space"][k] == space:
            m[case["first"][k]] = k
            m[case["second"][k]] = k
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# dyadic lattice soup
# ---------------------------------------------------------------------------------------------------------------------------
def dyadic_soup(n=6, seed=7):
    """n^3 small triangles (vertices: integer multiples of u3 = 3 * 2^-7; centroids on the lattice 12 * 2^-7 * (i, j, k)), face
    order shuffled, + queries.  Returns dict(verts, faces, cent, pts, mult, win): mult[q] centroids lie at the smallest squared
    distance of query q (1, 2, 4 or 8: lattice points, edge midpoints, face centres, cube centres), win[q] = the smallest face
    index among them.  Every value is exact in float32: the centroid sum (a + b) + c and / 3, each query's d = dx*dx, fma, fma."""
    rng = np.random.default_rng(seed)
    u = 2.0 ** -7
    L = 12                                                   # lattice step in units of u (a multiple of 3 and of 2)
    ijk = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    C = ijk * L                                              # centroids in units of u (multiples of 3)
    F = C.shape[0]
    a = rng.integers(-1, 2, (F, 3)) * 3
    b = rng.integers(-1, 2, (F, 3)) * 3
    a[np.all(a == 0, 1), 0] = 3                              # (non-degenerate enough: the warp divides by the face's frame)
    b[np.all(b == 0, 1), 1] = 3
    par = np.all(np.cross(a, b) == 0, 1)
    b[par] = np.array([0, 3, 3])
    a[par] = np.array([3, 0, 0])
    v0, v1, v2 = C + a, C + b, C - a - b                     # (v0 + v1 + v2) / 3 = C exactly
    perm = rng.permutation(F)                                # face f of the soup is lattice site perm[f]
    verts = np.stack([v0[perm], v1[perm], v2[perm]], 1).reshape(-1, 3) * u
    faces = np.arange(3 * F).reshape(F, 3)
    cent = (C[perm] * u).astype(np.float32)
    site_face = np.empty(F, np.int64)
    site_face[perm] = np.arange(F)
    h = L // 2
    inner = ijk[np.all(ijk < n - 1, 1)] * L                  # lower corners of the lattice cubes
    pts, mult, win = [], [], []
    for off, m in (((0, 0, 0), 1), ((h, 0, 0), 2), ((0, h, 0), 2), ((0, 0, h), 2), ((h, h, 0), 4), ((h, 0, h), 4), ((0, h, h), 4),
                   ((h, h, h), 8)):
        q = inner + np.array(off)
        pts.append(q)
        mult.append(np.full(q.shape[0], m))
        # the m tied sites: the corners of the cell spanned by the non-zero offset axes
        ax = [i for i in range(3) if off[i]]
        best = np.full(q.shape[0], np.iinfo(np.int64).max)
        for bits in range(1 << len(ax)):
            s = q - np.array(off)
            for j, i in enumerate(ax):
                if bits >> j & 1:
                    s[:, i] += L
            si = (s[:, 0] // L * n + s[:, 1] // L) * n + s[:, 2] // L
            best = np.minimum(best, site_face[si])
        win.append(best)
    pts = (np.concatenate(pts) * u).astype(np.float32)
    return dict(verts=verts.astype(np.float32), faces=faces, cent=cent, pts=pts, mult=np.concatenate(mult), win=np.concatenate(win))


def lexmin_f64(pts, cent):
    """float64 brute force: (squared distance, index) lexicographic minimum and the number of centroids at that distance"""
    d = ((pts.astype(np.float64)[:, None, :] - cent.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    m = d.min(1)
    return np.argmin(d, 1), (d == m[:, None]).sum(1)


# ---------------------------------------------------------------------------------------------------------------------------
# cell edges of a level
# ---------------------------------------------------------------------------------------------------------------------------
def parse_header(raw):
    """a level's 64-byte DsnGrid header (csrc/dsn_nn.h) -> dict"""
    raw = np.ascontiguousarray(np.asarray(raw, np.uint8)[:64])
    f, i = raw.view(np.float32), raw.view(np.int32)
    return dict(lo=f[0:3].copy(), cell=np.float32(f[3]), inv_cell=np.float32(f[4]), n=i[5:8].copy(), ncell=int(i[8]), ok=int(i[9]),
                total=int(i[10]), cap=int(i[11]), maxcell=int(i[12]), lazy=int(i[13]))


def read_header(scene, level):
    """the DsnGrid header of one nearest-face level of a _lib.Scene (synchronising copy)"""
    o = scene._nn_off[LEVELS.index(level)]
    return parse_header(scene.buf[o:o + 64].cpu().numpy())


def cell_of(hdr, pts):
    """the kernels' dsn_grid_cell_geom in float32 (no contraction): cell index or -1 outside the grid"""
    p = np.asarray(pts, np.float32)
    fr = (p - hdr["lo"]) * hdr["inv_cell"]
    ok = np.all(fr >= 0, 1)
    ix = np.where(ok[:, None], fr, 0).astype(np.int64)
    ok &= np.all(ix < hdr["n"], 1)
    c = (ix[:, 0] * hdr["n"][1] + ix[:, 1]) * hdr["n"][2] + ix[:, 2]
    return np.where(ok, c, -1)


def _reaches(hdr, a, x, k):
    return np.float32(np.float32(x - hdr["lo"][a]) * hdr["inv_cell"]) >= np.float32(k)


def boundary(hdr, a, k):
    """the first float32 x with (x - lo[a]) * inv_cell >= k, evaluated as the kernels do"""
    x = np.float32(hdr["lo"][a] + np.float32(k) * hdr["cell"])
    while _reaches(hdr, a, x, k):
        x = np.nextafter(x, np.float32(-np.inf))
    while not _reaches(hdr, a, x, k):
        x = np.nextafter(x, np.float32(np.inf))
    return x


def edge_points(hdr, base, outer=False):
    """points on cell boundaries of the level: for base point i, axis i % 3 is moved to the nearest boundary plane k (outer: the
    grid's first or last plane, 0 or n[a]) in four forms - the first float32 at which the cell index reaches k, one ulp below it,
    and +- GRID_GUARD around it.  The two other coordinates stay where the base point has them."""
    base = np.asarray(base, np.float32)
    out = []
    for i, p in enumerate(base):
        a = i % 3
        if outer:
            k = 0 if i % 2 == 0 else int(hdr["n"][a])
        else:
            k = int(np.clip(np.rint((p[a] - hdr["lo"][a]) * hdr["inv_cell"]), 1, int(hdr["n"][a]) - 1))
        x = boundary(hdr, a, k)
        for v in (x, np.nextafter(x, np.float32(-np.inf)), np.float32(x + GRID_GUARD), np.float32(x - GRID_GUARD)):
            q = p.copy()
            q[a] = v
            out.append(q)
    return np.asarray(out, np.float32).reshape(-1, 3)


def tie_mask(case, idx, space):
    """for face indices idx (an answer of the search in `space`): True where idx is one face of a pair whose two centroids are
    bit-identical in that space - a real tie (a world pair's canonical centroids coincide for about half of the pairs too)"""
    import oracle as O
    cent = O.centroids(case["xyz"] if space == "world" else case["canon"], case["faces"])
    same = np.all(cent[case["first"]] == cent[case["second"]], 1)
    k = pair_of(case)[np.asarray(idx)]
    return (k >= 0) & same[np.maximum(k, 0)]


def read_coarse_lists(scene, level="canon_coarse"):
    """(offsets, list) of a coarse level of a _lib.Scene: int32 face indices per cell (layout of dsn_grid_view, csrc/dsn_nn.h)"""
    a256 = lambda b: (b + 255) // 256 * 256
    maxcell = 16384                                           # = DSN_NN_COARSE_MAXCELL
    o = scene._nn_off[LEVELS.index(level)]
    h = read_header(scene, level)
    b = scene.buf[o:o + 256 + a256(4 * (maxcell + 1)) + a256(4 * maxcell) + 4 * h["total"]].cpu().numpy()
    off = b[256:256 + 4 * (h["ncell"] + 1)].view(np.int32)
    p = 256 + a256(4 * (maxcell + 1)) + a256(4 * maxcell)
    return off.copy(), b[p:p + 4 * h["total"]].view(np.int32).copy()
