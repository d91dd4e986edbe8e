"""GPU: the sampler's frame-size path (k_sample_gg_sweep + k_sample_gg_emit, csrc/dsn_geom.hip) - the two-level vertex cull (the
workgroup's 256 rays as one bundle, cone and plane, compacted survivors in LDS, then the per-wave bundle) and the emission that
classifies GG_EMIT_U stripes of samples per iteration (dsn_nns_classify_batch, csrc/dsn_nn.h).

Batches above 131 072 rays (512 blocks) take the frame-size path and R * S >= 2^20 the fused classification, so the batches here are
R = 140 001 rays of the 512 x 512 synthetic frame (its first rows, see batch()) with S = 8 (9: stripes straddle rays differently; 64: the frame's own): that count
is a multiple of neither 64 nor 256 - the last wave and the last block are ragged.  near / far / z / points against the oracle's full
sweep bit for bit, in raster order (narrow block cones, blocks that keep no vertex) and shuffled (wide cones: nothing is culled, every
vertex of a tile survives - the LDS list's worst case), one ray repeated (cos = 1, sin = 0 for both cones), and the fused geometry phase
against the exhaustive search with the cell ids, ranks and counters the sampler left in the workspace.

Checked once by hand against a build whose cull radius was tightened to 2 cm (below the spheres' 5 cm, so true hits are dropped):
every raster case, the repeated torso ray and both fused-geometry cases fail; the shuffled cases and the repeated ray that misses
pass, as they must - their bundles are so wide, or their rays so far from the body, that no radius culls a hit."""
import numpy as np
import pytest
import torch

import oracle as O
from helpers import state
from test_gpu_nns_block import FINE_MAXCELL, a256, geometry, read_geometry, same_geometry

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 140001                     # > 131 072 (512 blocks): the frame-size path; R % 64 = 33, R % 256 = 225
BLOCK = 256                    # = GG_THREADS
HW = 512
N_CHECK = 8192


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_ctx = {}


def ctx():
    """body, frame rays, scene and the oracle's answers on the checked subsets: built once, shared, never modified"""
    if _ctx:
        return _ctx
    from dsnerf_amd import _lib, synth
    assert R > 131072 and R % 64 and R % BLOCK and R * 8 >= 1 << 20
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon, seed=3)
    rays = synth.make_rays(HW, HW, xyz, fit_box=True)
    pk = _lib.PackedParams(DEV).update({k: torch.from_numpy(v) for k, v in state().items()})
    sc = _lib.Scene(torch.from_numpy(canon), torch.from_numpy(faces), DEV)
    poses = torch.from_numpy(synth.make_poses())
    sc.set_frame(pk, torch.from_numpy(xyz), poses, 5)
    _ctx.update(lib=_lib, synth=synth, canon=canon, faces=faces, xyz=xyz, rays=rays, pk=pk, sc=sc, poses=poses, ref={}, miss_block=None)
    return _ctx


MISS_BLOCK = 1                 # block of the raster batch whose rays all miss the body


def batch(c, order):
    """ray indices (into the frame) of the batch: the frame's first rays in raster order, or a fixed permutation of them.  No half image
    row of this frame misses the body (it stands in the middle columns), so one block of the batch - MISS_BLOCK - is a 64 x 4 pixel
    patch of the image's corner instead, one row segment per wave, 160 pixels from the nearest ray that hits: a block that keeps no
    vertex"""
    patch = (np.arange(4)[:, None] * HW + np.arange(64)[None, :]).reshape(-1)
    idx = np.concatenate([np.arange(MISS_BLOCK * BLOCK), patch, np.arange(MISS_BLOCK * BLOCK, R - BLOCK)])
    assert idx.size == R
    return np.random.default_rng(5).permutation(idx) if order == "shuffled" else idx


def checked_positions(c, order):
    """8192 positions of the batch: the whole first and last block, in raster order the whole of a block whose rays all miss the body
    (the oracle says so), and a fixed random rest that covers every lane position of a block"""
    last = np.arange((R - 1) // BLOCK * BLOCK, R)
    parts = [np.arange(BLOCK), last]
    if order == "raster":
        if c["miss_block"] is None:
            # the oracle's sweep leaves near / far of all the rays of MISS_BLOCK alone
            rays = c["rays"]
            p = batch(c, order)[MISS_BLOCK * BLOCK:(MISS_BLOCK + 1) * BLOCK]
            n0, f0 = rays["near"][p].copy(), rays["far"][p].copy()
            o = O.sample_gg(rays["ray_o"][p], rays["ray_d"][p], n0, f0, c["xyz"], 8, t_vals=np.linspace(0, 1, 8, dtype=np.float32))
            assert np.array_equal(o["near"], rays["near"][p]) and np.array_equal(o["far"], rays["far"][p]), "MISS_BLOCK hits the body"
            c["miss_block"] = MISS_BLOCK
        b = c["miss_block"]
        parts.append(np.arange(b * BLOCK, (b + 1) * BLOCK))
    fixed = np.unique(np.concatenate(parts))
    rest = np.setdiff1d(np.arange(R), fixed)
    rest = np.random.default_rng(17).choice(rest, N_CHECK - fixed.size, replace=False)
    sel = np.sort(np.concatenate([fixed, rest]))
    assert sel.size == N_CHECK and np.unique(sel % BLOCK).size == BLOCK
    return sel


def reference(c, order, S, jitter):
    """the oracle's sweep on the checked subset of a batch (cached per case)"""
    key = (order, S, jitter)
    if key not in c["ref"]:
        idx, sel = batch(c, order), checked_positions(c, order)
        rays = c["rays"]
        tv = torch.linspace(0.0, 1.0, steps=S).numpy()
        jit = c["synth"].hash_uniform(R * S, 91).reshape(R, S).astype(np.float32) if jitter else None
        n0, f0 = rays["near"][idx][sel].copy(), rays["far"][idx][sel].copy()
        o = O.sample_gg(rays["ray_o"][idx][sel], rays["ray_d"][idx][sel], n0, f0, c["xyz"], S, None if jit is None else jit[sel], tv)
        c["ref"][key] = (idx, sel, jit, {k: np.array(o[k]) for k in ("near", "far", "z_vals", "pts")})
    return c["ref"][key]


def run_sampler(c, idx, S, jit):
    rays = c["rays"]
    near, far = T(rays["near"][idx]), T(rays["far"][idx])
    tv = torch.linspace(0.0, 1.0, steps=S).to(DEV)
    pts, z = c["lib"].sample(c["sc"], T(rays["ray_o"][idx]), T(rays["ray_d"][idx]), near, far, S, tv, None if jit is None else T(jit))
    torch.cuda.synchronize()
    return near, far, z, pts


def check_against_oracle(c, order, S, jitter):
    idx, sel, jit, o = reference(c, order, S, jitter)
    near, far, z, pts = run_sampler(c, idx, S, jit)
    s = torch.from_numpy(sel).to(DEV)
    got = dict(near=near[s], far=far[s], z_vals=z[s], pts=pts[s])
    hit = o["near"] != c["rays"]["near"][idx][sel]
    print(f"{order}, S {S}, jitter {jitter}: {int(hit.sum())} of {sel.size} checked rays get an interval from the body")
    assert hit.sum() > 500 and (~hit).sum() > 500
    for k, v in got.items():
        assert v.cpu().numpy().tobytes() == o[k].tobytes(), (order, S, jitter, k)
    if order == "raster":       # the block that misses the body: untouched near / far
        b = slice(c["miss_block"] * BLOCK, (c["miss_block"] + 1) * BLOCK)
        assert torch.equal(near[b].cpu(), torch.from_numpy(c["rays"]["near"][idx[b]]))


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("order", ["raster", "shuffled"])
def test_frame_size_sampler_equals_the_oracle(order, jitter):
    """R = 140 001, S = 8: near / far / z / points of 8192 rays (first and last block, every lane position, a whole block that misses the
    body) bit for bit the oracle's, in raster order and shuffled (nothing culled: every vertex of a tile in the LDS list)"""
    check_against_oracle(ctx(), order, 8, jitter)


@pytest.mark.parametrize("order", ["raster", "shuffled"])
def test_stripes_that_straddle_rays_equal_the_oracle(order):
    """S = 9: a stripe of 256 samples begins and ends inside rays, differently in each of the batched stripes"""
    check_against_oracle(ctx(), order, 9, True)


@pytest.mark.parametrize("order", ["raster", "shuffled"])
def test_frame_depth_equals_the_oracle(order):
    """S = 64 on the same rays (the frame's own depth: one ray per wave and stripe, 64 stripes per block in batches of GG_EMIT_U)"""
    check_against_oracle(ctx(), order, 64, False)


@pytest.mark.parametrize("where", ["torso", "miss"])
def test_one_ray_repeated_equals_the_oracle(where):
    """a degenerate batch: R copies of one ray - cos = 1, sin = 0 for the wave's and the block's cone.  One ray through the torso, one
    that misses the body; every copy must get the oracle's answer for that ray"""
    c = ctx()
    rays, S = c["rays"], 8
    tv = torch.linspace(0.0, 1.0, steps=S)
    k = (HW // 2) * HW + HW // 2 if where == "torso" else 0
    one = lambda a: np.ascontiguousarray(np.repeat(a[k:k + 1], 4, axis=0))
    n0, f0 = one(rays["near"]).copy(), one(rays["far"]).copy()
    o = O.sample_gg(one(rays["ray_o"]), one(rays["ray_d"]), n0, f0, c["xyz"], S, t_vals=tv.numpy())
    hit = o["near"][0] != rays["near"][k]
    assert hit == (where == "torso"), (where, o["near"][0], rays["near"][k])
    rep = lambda a: T(np.ascontiguousarray(np.repeat(a[k:k + 1], R, axis=0)))
    near, far = rep(rays["near"]), rep(rays["far"])
    pts, z = c["lib"].sample(c["sc"], rep(rays["ray_o"]), rep(rays["ray_d"]), near, far, S, tv.to(DEV), None)
    torch.cuda.synchronize()
    assert torch.equal(near, T(o["near"][:1]).expand(R)) and torch.equal(far, T(o["far"][:1]).expand(R))
    assert torch.equal(z, T(o["z_vals"][:1]).expand(R, S)) and torch.equal(pts, T(o["pts"][:1]).expand(R, S, 3))


def read_classification(ws, n):
    """cell ids [N], ranks [N], per-cell counters and the outside counter the sampler's classification left in the workspace (layout of
    dsn_carve, csrc/dsn_api.hip: cells and ranks at the start of G, the counters at the start of the cell-major search's small scratch)"""
    from dsnerf_amd import _lib
    b = ws.buf
    g = _lib.CNT_BYTES + a256(4 * n) + a256(n) + a256(4 * n) + a256(12 * n) + a256(4 * n)
    cell = b[g:g + 4 * n].view(torch.int32).cpu().numpy().copy()
    rank = b[g + 4 * n:g + 8 * n].view(torch.int32).cpu().numpy().copy()
    small = g + 12 * n + a256(12 * n + 256) + a256(4 * n)
    counts = b[small:small + 4 * FINE_MAXCELL].view(torch.int32).cpu().numpy().copy()
    totals = small + 3 * a256(4 * (FINE_MAXCELL + 1))
    outside = int(b[totals:totals + 256].view(torch.int32)[2])
    return cell, rank, counts, outside


@pytest.mark.parametrize("S", [8, 9])
def test_fused_geometry_phase_equals_the_exhaustive_search(S):
    """the geometry phase of the batch (the sampler classifies while it writes z, GG_EMIT_U stripes at a time): transparency flags and
    canonical points of the exhaustive sweep bit for bit, the same active set, on every cell's lists and on lazily built ones; and in the
    workspace every sample in exactly one cell, the ranks of a cell's samples 0 .. count - 1 each once, the counters a host count of
    the cell ids"""
    c = ctx()
    _lib, rays = c["lib"], c["rays"]
    n = R * S
    assert n >= 1 << 20                     # = DSN_CELLMAJOR_MIN: the sampler classifies
    idx = batch(c, "raster")
    o, d, near, far = (T(rays[k][idx]) for k in ("ray_o", "ray_d", "near", "far"))
    sc = _lib.Scene(torch.from_numpy(c["canon"]), torch.from_numpy(c["faces"]), DEV)

    def run(lazy, **kw):
        sc.set_frame(c["pk"], torch.from_numpy(c["xyz"]), c["poses"], 5, lazy=lazy)
        ws, z = geometry(sc, c["pk"], o, d, near, far, S, **kw)
        assert sc.nn_overflow == {}
        return ws, read_geometry(ws, R, S), z

    _, ref, z_ref = run(False, exhaustive=True)
    assert ref["active"].size > 10000
    _, sel, _, oz = reference(c, "raster", S, False)          # (the frame's own z: what the classification saw)
    assert z_ref.cpu().numpy()[sel].tobytes() == oz["z_vals"].tobytes()
    for lazy in (False, True):
        ws, got, z = run(lazy)
        what = "fused, lazily built lists" if lazy else "fused, every cell's lists"
        assert torch.equal(z, z_ref), what
        same_geometry(got, ref, what)
        cell, rank, counts, outside = read_classification(ws, n)
        inside = cell >= 0
        assert cell.max() < FINE_MAXCELL and outside == int((~inside).sum()), (what, outside, int((~inside).sum()))
        host = np.bincount(cell[inside], minlength=FINE_MAXCELL)
        assert np.array_equal(counts, host), what                      # no sample left out, none counted twice
        # ranks: within every cell exactly 0 .. count - 1 - sorted by (cell, rank) they are position minus the cell's first position
        order = np.lexsort((rank[inside], cell[inside]))
        cs, rs = cell[inside][order], rank[inside][order]
        first = np.concatenate([[0], np.cumsum(host)])[cs]
        assert np.array_equal(rs, np.arange(cs.size) - first), what
        print(f"S {S}, {what}: {int(inside.sum())} samples in {int((host > 0).sum())} cells, {outside} outside, largest cell {int(host.max())}")
