"""The persistent field and lighting kernels, tile by tile, against float64 (tests/field_restate.py).

k_field16 (single launch, forward, reverse), k_field, k_light16 (with and without the factor output) walk
`tile = blockIdx.x; tile < ntiles; tile += gridDim.x` over tiles of 128 points with one workgroup per compute unit, and fetch the
next tiles' list entries and coordinates while they work on the current one; k_light takes one tile per workgroup.  The stage tests
(test_gpu_stages.py) stop at 96 tiles: no workgroup takes that loop twice there.  Here every kernel runs on counts from 0 to
3 G T + 37 T + 77 points (G workgroups, T = 128: four tiles for 38 workgroups and three for the rest on 256 compute units), dense and
through a shuffled list whose count lies in a device counter far below the array length, and every output is judged per point.

Points: a pool of 4096 distinct canonical points per weight set - 2048 `near` (the first non-transparent x_c of full_eval), 1024
`shell` (non-transparent x_c + 0.2 N(0,1)), 1024 `far` (N(0,1) U(1,60) m: encoding arguments up to 3e4 rad, the regime of
dsn_sincos; on w3 |sigma| reaches 2e4 there and the fp16-range fallback fires in the middle of a multi-tile launch).  Slot i of a
launch holds pool entry src[i], src a chain of seeded permutations: every tile mixes the bands, every pool point recurs in other
tiles, waves and loop rounds.  Output i is judged against truth[src[i]], the float64 restatement, computed once per weight set.

Asserted, per band (so that the far band's magnitudes do not loosen the near band's bar):
 1. sigma, essence: error <= the project's bar on that band's truth (helpers.ref_tol's rule: 1e-4 where max |.| <= 100, 4e-6 max |.|
    above) and <= 1.5 x the float32 C oracle's error against the same truth + 1e-5 (test_field's rule; the oracle's error over the
    band of the pool, which is "the same points" from 4096 points up - ORACLE_RULE below says why not on a handful of points).
 2. d sigma/dx where sigma > 0 in float64 and on the device (points with |sigma64| inside the sigma bar left out: at most 1 % of a
    band): rel = |g - g64| / max(|g64|, 1), median < 2e-6, share(rel > 1e-4) <= the oracle's share on those points + 2e-3.
 3. colours (and the factor ELU + 1): <= 1e-5 max(1, max |colour|) and <= 1.5 x the oracle's error + 1e-6.
 4. position independence, bit for bit: every copy of a pool point holds the same bits in every output - within a launch, across the
    counts and between the dense and the listed form (a table of the pool's bits per kernel is filled by the first launch that meets
    a point and holds for every later one).
 5. nothing else is written: unlisted rows keep the binding's zeros; the sigma > 0 list holds exactly the evaluated points with
    sigma > 0, each once; a listed count of 0 succeeds, writes nothing and leaves the sigma > 0 count at 0.
 6. forward + reverse == the single launch, bit for bit, on every count.
The density screen (k_screen16 with 8 and 4 waves, k_screen16x2; tiles of 256 / 128 / 256 points) is checked for 4. and for its
variants agreeing bit for bit at every count; it is a plain-fp16 estimate with a calibrated margin, no float64 bar applies.

Not reached from here: k_light16_multi.  `_lib.shade(want_factor=True)` runs k_light16<true> (dsn_launch_light16 with a factor
array); k_light16_multi is launched by whole frames only (dsn_render_rays_lights / _maps), whose per-sample colours are indexed by
list slot inside the frame's workspace.  Its tile loop is the same text as k_light16's and both run the same light16_* helpers;
test_gpu_relight.py::test_bench_frame_vis_lighting_angles pins its frames to k_light16's bit for bit at 512 x 512 x 64.

Position independence HELD for every kernel here, the lighting kernels included (k_light16, k_light16<true>, k_light; the
normal search in front of them too), at the commit that introduced this module: an MFMA output column depends on its own column
only, the fp16-range fallback re-evaluates a flagged sample alone, and no output is accumulated across samples.

That the battery bites: three deliberate edits of csrc/dsn_field16.hip, one at a time, each run once against test_gpu_stages.py and
this module on the MI355X -
  k_field16 fetches the next tile's point as tile_point(tile, ..) instead of tile + gridDim.x: 222 / 222 stage tests pass; here
      test_field_tiles[*-k_field16] and test_forward_reverse_tiles[*] fail (6 of 24: from G T + 1 points on, the slots of a
      workgroup's second round hold another point's bits and the rows of its later tiles are wrong, e.g. sigma off by 1.55);
  valid_n forced true for the prefetched tile: 222 / 222 pass; here test_forward_reverse_tiles[*] fail (3 of 24: the lanes past
      the count of a ragged last tile reached on a later round append the last point to the sigma > 0 list again - count 16618
      for 16491 positive points at G T + 1; the single launch only rewrites the last point's own values and stays green);
  k_light16 fetches the list entry tile + gridDim.x instead of tile + 2 gridDim.x: 222 / 222 pass; here test_light_tiles[*-k_light16]
      and test_shade_tiles[*] fail (9 of 24: from a workgroup's third round on, i.e. from 2 G T + T/2 + 5 points).

MEASURED on the MI355X (G = 256), largest figure over all counts and both forms | the float32 oracle's on the band of the pool
(sigma, essence: max abs error against float64; gradient and lighting: the oracle's figure on the points of the launch that gave
the kernel's):
  default k_field16 near  sigma 4.87e-06 | 5.56e-06, essence 2.8e-07 | 4.61e-07, grad median rel 3.52e-07 | 4.47e-07, share rel > 1e-4 0 | 0
  default k_field16 shell sigma 5.24e-06 | 6.73e-06, essence 2.61e-07 | 3.87e-07, grad median rel 3.81e-07 | 4.92e-07, share rel > 1e-4 0 | 0
  default k_field16 far   sigma 7.81e-05 | 0.000137, essence 4.93e-06 | 5.79e-06, grad median rel 3.79e-07 | 3.1e-07, share rel > 1e-4 0 | 0
  default k_field   near  sigma 5.52e-06 | 5.56e-06, essence 3.49e-07 | 4.61e-07, grad median rel 7.32e-07 | 8.1e-07, share rel > 1e-4 0 | 0
  default k_field   shell sigma 6.14e-06 | 6.73e-06, essence 3.31e-07 | 3.87e-07, grad median rel 7.81e-07 | 5.55e-07, share rel > 1e-4 0 | 0
  default k_field   far   sigma 7.58e-05 | 0.000137, essence 5.56e-06 | 5.79e-06, grad median rel 6.19e-07 | 6.23e-07, share rel > 1e-4 0 | 0
  w4      k_field16 near  sigma 0.000855 | 0.000734, essence 3e-06 | 3.86e-06, grad median rel 2.58e-07 | 4.05e-07, share rel > 1e-4 0 | 0
  w4      k_field16 shell sigma 0.000267 | 0.00039, essence 1.71e-06 | 3.17e-06, grad median rel 5.33e-07 | 1e-06, share rel > 1e-4 0 | 0
  w4      k_field16 far   sigma 0.000186 | 0.000302, essence 1.04e-06 | 1.81e-06, grad median rel 7.08e-07 | 5.62e-07, share rel > 1e-4 0 | 0
  w4      k_field   near  sigma 0.000526 | 0.000734, essence 3.6e-06 | 3.86e-06, grad median rel 4.46e-07 | 4.05e-07, share rel > 1e-4 0 | 0
  w4      k_field   shell sigma 0.00035 | 0.00039, essence 1.25e-06 | 3.17e-06, grad median rel 8.7e-07 | 1e-06, share rel > 1e-4 0 | 0
  w4      k_field   far   sigma 0.000248 | 0.000302, essence 1.96e-06 | 1.81e-06, grad median rel 1.89e-07 | 5.62e-07, share rel > 1e-4 0 | 0
  w3      k_field16 near  sigma 0.00108 | 0.00118, essence 0.000136 | 0.000225, grad median rel 3.61e-07 | 5.74e-07, share rel > 1e-4 0 | 0
  w3      k_field16 shell sigma 0.00108 | 0.00144, essence 0.000116 | 0.000188, grad median rel 3.57e-07 | 5.61e-07, share rel > 1e-4 0.00143 | 0
  w3      k_field16 far   sigma 0.0146 | 0.0291, essence 0.00226 | 0.0031, grad median rel 3.54e-07 | 5.41e-07, share rel > 1e-4 0 | 0
  w3      k_field   near  sigma 0.00124 | 0.00118, essence 0.000195 | 0.000225, grad median rel 5.68e-07 | 5.74e-07, share rel > 1e-4 0 | 0
  w3      k_field   shell sigma 0.00126 | 0.00144, essence 0.00017 | 0.000188, grad median rel 5.43e-07 | 5.63e-07, share rel > 1e-4 0 | 0
  w3      k_field   far   sigma 0.0167 | 0.0291, essence 0.00326 | 0.0031, grad median rel 5.46e-07 | 5.41e-07, share rel > 1e-4 0 | 0
  default k_light16 colour 1.71e-07 | 1.38e-07; k_light colour 2.01e-07 | 2.34e-07; shade colour 1.76e-07 | 1.91e-07; shade factor colour 1.76e-07 | 1.91e-07; shade factor factor 1.7e-07 | 2.08e-07
  w4      k_light16 colour 9.78e-08 | 1.01e-07; k_light colour 8.78e-08 | 1.01e-07; shade colour 1.06e-07 | 8.97e-08; shade factor colour 1.06e-07 | 8.97e-08; shade factor factor 1.31e-07 | 9.62e-08
  w3      k_light16 colour 2.35e-06 | 3.2e-06; k_light colour 2.5e-06 | 3.2e-06; shade colour 2.61e-06 | 3.31e-06; shade factor colour 2.61e-06 | 3.31e-06; shade factor factor 3.45e-06 | 4.08e-06
"""
import os

import numpy as np
import pytest
import torch

import field_restate as FR
import oracle as O
from helpers import load, state

pytestmark = pytest.mark.gpu

T = 128                       # points per tile of k_field16 / k_field / k_light16 / k_light
M = 4096                      # pool size
BANDS = ("near", "shell", "far")
BAND_OF = np.repeat(np.arange(3), [2048, 1024, 1024])
SETS = {"default": "full_eval", "w4": "full_eval_w4", "w3": "full_eval_w3"}


def groups():
    """number of persistent workgroups: dsn_cu_count_raw (csrc/dsn_kernels.h)"""
    e = os.environ.get("DSN_PERSISTENT_GROUPS", "")
    try:
        if int(e) > 0:
            return int(e)
    except ValueError:
        pass
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def counts(G, tile=T):
    return [0, 1, 31, 32, 33, 127, 128, 129, G * tile - 1, G * tile, G * tile + 1, 2 * G * tile + tile // 2 + 5,
            3 * G * tile + 37 * tile + 77]


def counts_of(tag, G):
    """default and w4: every count; w3: the two largest"""
    c = counts(G)
    return c[-2:] if tag == "w3" else c


def tiles_per_group(count, G, tile=T):
    nt = -(-count // tile)
    return -(-nt // G), nt // G          # (busiest, idlest)


def bar_of(truth):
    """helpers.ref_tol's rule on an array of float64 truth"""
    m = float(np.abs(truth).max()) if truth.size else 0.0
    return 1e-4 if m <= 100.0 else 4e-6 * m


def src_for(n, seed):
    """pool entries of n slots: seeded permutations of the pool, chained"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(M) for _ in range(n // M + 1)])[:n]


def Tn(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Ctx:
    """device state and the float64 truth / float32 oracle of the pool, per weight set (built on first use, then left unchanged)"""

    def __init__(self):
        from dsnerf_amd import _lib
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.lib, self.dev, self.G = _lib, torch.device("cuda:0"), groups()
        self.sets, self.bits = {}, {}
        g = load("full_eval")
        nt = np.nonzero(~g["transparent"])[0]
        rng = np.random.default_rng(2024)
        near = g["x_c"][nt[:2048]]
        shell = g["x_c"][nt[rng.integers(0, len(nt), 1024)]] + 0.2 * rng.standard_normal((1024, 3))
        far = rng.standard_normal((1024, 3)) * rng.uniform(1.0, 60.0, (1024, 1))
        self.x = np.ascontiguousarray(np.concatenate([near, shell, far]).astype(np.float32))
        assert self.x.shape == (M, 3) and len(np.unique(self.x, axis=0)) == M, "the pool's points are distinct"

    def set(self, tag):
        if tag in self.sets:
            return self.sets[tag]
        name = SETS[tag]
        g, sd = load(name), state(name)
        s = dict(g=g, sd=sd, P=O.Params(sd))
        s["packed"] = self.lib.PackedParams(self.dev).update({k: torch.from_numpy(v) for k, v in sd.items()})
        sc = self.lib.Scene(torch.from_numpy(g["canonical_vertex"]), torch.from_numpy(g["faces"].astype(np.int64)), self.dev)
        sc.set_frame(s["packed"], torch.from_numpy(g["xyz"]), torch.from_numpy(g["poses"]), int(g["frame"]))
        s["scene"] = sc
        # the field: truth and oracle on the pool
        s["sig"], s["ess"], s["grad"] = FR.field64(self.x, sd, g["poses"], int(g["frame"]))
        code = sd["nerf.embedding.weight"][int(g["frame"])]
        s["o_sig"], s["o_ess"], s["o_grad"] = O.field(self.x, s["P"], code, O.pose_feat(g["poses"], s["P"])[1])
        s["sig_bar"] = np.array([bar_of(s["sig"][BAND_OF == b]) for b in range(3)])
        s["ess_bar"] = np.array([bar_of(s["ess"][BAND_OF == b]) for b in range(3)])
        s["clear"] = np.abs(s["sig"]) > s["sig_bar"][BAND_OF]          # sigma64 clear of zero: its sign is the device's too
        for b in range(3):
            assert np.mean(~s["clear"][BAND_OF == b]) <= 0.01, (tag, BANDS[b], "more than 1 % of the band within the bar of sigma = 0")
        gn = np.maximum(np.linalg.norm(s["grad"], axis=-1), 1.0)
        s["gn"] = gn
        s["o_rel"] = np.linalg.norm(s["o_grad"].astype(np.float64) - s["grad"], axis=-1) / gn
        # the lighting MLP: pool entry j sits on golden row rows[j] (x_c, d sigma/dx and world point of a real sample: the normal
        # search of `shade` has real inputs); normal (dense `light` only), view direction and essence are drawn
        rng = np.random.default_rng(77)
        nt = np.nonzero(~g["transparent"])[0]
        rows = nt[np.arange(M) % len(nt)]
        unit = lambda a: (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)       # noqa: E731
        L = dict(x_c=g["x_c"][rows], grad=g["grad_sigma"][rows], x_w=g["pts"].reshape(-1, 3)[rows],
                 n=unit(rng.standard_normal((M, 3))), view=unit(rng.standard_normal((M, 3))), ess=rng.random((M, 3)).astype(np.float32))
        L = {k: np.ascontiguousarray(v, np.float32) for k, v in L.items()}
        v64 = L["view"].astype(np.float64)
        L["view64"] = v64 / np.linalg.norm(v64, axis=-1, keepdims=True)      # the kernels normalise the direction they are given
        L["col"], L["fac"] = FR.light64(L["n"], L["x_w"], L["view64"], L["ess"], sd)
        L["o_col"] = O.lighting(L["n"], L["x_w"], L["view"], L["ess"], s["P"])
        s["L"] = L
        self.sets[tag] = s
        return s

    def same_bits(self, key, src, arr):
        """slots whose bits differ from the pool table of `key` (filled by the first copy met); arr [n, ...] float32 / int32"""
        if len(src) == 0:
            return np.zeros(0, np.int64)
        a = np.ascontiguousarray(arr).view(np.int32).reshape(len(src), -1)
        if key not in self.bits:
            self.bits[key] = (np.zeros((M, a.shape[1]), np.int32), np.zeros(M, bool))
        tab, seen = self.bits[key]
        new = np.nonzero(~seen[src])[0]
        if len(new):
            u, first = np.unique(src[new], return_index=True)
            tab[u] = a[new[first]]
            seen[u] = True
        return np.nonzero((tab[src] != a).any(axis=1))[0]


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


def forms(count, seed):
    """(form, N, rows, src): dense - N = count, rows = all; listed - N = count + 3 T + 9 rows, a shuffled list of `count` of them.
    src [N]: the pool entry of every row (unlisted rows hold real points too)."""
    out = []
    if count > 0:
        out.append(("dense", count, np.arange(count), src_for(count, seed)))
    N = count + 3 * T + 9
    perm = np.random.default_rng(seed + 1).permutation(N)
    out.append(("listed", N, perm[:count], src_for(N, seed + 2)))
    return out


def active(ctx, N, rows):
    """the list as test_field_active_list builds it: [N] entries, the count in a device counter; the tail of the array names an
    UNLISTED row, so that an entry read past the count shows up as a row that should have kept its zeros"""
    lst = np.full(N, N - 1 if len(rows) == 0 else np.setdiff1d(np.arange(N), rows)[0], np.int32)
    lst[:len(rows)] = rows
    cnt = torch.zeros(64, dtype=torch.int32, device=ctx.dev)
    cnt[0] = len(rows)
    return Tn(lst, ctx.dev), cnt


def where(slots, src, rows, G):
    """readable position of the first few wrong slots: (slot, pool entry, band, tile, wave, loop round)"""
    return [dict(slot=int(i), row=int(rows[i]), pool=int(src[rows[i]]), band=BANDS[BAND_OF[src[rows[i]]]], tile=int(i // T),
                 wave=int(i % T // 32), round=int(i // T // G)) for i in slots[:6]]


def worst(figs, key, value, other):
    if key not in figs or value > figs[key][0]:
        figs[key] = (value, other)


# ORACLE_RULE.  "No further from float64 than 1.5 x the float32 oracle on the same points + 1e-5" compares the maxima of two error
# populations; test_field applies it to 12288 points.  On a handful of points it is not a property of a correct float32
# implementation: where one ulp of sigma is above 1e-5 (w4, w3: |sigma| ~ 1e3, ulp 6e-5) two independent float32 evaluations of one
# point differ by several ulps either way.  The REFERENCE's own float32 run (golden sigma of full_eval_w4 against field64, beside the
# oracle on the same points) misses the rule on 22 % of random subsets of 1 point, 10 % of 31, 9 % of 128, 0.5 % of 1024 and none of
# all 3597 (full_eval_w3: 34 %, 2 %, 0 %, 0 %, 0 %; full_eval: never, its ulp is below 1e-5); both exact-fp32 k_field and k_field16 missed
# it the same way at counts 1 .. 129 on w4 and at no larger count.  So the oracle's error is taken over the whole band of the POOL -
# the population every launch draws from, and, outputs being position-independent bit for bit (assertion 4), the set the device's
# errors over all launches come from: 7.3e-4 / 3.9e-4 / 3.0e-4 on w4's near / shell / far, the figures the bound is 1.5 x of.  A
# launch of 4096 points or more holds every pool point: there this IS the oracle on the same points.  The project's bar (first
# check) stays per launch.
def judge_field(s, tag, what, pool, sig, ess, grad, problems, figs, at):
    """assertions 1 and 2 on the evaluated slots (pool [n]: their pool entries)"""
    band = BAND_OF[pool]
    for b in range(3):
        m = band == b
        if not m.any():
            continue
        p = pool[m]
        for key, out, tru, orc, bars in (("sigma", sig, s["sig"], s["o_sig"], s["sig_bar"]), ("essence", ess, s["ess"], s["o_ess"], s["ess_bar"])):
            err = float(np.abs(out[m].astype(np.float64) - tru[p]).max())
            oerr = float(np.abs(orc.astype(np.float64) - tru)[BAND_OF == b].max())          # (the band of the POOL: see ORACLE_RULE)
            worst(figs, (tag, what, BANDS[b], key), err, oerr)
            if not err <= bars[b]:
                problems.append((at, BANDS[b], key, "error %.3g above the bar %.3g" % (err, bars[b])))
            if not err <= 1.5 * oerr + 1e-5:
                problems.append((at, BANDS[b], key, "error %.3g above 1.5 x the oracle's %.3g + 1e-5" % (err, oerr)))
        pos = m & (sig > 0) & (s["sig"][pool] > 0) & s["clear"][pool]
        if pos.any():
            q = pool[pos]
            rel = np.linalg.norm(grad[pos].astype(np.float64) - s["grad"][q], axis=-1) / s["gn"][q]
            med, share, oshare = float(np.median(rel)), float(np.mean(rel > 1e-4)), float(np.mean(s["o_rel"][q] > 1e-4))
            worst(figs, (tag, what, BANDS[b], "grad median"), med, float(np.median(s["o_rel"][q])))
            worst(figs, (tag, what, BANDS[b], "grad share"), share, oshare)
            if not med < 2e-6:
                problems.append((at, BANDS[b], "grad", "median rel %.3g (%d points)" % (med, int(pos.sum()))))
            if not share <= oshare + 2e-3:
                problems.append((at, BANDS[b], "grad", "share of rel > 1e-4: %.3g, the oracle's %.3g (%d points)" % (share, oshare, int(pos.sum()))))


def report(figs, problems):
    for k in sorted(figs):
        print("FIG", *k, "%.3g | %.3g" % figs[k])
    for p in problems:
        print("PROBLEM", *p)
    assert not problems, "%d problems, the first: %r" % (len(problems), problems[0])


def test_the_largest_count_walks_the_tile_loop(ctx):
    """the counts are built from the number of workgroups of THIS device: the largest one gives the busiest workgroup at least four
    tiles and the idlest at least three, 2 G T + T/2 + 5 at least three and two - on any number of compute units"""
    G = ctx.G
    c = counts(G)
    print("G =", G, "counts", c)
    assert c[8:11] == [G * T - 1, G * T, G * T + 1]
    busiest, idlest = tiles_per_group(c[-1], G)
    assert busiest >= 4 and idlest >= 3, (G, busiest, idlest)
    busiest, idlest = tiles_per_group(c[-2], G)
    assert busiest >= 3 and idlest >= 2, (G, busiest, idlest)
    assert tiles_per_group(G * T, G) == (1, 1) and tiles_per_group(G * T + 1, G) == (2, 1)
    assert c[-1] % T not in (0,) and c[-2] % T not in (0,)          # ragged last tiles, held by a workgroup on a later round


@pytest.mark.parametrize("fp32", [False, True], ids=["k_field16", "k_field"])
@pytest.mark.parametrize("tag", list(SETS))
def test_field_tiles(ctx, tag, fp32):
    """_lib.field: k_field16 in one launch (+ its exact-fp32 range fallback) / k_field - assertions 1, 2, 4, 5"""
    s, G = ctx.set(tag), ctx.G
    what = "k_field" if fp32 else "k_field16"
    problems, figs = [], {}
    for count in counts_of(tag, G):
        for form, N, rows, src in forms(count, 1000 + count % 997):
            at = "%s count %d" % (form, count)
            x = Tn(ctx.x[src], ctx.dev)
            act = active(ctx, N, rows) if form == "listed" else None
            out = [t.cpu().numpy() for t in ctx.lib.field(s["scene"], s["packed"], x, active=act, fp32=fp32)]
            torch.cuda.synchronize()
            un = np.ones(N, bool)
            un[rows] = False
            for k, o in zip(("sigma", "essence", "grad"), out):
                if un.any() and np.any(o[un].view(np.int32) != 0):
                    problems.append((at, "-", k, "rows off the list were written: %r" % np.nonzero(un & (o.reshape(N, -1).view(np.int32) != 0).any(1))[0][:6].tolist()))
                bad = ctx.same_bits((tag, what, k), src[rows], o[rows])
                if len(bad):
                    problems.append((at, "-", k, "%d slots differ from their pool point's bits elsewhere: %r" % (len(bad), where(bad, src, rows, G))))
            if count:
                judge_field(s, tag, what, src[rows], out[0][rows], out[1][rows], out[2][rows], problems, figs, at)
    report(figs, problems)


@pytest.mark.parametrize("tag", list(SETS))
def test_forward_reverse_tiles(ctx, tag):
    """_lib.field_forward + _lib.field_reverse (k_field16's forward and reverse modes, the sigma > 0 list in between) == the single
    launch, bit for bit, on every count - assertions 5 and 6 (1, 2, 4 follow: test_field_tiles judges the single launch's bits)"""
    s, G = ctx.set(tag), ctx.G
    problems = []
    for count in counts_of(tag, G):
        for form, N, rows, src in forms(count, 1000 + count % 997):
            at = "%s count %d" % (form, count)
            x = Tn(ctx.x[src], ctx.dev)
            act = active(ctx, N, rows) if form == "listed" else None
            d_sig, d_ess, d_gr = (t.cpu().numpy() for t in ctx.lib.field(s["scene"], s["packed"], x, active=act))
            sig, ess, rec, pos = ctx.lib.field_forward(s["scene"], s["packed"], x, active=act)
            gr = ctx.lib.field_reverse(s["scene"], s["packed"], x, rec, pos, sig, ess)
            torch.cuda.synchronize()
            sig, ess, gr = sig.cpu().numpy(), ess.cpu().numpy(), gr.cpu().numpy()
            n_pos, plist = int(pos[1][0]), pos[0].cpu().numpy()
            listed = np.zeros(N, bool)
            listed[rows] = True
            want = listed & (d_sig > 0)
            bits = lambda a: a.view(np.int32)       # noqa: E731
            for k, a, b in (("sigma", sig, d_sig), ("essence", ess, d_ess)):
                bad = np.nonzero((bits(a) != bits(b)).reshape(N, -1).any(1))[0]
                if len(bad):
                    problems.append((at, k, "%d rows differ from the single launch (rows off the list: %d): %r"
                                     % (len(bad), int((~listed[bad]).sum()), bad[:6].tolist())))
            bad = np.nonzero((bits(gr) != np.where(want[:, None], bits(d_gr), 0)).any(1))[0]
            if len(bad):
                problems.append((at, "grad", "%d rows differ from the single launch where sigma > 0 / from zero elsewhere: %r" % (len(bad), bad[:6].tolist())))
            if n_pos != int(want.sum()):
                problems.append((at, "pos", "count %d, %d listed points have sigma > 0" % (n_pos, int(want.sum()))))
            elif not np.array_equal(np.sort(plist[:n_pos]), np.nonzero(want)[0]):
                problems.append((at, "pos", "not the listed points with sigma > 0, each once"))
            if np.any(plist[max(n_pos, 0):] != 0):
                problems.append((at, "pos", "entries beyond the count were written"))
            if count == 0 and (n_pos != 0 or np.any(bits(sig) != 0) or np.any(bits(ess) != 0) or np.any(bits(gr) != 0)):
                problems.append((at, "-", "a count of 0 wrote something"))
    report({}, problems)


def judge_light(s, tag, what, truth, otruth, out, key, problems, figs, at, scale=None):
    """assertion 3: out, truth (float64), otruth (oracle) on the same slots"""
    err = float(np.abs(out.astype(np.float64) - truth).max())
    oerr = float(np.abs(otruth.astype(np.float64) - truth).max())
    bar = 1e-5 * max(1.0, float(np.abs(truth if scale is None else scale).max()))
    worst(figs, (tag, what, "-", key), err, oerr)
    if not err <= bar:
        problems.append((at, key, "error %.3g above the bar %.3g" % (err, bar)))
    if not err <= 1.5 * oerr + 1e-6:
        problems.append((at, key, "error %.3g above 1.5 x the oracle's %.3g + 1e-6" % (err, oerr)))


@pytest.mark.parametrize("fp32", [False, True], ids=["k_light16", "k_light"])
@pytest.mark.parametrize("tag", list(SETS))
def test_light_tiles(ctx, tag, fp32):
    """_lib.light, dense: k_light16 / k_light on drawn unit normals - assertions 3 and 4"""
    s, G = ctx.set(tag), ctx.G
    L = s["L"]
    what = "k_light" if fp32 else "k_light16"
    problems, figs = [], {}
    for count in counts_of(tag, G):
        if count == 0:
            continue          # (dsn_light takes N > 0; the empty list goes through `shade` below)
        src = src_for(count, 3000 + count % 997)
        at = "dense count %d" % count
        col = ctx.lib.light(s["packed"], *(Tn(L[k][src], ctx.dev) for k in ("n", "x_w", "view", "ess")), fp32=fp32).cpu().numpy()
        bad = ctx.same_bits((tag, what, "colour"), src, col)
        if len(bad):
            problems.append((at, "colour", "%d slots differ from their pool point's bits elsewhere: %r" % (len(bad), where(bad, src, np.arange(count), G))))
        judge_light(s, tag, what, L["col"][src], L["o_col"][src], col, "colour", problems, figs, at)
    report(figs, problems)


@pytest.mark.parametrize("factor", [False, True], ids=["k_light16", "k_light16_factor"])
@pytest.mark.parametrize("tag", list(SETS))
def test_shade_tiles(ctx, tag, factor):
    """_lib.shade through a list and dense (the normal search, then k_light16; want_factor: k_light16<true>, the factor ELU + 1 beside
    the colour) - assertions 3, 4, 5.  The colours are judged against light64 fed shade's OWN returned n_w, on the evaluated rows."""
    s, G = ctx.set(tag), ctx.G
    L = s["L"]
    what = "shade factor" if factor else "shade"
    problems, figs = [], {}
    one = np.ones((1, 3), np.float32)
    for count in counts_of(tag, G):
        for form, N, rows, src in forms(count, 5000 + count % 997):
            at = "%s count %d" % (form, count)
            act = active(ctx, N, rows) if form == "listed" else None
            a = [Tn(L[k][src], ctx.dev) for k in ("x_c", "grad", "x_w", "view", "ess")]
            out = [t.cpu().numpy() for t in ctx.lib.shade(s["scene"], s["packed"], *a, 1, active=act, want_factor=factor)]
            names = ("idx", "n_w", "colour", "factor")[:len(out)]
            un = np.ones(N, bool)
            un[rows] = False
            for k, o in zip(names, out):
                if un.any() and np.any(o[un].view(np.int32) != 0):
                    problems.append((at, k, "rows off the list were written: %r" % np.nonzero(un & (o.reshape(N, -1).view(np.int32) != 0).any(1))[0][:6].tolist()))
                # (the colour's bits are the same with and without the factor output: one table for both)
                bad = ctx.same_bits((tag, "shade", k), src[rows], o[rows])
                if len(bad):
                    problems.append((at, k, "%d slots differ from their pool point's bits elsewhere: %r" % (len(bad), where(bad, src, rows, G))))
            if count == 0:
                continue
            p = src[rows]
            n_w = out[1][rows]
            if not np.all(np.isfinite(n_w)):
                problems.append((at, "n_w", "not finite"))
                continue
            col64, fac64 = FR.light64(n_w, L["x_w"][p], L["view64"][p], L["ess"][p], s["sd"])
            judge_light(s, tag, what, col64, O.lighting(n_w, L["x_w"][p], L["view"][p], L["ess"][p], s["P"]), out[2][rows], "colour", problems, figs, at)
            if factor:
                o_fac = O.lighting(n_w, L["x_w"][p], L["view"][p], np.broadcast_to(one, (len(p), 3)), s["P"])[:, 0]
                judge_light(s, tag, what, fac64, o_fac, out[3][rows], "factor", problems, figs, at)
    report(figs, problems)


@pytest.mark.parametrize("tag", ["default", "w4"])
def test_screen_tiles(ctx, tag, monkeypatch):
    """the density screen's kernels (DSN_SCREEN_WAVES unset: k_screen16<8>, tiles of 256 points on G workgroups; 4: k_screen16<4>, 128
    points on 2 G workgroups; 2: k_screen16x2, 256 points on G) on the counts above for both tile sizes: every copy of a pool point
    holds the same sigma~ and S1, and the three variants agree bit for bit at every count (NaN bits included)"""
    s, G = ctx.set(tag), ctx.G
    problems = []
    both = sorted(set(counts(G, 256) + counts(2 * G, 128)) - {0})          # (dsn_debug_screen takes N > 0)
    for tile, g in ((256, G), (128, 2 * G)):
        busiest, idlest = tiles_per_group(both[-1], g, tile)
        assert busiest >= 4 and idlest >= 3, (tile, g, busiest, idlest)
    for count in both:
        src = src_for(count, 7000 + count % 997)
        x = Tn(ctx.x[src], ctx.dev)
        got = {}
        for waves in (None, "4", "2"):
            if waves is None:
                monkeypatch.delenv("DSN_SCREEN_WAVES", raising=False)
            else:
                monkeypatch.setenv("DSN_SCREEN_WAVES", waves)
            sg, s1 = ctx.lib.screen_debug(s["scene"], s["packed"], x)
            torch.cuda.synchronize()
            got[waves] = np.stack([sg.cpu().numpy(), s1.cpu().numpy()], 1)
        monkeypatch.delenv("DSN_SCREEN_WAVES", raising=False)
        bad = ctx.same_bits((tag, "screen", "sg s1"), src, got[None])
        if len(bad):
            problems.append(("count %d" % count, "%d slots differ from their pool point's bits elsewhere: %r" % (len(bad), bad[:6].tolist())))
        for waves in ("4", "2"):
            bad = np.nonzero((got[waves].view(np.int32) != got[None].view(np.int32)).any(1))[0]
            if len(bad):
                problems.append(("count %d" % count, "DSN_SCREEN_WAVES=%s differs from the default kernel on %d slots: %r" % (waves, len(bad), bad[:6].tolist())))
        if not float(np.nanmax(np.abs(got[None][:, 1]))) > 0:
            problems.append(("count %d" % count, "S1 is zero everywhere"))
    report({}, problems)
