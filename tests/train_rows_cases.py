"""TEST INFRASTRUCTURE: training batches whose two device-side row lists hold a CHOSEN number of rows (pure numpy / torch / oracle).

The training backward (csrc/dsn_train.hip, k_field16<train> / k_tangent16 / k_adjoint16) walks list1 - the rows the forward evaluates,
all but transparent samples whose noise is <= 0 - and list2 - the rows with a non-zero cotangent.  The number of rows in a list picks
the code path of every kernel (short prologues of the weight-gradient products, register-load tails, empty shares, the one- or
four-address staging), so the builders here fix those numbers:

  family A  module mode (dsn_module_grad): N explicit points, cotangents on a chosen support of B rows -> list2 holds exactly B
  family B  ray mode (dsn_render_rays_grad): all-transparent rays with noise +0.6 on exactly F samples, -1 elsewhere -> list1 holds F
  family C  degenerate batches: F = 0, B = 0, tiny (R, S)

The reference is oracle/train_oracle.py::render in float64 on the geometry of the float32 oracle warp; it is DENSE, a dead row adds an
exact zero to it.  The bar of a case comes from that reference alone (bar()): a tenth of what the float64 gradient moves when the
last listed row is made dead.  tests/test_train_rows_host.py checks the builders and the bars without a GPU,
tests/test_gpu_train_rows.py runs the cases on the device."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import oracle as O
import train_oracle as TO
from cases import load, rel, state

PARAM_SETS = ("full_train_grads", "full_train_grads_w4")      # default (hash-random) and converged parameters
S = 16                                                          # z_vals[:, ::4] of the S = 64 fixtures
A1_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
A2_N = 320
COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 96, 112, 127, 128, 129, 255, 256, 257)
SUPPORTS = ("prefix", "stride", "blocks")
PURE_RAYS, HIT_RAYS, MIXED_TRANSPARENT_RAYS = 64, 8, 32
MIXED_F = (128, 129, 144, 160, 176, 192, 193, 255, 256, 257)
TINY = ((1, 1), (1, 2), (3, 2), (1, 16), (1, 64))
HISTORY_COUNTS = (17, 80, 257)                                   # cases that also run behind a count-1 batch (stale list slots)
RENDERER_RAYS, RENDERER_F = 10, 80                               # the Renderer case: see renderer_case()
LIVE, DEAD, KILL = 0.6, -1.0, -1e30                              # noise of a live / dead transparent sample; what kills a non-transparent one
CEILING = 5e-3                                                   # the suite's fixed ceiling (test_backward_matches_oracle_all_cotangents)
OUT_KEYS = ("color", "acc_map", "depth_map", "weights")


# ---- the fixtures' geometry: one float32 oracle warp of the 128 x 16 samples, shared by every pool ---------------------------------
@functools.lru_cache(maxsize=None)
def fixture(name):
    return dict(load(name).items())


@functools.lru_cache(maxsize=None)
def geometry():
    """sample points of the fixtures' rays at z_vals[:, ::4] through the float32 oracle warp (both parameter sets share body, pose and
    rays: same_rays()) -> arrays per ray and sample"""
    g = fixture(PARAM_SETS[0])
    z = np.ascontiguousarray(g["render:z_vals"][:, ::4])
    geo = warp_samples(g, g["ray_o"], g["ray_d"], z)
    geo["z"] = z
    return geo


def warp_samples(g, o, d, z):
    R, s = z.shape
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).astype(np.float32)
    wp = O.warp(pts.reshape(-1, 3), None, g["xyz"], g["canonical_vertex"], g["faces"])
    cent = O.centroids(g["canonical_vertex"], g["faces"])
    idx = O.nearest_face(wp["x_c"], cent).astype(np.int64)
    return {"pts": pts, "x_c": wp["x_c"].reshape(R, s, 3), "transparent": wp["transparent"].reshape(R, s), "idx": idx.reshape(R, s)}


def same_rays():
    a, b = fixture(PARAM_SETS[0]), fixture(PARAM_SETS[1])
    return all(np.array_equal(a[k], b[k]) for k in ("ray_o", "ray_d", "render:z_vals", "xyz", "canonical_vertex", "faces", "poses", "frame"))


def pure_rays():
    """the first 64 rays whose 16 samples are all transparent"""
    return np.nonzero(geometry()["transparent"].all(1))[0][:PURE_RAYS]


def hit_rays():
    """the first 8 rays whose 16 samples are all non-transparent"""
    return np.nonzero((~geometry()["transparent"]).all(1))[0][:HIT_RAYS]


def mixed_rays():
    return np.concatenate([hit_rays(), pure_rays()[:MIXED_TRANSPARENT_RAYS]])


# ---- supports of family A ------------------------------------------------------------------------------------------------------------
def support(kind, B, N=A2_N):
    """B of N rows, ascending.  prefix: 0 .. B-1 (every four listed rows consecutive: the one-address DMA form).  stride: 0, 2, 4, ...
    (never four in a run: the four-address form); where 2 B > N - the counts 255 ... 257 - no such support exists in N rows, the
    N - B dead rows are then spread evenly, which still breaks most groups of four.  blocks: four consecutive rows, then four rows
    two apart, and again (the form changes from step to step); counts the pattern cannot hold in N rows take the rest from the top."""
    if kind == "prefix":
        rows = np.arange(B)
    elif kind == "stride":
        if 2 * B <= N:
            rows = 2 * np.arange(B)
        else:
            dead = np.floor((np.arange(N - B) + 0.5) * N / (N - B)).astype(np.int64)
            rows = np.setdiff1d(np.arange(N), dead)
    elif kind == "blocks":
        pat, r = [], 0
        while r < N:
            pat += [r, r + 1, r + 2, r + 3, r + 5, r + 7, r + 9, r + 11]
            r += 13
        pat = np.asarray([p for p in pat if p < N], np.int64)
        if B <= len(pat):
            rows = pat[:B]
        else:
            rest = np.setdiff1d(np.arange(N), pat)[::-1][:B - len(pat)]
            rows = np.sort(np.concatenate([pat, rest]))
    else:
        raise ValueError(kind)
    rows = np.asarray(rows, np.int64)
    assert len(rows) == B and len(np.unique(rows)) == B and (B == 0 or (rows[0] >= 0 and rows[-1] < N))
    return rows


def staging_forms(rows):
    """per full group of four LISTED rows (what one wave stages per step): True = consecutive (one address), False = four addresses"""
    rows = np.asarray(rows)
    n = len(rows) // 4
    return np.asarray([rows[4 * k + 3] - rows[4 * k] == 3 for k in range(n)], bool)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def module_points():
    """the first 320 non-transparent samples: world point, oracle canonical point, nearest canonical face, view direction - and their
    cotangents gc ~ N(0,1), gs ~ 0.1 N(0,1)"""
    g, geo = fixture(PARAM_SETS[0]), geometry()
    keep = np.nonzero(~geo["transparent"].reshape(-1))[0][:A2_N]
    assert len(keep) == A2_N
    view = np.repeat(g["ray_d"][:, None, :], S, 1).reshape(-1, 3)[keep]
    rng = np.random.default_rng(9)
    gc = rng.standard_normal((A2_N, 3)).astype(np.float32)
    gs = (rng.standard_normal(A2_N) * 0.1).astype(np.float32)
    return {"x_w": np.ascontiguousarray(geo["pts"].reshape(-1, 3)[keep]), "x_c": np.ascontiguousarray(geo["x_c"].reshape(-1, 3)[keep]),
            "idx": geo["idx"].reshape(-1)[keep], "view": np.ascontiguousarray(view), "gc": gc, "gs": gs}


def module_case(name, N, rows, label):
    """the first N points (beyond 320: the points again, module_fill), cotangents zeroed outside `rows`"""
    p = module_points()
    rows = np.asarray(rows, np.int64)
    sel = np.arange(N) % A2_N
    on = np.zeros(N, bool)
    on[rows] = True
    gc = np.where(on[:, None], p["gc"][sel], 0.0).astype(np.float32)
    gs = np.where(on, p["gs"][sel], 0.0).astype(np.float32)
    return SimpleNamespace(mode="module", name=name, label=label, N=N, sel=sel, rows=rows, gc=gc, gs=gs, backward=len(rows),
                           last=int(rows[-1]) if len(rows) else None, full=None, x_w=p["x_w"][sel], x_c=p["x_c"][sel], view=p["view"][sel])


def module_fill(name, N):
    """N explicit points with a cotangent on every one: behind it list2 holds all N row numbers of a batch of N samples"""
    return module_case(name, N, np.arange(N), f"module fill {name} N={N}")


def a1_case(name, N):
    return module_case(name, N, np.arange(N), f"A1 {name} N={N}")


def a2_case(name, B, kind):
    return module_case(name, A2_N, support(kind, B), f"A2 {name} B={B} {kind}")


def fill_order(R, s=S):
    """flat sample indices in the order the live noise is handed out: the first four samples of ray 0, of ray 1, ... and, once every
    ray has four, samples 4 .. 7 of ray 0 and so on"""
    return np.asarray([r * s + 4 * b + j for b in range(s // 4) for r in range(R) for j in range(4)], np.int64)


def ray_cotangents(R, s, seed=4):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal(shape).astype(np.float32) for k, shape in
            (("color", (R, 3)), ("disp_map", (R,)), ("acc_map", (R,)), ("depth_map", (R,)), ("weights", (R, s)))}


def ray_case(name, rays, F_extra, label, zero_rays=(), noise_free=False, disp=False, hit_scale=1.0, prepared=True):
    """rays of the fixture (indices) at S = 16; noise 0 on non-transparent samples, +0.6 on the first F_extra transparent samples in
    fill_order() over the all-transparent rays, -1 on the others.  Cotangents on every output but disparity (disp=True: on the hit
    rays, where the oracle's acc > 1e-3: reference()); the rays in zero_rays carry exactly zero cotangents"""
    geo = geometry()
    rays = np.asarray(rays, np.int64)
    R = len(rays)
    tr = geo["transparent"][rays]
    noise = None
    if not noise_free:
        noise = np.where(tr, np.float32(DEAD), np.float32(0.0)).astype(np.float32)
        tr_rays = np.nonzero(tr.all(1))[0]
        order = fill_order(len(tr_rays))[:F_extra]
        flat = noise.reshape(R, S)
        for k in order:
            flat[tr_rays[k // S], k % S] = LIVE
    cot = ray_cotangents(R, S)
    if not disp:
        cot["disp_map"] = None
    else:
        cot["disp_map"] = np.where((~tr).all(1), cot["disp_map"] * np.float32(1e-2), 0.0).astype(np.float32)
    if hit_scale != 1.0:
        for k in cot:
            if cot[k] is not None:
                cot[k][(~tr).all(1)] *= np.float32(hit_scale)
    for r in zero_rays:
        for k in cot:
            if cot[k] is not None:
                cot[k][r] = 0.0
    c = SimpleNamespace(mode="rays", name=name, label=label, g=fixture(name), o=np.ascontiguousarray(fixture(name)["ray_o"][rays]),
                        d=np.ascontiguousarray(fixture(name)["ray_d"][rays]), z=np.ascontiguousarray(geo["z"][rays]), R=R, S=S, N=R * S,
                        x_c=geo["x_c"][rays].reshape(-1, 3), transparent=tr.reshape(-1), idx=geo["idx"][rays].reshape(-1), noise=noise,
                        cot=cot, disp_ok=None, zero_rays=tuple(zero_rays))
    finish_ray_case(c)
    return prepare(c) if prepared else c


def prepare(c):
    """finishes a ray-mode case with ONE float64 run of the dense oracle, inside the builder, so that nothing about a case depends on
    what a test does first: c.disp_ok / c.cot["disp_map"] (the disparity cotangent only on rays whose oracle acc > 1e-3), c.cot_rows /
    c.backward (list2 by the oracle), c.last (the row the bar is measured on) and c.full (the float64 gradient itself)"""
    c.disp_ok, c.cot_rows, c.backward, c.last, c.full = None, None, None, None, None
    c.cot = {k: (None if v is None else v.copy()) for k, v in c.cot.items()}
    c.full = _ray_oracle(c, np.arange(c.R), c.noise, torch.float64, preparing=True)
    assert c.cot_rows is not None
    return c


def finish_ray_case(c):
    """the forward count by the oracle's own flags (the backward's rows and the last listed row: prepare())"""
    live = live_rows(c)
    c.forward = int(live.sum())
    carrying = np.ones(c.R, bool)
    carrying[list(c.zero_rays)] = False
    c.live_with_cotangent = int((live.reshape(c.R, c.S) & carrying[:, None]).sum())
    c.cot_rows, c.backward, c.last, c.full = None, None, None, None


def live_rows(c):
    """the forward's rule by the oracle's flags: everything except transparent samples whose noise is <= 0"""
    return (~c.transparent) | ((c.noise.reshape(-1) > 0) if c.noise is not None else False)


def pure_case(name, F, **kw):
    return ray_case(name, pure_rays(), F, kw.pop("label", f"B pure {name} F={F}"), **kw)


def mixed_case(name, F, **kw):
    return ray_case(name, mixed_rays(), F - HIT_RAYS * S, kw.pop("label", f"B mixed {name} F={F}"), disp=True,
                    hit_scale=kw.pop("hit_scale", None) or mixed_hit_scale(name), **kw)


@functools.lru_cache(maxsize=None)
def mixed_hit_scale(name):
    """what the cotangents of the mixed pool's 8 hit rays are multiplied with.  With unit cotangents everywhere the 128 hit rows own
    the gradient - converged parameters: |sigma| ~ 1e3, |d sigma/dx| ~ 2e5 against an alpha of 0.6 x a sample distance on a
    transparent row - and a transparent row, the last listed one among them, then moves the sum by 4e-5: less than the float32
    oracle differs from the float64 one, so no bar could tell a dropped row from rounding.  The hit rays' cotangents are therefore
    scaled until both halves of the pool weigh the same in the float64 oracle: the power of two next to the ratio of the two halves'
    gradient norms (median over the tensors) at F = 256, unit cotangents.  From the reference alone, one number per parameter set"""
    c = ray_case(name, mixed_rays(), MIXED_TRANSPARENT_RAYS * 4, "mixed pool, unit cotangents", disp=True, prepared=False)
    c.disp_ok = np.zeros(c.R, bool)
    c.cot_rows = np.zeros(c.N, bool)        # (nothing of this probe is a case)
    hit = norms(_ray_oracle(c, np.arange(HIT_RAYS), c.noise, torch.float64))
    rest = norms(_ray_oracle(c, np.arange(HIT_RAYS, c.R), c.noise, torch.float64))
    ratio = float(np.median([rest[k] / hit[k] for k in hit if hit[k] > 0 and rest[k] > 0]))
    return float(min(1.0, 2.0 ** round(np.log2(ratio))))


def zero_cotangent_case(name):
    return mixed_case(name, 256, zero_rays=tuple(range(1, HIT_RAYS + MIXED_TRANSPARENT_RAYS, 2)), label=f"B zero-cotangent rays {name} F=256")


def with_zero_cotangents(c):
    """the same batch with every cotangent exactly zero (B = 0)"""
    z = SimpleNamespace(**vars(c))
    z.label = c.label + " all cotangents zero"
    if c.mode == "module":
        z.gc, z.gs, z.rows, z.backward, z.last, z.full = np.zeros_like(c.gc), np.zeros_like(c.gs), np.zeros(0, np.int64), 0, None, None
    else:
        z.cot = {k: (None if v is None else np.zeros_like(v)) for k, v in c.cot.items()}
        z.zero_rays = tuple(range(c.R))
        finish_ray_case(z)
        prepare(z)
    return z


def tiny_case(name, R, s):
    """R hit rays x s samples taken evenly from the fixture's 64, all cotangents (disparity where the oracle's acc > 1e-3), no noise;
    its geometry is a warp of its own.  S = 1 and S = 2: the evenly spaced columns (32; 16 and 48) moved on by the smallest number of
    columns - then, where no shift will do, 4 columns closer together - at which every sample has a positive density in the float64 oracle - a sample with sigma <= 0 has alpha = 0, and a
    batch of them has no gradient at all (default parameters at 16 / 48)"""
    g = fixture(name)
    rays = hit_rays()[:R]
    o, d = np.ascontiguousarray(g["ray_o"][rays]), np.ascontiguousarray(g["ray_d"][rays])
    cols = np.arange(64) if s == 64 else (np.arange(s) * (64 // s) + (64 // s) // 2 if s < 16 else np.arange(0, 64, 4))
    if s < 16:
        cols = _tiny_columns(name, tuple(int(r) for r in rays), tuple(int(k) for k in cols))
    z = np.ascontiguousarray(g["render:z_vals"][rays][:, cols])
    geo = warp_samples(g, o, d, z)
    cot = ray_cotangents(R, s, seed=5)
    cot["disp_map"] = (cot["disp_map"] * np.float32(1e-2)).astype(np.float32)
    c = SimpleNamespace(mode="rays", name=name, label=f"C tiny {name} R={R} S={s}", g=g, o=o, d=d, z=z, R=R, S=s, N=R * s,
                        x_c=geo["x_c"].reshape(-1, 3), transparent=geo["transparent"].reshape(-1), idx=geo["idx"].reshape(-1), noise=None,
                        cot=cot, disp_ok=None, zero_rays=())
    finish_ray_case(c)
    return prepare(c)


@functools.lru_cache(maxsize=None)
def _tiny_columns(name, rays, cols):
    g = fixture(name)
    rays = np.asarray(rays)
    o, d = np.ascontiguousarray(g["ray_o"][rays]), np.ascontiguousarray(g["ray_d"][rays])
    z = np.ascontiguousarray(g["render:z_vals"][rays])
    geo = warp_samples(g, o, d, z)
    params = oracle_params(name, torch.float64)
    geom = {"x_c": torch.from_numpy(geo["x_c"].reshape(-1, 3)), "transparent": torch.from_numpy(geo["transparent"].reshape(-1)),
            "idx_canon": torch.from_numpy(geo["idx"].reshape(-1))}
    gg = dict(g)
    gg["ray_o"], gg["ray_d"] = o, d
    sig = TO.render(params, gg, jitter_z=z, geom=geom, dtype=torch.float64)["sigma"].detach().numpy().reshape(len(rays), 64)
    n = len(cols)
    gap0 = 64 // n
    for gap in range(gap0, 0, -4):                       # (closer together where no shift of the even spacing will do)
        for first in list(range(cols[0], 64 - gap * (n - 1))) + list(range(cols[0])):
            pick = first + gap * np.arange(n)
            if pick[-1] < 64 and (sig[:, pick] > 0).all():
                return pick
    raise AssertionError("no columns with a positive density on every ray")


def all_live(c):
    """the batch that runs on a workspace in front of a case: same pool / same N, every row live, every cotangent non-zero.  In
    module mode and on the all-transparent rays it fills both lists.  On hit rays it fills list1 only - the transmittance underflows
    along a hit ray, and the samples behind carry an exactly zero cotangent - so the tests run module_fill(name, N) behind it, which
    fills list2 of a batch of the same N"""
    if c.mode == "module":
        return module_fill(c.name, c.N)
    p = SimpleNamespace(**vars(c))
    p.label = c.label + " (all live)"
    p.noise = np.full((c.R, c.S), LIVE, np.float32)
    p.cot = ray_cotangents(c.R, c.S, seed=6)
    p.cot["disp_map"] = None
    p.zero_rays = ()
    finish_ray_case(p)
    p.full = None               # (a history batch: never compared, never prepared)
    return p


@functools.lru_cache(maxsize=None)
def renderer_seed(name):
    """the seed at which the Renderer case holds RENDERER_F live rows (renderer_case)"""
    g = fixture(name)
    rays = pure_rays()[:RENDERER_RAYS]
    for seed in range(4000):
        torch.manual_seed(seed)
        torch.rand(1, RENDERER_RAYS, S)
        if int((torch.randn(RENDERER_RAYS, S) > 0).sum()) != RENDERER_F:
            continue
        c = renderer_case_from_draw(name, rays, seed, 1.0, prepared=False)
        if c.forward == RENDERER_F:
            return seed
    raise AssertionError("no seed gives the chosen row count")


def renderer_draw(seed, R, noise_std):
    """what Renderer._draws takes from the seeded CPU generator: the sampler's jitter, then the density noise"""
    torch.manual_seed(seed)
    jitter = torch.rand(1, R, S).numpy()[0]
    noise = (torch.randn(R, S) * noise_std).numpy() if noise_std > 0 else None
    return jitter, noise


def renderer_case_from_draw(name, rays, seed, noise_std, z=None, prepared=True, noise=None):
    """the batch Renderer.render(...) evaluates in train mode for these rays after torch.manual_seed(seed): z_vals from the oracle's
    sampler (bit-exact against the device's; z: what the renderer returned, when it is at hand), the noise the renderer drew"""
    g = fixture(name)
    o, d = np.ascontiguousarray(g["ray_o"][rays]), np.ascontiguousarray(g["ray_d"][rays])
    R = len(rays)
    jitter, drawn = renderer_draw(seed, R, noise_std)
    noise = drawn if noise is None else noise          # (noise: what the renderer handed to its forward, when it is at hand)
    if z is None:
        z = O.sample_gg(o, d, g["near"][rays], g["far"][rays], g["xyz"], S, jitter, torch.linspace(0.0, 1.0, steps=S).numpy())["z_vals"]
    geo = warp_samples(g, o, d, z)
    cot = ray_cotangents(R, S, seed=8)
    cot["disp_map"] = None
    c = SimpleNamespace(mode="rays", name=name, label=f"B renderer {name} seed={seed} std={noise_std}", g=g, o=o, d=d, z=np.ascontiguousarray(z),
                        R=R, S=S, N=R * S, x_c=geo["x_c"].reshape(-1, 3), transparent=geo["transparent"].reshape(-1),
                        idx=geo["idx"].reshape(-1), noise=noise, cot=cot, disp_ok=None, zero_rays=(), rays=rays, seed=seed)
    finish_ray_case(c)
    return prepare(c) if prepared else c


def renderer_case(name, F, z=None, noise=None):
    """Renderer.render in train mode draws its own noise, N(0,1) per sample, so half of a batch's transparent samples are live: the
    case is the first RENDERER_RAYS = 10 rays of the pure pool (160 samples) at the first seed whose draw leaves exactly F = 80 of
    them live (renderer_seed); F = 0 is the same batch at raw_noise_std = 0 (no noise is drawn)"""
    rays = pure_rays()[:RENDERER_RAYS]
    if F == 0:
        return renderer_case_from_draw(name, rays, 0, 0.0, z)
    assert F == RENDERER_F
    return renderer_case_from_draw(name, rays, renderer_seed(name), 1.0, z, noise=noise)


def forward_f0_batch(name):
    """the 64 pure-pool rays as the training FORWARD takes them (origins, directions, near / far; it samples z itself): z by the
    oracle's sampler without jitter, and the oracle's flags of those samples - all transparent, so with noise = None or noise <= 0
    list1 is empty and colour, acc and weights are exactly zero"""
    g = fixture(name)
    rays = pure_rays()
    o, d = np.ascontiguousarray(g["ray_o"][rays]), np.ascontiguousarray(g["ray_d"][rays])
    near, far = np.ascontiguousarray(g["near"][rays]), np.ascontiguousarray(g["far"][rays])
    z = O.sample_gg(o, d, near, far, g["xyz"], S, None, torch.linspace(0.0, 1.0, steps=S).numpy())["z_vals"]
    return SimpleNamespace(name=name, o=o, d=d, near=near, far=far, z=z, R=len(rays), S=S,
                           transparent=warp_samples(g, o, d, z)["transparent"], dead_noise=np.full((len(rays), S), DEAD, np.float32))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def oracle_params(name, dtype):
    """the parameters as oracle.train_oracle.loss_and_grads takes them: float64 everywhere but the pose MLP, whose input the
    reference builds in float32"""
    return {k: torch.from_numpy(np.array(v)).to(dtype if not k.startswith("pose_mlp") else torch.float32).requires_grad_(True)
            for k, v in state(name).items()}


def _grads(params):
    return {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().numpy() for k, p in params.items()}


def _module_oracle(name, sel, gc, gs, dtype):
    p = module_points()
    sel = np.asarray(sel)
    n = len(sel)
    params = oracle_params(name, dtype)
    geom = {"x_c": torch.from_numpy(p["x_c"][sel]), "transparent": torch.zeros(n, dtype=torch.bool), "idx_canon": torch.from_numpy(p["idx"][sel])}
    gg = dict(fixture(name))
    gg["ray_o"], gg["ray_d"] = p["x_w"][sel], p["view"][sel]
    out = TO.render(params, gg, jitter_z=np.zeros((n, 1), np.float32), geom=geom, dtype=dtype)
    L = (torch.from_numpy(gc).to(dtype) * out["colour"]).sum() + (torch.from_numpy(gs).to(dtype) * out["sigma"]).sum()
    L.backward()
    return _grads(params)


def _ray_oracle(c, rays, noise, dtype, want_out=False, preparing=False):
    """sum(cotangent * output) over the rays `rays` (indices into the case) -> gradients (, outputs).  c.disp_ok - the rays whose
    disparity carries a cotangent - is fixed by the first float64 run of the whole case"""
    rays = np.asarray(rays, np.int64)
    rows = (rays[:, None] * c.S + np.arange(c.S)[None, :]).reshape(-1)
    params = oracle_params(c.name, dtype)
    geom = {"x_c": torch.from_numpy(np.ascontiguousarray(c.x_c[rows])), "transparent": torch.from_numpy(np.ascontiguousarray(c.transparent[rows])),
            "idx_canon": torch.from_numpy(np.ascontiguousarray(c.idx[rows]))}
    gg = dict(c.g)
    gg["ray_o"], gg["ray_d"] = c.o[rays], c.d[rays]
    out = TO.render(params, gg, jitter_z=c.z[rays], noise=None if noise is None else noise.reshape(c.R, c.S)[rays], geom=geom, dtype=dtype)
    out["sigma"].retain_grad()
    out["colour"].retain_grad()
    L = sum((torch.from_numpy(c.cot[k][rays]).to(dtype) * out[k]).sum() for k in OUT_KEYS)
    if c.cot["disp_map"] is not None:
        if c.disp_ok is None:
            assert preparing and len(rays) == c.R and dtype == torch.float64, "prepare(c) comes first (the builders call it)"
            c.disp_ok = (out["acc_map"].detach().numpy() > 1e-3) & (c.cot["disp_map"] != 0)
            c.cot["disp_map"] = np.where(c.disp_ok, c.cot["disp_map"], 0.0).astype(np.float32)
        ok = torch.from_numpy(c.disp_ok[rays])
        if bool(ok.any()):
            L = L + (torch.from_numpy(c.cot["disp_map"][rays]).to(dtype)[ok] * out["disp_map"][ok]).sum()
    L.backward()
    g = _grads(params)
    if preparing:
        # list2 by the oracle: the samples whose (colour, density) cotangent of the compositing adjoint is not all zero
        ds = out["sigma"].grad
        dc = out["colour"].grad
        on = (torch.zeros(c.N, dtype=torch.bool) if ds is None else ds != 0) | (torch.zeros(c.N, dtype=torch.bool) if dc is None else (dc != 0).any(-1))
        c.cot_rows = on.numpy()
        c.backward = int(c.cot_rows.sum())
        c.last = None
        c.true_last = int(np.nonzero(c.cot_rows)[0][-1]) if c.backward else None      # the oracle's last listed row, whatever it weighs
        if c.backward:
            # The last listed row THAT CARRIES WEIGHT.  On a hit ray the transmittance falls by many orders of magnitude along the
            # ray (converged parameters: to 1e-42 and below), so the oracle's last row with a non-zero cotangent can be one whose
            # removal moves nothing float32 could see; a bar derived from it would be zero.  Each row's cotangent is scored against
            # the batch's largest (density and colour apart); the row taken is the last one within two orders of magnitude of the
            # largest.  On the all-transparent rays every filled sample scores alike and this IS the last listed row.
            sc_s = torch.zeros(c.N, dtype=torch.float64) if ds is None else ds.abs().double()
            sc_c = torch.zeros(c.N, dtype=torch.float64) if dc is None else dc.norm(dim=-1).double()
            score = torch.maximum(sc_s / sc_s.max().clamp_min(1e-300), sc_c / sc_c.max().clamp_min(1e-300)).numpy()
            ok = c.cot_rows & (score >= 1e-2 * score.max())
            c.last = int(np.nonzero(ok)[0][-1])
    return (g, {k: out[k].detach().numpy() for k in OUT_KEYS}) if want_out else g


def reference(c, dtype=torch.float64, want_out=False):
    """the dense oracle's gradient of the case: {tensor: float64 array}"""
    if dtype == torch.float64 and not want_out and c.full is not None:
        return c.full
    if c.mode == "module":
        g = _module_oracle(c.name, c.sel, c.gc, c.gs, dtype)
        if dtype == torch.float64:
            c.full = g
        return g
    return _ray_oracle(c, np.arange(c.R), c.noise, dtype, want_out)


@functools.lru_cache(maxsize=None)
def _module_row(name, row):
    p = module_points()
    return _module_oracle(name, np.asarray([row]), p["gc"][row:row + 1], p["gs"][row:row + 1], torch.float64)


def row_change(c, row):
    """{tensor: float64 array}: what the float64 oracle's gradient loses when listed row `row` is made dead - module mode: its
    cotangents zeroed; ray mode: its noise set to -1 (a non-transparent sample: to -1e30, alpha = 0 exactly).  The oracle's loss is a
    sum over points (module mode) / over rays (ray mode), so the change is that point's / that ray's own"""
    if c.mode == "module":
        return _module_row(c.name, int(row))
    ray = int(row) // c.S
    noise = np.zeros((c.R, c.S), np.float32) if c.noise is None else c.noise.copy().reshape(c.R, c.S)
    dead = noise.copy()
    dead.reshape(-1)[row] = DEAD if c.transparent[row] else KILL
    a = _ray_oracle(c, [ray], None if c.noise is None else noise, torch.float64)
    b = _ray_oracle(c, [ray], dead, torch.float64)
    return {k: a[k] - b[k] for k in a}


def norms(g):
    return {k: float(np.linalg.norm(v.reshape(-1))) for k, v in g.items()}


def delta(c, full, row=None):
    """{tensor with a non-zero oracle gradient: relative L2 change of it when `row` (default: the last listed row) is made dead}"""
    row = c.last if row is None else row
    ch, n = norms(row_change(c, row)), norms(full)
    return {k: ch[k] / n[k] for k in n if n[k] > 0.0}


def bar(c, full):
    """(bar, median delta).  Dropping, duplicating or mis-reading one row moves nearly every tensor by about delta: a tenth of its
    median over the tensors fails on a tenth of a row.  A batch without a listed row has no gradient: every tensor is exactly zero"""
    if c.last is None:
        return 0.0, 0.0
    d = delta(c, full)
    med = float(np.median(list(d.values()))) if d else 0.0
    return 0.1 * med, med


def errors(got, full):
    """{tensor: cases.rel against the oracle} - and the tensors the oracle leaves exactly zero where `got` does not"""
    err, nonzero = {}, []
    for k, w in full.items():
        a = np.asarray(got[k], np.float64).reshape(-1)
        if not np.any(w):
            if np.any(a):
                nonzero.append((k, float(np.abs(a).max())))
            continue
        err[k] = rel(a, w)
    return err, nonzero


# ---- the list of cases both test modules walk ----------------------------------------------------------------------------------------
def all_cases():
    """[(id, family, builder)]: builders are called inside the tests (every one is cheap; the geometry behind them is cached)"""
    out = []
    for name in PARAM_SETS:
        tag = "w4" if name.endswith("_w4") else "default"
        for N in A1_N:
            out.append((f"A1-{tag}-N{N}", "A", functools.partial(a1_case, name, N)))
        for kind in SUPPORTS:
            for B in COUNTS:
                out.append((f"A2-{tag}-{kind}-B{B}", "A", functools.partial(a2_case, name, B, kind)))
        for F in COUNTS:
            out.append((f"B-pure-{tag}-F{F}", "B", functools.partial(pure_case, name, F)))
        for F in MIXED_F:
            out.append((f"B-mixed-{tag}-F{F}", "B", functools.partial(mixed_case, name, F)))
        out.append((f"B-zerocot-{tag}", "B", functools.partial(zero_cotangent_case, name)))
        out.append((f"C-F0-nonoise-{tag}", "C", functools.partial(pure_case, name, 0, noise_free=True, label=f"C pure {name} F=0 noise=None")))
        out.append((f"C-F0-deadnoise-{tag}", "C", functools.partial(pure_case, name, 0, label=f"C pure {name} F=0 noise<=0")))
        out.append((f"C-B0-module-{tag}", "C", lambda name=name: with_zero_cotangents(a1_case(name, A2_N))))
        out.append((f"C-B0-rays-{tag}", "C", lambda name=name: with_zero_cotangents(pure_case(name, 64))))
        for R, s in TINY:
            out.append((f"C-tiny-{tag}-R{R}-S{s}", "C", functools.partial(tiny_case, name, R, s)))
    return out


def listed_rows(c):
    """the rows of the backward's list by the oracle (ray mode: after reference())"""
    return c.rows if c.mode == "module" else np.nonzero(c.cot_rows)[0]


def row_weight(c, full, row):
    d = delta(c, full, row)
    return float(np.median(list(d.values()))) if d else 0.0
