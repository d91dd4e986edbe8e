"""dsn_adam_step's rule without a GPU: the float32 restatement (tests/adam_restate.py) against its float64 twin at derived bars, against
torch.optim.Adam on the CPU over 50 steps of a fixed quadratic problem with the model's 33 shapes, the state_dict round trips
between dsnerf_amd.optim.Adam's layout and torch's, the library's host scalars and its argument checks.

    python tests/test_adam_host.py --record      rewrites tests/golden/adam_errors.json (the distances test 2 measures)
"""
import copy
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import adam_restate as AR
from helpers import GOLDEN

ERRORS = os.path.join(GOLDEN, "adam_errors.json")
BETAS, EPS = (0.9, 0.999), 1e-8
STEPS = 50
MARGIN = 2.0          # both are float32 implementations of one formula that round differently
NAMES = None


def names():
    global NAMES
    if NAMES is None:
        import dsnerf_amd
        NAMES = list(dsnerf_amd._lib.PARAM_ORDER)
    return NAMES


# ---- 1. float32 against float64, one step ---------------------------------------------------------------------------------------
def bars(p, g, m, v, s, x):
    """Absolute error bars of one float32 step against the float64 twin from identical float32 state, u = 2^-24, first order in u
    with the last unit of each count paying for the higher orders.  s: the double scalars, x: the twin's intermediates.
    G = |g| + wd |p| bounds |g'|.
      g'  three roundings (wd, wd p, the sum), each relative to at most G:                      |dg'| <= 3 u G        (0 without decay)
      m'  = m + w1 (g' - m) cancels, so the bar is relative to M = |m| + G, which bounds |g' - m|, w1 |g' - m| and |m'|: the three
          roundings of g', then g' - m, w1, the product and the sum - 7 roundings, each at most u M:   |dm'| <= 8 u M
      v'  = b2 v + w2 g' g' has no cancellation; with V = b2 v + w2 G^2 >= v': the roundings of g' count twice in the square (6), then
          the square, w2, the product (3 more on the w2 G^2 part), b2 and its product (2 on the b2 v part), the sum (1 on v'):
          |dv'| <= 10 u V, with the spare unit                                                      |dv'| <= 11 u V
      p'  = p - ss q, q = m' / D, D = sqrt(v') / c2 + eps.  sqrt is 1/2-Lipschitz in relative terms and |sqrt a - sqrt b| =
          |a - b| / (sqrt a + sqrt b) <= |dv'| / sqrt(v') (taken as 0 where dv' = 0); then sqrt, c2, the division, eps and the sum round
          once each, every one relative to at most D:      |dD| <= |dv'| / (c2 sqrt(v')) + 5 u D, spare unit: 6 u D
          |dq| <= |dm'| / D + |q| |dD| / D + u |q| (the division);  ss and the product: 2 u ss |q|;  the difference: u |p'|:
          |dp'| <= ss (|dm'| / D + |q| |dD| / D + 3 u |q|) + u |p'|, and one more u (ss |q| + |p'|) for the higher orders.
    Derived, not tuned: nothing here was read off a result."""
    u = AR.U
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    G, D, q = x["G"], x["den"], np.abs(x["q"])
    M = np.abs(m) + G
    bm = 8 * u * M
    V = s["b2"] * v + s["w2"] * G * G
    bv = 11 * u * V
    with np.errstate(all="ignore"):
        droot = np.where(bv > 0, bv / x["root"], 0.0)
        dD = droot / s["c2"] + 6 * u * D
        p1 = p - s["ss"] * x["q"]
        bp = s["ss"] * (bm / D + q * dD / D + 3 * u * q) + u * np.abs(p1) + u * (s["ss"] * q + np.abs(p1))
    return bp, bm, bv


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_float32_step_within_derived_bars_of_float64(wd, t):
    """the bars: see bars() - derived from the number of roundings on each output's path, relative to the magnitudes that enter"""
    rng = np.random.RandomState(11 + t)
    n = 20000
    p = rng.randn(n).astype(np.float32)
    g = (rng.randn(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
    m = (g * rng.uniform(0.5, 1.5, n) * (rng.rand(n) < 0.8)).astype(np.float32) if t > 1 else np.zeros(n, np.float32)     # near-cancelling g' - m
    v = ((g.astype(np.float64) ** 2) * rng.uniform(0.0, 2.0, n)).astype(np.float32) if t > 1 else np.zeros(n, np.float32)
    g[:50] = 0.0                                                                                                          # g = 0 (v = 0 at t = 1)
    for lr in (5e-4, 0.0):
        p1, m1, v1 = AR.step32(p, g, m, v, AR.scalars(lr, wd, BETAS, EPS, t))
        s64 = AR.scalars64(lr, wd, BETAS, EPS, t)
        q1, n1, w1, x = AR.step64(p, g, m, v, s64)
        bp, bm, bv = bars(p, g, m, v, s64, x)
        for name, got, want, bar in (("m", m1, n1, bm), ("v", v1, w1, bv), ("p", p1, q1, bp)):
            err = np.abs(got.astype(np.float64) - want)
            worst = float(np.max(err / np.where(bar > 0, bar, 1.0)))
            print(f"t {t} wd {wd} lr {lr} {name}': largest error / bar = {worst:.3f}")
            assert np.all(err <= bar), (name, t, wd, lr, float(err.max()))
        if lr == 0.0:
            assert np.array_equal(p1.view(np.uint32), p.view(np.uint32))          # the frozen group: p keeps its bits


# ---- 2. against torch.optim.Adam over 50 steps ----------------------------------------------------------------------------------
def problem():
    """loss = 1/2 sum a (p - c)^2 per tensor: the gradient a (p - c), two rounded float32 operations in numpy and torch alike"""
    rng = np.random.RandomState(5)
    out = []
    for shape in AR.SHAPES:
        fan = shape[-1] if len(shape) > 1 else 16
        p0 = (rng.randn(*shape) / np.sqrt(fan)).astype(np.float32)
        a = (10.0 ** rng.uniform(-2, 1, shape)).astype(np.float32)
        c = (rng.randn(*shape) / np.sqrt(fan)).astype(np.float32)
        out.append((p0, a, c))
    return out


CASES = {"plain": dict(wd=0.0), "decay": dict(wd=0.01), "two_groups": dict(wd=0.0, frozen=range(0, 9)),
         "lambda_lr": dict(wd=0.01, sched=(10.0, 30.0, 45.0, 0.1))}
BASE_LR = 5e-4


def lr_of(case, i, k):
    cfg = CASES[case]
    if i in cfg.get("frozen", ()):
        return 0.0
    return BASE_LR * (AR.schedule(*cfg["sched"])(k) if "sched" in cfg else 1.0)


def run_restatement(case, prob=None, steps=STEPS):
    prob = prob or problem()
    wd = CASES[case]["wd"]
    state = [[p0.copy(), np.zeros_like(p0), np.zeros_like(p0)] for p0, _, _ in prob]
    for k in range(steps):
        for i, (st, (_, a, c)) in enumerate(zip(state, prob)):
            g = a * (st[0] - c)
            st[0], st[1], st[2] = AR.step32(st[0], g, st[1], st[2], AR.scalars(lr_of(case, i, k), wd, BETAS, EPS, k + 1))
    return state


def torch_optimizer(case, params, cls=torch.optim.Adam, **kw):
    cfg = CASES[case]
    if "frozen" in cfg:
        groups = [{"params": [params[i] for i in cfg["frozen"]], "lr": 0.0},
                  {"params": [p for i, p in enumerate(params) if i not in cfg["frozen"]], "lr": BASE_LR}]
        opt = cls(groups, lr=BASE_LR, betas=BETAS, weight_decay=cfg["wd"], **kw)
    else:
        opt = cls(params, lr=BASE_LR, betas=BETAS, weight_decay=cfg["wd"], **kw)
    sched = None
    if "sched" in cfg:
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=[AR.schedule(*cfg["sched"])] * len(opt.param_groups))
    return opt, sched


def run_torch(case, dtype, prob=None, steps=STEPS, start=None):
    """torch.optim.Adam(foreach=False) on the CPU; returns (params, optimizer)"""
    prob = prob or problem()
    params = [torch.from_numpy(p0.copy()).to(dtype).requires_grad_() for p0, _, _ in prob]
    a = [torch.from_numpy(x).to(dtype) for _, x, _ in prob]
    c = [torch.from_numpy(x).to(dtype) for _, _, x in prob]
    opt, sched = torch_optimizer(case, params, foreach=False)
    if start is not None:
        opt.load_state_dict(start["optimizer"])
        with torch.no_grad():
            for p, q in zip(params, start["params"]):
                p.copy_(torch.as_tensor(q))
    for _ in range(steps):
        with torch.no_grad():
            for p, ai, ci in zip(params, a, c):
                p.grad = ai * (p - ci)
        opt.step()
        if sched is not None:
            sched.step()
    return params, opt


def distance(x, ref):
    x, ref = np.asarray(x, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def measure():
    out = {}
    prob = problem()
    for case in CASES:
        mine = run_restatement(case, prob)
        t32, _ = run_torch(case, torch.float32, prob)
        t64, _ = run_torch(case, torch.float64, prob)
        rec = {}
        for i, k in enumerate(names()):
            ref = t64[i].detach().numpy()
            rec[k] = {"restatement": distance(mine[i][0], ref), "torch_float32": distance(t32[i].detach().numpy(), ref),
                      "same_bits": bool(np.array_equal(mine[i][0].view(np.uint32), t32[i].detach().numpy().view(np.uint32)))}
        out[case] = rec
    return out


@pytest.fixture(scope="module")
def measured():
    return measure()


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_against_torch_adam(measured, case):
    """50 steps of the quadratic problem on the model's 33 shapes: per tensor, the restatement's relative L2 distance from torch's
    float64 run is at most twice torch-float32's own (MARGIN).  The two float32 runs are NOT bit-identical on the machine the
    fixture was recorded on (torch 2.10 CPU: only the one- and three-element tensors end on the same bits, "same_bits" in
    tests/golden/adam_errors.json - torch's vectorised CPU kernels contract some of the products); both sit at 1.0e-7 ... 3.6e-7
    from float64 and within 2.4 % of each other."""
    for k, r in measured[case].items():
        print(case, k, r)
        assert r["restatement"] <= MARGIN * r["torch_float32"], (case, k, r)
    frozen = CASES[case].get("frozen", ())
    if frozen:          # lr = 0: the frozen tensors keep p0's bits while their moments move
        prob = problem()
        state = run_restatement(case, prob, steps=3)
        for i in frozen:
            assert np.array_equal(state[i][0].view(np.uint32), prob[i][0].view(np.uint32)), names()[i]
            assert state[i][1].any() and state[i][2].any()
            assert measured[case][names()[i]]["restatement"] == 0.0 == measured[case][names()[i]]["torch_float32"]


def test_recorded_distances_cover_every_case_and_tensor():
    with open(ERRORS) as f:
        rec = json.load(f)
    assert rec["steps"] == STEPS and rec["margin"] == MARGIN and set(rec["cases"]) == set(CASES)
    for case in CASES:
        assert set(rec["cases"][case]) == set(names())
        for r in rec["cases"][case].values():
            assert 0.0 <= r["restatement"] <= MARGIN * r["torch_float32"] < 1e-5


# ---- 3. state_dict round trips --------------------------------------------------------------------------------------------------
def restatement_state_dict(case, state, steps):
    """the state of a restatement run in torch.optim.Adam's state_dict layout (what dsnerf_amd.optim.Adam keeps)"""
    params = [torch.from_numpy(s[0].copy()).requires_grad_() for s in state]
    opt, sched = torch_optimizer(case, params, foreach=False)
    sd = opt.state_dict()
    order = [i for g in opt.param_groups for p in g["params"] for i, q in enumerate(params) if q is p]
    sd["state"] = {j: {"step": torch.tensor(float(steps), dtype=torch.float32), "exp_avg": torch.from_numpy(state[i][1].copy()),
                       "exp_avg_sq": torch.from_numpy(state[i][2].copy())} for j, i in enumerate(order)}
    return sd


@pytest.mark.parametrize("case", ["decay", "two_groups"])
def test_state_dict_round_trips(case):
    """restatement -> torch: a CPU torch Adam that loads the restatement's state after 20 steps holds identical state tensors, and
    continues to the parameters of 30 uninterrupted restatement steps within MARGIN x the recorded float32 distance (frozen tensors:
    identical).  torch -> dsnerf_amd.optim.Adam's layout: equal keys, equal dtypes, a float32 0-dim `step` on the CPU."""
    prob = problem()
    part = run_restatement(case, prob, steps=20)
    whole = run_restatement(case, prob, steps=30)
    sd = restatement_state_dict(case, part, 20)
    # (load_state_dict keeps the tensors it is given where dtype and device already fit: each optimizer gets its own copy)
    params, opt = run_torch(case, torch.float32, prob, steps=10, start={"optimizer": copy.deepcopy(sd), "params": [s[0] for s in part]})
    with open(ERRORS) as f:
        rec = json.load(f)["cases"][case]
    after = opt.state_dict()
    order = [i for g in opt.param_groups for p in g["params"] for i, q in enumerate(params) if q is p]
    loaded = run_torch(case, torch.float32, prob, steps=0, start={"optimizer": copy.deepcopy(sd), "params": [s[0] for s in part]})[1].state_dict()
    for j, i in enumerate(order):
        st = after["state"][j]
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 30.0
        assert float(loaded["state"][j]["step"]) == 20.0
        for k, want in (("exp_avg", part[i][1]), ("exp_avg_sq", part[i][2])):          # the round trip itself: identical state tensors
            assert np.array_equal(loaded["state"][j][k].numpy().view(np.uint32), want.view(np.uint32)), (case, names()[i], k)
        if i in CASES[case].get("frozen", ()):
            assert np.array_equal(params[i].detach().numpy().view(np.uint32), whole[i][0].view(np.uint32))
        else:           # ten torch steps against ten restatement steps: two float32 roundings of one formula, the bar of test 2
            assert distance(params[i].detach().numpy(), whole[i][0]) <= MARGIN * rec[names()[i]]["torch_float32"], (case, names()[i])
    # the layout of a fresh torch Adam's state_dict and of the one built from the restatement are the same, key for key
    fresh = run_torch(case, torch.float32, prob, steps=1)[1].state_dict()
    assert set(fresh) == set(sd) and [set(g) for g in fresh["param_groups"]] == [set(g) for g in sd["param_groups"]]
    assert set(fresh["state"]) == set(sd["state"])
    for j in fresh["state"]:
        assert set(fresh["state"][j]) == set(sd["state"][j]) == {"step", "exp_avg", "exp_avg_sq"}
        for k in fresh["state"][j]:
            assert fresh["state"][j][k].dtype == sd["state"][j][k].dtype and fresh["state"][j][k].shape == sd["state"][j][k].shape
            assert fresh["state"][j][k].device == sd["state"][j][k].device
    # dsnerf_amd.optim.Adam declares the same group keys (its tensors need a GPU: tests/test_gpu_adam.py loads state both ways there)
    import dsnerf_amd
    declared = {"lr", "betas", "eps", "weight_decay", "params"} | set(dsnerf_amd.optim._TORCH_GROUP_DEFAULTS)
    assert all(set(g) == declared for g in fresh["param_groups"]), (fresh["param_groups"][0].keys(), declared)


def test_public_optimizer_rejects_what_it_does_not_implement():
    import dsnerf_amd
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="GPU"):
        dsnerf_amd.optim.Adam([p])                               # a CPU tensor: no other arithmetic to fall back to
    for kw in ("amsgrad", "maximize", "capturable", "differentiable", "fused", "foreach"):
        with pytest.raises(ValueError, match=kw):
            dsnerf_amd.optim.Adam([p], **{kw: True})
    with pytest.raises(ValueError, match="beta"):
        dsnerf_amd.optim.Adam([p], betas=(1.0, 0.999))
    with pytest.raises(TypeError):
        dsnerf_amd.optim.Adam([p], nesterov=True)
    from types import SimpleNamespace
    cfg = SimpleNamespace(SOLVER=SimpleNamespace(WEIGHT_DECAY=0.0, BASE_LR=5e-4, OPTIMIZER_NAME="SGD"))
    with pytest.raises(ValueError, match="OPTIMIZER_NAME"):
        dsnerf_amd.optim.make_optimizer(cfg, torch.nn.Linear(2, 2))


# ---- 4. the library's host side -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    return dsnerf_amd._lib


def test_host_scalars_are_the_restatements(L):
    assert (L.ADAM_TABLE, L.ADAM_BLOCK) == (AR.TABLE, AR.BLOCK) and AR.TABLE >= len(AR.SHAPES)
    for lr, wd, betas, eps, t in ((5e-4, 0.0, BETAS, EPS, 1), (5e-4, 0.01, BETAS, EPS, 2), (1e-3, 1e-4, (0.5, 0.9), 1e-6, 1000),
                                  (0.0, 0.0, BETAS, EPS, 7), (3e-4, 0.0, (0.0, 0.0), 0.0, 3), (5e-4, 0.0, BETAS, EPS, 123457)):
        got, want = L.adam_scalars(lr, wd, betas, eps, t), AR.scalars(lr, wd, betas, eps, t)
        for k in want:
            assert np.float32(got[k]).view(np.uint32) == want[k].view(np.uint32), (k, got[k], want[k])


def test_argument_checks(L):
    lib = L.lib()
    n = 3
    one = (C.c_void_p * n)(*[64] * n)              # (never dereferenced: every call below is refused before anything is enqueued)
    ns = (C.c_int64 * n)(*[4] * n)
    lr, wd = (C.c_double * n)(*[5e-4] * n), (C.c_double * n)(*[0.0] * n)

    def call(params=one, grads=one, m=one, v=one, ns=ns, count=n, lr=lr, wd=wd, b1=0.9, b2=0.999, eps=1e-8, t=1.0, packed=None):
        return lib.dsn_adam_step(params, grads, m, v, ns, count, lr, wd, b1, b2, eps, t, packed, None)

    def refused(msg, **kw):
        assert call(**kw) != 0, kw
        err = lib.dsn_last_error()
        assert b"dsn_adam_step" in err and msg in err, (kw, err)

    for which in ("params", "grads", "m", "v", "ns", "lr", "wd"):
        refused(b"null argument", **{which: None})
    refused(b"count", count=-1)
    refused(b"length", ns=(C.c_int64 * n)(4, -1, 4))
    refused(b"length", ns=(C.c_int64 * n)(4, (1 << 33) + 1, 4))
    refused(b"null tensor pointer", m=(C.c_void_p * n)(64, None, 64))
    for kw in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan")), dict(t=0.0), dict(t=0.5), dict(t=float("inf")),
               dict(eps=-1e-8), dict(eps=float("nan"))):
        refused(b"betas must lie in [0, 1)", **kw)
    refused(b"lr and weight_decay", lr=(C.c_double * n)(5e-4, -1.0, 5e-4))
    refused(b"lr and weight_decay", wd=(C.c_double * n)(0.0, 0.0, float("inf")))
    # packed: the model's 33 tensors, with their lengths and no null parameter
    refused(b"33 tensors", packed=C.c_void_p(64))
    N = 33
    sizes = [int(np.prod(s)) for s in AR.SHAPES]
    p33 = (C.c_void_p * N)(*[64] * N)
    d33 = (C.c_double * N)(*[0.0] * N)
    wrong = list(sizes)
    wrong[5] += 1
    refused(b"33 tensors", params=p33, grads=p33, m=p33, v=p33, ns=(C.c_int64 * N)(*wrong), count=N, lr=d33, wd=d33, packed=C.c_void_p(64))
    holed = (C.c_void_p * N)(*[64] * 7 + [None] + [64] * 25)
    none = (C.c_void_p * N)()
    refused(b"33 tensors", params=holed, grads=none, m=p33, v=p33, ns=(C.c_int64 * N)(*sizes), count=N, lr=d33, wd=d33, packed=C.c_void_p(64))
    assert lib.dsn_adam_scalars_host(5e-4, 0.0, 0.9, 0.999, 1e-8, 0.0, (C.c_float * 7)()) != 0 and b"dsn_adam_scalars_host" in lib.dsn_last_error()
    assert lib.dsn_adam_scalars_host(5e-4, 0.0, 0.9, 0.999, 1e-8, 1.0, None) != 0


if __name__ == "__main__":
    if "--record" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        with open(ERRORS, "w") as f:
            json.dump({"what": "relative L2 distance per tensor from torch.optim.Adam in float64 after 50 CPU steps of the quadratic problem of "
                               "tests/test_adam_host.py: the numpy float32 restatement of dsn_adam_step's rule and torch.optim.Adam(foreach=False) "
                               "in float32; same_bits: the two float32 runs ended bit-identical",
                       "steps": STEPS, "margin": MARGIN, "torch": torch.__version__, "cases": measure()}, f, indent=1)
            f.write("\n")
        print("wrote", ERRORS)
